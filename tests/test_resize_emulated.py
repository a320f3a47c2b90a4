"""The two resize kernels of csrc/preprocess.hip run on the CPU through tests/hipemu, against the installed Pillow: uint8
output bit-equal, float output torch.equal to `_normalised` of Pillow's result."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import resize_reference as rr


@pytest.fixture(scope="module")
def emu():
    from hipemu import emu_lib
    from patch2pix_amd import _lib as real
    lib = emu_lib.load()
    lib.p2p_resize_workspace_bytes.restype = ctypes.c_size_t
    lib.p2p_resize_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.p2p_resize_bicubic_batch.restype = ctypes.c_int
    lib.p2p_resize_bicubic_batch.argtypes = ([ctypes.POINTER(real.ResizeItem)] + [ctypes.c_int] * 3 +
                                             [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p])
    return lib


def _lut():
    from patch2pix_amd.utils.datasets import preprocess
    v = np.arange(256, dtype=np.float32)[None, :].repeat(3, 0).reshape(3, 256, 1)
    v /= 255.0
    return ((torch.from_numpy(v) - torch.from_numpy(preprocess._MEAN)) / torch.from_numpy(preprocess._STD)).reshape(3, 256).contiguous()


def run(emu, images, out_hw, floats_into=None, misalign=0):
    """images: uint8 [h,w,3] arrays -> (uint8 [B,oh,ow,3], float32 [B,3,oh,ow]) through the emulated library.  misalign:
    byte offset of every source image from a 16-byte boundary (device allocations are aligned, slices of them are not)."""
    from patch2pix_amd import _lib as real
    from patch2pix_amd.utils.datasets import preprocess
    oh, ow = out_hw
    nb = len(images)
    keep, desc = [], (real.ResizeItem * nb)()
    for i, img in enumerate(images):
        h, w = img.shape[:2]
        buf = torch.zeros(img.size + 32, dtype=torch.uint8)
        off = (-buf.data_ptr()) % 16 + misalign
        buf[off:off + img.size] = torch.from_numpy(img.reshape(-1).copy())
        keep.append(buf)
        desc[i].pixels, desc[i].in_h, desc[i].in_w = buf.data_ptr() + off, h, w
        if w != ow:
            t = torch.from_numpy(preprocess._packed_table(w, ow).copy())
            keep.append(t)
            desc[i].table_x, desc[i].ksize_x = t.data_ptr(), preprocess.resize_ksize(w, ow)
        if h != oh:
            t = torch.from_numpy(preprocess._packed_table(h, oh).copy())
            keep.append(t)
            desc[i].table_y, desc[i].ksize_y = t.data_ptr(), preprocess.resize_ksize(h, oh)
    need = emu.p2p_resize_workspace_bytes(nb, max(i.shape[0] for i in images), max(i.shape[1] for i in images), oh, ow)
    assert need > 0
    ws = torch.empty(need + 16, dtype=torch.uint8)
    wsp = (ws.data_ptr() + 15) & ~15
    out_u8 = torch.full((nb, oh, ow, 3), 77, dtype=torch.uint8)
    out_f = torch.full((nb, 3, oh, ow), -9.0) if floats_into is None else floats_into
    lut = _lut()
    st = emu.p2p_resize_bicubic_batch(desc, nb, oh, ow, out_u8.data_ptr(), out_f.data_ptr(), 3 * oh * ow, lut.data_ptr(), wsp, need,
                                      None)
    assert st == 0, emu.p2p_last_error()
    del keep
    return out_u8, out_f


def _want(img, out_hw):
    from patch2pix_amd.utils.datasets import preprocess
    pil = Image.fromarray(img, "RGB").resize((out_hw[1], out_hw[0]), Image.BICUBIC)
    return np.array(pil, dtype=np.uint8), preprocess._normalised(pil)


@pytest.mark.parametrize("case", [c for c in rr.CASES if c != rr.BIG_CASE], ids=rr.case_id)
def test_emulated_kernels_equal_pillow(emu, case):
    (ih, iw), out_hw = case
    images = [rr.make_image(ih, iw, c) for c in rr.CONTENTS]
    got_u8, got_f = run(emu, images, out_hw)                      # the five contents as one batch of equal sizes
    for i, img in enumerate(images):
        want_u8, want_f = _want(img, out_hw)
        assert np.array_equal(got_u8[i].numpy(), want_u8), rr.CONTENTS[i]
        assert torch.equal(got_f[i], want_f), rr.CONTENTS[i]


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_emulated_unaligned_sources(emu, misalign):
    """A source that starts off a dword boundary: the staging loads of the horizontal kernel and the direct reads of the
    vertical one (no horizontal pass) take their byte paths at the ends of the image."""
    for (ih, iw), out_hw in [((37, 53), (16, 32)), ((48, 64), (16, 64)), ((32, 32), (32, 32))]:
        img = rr.make_image(ih, iw, "noise", seed=misalign)
        got_u8, got_f = run(emu, [img], out_hw, misalign=misalign)
        want_u8, want_f = _want(img, out_hw)
        assert np.array_equal(got_u8[0].numpy(), want_u8)
        assert torch.equal(got_f[0], want_f)


def test_emulated_mixed_batch(emu):
    sizes, out_hw = rr.MIXED_BATCH
    for content in rr.CONTENTS:
        images = [rr.make_image(h, w, content, seed=i) for i, (h, w) in enumerate(sizes)]
        got_u8, got_f = run(emu, images, out_hw)
        for i, img in enumerate(images):
            want_u8, want_f = _want(img, out_hw)
            assert np.array_equal(got_u8[i].numpy(), want_u8), (content, i)
            assert torch.equal(got_f[i], want_f), (content, i)


def test_emulated_odd_output_width_and_long_taps(emu):
    """Output widths that are no multiple of 4 pixels (the tail of the vertical kernel's 12-byte groups, unaligned float
    rows) and a ratio whose taps leave room for a single output column per work-group."""
    for (ih, iw), out_hw in [((29, 41), (13, 19)), ((9, 3000), (9, 5)), ((40, 700), (21, 150))]:
        img = rr.make_image(ih, iw, "noise")
        got_u8, got_f = run(emu, [img], out_hw)
        want_u8, want_f = _want(img, out_hw)
        assert np.array_equal(got_u8[0].numpy(), want_u8), (ih, iw, out_hw)
        assert torch.equal(got_f[0], want_f)
