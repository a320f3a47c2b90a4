"""Bicubic resize + normalise on the MI355X (csrc/preprocess.hip) against the installed Pillow: every bar is equality."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import golden_util as gu
import resize_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pp():
    from patch2pix_amd.utils.datasets import preprocess
    return preprocess


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


def _want(pp, img, out_hw):
    pil = Image.fromarray(img, "RGB").resize((out_hw[1], out_hw[0]), Image.BICUBIC)
    return np.array(pil, dtype=np.uint8), pp._normalised(pil)


def _photo(pair, which):
    return os.path.join(gu.GOLDEN, "images", pair, f"{which}.jpg")


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_every_case_and_content_equals_pillow(case, dev, pp):
    (ih, iw), out_hw = case
    images = [rr.make_image(ih, iw, c) for c in rr.CONTENTS]
    pixels = [torch.from_numpy(i).to(dev) for i in images]
    got_u8 = pp.resize_pixels_device(pixels, out_hw).cpu()
    got_f = pp.resize_pixels_device(pixels, out_hw, normalise=True).cpu()
    assert got_u8.dtype == torch.uint8 and tuple(got_u8.shape) == (len(images),) + tuple(out_hw) + (3,)
    assert got_f.dtype == torch.float32 and tuple(got_f.shape) == (len(images), 3) + tuple(out_hw)
    for i, img in enumerate(images):
        want_u8, want_f = _want(pp, img, out_hw)
        assert np.array_equal(got_u8[i].numpy(), want_u8), rr.CONTENTS[i]
        assert torch.equal(got_f[i], want_f), rr.CONTENTS[i]
        alone = pp.resize_pixels_device(pixels[i], out_hw).cpu()             # a single tensor instead of a list
        assert torch.equal(alone[0], got_u8[i])


def test_odd_widths_long_taps_and_unaligned_sources(dev, pp):
    """Output widths that are no multiple of 4 pixels, a ratio that leaves one output column per work-group, and sources
    that start 1..3 bytes off a dword boundary (slices of one allocation)."""
    for (ih, iw), out_hw in [((29, 41), (13, 19)), ((9, 3000), (9, 5)), ((40, 700), (21, 150))]:
        img = rr.make_image(ih, iw, "noise")
        want_u8, want_f = _want(pp, img, out_hw)
        assert np.array_equal(pp.resize_pixels_device(torch.from_numpy(img).to(dev), out_hw)[0].cpu().numpy(), want_u8)
        assert torch.equal(pp.resize_pixels_device(torch.from_numpy(img).to(dev), out_hw, normalise=True)[0].cpu(), want_f)
    for off in (1, 2, 3):
        for (ih, iw), out_hw in [((37, 53), (16, 32)), ((48, 64), (16, 64)), ((32, 32), (32, 32))]:
            img = rr.make_image(ih, iw, "noise", seed=off)
            flat = torch.zeros(img.size + 8, dtype=torch.uint8, device=dev)
            flat[off:off + img.size] = torch.from_numpy(img.reshape(-1)).to(dev)
            src = flat[off:off + img.size].view(ih, iw, 3)
            assert src.data_ptr() % 4 == off
            want_u8, want_f = _want(pp, img, out_hw)
            assert np.array_equal(pp.resize_pixels_device(src, out_hw)[0].cpu().numpy(), want_u8)
            assert torch.equal(pp.resize_pixels_device(src, out_hw, normalise=True)[0].cpu(), want_f)


def test_mixed_batch_equals_items_alone_and_pillow(dev, pp):
    sizes, out_hw = rr.MIXED_BATCH
    for content in rr.CONTENTS:
        images = [rr.make_image(h, w, content, seed=i) for i, (h, w) in enumerate(sizes)]
        pixels = [torch.from_numpy(i).to(dev) for i in images]
        got_u8 = pp.resize_pixels_device(pixels, out_hw)
        got_f = pp.resize_pixels_device(pixels, out_hw, normalise=True)
        for i, img in enumerate(images):
            assert torch.equal(got_u8[i], pp.resize_pixels_device(pixels[i], out_hw)[0])
            assert torch.equal(got_f[i], pp.resize_pixels_device(pixels[i], out_hw, normalise=True)[0])
            want_u8, want_f = _want(pp, img, out_hw)
            assert np.array_equal(got_u8[i].cpu().numpy(), want_u8) and torch.equal(got_f[i].cpu(), want_f)


def test_more_items_than_one_launch_group(dev, pp):
    """70 items: the library launches in groups of 64."""
    images = [rr.make_image(20 + i % 7, 24 + i % 5, "noise", seed=i) for i in range(70)]
    got = pp.resize_pixels_device([torch.from_numpy(i).to(dev) for i in images], (16, 16)).cpu().numpy()
    for i, img in enumerate(images):
        assert np.array_equal(got[i], rr.pil_resize(img, (16, 16))), i


def test_slot_of_a_larger_batch_tensor(dev, pp):
    """The float output goes straight into the caller's slots; the neighbours keep their contents."""
    out_hw = (32, 32)
    images = [rr.make_image(37, 53, "noise", seed=1), rr.make_image(131, 97, "noise", seed=2)]
    batch = torch.full((5, 3) + out_hw, -7.0, device=dev)
    got = pp.resize_pixels_device([torch.from_numpy(i).to(dev) for i in images], out_hw, normalise=True, out=batch[2:4])
    assert got.data_ptr() == batch[2].data_ptr()
    host = batch.cpu()
    for i, img in enumerate(images):
        assert torch.equal(host[2 + i], _want(pp, img, out_hw)[1])
    assert (host[:2] == -7.0).all() and (host[4:] == -7.0).all()


@pytest.mark.parametrize("pair,which,imsize", [("pair_3", 1, 640), ("pair_2", 1, None), ("pair_1", 2, 256)])
def test_load_im_flexible_device_equals_host(pair, which, imsize, dev, pp):
    path = _photo(pair, which)
    want, want_scale = pp.load_im_flexible(path, 2, 16, imsize=imsize)
    got, scale = pp.load_im_flexible_device(path, dev, 2, 16, imsize=imsize)
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert scale == want_scale
    assert torch.equal(got.cpu(), want)


def test_estimate_matches_device_resize_switch(dev, net):
    from patch2pix_amd.utils.eval import model_helper
    a, b = _photo("pair_1", 1), _photo("pair_1", 2)
    host = model_helper.estimate_matches_device(net, a, b, ksize=2, io_thres=0.25, imsize=256, resize="host")
    device = model_helper.estimate_matches_device(net, a, b, ksize=2, io_thres=0.25, imsize=256, resize="device")
    assert host[0].shape[0] > 0
    for x, y in zip(host, device):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    with pytest.raises(ValueError):
        model_helper.estimate_matches_device(net, a, b, resize="gpu")


def test_stream_resize_switch(dev, net):
    """Pairs of different original sizes (400x400 / 300x400 and 769x899 / 768x1024); the last two share a batch."""
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    pairs = [(_photo("pair_1", 1), _photo("pair_1", 2)), (_photo("pair_2", 1), _photo("pair_2", 2)),
             (_photo("pair_2", 1), _photo("pair_2", 2))]
    host = list(estimate_matches_stream(net, pairs, ksize=2, io_thres=0.25, imsize=256, batch=2, workers=2, resize="host"))
    device = list(estimate_matches_stream(net, pairs, ksize=2, io_thres=0.25, imsize=256, batch=2, workers=2, resize="device"))
    assert len(host) == len(device) == len(pairs)
    for h, d in zip(host, device):
        for x, y in zip(h, d):
            assert x.dtype == y.dtype and np.array_equal(x, y)
