"""The fp16x2 convolution stack of the generic regressor (csrc/regress_generic_h2.hip, mode P2P_REGRESS_GENERIC_FP16X2) compiled
for the host and run on the CPU (tests/hipemu), on the "emu" inputs of tests/regressor_reference.py (48x64, 11 proposals): cases
A-E and R against the fp32 restatement at the project's bars, launch invariance bit for bit, the round trip between the two
modes, and the range variants of tests/generic_mode_reference.py.  Case R runs here too: one emulated run of its 11 proposals
takes about half a minute (case E, the slowest, a minute and a half).  The emulator sums an MFMA's K products one by one, so its
error bounds the hardware's from above (NOTES.md)."""
import ctypes
import os
import sys

import pytest
import torch

import generic_mode_reference as gm
import regressor_reference as rr
from patch2pix_amd import _lib as real
from patch2pix_amd.utils import synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


@pytest.fixture(scope="module")
def pyramids():
    return rr.inputs("emu")[:2]


PROPS = rr.inputs("emu")[2]


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "R"])
def test_cases_against_restatement(case, emu, pyramids):
    mid, fine = gm.emu_handles(emu, case)
    out = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], PROPS)
    rr.check_levels(out, pyramids[0], pyramids[1], PROPS, case, "emulated generic_fp16x2")
    gm.destroy(emu, mid, fine)


def _pyramid(levels):
    lv = [t.contiguous() for t in levels[:4]]
    q = real.Pyramid()
    for j in range(4):
        q.level[j] = lv[j].data_ptr()
    q.height, q.width = lv[0].shape[-2:]
    return q, lv


def _batch(emu, mid, fine, pyrs1, pyrs2, props, counts, dev_counts=None, sentinel=float("nan")):
    """p2p_regress_batch (dev_counts None: counts are the proposal counts) or p2p_regress_batch_dev (counts = the stride, once) over
    several items -> dict of concatenated outputs."""
    keep = [_pyramid(p) for p in pyrs1] + [_pyramid(p) for p in pyrs2]
    nb = len(pyrs1)
    a1 = (real.Pyramid * nb)(*[k[0] for k in keep[:nb]])
    a2 = (real.Pyramid * nb)(*[k[0] for k in keep[nb:]])
    props = props.contiguous()
    n = props.shape[0]
    out = {k: torch.full((n, c) if c > 1 else (n,), sentinel, dtype=torch.float32)
           for k, c in (("matches1", 4), ("probs1", 1), ("raw1", 5), ("matches2", 4), ("probs2", 1), ("raw2", 5))}
    need = emu.p2p_regress_workspace_bytes_for(mid, n)
    ws = torch.empty(need + 128, dtype=torch.uint8)
    wsp = ctypes.c_void_p((ws.data_ptr() + 127) & ~127)
    outs = [out[k].data_ptr() for k in ("matches1", "probs1", "raw1", "matches2", "probs2", "raw2")]
    if dev_counts is None:
        st = emu.p2p_regress_batch(mid, fine, nb, a1, a2, (ctypes.c_int * nb)(*counts), props.data_ptr(), 0, *outs, wsp, need, None)
    else:
        dc = torch.tensor(dev_counts, dtype=torch.int32)
        st = emu.p2p_regress_batch_dev(mid, fine, nb, a1, a2, dc.data_ptr(), counts, props.data_ptr(), 0, *outs, wsp, need, None)
    assert st == 0, emu.p2p_last_error()
    return out


@pytest.mark.parametrize("case", ["A", "C"])
def test_outputs_do_not_depend_on_the_launch(case, emu, pyramids):
    """A proposal's raw outputs, bit for bit: alone, inside a ragged 3-item batch with another image size in front and behind,
    with device-side counts (tests/test_gpu_regressor_configs.py: stride 64, counts 61 / 0 / 17; here stride 12, counts 11 / 0 / 3
    for the 11 proposals), and with a workspace of exactly one 8-proposal unit."""
    mid, fine = gm.emu_handles(emu, case)
    p1, p2 = pyramids
    base = rr.emu_regress(emu, mid, fine, p1, p2, PROPS)
    for i in (1, 10):
        one = rr.emu_regress(emu, mid, fine, p1, p2, PROPS[i:i + 1])
        assert torch.equal(one["raw1"][0], base["raw1"][i]) and torch.equal(one["raw2"][0], base["raw2"][i])
    # ragged batch: another pair of another size in front (3 proposals) and behind (2)
    q1, q2 = synthetic.make_pyramid(51, 32, 40), synthetic.make_pyramid(52, 32, 40)
    small = torch.tensor([[5, 6, 35, 25], [20, 15, 21, 16], [39, 31, 0, 0]], dtype=torch.int64)
    rag = _batch(emu, mid, fine, [q1, p1, q1], [q2, p2, q2], torch.cat([small, PROPS, small[:2]]), [3, 11, 2])
    for k in base:
        assert torch.equal(rag[k][3:14], base[k]), k
    assert torch.equal(rag["raw2"][:2], rag["raw2"][14:])
    # device-side counts: slots past the counts keep their sentinel
    stride, counts, sentinel = 12, (11, 0, 3), -7.5
    padded = torch.zeros((3, stride, 4), dtype=torch.int64)
    for b, c in enumerate(counts):
        padded[b, :c] = PROPS[:c]
    dev = _batch(emu, mid, fine, [p1] * 3, [p2] * 3, padded.view(-1, 4), stride, dev_counts=counts, sentinel=sentinel)
    for b, c in enumerate(counts):
        for k in base:
            got = dev[k][b * stride:(b + 1) * stride]
            assert torch.equal(got[:c], base[k][:c]), (k, b)
            assert bool((got[c:] == sentinel).all()), (k, b)
    # one unit of 8 proposals: two chunks
    unit = emu.p2p_regress_workspace_bytes_for(mid, 8)
    assert emu.p2p_regress_workspace_bytes_for(mid, 11) == 2 * unit
    chunked = rr.emu_regress(emu, mid, fine, p1, p2, PROPS, ws_bytes=unit)
    for k in base:
        assert torch.equal(chunked[k], base[k]), k
    with pytest.raises(AssertionError, match="returned -4"):              # below one unit: P2P_ENOMEM
        rr.emu_regress(emu, mid, fine, p1, p2, PROPS, ws_bytes=unit - 128)
    gm.destroy(emu, mid, fine)


def test_round_trip_between_the_modes(emu, pyramids):
    """generic -> generic_fp16x2 -> generic gives the first call's bits, generic_fp16x2 a second time the second call's; the two
    arithmetics differ in bits (the mode is not a relabelled one) and agree within the bars."""
    case = "A"
    mid, fine = gm.emu_handles(emu, case, mode=gm.GENERIC)
    run = lambda: rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], PROPS)

    def select(mode):
        for h in (mid, fine):
            assert emu.p2p_regressor_set_mode(h, mode) == gm.OK, emu.p2p_last_error()
    first = run()
    select(gm.GENERIC_FP16X2)
    second = run()
    select(gm.GENERIC)
    third = run()
    select(gm.GENERIC_FP16X2)
    fourth = run()
    for k in first:
        assert torch.equal(first[k], third[k]) and torch.equal(second[k], fourth[k]), k
    assert not torch.equal(first["raw2"], second["raw2"])
    dc = max((first[k] - second[k]).abs().max().item() for k in ("matches1", "matches2"))
    ds = max((first[k] - second[k]).abs().max().item() for k in ("probs1", "probs2"))
    print(f"case {case}: generic vs generic_fp16x2 coord {dc:.3g} px score {ds:.3g}")
    assert dc <= 2 * rr.COORD_TOL and ds <= 2 * rr.SCORE_TOL              # each within the bars of the same restatement
    gm.destroy(emu, mid, fine)


@pytest.mark.parametrize("variant", gm.VARIANTS)
def test_range_variants(variant, emu, pyramids):
    """Case A with layer 0's BatchNorm x 2^10 / x 2^-10 (the per-sample exponent of layer 1 at both ends) and with one channel's
    weight x 2^8 (an outlier channel under the sample's shared exponent), at the same bars."""
    case = "A"
    mid, fine = gm.emu_handles(emu, case, sd=gm.variant_state_dict(case, variant))
    out = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], PROPS)
    gm.check_variant(out, pyramids[0], pyramids[1], PROPS, case, variant, "emulated")
    gm.destroy(emu, mid, fine)
