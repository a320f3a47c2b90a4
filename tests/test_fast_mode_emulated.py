"""Mode 'fp16' on the kernels' own code executed on the CPU (tests/hipemu): accuracy against the fp64 yardstick under the error
model of tests/fast_mode_reference.py, the side of io_thres, and the launch invariants by bytes.

The bars are the MODEL's (derived from the operands of each case); the measured figures are printed (pytest -s) and recorded
in fast_mode_reference.MEASURED_EMULATED.  The invariants run one regressor level (the chain adds nothing to them here; the
GPU test runs both levels): a proposal and level is some seconds in the emulator.

Chunks.  A chunk of this mode is cut from the proposal count alone (whole units of 256, regress_common.h), never from the
workspace size, so "a small chunk" cannot be forced through the workspace: the workspace cases are the exact query (poisoned)
and a larger buffer.  Calls of more than one chunk (more than 3328 proposals) are hours in the emulator; they run on the GPU
(tests/test_gpu_fast_mode.py, test_more_proposals_than_a_chunk)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import fast_mode_reference as fm  # noqa: E402
import golden_util as gu  # noqa: E402
import range_reference as rr  # noqa: E402
from oracle import p2p_oracle as orc  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def test_winograd_form_of_the_model_is_the_direct_form():
    sd, p1, p2, props = fm.case_inputs("plain")
    p = rr.params64(sd)[0]
    d = lambda q: [t.double() for t in q]
    with torch.no_grad():
        f1 = orc.gather_patch_feats(d(p1), props[:1, 0], props[:1, 1])
        f2 = orc.gather_patch_feats(d(p2), props[:1, 2], props[:1, 3])
        raw, _ = fm.winograd_forward(torch.cat([f1, f2], 1), p, p["conv.0.weight"], fm.transformed_filters(p["conv.2.weight"]))
        want = orc.regressor_forward(f1, f2, p)[0]
    assert (raw - want).abs().max().item() <= 1e-11 * want.abs().max().item()


@pytest.mark.parametrize("name", list(fm.CASES))
def test_accuracy_within_the_model(name, emu):
    sd, p1, p2, props = fm.case_inputs(name)
    out = fm.emu_run(emu, sd, p1, p2, props)
    res = rr.measure(out, sd, p1, p2, props, with_f32=True)          # finite, in bounds, a sensitive case
    coord_bar, score_bar, score_b, p64 = fm.bounds(sd, p1, p2, props, out["matches1"])
    with torch.no_grad():
        p32 = orc.fine_level(p1, p2, out["matches1"], orc.split_params(sd)[2])[1]
    nflip, cap = fm.flips(out["probs2"], p64), fm.flip_cap(p32, p64, score_b)
    print(f"\nfp16[emulator] {name:>20s}: coord {res['coord']:.2e} px (model {coord_bar:.2e})  score {res['score']:.2e} "
          f"(model {score_bar:.2e})  | fp32 oracle {res['o32_coord']:.2e} px {res['o32_score']:.2e} | io_thres flips {nflip} (cap {cap})")
    assert res["coord"] <= coord_bar and res["score"] <= score_bar, res
    assert nflip <= cap
    # the emulator is deterministic CPU code: the figures recorded next to the model (fm.MEASURED_EMULATED) are
    # reproduced, so an operand class that silently lost (or gained) bits shows although the bound is 5-7x away
    rec = fm.MEASURED_EMULATED[name]
    assert abs(res["coord"] - rec[0]) <= 0.05 * rec[0] and abs(res["score"] - rec[2]) <= 0.05 * rec[2], (res, rec)
    assert abs(coord_bar - rec[1]) <= 0.02 * rec[1] and abs(score_bar - rec[3]) <= 0.02 * rec[3], (coord_bar, score_bar, rec)
    # the mode is a different arithmetic, not a relabelled one: far above the fp32 oracle's own error
    assert res["raw"] > 10 * res["o32_raw"]


@pytest.mark.parametrize("tag", ["int_mid", "float_fine"])
def test_against_the_reference_golden(tag, emu):
    """The reference's own fp32 outputs (fine_48x64.npz, the inputs tests/test_kernels_emulated.py feeds the other modes): mode
    fp16 lies within the model's per-proposal bound of them."""
    import regressor_reference as rg
    golden = fm.golden_level(tag, 4)
    p1, p2, props = golden[:3]
    reg, keep = fm.create(emu, fm.sub_sd(gu.state_dict(0), "regress_mid." if tag == "int_mid" else "regress_fine."), fm.MODE_ID)
    try:
        out = rg.emu_regress(emu, reg, None, p1, p2, props)
    finally:
        emu.p2p_regressor_destroy(reg)
    fm.assert_against_golden(tag, out["matches1"], out["probs1"], golden, "emulator")


def test_not_bit_equal_to_the_two_plane_mode(emu):
    sd, p1, p2, props = fm.case_inputs("plain")
    a = fm.emu_run(emu, sd, p1, p2, props[:1], two=False)
    b = fm.emu_run(emu, sd, p1, p2, props[:1], mode_id=4, two=False)
    assert not torch.equal(a["raw1"], b["raw1"])
    assert (a["raw1"] - b["raw1"]).abs().max().item() < 1e-2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, rows_a, rows_b, what):
    for k in ("matches1", "probs1", "raw1"):
        assert torch.equal(_bits(a[k])[rows_a], _bits(b[k])[rows_b]), f"{what}: {k}"


@pytest.fixture(scope="module")
def big(emu):
    """17 proposals (corners first) on a 64 x 96 pair, one level."""
    sd = gu.state_dict(0)
    p1, p2 = rr.pair("plain", 64, 96)
    props = rr.proposals(64, 96, 17)
    props[3] = torch.tensor([96, 0, 0, 64])
    props[4] = torch.tensor([0, 64, 96, 0])
    return sd, p1, p2, props, fm.emu_run(emu, sd, p1, p2, props, two=False)


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_proposal_alone_and_in_batches(n, big, emu):
    """Units of 8 rows per GEMM block and their edges; n = 17 is the big launch itself, n = 1 a corner proposal alone."""
    sd, p1, p2, props, ref = big
    lo = 0 if n > 1 else 3
    out = fm.emu_run(emu, sd, p1, p2, props[lo:lo + n], two=False)
    _same(out, ref, slice(0, n), slice(lo, lo + n), f"n = {n}")


def test_workspace_exact_poisoned_and_larger(big, emu):
    import ctypes
    import regressor_reference as rg
    sd, p1, p2, props, ref = big
    n = 9
    need = emu.p2p_regress_workspace_bytes_mode(n, fm.MODE_ID)
    out = fm.emu_run(emu, sd, p1, p2, props[:n], two=False, ws_bytes=need + 4096 * 5)
    _same(out, ref, slice(0, n), slice(0, n), "a larger workspace")
    # exactly the queried size, every byte a NaN pattern, guard bytes behind it intact
    mid, keep = fm.create(emu, fm.sub_sd(sd, "regress_mid."), fm.MODE_ID)
    try:
        from patch2pix_amd import _lib as real
        ws = torch.full(((need + 128 + 256) // 4 + 1,), float("nan"))
        base = (ws.data_ptr() + 127) & ~127
        guard_at = (base - ws.data_ptr() + need) // 4
        lv = [[t.contiguous() for t in p[:4]] for p in (p1, p2)]
        pyr = []
        for levels in lv:
            q = real.Pyramid()
            for j in range(4):
                q.level[j] = levels[j].data_ptr()
            q.height, q.width = levels[0].shape[-2:]
            pyr.append((real.Pyramid * 1)(q))
        o = {k: torch.full((n, c) if c > 1 else (n,), float("nan")) for k, c in (("matches1", 4), ("probs1", 1), ("raw1", 5))}
        pr = props[:n].contiguous()
        st = emu.p2p_regress_batch(mid, None, 1, pyr[0], pyr[1], (ctypes.c_int * 1)(n), pr.data_ptr(), 0, o["matches1"].data_ptr(),
                                   o["probs1"].data_ptr(), o["raw1"].data_ptr(), None, None, None, ctypes.c_void_p(base), need, None)
        assert st == 0, emu.p2p_last_error().decode()
        assert bool(torch.isnan(ws[guard_at:]).all()), "the launch wrote behind the queried size"
        _same(o, ref, slice(0, n), slice(0, n), "a poisoned workspace of exactly the queried size")
        # one byte less is refused (P2P_ENOMEM), not run
        st = emu.p2p_regress_batch(mid, None, 1, pyr[0], pyr[1], (ctypes.c_int * 1)(n), pr.data_ptr(), 0, o["matches1"].data_ptr(),
                                   o["probs1"].data_ptr(), o["raw1"].data_ptr(), None, None, None, ctypes.c_void_p(base), need - 1, None)
        assert st == -4
    finally:
        emu.p2p_regressor_destroy(mid)


def test_unrounded_image_and_device_counts(emu):
    """A 100 x 140 image (its pyramid levels round up, the gather clamps to dim // 2^j - 1) with corner proposals; the same
    proposals as two items with device-side counts, one of them empty, leave the same bytes and untouched empty slots."""
    import ctypes
    from patch2pix_amd import _lib as real
    sd = gu.state_dict(0)
    hh, ww = 100, 140
    p1, p2 = fm.unrounded_pair(hh, ww)
    props = torch.tensor([[0, 0, ww, hh], [ww, hh, 0, 0], [ww - 1, 3, 70, hh - 1]], dtype=torch.int64)
    ref = fm.emu_run(emu, sd, p1, p2, props, two=False)
    assert bool(torch.isfinite(ref["raw1"]).all())
    with torch.no_grad():
        want = orc.fine_level([t.double() for t in p1], [t.double() for t in p2], props, rr.params64(sd)[0])
    cb, sb, _, _ = fm.bounds(sd, p1, p2, props, want[0].float())
    assert (ref["matches1"].double() - want[0]).abs().max().item() <= cb and (ref["probs1"].double() - want[1]).abs().max().item() <= sb
    # two items of stride 4: counts (3, 0) on the device
    mid, keep = fm.create(emu, fm.sub_sd(sd, "regress_mid."), fm.MODE_ID)
    try:
        stride, nitems = 4, 2
        lv = [[t.contiguous() for t in p] for p in (p1, p2)]
        arrs = []
        for levels in lv:
            q = real.Pyramid()
            for j in range(4):
                q.level[j] = levels[j].data_ptr()
            q.height, q.width = hh, ww
            arrs.append((real.Pyramid * nitems)(q, q))
        slots = torch.zeros(nitems * stride, 4, dtype=torch.int64)
        slots[:3] = props
        counts = torch.tensor([3, 0], dtype=torch.int32)
        need = emu.p2p_regress_workspace_bytes_mode(nitems * stride, fm.MODE_ID)
        ws = torch.full((need // 4 + 64,), float("nan"))
        base = (ws.data_ptr() + 127) & ~127
        mark = 12345.0
        o = {k: torch.full((nitems * stride, c) if c > 1 else (nitems * stride,), mark) for k, c in (("matches1", 4), ("probs1", 1), ("raw1", 5))}
        emu.p2p_regress_batch_dev.argtypes, emu.p2p_regress_batch_dev.restype = real.p2p_regress_batch_dev.argtypes, ctypes.c_int
        st = emu.p2p_regress_batch_dev(mid, None, nitems, arrs[0], arrs[1], counts.data_ptr(), stride, slots.data_ptr(), 0,
                                       o["matches1"].data_ptr(), o["probs1"].data_ptr(), o["raw1"].data_ptr(), None, None, None,
                                       ctypes.c_void_p(base), need, None)
        assert st == 0, emu.p2p_last_error().decode()
        _same(o, ref, slice(0, 3), slice(0, 3), "device-side counts")
        assert bool((o["matches1"][3:] == mark).all()) and bool((o["probs1"][3:] == mark).all()), "an empty slot was written"
    finally:
        emu.p2p_regressor_destroy(mid)
