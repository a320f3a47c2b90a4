"""The generic consensus kernels (csrc/consensus_generic.hip) compiled for the host and run on the CPU (tests/hipemu): every
case x volume of tests/ncn_reference.py against the fp64 restatement at 4 x the reference's own fp32 error, bit-identity of a
volume's output under batching and workspace size, the one-branch case, and the released stack through the generic handle
beside the tuned kernel inside forward_coarse_match."""
import ctypes
import os
import sys

import pytest
import torch

import ncn_reference as nr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


_handles = {}


def _handle(emu, case, layout=None):
    key = (case, str(layout))
    if key not in _handles:
        st, h = nr.create_config(emu, nr.weights(case), layout or nr.CASES[case])
        assert st == 0, emu.p2p_last_error()
        assert emu.p2p_ncn_is_generic(h) == 1
        _handles[key] = h
    return _handles[key]


@pytest.mark.parametrize("vol", list(nr.VOLUMES))
@pytest.mark.parametrize("case", list(nr.CASES))
def test_cases_against_fp64(case, vol, emu):
    x, _ = nr.expected(case, vol)
    y = nr.emu_consensus(emu, _handle(emu, case), x)
    nr.check(y, case, vol, "emulated")
    g = torch.from_numpy(nr.load_golden(case)[f"y_{vol}"])
    scale = nr.expected(case, vol)[1].abs().max().item()
    err = (y - g).abs().max().item()
    print(f"case {case} volume {vol} against the golden: {err:.3g}, bar {nr.BAR_GOLDEN * nr.REF_ERR[case] * scale:.3g}")
    assert err <= nr.BAR_GOLDEN * nr.REF_ERR[case] * scale


@pytest.mark.parametrize("case", list(nr.CASES))
def test_a_volume_does_not_depend_on_the_launch(case, emu):
    """Pair 1 of the batch of 3: alone, and with a workspace capped to one volume (three groups), bit for bit."""
    h = _handle(emu, case)
    x, _ = nr.expected(case, "big")
    full = nr.emu_consensus(emu, h, x)
    alone = nr.emu_consensus(emu, h, x[1:2])
    chunked = nr.emu_consensus(emu, h, x, ws_volumes=1)
    assert torch.equal(alone[0], full[1]) and torch.equal(chunked, full)
    per = emu.p2p_neigh_consensus_workspace_bytes(h, *x.shape[1:])
    assert per >= 256 and per % 256 == 0
    nr.emu_consensus(emu, h, x, ws_bytes=per - 256, expect_status=-4)          # below one volume: P2P_ENOMEM


def test_one_branch_is_the_direct_branch(emu):
    """Case M (symmetric_mode=False) equals the direct addend of the same weights run symmetric, and the fp64 direct branch."""
    x, y64 = nr.expected("M", "big")
    assert torch.equal(y64, nr.restate(x, nr.weights("M"), nr.CASES["M"], branch="direct"))
    one = nr.emu_consensus(emu, _handle(emu, "M"), x)
    both = nr.emu_consensus(emu, _handle(emu, "M", dict(nr.CASES["M"], symmetric_mode=True)), x)
    t64 = nr.restate(x, nr.weights("M"), nr.CASES["M"], branch="transposed")
    assert not torch.equal(one, both)
    scale = (y64 + t64).abs().max().item()
    assert ((both.double() - (y64 + t64)).abs().max().item()) <= nr.BAR_F64 * nr.REF_ERR["M"] * scale
    # the transposed addend is added to the stored direct one in fp32: both - one is it up to one rounding of the sum
    assert ((both - one).double() - t64).abs().max().item() <= nr.BAR_F64 * nr.REF_ERR["M"] * scale + 2.0 ** -24 * scale


def test_generic_handles_in_the_other_entry_points(emu):
    h = _handle(emu, "N")
    assert emu.p2p_ncn_set_tile(h, 0, 5, 8) == -3
    tuned = emu_lib.ncn_create(emu, {"ncn." + k: v for k, v in nr.weights("R").items()})
    assert emu.p2p_ncn_is_generic(tuned) == 0
    assert emu.p2p_neigh_consensus_workspace_bytes(tuned, 6, 7, 5, 8) == 4
    assert emu.p2p_coarse_workspace_bytes_for(tuned, 32, 6, 8, 8, 6, 1) == emu.p2p_coarse_workspace_bytes(32, 6, 8, 8, 6, 1)
    assert emu.p2p_coarse_workspace_bytes_for(h, 32, 6, 8, 8, 6, 1) > emu.p2p_coarse_workspace_bytes(32, 6, 8, 8, 6, 1)
    assert emu.p2p_coarse_workspace_bytes_for(h, 32, 0, 8, 8, 6, 1) == 0 and emu.p2p_neigh_consensus_workspace_bytes(h, 6, 7, 0, 8) == 0
    emu.p2p_ncn_destroy(tuned)


def _coarse(emu, ncn, fa, fb, ksize, ws_pairs=None):
    """emu_lib.coarse_forward_batch with the workspace sized for the handle."""
    nb, c, ha, wa = fa.shape
    hb, wb = fb.shape[2:]
    k = max(ksize, 1)
    shape = (nb, ha // k, wa // k, hb // k, wb // k)
    corr = torch.empty(shape)
    delta = torch.empty(shape, dtype=torch.uint8) if ksize > 1 else None
    per = emu.p2p_coarse_workspace_bytes_for(ncn, c, ha, wa, hb, wb, ksize)
    n = (ws_pairs or nb) * per
    ws = torch.empty(n + 256, dtype=torch.uint8)
    st = emu.p2p_coarse_forward_batch(emu_lib.ptr(fa), emu_lib.ptr(fb), nb, c, ha, wa, hb, wb, ksize, ncn, emu_lib.ptr(corr),
                                      emu_lib.ptr(delta), ctypes.c_void_p((ws.data_ptr() + 255) & ~255), n, None)
    assert st == 0, emu.p2p_last_error()
    return corr, delta


@pytest.mark.parametrize("ksize,sides", [(1, (6, 8, 8, 6)), (2, (12, 16, 16, 12))])
def test_released_stack_generic_beside_tuned_in_the_coarse_stage(ksize, sides, emu):
    """Case R inside forward_coarse_match (32-channel features: the correlation kernel takes multiples of 32): the generic and
    the tuned handle agree within the sum of both bars, and extract the same match rows wherever the fp64 pipeline's
    top-two gap exceeds twice the bar; the rows left out stay under the cap."""
    sd, lay = nr.weights("R"), nr.CASES["R"]
    fa, fb = nr.features(nr.COARSE_SEEDS[ksize], (2,) + sides, channels=32, shift=nr.COARSE_SHIFT)
    gen = _handle(emu, "R")
    tuned = emu_lib.ncn_create(emu, {"ncn." + k: v for k, v in sd.items()})
    cg, dg = _coarse(emu, gen, fa, fb, ksize)
    ct, dt = _coarse(emu, tuned, fa, fb, ksize)
    c1, _ = _coarse(emu, gen, fa, fb, ksize, ws_pairs=1)                     # two groups of one pair
    assert torch.equal(c1, cg)
    assert dg is None or torch.equal(dg, dt)
    up = 8
    mg, _ = emu_lib.coarse_matches_batch(emu, cg, dg, ksize, up)
    mt, _ = emu_lib.coarse_matches_batch(emu, ct, dt, ksize, up)
    left_out = total = 0
    for b in range(2):
        corr64, y64, _ = nr.pipeline(fa[b], fb[b], ksize, sd, lay)
        both = nr.handles_bar("R", y64)
        diff = (cg[b] - ct[b]).abs().max().item()
        print(f"ksize {ksize} pair {b}: generic - tuned {diff:.3g}, sum of bars {both:.3g}; generic - fp64 "
              f"{(cg[b].double() - corr64).abs().max().item():.3g}, tuned - fp64 {(ct[b].double() - corr64).abs().max().item():.3g}")
        assert diff <= both
        ok = nr.decidable(corr64, nr.coarse_bar("R", y64))
        assert torch.equal(mg[b][ok], mt[b][ok])
        # the fp32 restatement alone decides the same rows as the fp64 one (how the seed was chosen)
        c32 = nr.pipeline(fa[b], fb[b], ksize, sd, lay, torch.float32)[0]
        assert torch.equal(nr.best_cells(c32)[0][ok], nr.best_cells(corr64)[0][ok])
        left_out += int((~ok).sum())
        total += ok.numel()
    print(f"ksize {ksize}: {left_out} of {total} rows undecidable")
    assert left_out <= nr.UNDECIDED_CAP * total
    emu.p2p_ncn_destroy(tuned)
