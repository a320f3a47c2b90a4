"""P2P_COARSE_GENERIC_FP16X2 (csrc/consensus_generic_h2.hip) through the kernel emulator: the setter matrix on tuned and generic
handles, every case x volume against the fp64 restatement and the reference's fp32 outputs per pair, bit-identity of the
single-layer case in both modes and of the default mode after a round trip, the two modes against each other, invariance under
batching and workspace size, the mixed-magnitude batch, an all-zero pair, a pair holding an inf, the range variants and the
workspace bound.  Bars: tests/ncn_mode_reference.py.  No GPU."""
import os
import sys

import pytest
import torch

import ncn_mode_reference as nm
import ncn_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
import emu_lib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


_handles = {}


def _handle(emu, case, mode, variant=None):
    """One handle per (case, variant), switched to `mode` (switching back and forth is part of what is tested)."""
    key = (case, variant)
    if key not in _handles:
        _handles[key] = nm.create(emu, case, variant)
    assert emu.p2p_ncn_set_mode(_handles[key], mode) == nm.OK, emu.p2p_last_error()
    return _handles[key]


def test_setter_matrix(emu):
    tuned = emu_lib.ncn_create(emu, {"ncn." + k: v for k, v in nr.weights("R").items()})
    gen = nm.create(emu, "N")
    assert emu.p2p_ncn_get_mode(None) == -1 and emu.p2p_ncn_set_mode(None, 17) == nm.EINVAL
    assert emu.p2p_ncn_get_mode(tuned) == 0 and emu.p2p_ncn_get_mode(gen) == 0
    for bad in (-1, 2, 5, 7, 16, 18):
        for h in (tuned, gen):
            assert emu.p2p_ncn_set_mode(h, bad) == nm.EINVAL and emu.p2p_ncn_get_mode(h) == 0, bad
    assert emu.p2p_ncn_set_mode(tuned, 17) == nm.EUNSUPPORTED and emu.p2p_ncn_get_mode(tuned) == 0
    assert emu.p2p_ncn_set_mode(tuned, 1) == nm.OK and emu.p2p_ncn_set_mode(tuned, 17) == nm.EUNSUPPORTED and emu.p2p_ncn_get_mode(tuned) == 1
    assert emu.p2p_ncn_set_mode(gen, 1) == nm.EUNSUPPORTED and emu.p2p_ncn_get_mode(gen) == 0
    for mode in (17, 17, 0, 17):
        assert emu.p2p_ncn_set_mode(gen, mode) == nm.OK and emu.p2p_ncn_get_mode(gen) == mode
    assert emu.p2p_ncn_set_mode(gen, 1) == nm.EUNSUPPORTED and emu.p2p_ncn_get_mode(gen) == 17
    assert emu.p2p_ncn_set_tile(gen, 0, 5, 8) == nm.EUNSUPPORTED
    emu.p2p_ncn_destroy(tuned)
    emu.p2p_ncn_destroy(gen)


@pytest.mark.parametrize("vol", list(nm.VOLUMES))
@pytest.mark.parametrize("case", list(nr.CASES))
def test_cases_against_fp64_and_golden(case, vol, emu):
    x, y64 = nm.expected(case, vol)
    y = nr.emu_consensus(emu, _handle(emu, case, 17), x)
    nm.check_pairs(y, y64, case, vol, "emulated fp16x2")
    g = torch.from_numpy(nm.load_golden(case)[f"y_{vol}"] if vol == nm.TILE else nr.load_golden(case)[f"y_{vol}"])
    nm.check_pairs(y, y64, case, vol, "emulated fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=g)


@pytest.mark.parametrize("vol", ["big", nm.TILE])
def test_single_layer_stack_is_bit_equal_in_both_modes(vol, emu):
    x = nm.expected("S", vol)[0]
    assert torch.equal(nr.emu_consensus(emu, _handle(emu, "S", 0), x), nr.emu_consensus(emu, _handle(emu, "S", 17), x))
    h = _handle(emu, "S", 17)
    assert emu.p2p_neigh_consensus_workspace_bytes(h, *x.shape[1:]) == emu.p2p_neigh_consensus_workspace_bytes(_handle(emu, "S", 0), *x.shape[1:])


@pytest.mark.parametrize("case", ["N", "M"])
def test_modes_differ_within_the_bar_and_the_default_returns(case, emu):
    """The default's bits before and after a stay in mode 17 are the same (and those of a handle that never left it); the two modes
    differ in their bits and by at most nr.handles_bar per pair."""
    x, y64 = nm.expected(case, nm.TILE)
    fresh = nm.create(emu, case)
    never = nr.emu_consensus(emu, fresh, x)
    emu.p2p_ncn_destroy(fresh)
    before = nr.emu_consensus(emu, _handle(emu, case, 0), x)
    h2 = nr.emu_consensus(emu, _handle(emu, case, 17), x)
    after = nr.emu_consensus(emu, _handle(emu, case, 0), x)
    assert torch.equal(before, after) and torch.equal(before, never)
    assert not torch.equal(before, h2)
    for z, bar in enumerate(nm.handles_bar_pairs(case, y64)):
        diff = (before[z] - h2[z]).abs().max().item()
        print(f"case {case} pair {z}: generic - generic_fp16x2 {diff:.3g}, bar {bar:.3g}")
        assert diff <= bar


@pytest.mark.parametrize("case", ["R", "M"])
def test_a_pair_does_not_depend_on_the_launch(case, emu):
    h = _handle(emu, case, 17)
    x = nm.expected(case, "big")[0]
    full = nr.emu_consensus(emu, h, x)
    alone = nr.emu_consensus(emu, h, x[1:2].contiguous())
    chunked = nr.emu_consensus(emu, h, x, ws_volumes=1)
    moved = nr.emu_consensus(emu, h, torch.stack([x[1], x[0]]))
    assert torch.equal(alone[0], full[1]) and torch.equal(chunked, full) and torch.equal(moved[0], full[1]) and torch.equal(moved[1], full[0])


@pytest.mark.parametrize("case", ["R", "M"])
def test_mixed_magnitude_batch(case, emu):
    x, y64 = nm.mixed(case)
    y = nr.emu_consensus(emu, _handle(emu, case, 17), x)
    nm.check_pairs(y, y64, case, "mixed", "emulated fp16x2")
    nm.check_pairs(y, y64, case, "mixed", "emulated fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=torch.from_numpy(nm.load_golden(case)["y_mixed"]))


def test_zero_and_inf_pairs(emu):
    """An all-zero pair gives the finite bias / ReLU chain of the fp64 restatement.  A pair holding an inf leaves the other pairs'
    bits untouched; inside its own pair the inf scales the pair by 2^-116 and splits into inf - inf: every cell the inf reaches
    through the taps of the layers behind the first is NaN or inf, and what the last ReLU does with a NaN is its own (fmaxf
    returns the other operand: 0) -- nothing is asserted about that pair beyond the call returning."""
    case = "N"
    h = _handle(emu, case, 17)
    x = nm.expected(case, "big")[0].clone()
    base = nr.emu_consensus(emu, h, x)
    x[1] = 0.0
    y = nr.emu_consensus(emu, h, x)
    y64 = nr.restate(x, nr.weights(case), nr.CASES[case])
    assert torch.isfinite(y).all() and torch.equal(y[0], base[0]) and torch.equal(y[2], base[2])
    assert (y[1].double() - y64[1]).abs().max().item() <= nr.BAR_F64 * nr.REF_ERR[case] * max(y64[1].abs().max().item(), 1e-30)
    x[1, 2, 3, 1, 4] = float("inf")
    y = nr.emu_consensus(emu, h, x)
    assert torch.equal(y[0], base[0]) and torch.equal(y[2], base[2])


@pytest.mark.parametrize("variant", nm.VARIANTS)
@pytest.mark.parametrize("case", ["R", "M"])
def test_range_variants(case, variant, emu):
    x, y64 = nm.expected(case, nm.TILE, variant)
    key = nm.input_key(nm.TILE, variant)
    if variant == "outlier":
        assert int(nm.load_golden(case)["outlier_channel"]) == nm.outlier_channel(case)
    y = nr.emu_consensus(emu, _handle(emu, case, 17, variant), x)
    nm.check_pairs(y, y64, case, key, "emulated fp16x2")
    nm.check_pairs(y, y64, case, key, "emulated fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=torch.from_numpy(nm.load_golden(case)[f"y_{key}"]))


def test_workspace_follows_the_mode(emu):
    case = "N"
    x = nm.expected(case, "thin")[0]
    h = _handle(emu, case, 0)
    exact = emu.p2p_neigh_consensus_workspace_bytes(h, *x.shape[1:])
    cexact = emu.p2p_coarse_workspace_bytes_for(h, 32, 4, 6, 4, 6, 2)
    h = _handle(emu, case, 17)
    need = emu.p2p_neigh_consensus_workspace_bytes(h, *x.shape[1:])
    assert need > exact and emu.p2p_coarse_workspace_bytes_for(h, 32, 4, 6, 4, 6, 2) == cexact + (need - exact)
    nr.emu_consensus(emu, h, x, ws_bytes=exact, expect_status=nm.ENOMEM)       # the default's size is below the mode's
    nr.emu_consensus(emu, h, x, ws_bytes=need - 1, expect_status=nm.ENOMEM)
    assert torch.isfinite(nr.emu_consensus(emu, h, x, ws_bytes=need)).all()
    h = _handle(emu, case, 0)
    assert emu.p2p_neigh_consensus_workspace_bytes(h, *x.shape[1:]) == exact
