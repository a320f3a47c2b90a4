"""Coarse mode 'fp16' (P2P_COARSE_FP16) on the CPU build of the kernels (tests/hipemu): the element-wise stage bounds of
tests/coarse_mode_reference.py in both modes, the index assertions on the decidable rows, and bit equality across tiles, batch
mates, workspace sizes and mode round trips.  tests/test_gpu_coarse_mode.py asserts the same through the real library on the
MI355X."""
import ctypes
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import golden_util as gu  # noqa: E402
import coarse_mode_reference as cm  # noqa: E402

TILE_CASE = "c32_12x16_k1_tiles"
BATCH_CASE = "c32_8x8_k2_batch3"


@functools.lru_cache(maxsize=None)
def _emu():
    return cm.bind(emu_lib.load())


def _sd():
    return gu.state_dict(0)


@functools.lru_cache(maxsize=None)
def _run(name, modes=(), tile=None, pair=None, ws_pairs=None):
    """One emulated coarse stage of a case on a fresh handle: p2p_ncn_set_mode for every entry of `modes` in turn (none: the
    handle never sees the setter); cached, so every variant runs once for all the tests that look at it."""
    emu = _emu()
    fa, fb = cm.case_inputs(name)
    if pair is not None:
        fa, fb = fa[pair:pair + 1], fb[pair:pair + 1]
    ncn = cm.ncn_create(emu, _sd())
    try:
        assert emu.p2p_ncn_get_mode(ncn) == 0
        for m in modes:
            cm.set_mode(emu, ncn, m)
        if tile:
            emu_lib.check(emu, emu.p2p_ncn_set_tile(ncn, *tile), "p2p_ncn_set_tile")
        out = cm.run_coarse(emu, ncn, fa, fb, cm.CASES[name][3], ws_pairs=ws_pairs)
        out["rows"], out["scores"] = cm.run_matches(emu, out["corr"], out["delta"], cm.CASES[name][3])
    finally:
        emu.p2p_ncn_destroy(ncn)
    return out


@pytest.mark.parametrize("name", cm.EMU_CASES)
def test_stage_bounds_in_both_modes(name):
    """Every stage output within its bound element-wise in mode 'fp16'; the default mode inside its own, much smaller bound on
    the same inputs; the two outputs differ (the switch does something)."""
    share = cm.assert_decidable_share(name, _sd())
    fast, default = _run(name, ("fp16",)), _run(name)
    rf = cm.check_stages(fast, name, _sd(), "fp16", "emulated ")
    rd = cm.check_stages(default, name, _sd(), "fp16x2", "emulated ")
    print(f"emulated {name}: decidable share {share:.3f}; measured / bound fp16 {rf}, fp16x2 {rd}")
    assert not torch.equal(fast["corr"], default["corr"]), "mode 'fp16' gave the default mode's bits"
    assert not torch.equal(fast["x"], default["x"]) and not torch.equal(fast["y"], default["y"])


@pytest.mark.parametrize("name", cm.EMU_CASES)
def test_decidable_rows_name_the_fp64_winner(name):
    """Every decidable row of cal_coarse_matches equals the fp64 winner in both modes; rows on which the modes differ are
    undecidable under the 'fp16' bound."""
    fast, default = _run(name, ("fp16",)), _run(name)
    bad_f, dec_f, tot = cm.check_rows(fast["rows"], name, _sd(), "fp16")
    bad_d, dec_d, _ = cm.check_rows(default["rows"], name, _sd(), "fp16x2")
    print(f"emulated {name}: {dec_f} / {tot} rows decidable in fp16 ({bad_f} differ from fp64), {dec_d} in fp16x2 ({bad_d} differ)")
    dec = torch.cat([y.decidable()[1] for y in cm.yardsticks(name, _sd(), "fp16")]).view(fast["rows"].shape[0], -1)
    differ = (fast["rows"] != default["rows"]).any(dim=-1)
    assert not bool((differ & dec).any()), "the modes differ on a row that is decidable under the fp16 bound"


def test_tile_independence_inside_the_mode():
    base = _run(TILE_CASE, ("fp16",))
    for tile in ((2, 3, 2), (4, 6, 6), (0, 2, 5), (3, 4, 3), (12, 10, 8), (1, 5, 8)):
        got = _run(TILE_CASE, ("fp16",), tile)
        assert torch.equal(got["corr"], base["corr"]) and torch.equal(got["y"], base["y"]), f"tile {tile} changes the volume"


def test_batch_and_workspace_independence_inside_the_mode():
    batch = _run(BATCH_CASE, ("fp16",))
    small = _run(BATCH_CASE, ("fp16",), None, None, 1)                 # the workspace holds one pair at a time
    assert torch.equal(small["corr"], batch["corr"]) and torch.equal(small["delta"], batch["delta"])
    for z in range(3):
        one = _run(BATCH_CASE, ("fp16",), None, z)
        assert torch.equal(one["corr"][0], batch["corr"][z]) and torch.equal(one["delta"][0], batch["delta"][z]), f"pair {z}"
        assert torch.equal(one["x"][0], batch["x"][z]) and torch.equal(one["y"][0], batch["y"][z])


@pytest.mark.parametrize("name", ["c64_12x16_k2", BATCH_CASE])
def test_mode_round_trip_gives_the_first_bits(name):
    """fp16x2 -> fp16 -> fp16x2 on one handle: the bits of a handle that never saw the setter (nothing is re-packed)."""
    never, back = _run(name), _run(name, ("fp16x2", "fp16", "fp16x2"))
    for key in ("corr", "delta", "x", "y", "rows", "scores"):
        assert torch.equal(never[key], back[key]), key


@pytest.mark.parametrize("name", ["c32_6x8_k1", TILE_CASE])
def test_consensus_entry_point_equals_the_stage_leg(name):
    """p2p_neigh_consensus_batch on the stage's own input volume gives the consensus leg of the whole-stage run, in both modes."""
    emu = _emu()
    for modes in ((), ("fp16",)):
        stage = _run(name, modes)
        ncn = cm.ncn_create(emu, _sd())
        try:
            for m in modes:
                cm.set_mode(emu, ncn, m)
            y = cm.run_consensus(emu, ncn, stage["x"])
        finally:
            emu.p2p_ncn_destroy(ncn)
        assert torch.equal(y, stage["y"]), modes
    assert not torch.equal(_run(name)["y"], _run(name, ("fp16",))["y"])


def test_setter_errors():
    emu = _emu()
    ncn = cm.ncn_create(emu, _sd())
    try:
        for bad in (-1, 2, 7):
            assert emu.p2p_ncn_set_mode(ncn, bad) == -1 and b"mode" in emu.p2p_last_error()
            assert emu.p2p_ncn_get_mode(ncn) == 0
        assert emu.p2p_ncn_set_mode(None, 1) == -1 and emu.p2p_ncn_get_mode(None) == -1
    finally:
        emu.p2p_ncn_destroy(ncn)
