"""Backbone mode 'fp16' (P2P_CONV_FP16) on the CPU build of the kernels (tests/hipemu): the element-wise error bounds of
tests/backbone_mode_reference.py in both modes and both directions, and bit equality across tiles, batch mates and mode
round trips.  tests/test_gpu_backbone_mode.py asserts the same through the real library on the MI355X."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import backbone_mode_reference as bm  # noqa: E402


@functools.lru_cache(maxsize=None)
def _emu():
    return bm.bind(emu_lib.load())


@functools.lru_cache(maxsize=None)
def _run(case, modes=(), tile=None, first_image_only=False):
    """One emulated launch of a case; cached, so every (case, modes, tile) runs once for all the tests that look at it."""
    wt, bn, x, sk = bm.case_inputs(case)
    _, _, _, stride, _, relu = bm.LAYERS[case[0]]
    if first_image_only:
        x, sk = x[:1].contiguous(), None if sk is None else sk[:1].contiguous()
    return bm.emu_conv(_emu(), wt, bn, stride, x, sk, relu, modes, tile)


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_error_bounds_in_both_modes(case):
    """|out - fp64| <= bound element-wise in mode 'fp16'; (a) the default mode stays inside its own, much smaller bound on the
    same inputs; (b) the two outputs differ (the switch does something)."""
    fast, _ = _run(case, ("fp16",))
    default, _ = _run(case)
    bm.check_layer(fast, case, "fp16", "emulated ")
    bm.check_layer(default, case, "fp16x2", "emulated ")
    assert not torch.equal(fast, default), "mode 'fp16' gave the default mode's bits"


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_tile_independence_inside_the_mode(case):
    fast, fmax = _run(case, ("fp16",))
    for tile in bm.tiles_of(bm.LAYERS[case[0]][1]):
        got, gmax = _run(case, ("fp16",), tile)
        assert torch.equal(got, fast) and torch.equal(gmax, fmax), f"tile {tile}"
    assert torch.equal(fmax, fast.abs().amax(dim=(1, 2, 3)))          # what the next layer scales its operands by


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_batch_independence_inside_the_mode(case):
    fast, fmax = _run(case, ("fp16",))
    one, omax = _run(case, ("fp16",), None, True)
    assert torch.equal(one[0], fast[0]) and torch.equal(omax[0], fmax[0])


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_default_mode_untouched(case):
    """A handle whose mode was never set, one set to 'fp16x2' and one switched 'fp16' -> 'fp16x2': the same bits."""
    never, nmax = _run(case)
    for modes in (("fp16x2",), ("fp16", "fp16x2")):
        got, gmax = _run(case, modes)
        assert torch.equal(got, never) and torch.equal(gmax, nmax), modes


def test_stem_bounds_and_round_trip():
    emu = _emu()
    wt, bn, image = bm.stem_inputs()
    never = bm.emu_stem(emu, wt, bn, image)
    fast = bm.emu_stem(emu, wt, bn, image, "fp16")
    bm.check_stem(fast, "fp16", "emulated ")
    bm.check_stem(never, "fp16x2", "emulated ")
    assert not torch.equal(fast, never)
    assert torch.equal(bm.emu_stem(emu, wt, bn, image, "fp16x2"), never)
    one = bm.emu_stem(emu, wt, bn, image[:1].contiguous(), "fp16")
    assert torch.equal(one[0], fast[0])


def test_bound_can_fail():
    """The bound is no formality: the default mode's bound rejects the 'fp16' output of the same case, and the 'fp16' bound
    rejects an output that is off by 2^-4 of its value."""
    case = ("l1_3x3_relu", (10, 18))
    fast, _ = _run(case, ("fp16",))
    with pytest.raises(AssertionError):
        bm.check_layer(fast, case, "fp16x2")
    with pytest.raises(AssertionError):
        bm.check_layer(fast * (1 + 2.0 ** -4), case, "fp16")
