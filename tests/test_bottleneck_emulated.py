"""Every distinct convolution of a Bottleneck block up to layer3 (64 ... 1024 channels, 1x1 and 3x3, stride 1 and 2) on the CPU
build of csrc/backbone.hip (tests/hipemu), in its role (ReLU / skip + ReLU / neither) and in both modes, against the fp64
evaluation; shapes, inputs and bars in tests/bottleneck_reference.py.  The MI355X runs the same layers inside the pyramids of
tests/test_gpu_bottleneck.py."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import backbone_mode_reference as bm  # noqa: E402
import bottleneck_reference as br  # noqa: E402


@functools.lru_cache(maxsize=None)
def _emu():
    return bm.bind(emu_lib.load())


@pytest.mark.parametrize("mode", ["fp16x2", "fp16"])
@pytest.mark.parametrize("name", list(br.LAYERS))
def test_bottleneck_convolution(name, mode):
    wt, bn, x, sk = br.layer_inputs(name)
    _, _, _, stride, _, relu = br.LAYERS[name]
    got, gmax = bm.emu_conv(_emu(), wt, bn, stride, x, sk, relu, modes=(mode,) if mode != "fp16x2" else ())
    br.check_layer(got, name, mode, "emulated ")
    assert torch.equal(gmax, got.abs().amax(dim=(1, 2, 3)))          # what the next layer scales its operands by


@pytest.mark.parametrize("name", ["l3_conv3_256_1024", "l3_conv1_1024_256", "l2_down_256_512_s2"])
def test_role_does_not_change_the_sums(name):
    """The same layer without its skip / ReLU: the epilogue options apply to one and the same accumulator (relu(y + skip) of the
    plain output, bit for bit where no rounding intervenes: without a skip)."""
    wt, bn, x, sk = br.layer_inputs(name)
    _, _, _, stride, _, relu = br.LAYERS[name]
    plain, _ = bm.emu_conv(_emu(), wt, bn, stride, x, None, False)
    with_relu, _ = bm.emu_conv(_emu(), wt, bn, stride, x, None, True)
    assert torch.equal(with_relu, plain.relu())
    ref = bm.yardstick(x, wt, bn, stride, None, False)
    bound = bm.layer_bound(x.double().abs(), wt, bn, stride, "fp16x2")
    assert bool(((plain.double() - ref).abs() <= bound).all())


def test_every_tile_gives_the_same_bits_at_1024_channels():
    name = "l3_conv3_256_1024"
    wt, bn, x, sk = br.layer_inputs(name)
    base, _ = bm.emu_conv(_emu(), wt, bn, 1, x, sk, True)
    for tile in bm.tiles_of(1024):
        got, _ = bm.emu_conv(_emu(), wt, bn, 1, x, sk, True, tile=tile)
        assert torch.equal(got, base), tile
