"""Backbone mode 'fp16' (P2P_CONV_FP16), host side: the ABI (constants, symbols, version, refusal of an unknown mode), the
Python names (set_mode strings, P2P_BACKBONE_MODE) and the module-level choice surviving a re-pack.  No GPU: the C entry
points are reached through the CPU build of tests/hipemu, the packing through stand-ins for ops.ConvBN / ops.Stem."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import backbone_mode_reference as bm  # noqa: E402
from patch2pix_amd import _lib as real  # noqa: E402
from patch2pix_amd import ops  # noqa: E402

NEW_SYMBOLS = ["p2p_conv_set_mode", "p2p_conv_get_mode", "p2p_stem_set_mode", "p2p_stem_get_mode"]


@pytest.fixture(scope="module")
def emu():
    return bm.bind(emu_lib.load())


def test_version_symbols_and_constants():
    assert real.p2p_version() & ~real.VERSION_EXPERIMENT == 112
    header = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in real.EXPORTS and hasattr(real.lib, name), name
        assert re.search(rf"\bint {name}\(", header), name
    assert re.search(r"#define\s+P2P_CONV_FP16X2\s+0\b", header) and re.search(r"#define\s+P2P_CONV_FP16\s+1\b", header)
    assert real.BACKBONE_MODES == {"fp16x2": 0, "fp16": 1} == bm.MODE_IDS


def test_mode_names_and_environment(monkeypatch):
    assert ops.backbone_mode_id("fp16x2") == 0 and ops.backbone_mode_id("fp16") == 1
    for bad in ("fp32", "FP16", "", None, 1):
        with pytest.raises(ValueError):
            ops.backbone_mode_id(bad)
    monkeypatch.delenv("P2P_BACKBONE_MODE", raising=False)
    assert ops.default_backbone_mode() == "fp16x2"
    monkeypatch.setenv("P2P_BACKBONE_MODE", "fp16")
    assert ops.default_backbone_mode() == "fp16"
    monkeypatch.setenv("P2P_BACKBONE_MODE", "half")          # an unknown name fails where a handle would take it
    with pytest.raises(ValueError):
        ops.backbone_mode_id(ops.default_backbone_mode())
    for cls in (ops.ConvBN, ops.Stem):
        assert callable(cls.set_mode) and isinstance(cls.mode, property)


def test_c_setters_refuse_an_unknown_mode(emu):
    wt, bn, _, _ = bm.case_inputs(("l1_3x3", (8, 16)))
    keep = [wt.contiguous()] + [t.contiguous() for t in bn]
    b = real.BnParams(*[t.data_ptr() for t in keep[1:]])
    h = ctypes.c_void_p()
    assert emu.p2p_conv_create(emu_lib.ptr(keep[0]), ctypes.byref(b), 64, 64, 3, 1, ctypes.byref(h)) == 0
    try:
        assert emu.p2p_conv_get_mode(h) == 0                                 # P2P_CONV_FP16X2 is where a handle starts
        for bad in (2, -1, 5):
            assert emu.p2p_conv_set_mode(h, bad) == -1 and b"unknown mode" in emu.p2p_last_error()      # P2P_EINVAL
            assert emu.p2p_conv_get_mode(h) == 0
        assert emu.p2p_conv_set_mode(h, 1) == 0 and emu.p2p_conv_get_mode(h) == 1
        assert emu.p2p_conv_set_tile(h, 1, 2, 1) == 0 and emu.p2p_conv_get_mode(h) == 1        # the tile setter leaves the mode
        assert emu.p2p_conv_set_mode(h, 0) == 0 and emu.p2p_conv_get_mode(h) == 0
        assert emu.p2p_conv_set_mode(None, 1) == -1
    finally:
        emu.p2p_conv_destroy(h)
    swt, sbn, _ = bm.stem_inputs()
    keep = [swt.contiguous()] + [t.contiguous() for t in sbn]
    b = real.BnParams(*[t.data_ptr() for t in keep[1:]])
    s = ctypes.c_void_p()
    assert emu.p2p_stem_create(emu_lib.ptr(keep[0]), ctypes.byref(b), ctypes.byref(s)) == 0
    try:
        assert emu.p2p_stem_get_mode(s) == 0
        assert emu.p2p_stem_set_mode(s, 2) == -1 and emu.p2p_stem_get_mode(s) == 0
        assert emu.p2p_stem_set_mode(s, 1) == 0 and emu.p2p_stem_get_mode(s) == 1
    finally:
        emu.p2p_stem_destroy(s)


class _FakeLayer:
    """What networks/resnet.py needs of ops.ConvBN / ops.Stem to pack: a constructor and set_mode."""
    made = []

    def __init__(self, *args):
        self.mode = "fp16x2"
        _FakeLayer.made.append(self)

    def set_mode(self, mode):
        ops.backbone_mode_id(mode)
        self.mode = mode


def test_module_mode_survives_a_repack(monkeypatch):
    from patch2pix_amd.networks import resnet
    monkeypatch.setattr(ops, "ConvBN", _FakeLayer)
    monkeypatch.setattr(ops, "Stem", _FakeLayer)
    monkeypatch.delenv("P2P_BACKBONE_MODE", raising=False)
    _FakeLayer.made = []
    net = resnet.ResNet34()
    net.change_stride("layer3")
    assert net.mode == "fp16x2"
    with pytest.raises(ValueError):
        net.set_mode("fp32")
    assert net.mode == "fp16x2"
    net.set_mode("fp16")                                     # before anything is packed: remembered
    assert net.mode == "fp16" and not _FakeLayer.made
    stem, trunk = net._hip_trunk("cuda:0")
    first = list(_FakeLayer.made)
    blocks = [blk for name in ("layer1", "layer2", "layer3") for blk in getattr(net, name)]
    assert len(first) == 1 + sum(2 + (blk.downsample is not None) for blk in blocks)         # the stem and every convolution
    assert all(l.mode == "fp16" for l in first)
    net.load_state_dict(net.state_dict())                    # moves the version counters: everything is packed again
    net._hip_trunk("cuda:0")
    second = _FakeLayer.made[len(first):]
    assert len(second) == len(first) and all(l.mode == "fp16" for l in second)
    net.set_mode("fp16x2")                                   # on packed layers: applied at once, no re-pack
    assert all(l.mode == "fp16x2" for l in second) and len(_FakeLayer.made) == 2 * len(first)
    import copy
    net.set_mode("fp16")
    assert copy.deepcopy(net).mode == "fp16"                 # the choice belongs to the module, the packed cache does not
    # the torch path never looks at it: a CPU tensor takes it whatever the mode
    with torch.no_grad():
        feats = net.eval().pyramid(torch.zeros(1, 3, 32, 32))
    assert len(feats) == 5 and len(_FakeLayer.made) == 2 * len(first)
