"""Coarse mode 'fp16' (P2P_COARSE_FP16), host side: the ABI (constants, symbols), the Python names (set_mode strings,
P2P_COARSE_MODE), the refusal of generic handles, and the bound functions of tests/coarse_mode_reference.py against a brute-force
fp64 evaluation of single-rounded operands.  No GPU."""
import os
import re

import pytest
import torch

import coarse_mode_reference as cm
from oracle import p2p_oracle as orc
from patch2pix_amd import _lib as real
from patch2pix_amd import ops
from patch2pix_amd.networks import patch2pix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_constants():
    header = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    for name in ("p2p_ncn_set_mode", "p2p_ncn_get_mode"):
        assert name in real.EXPORTS and hasattr(real.lib, name), name
        assert re.search(rf"\bint {name}\(", header), name
    ids = {k: int(re.search(rf"#define\s+P2P_COARSE_{k.upper()}\s+(\d+)\b", header).group(1)) for k in ("fp16x2", "fp16")}
    assert ids == real.COARSE_MODES == cm.MODE_IDS == {"fp16x2": 0, "fp16": 1}
    assert real.p2p_ncn_set_mode(None, 1) == -1 and real.p2p_ncn_get_mode(None) == -1      # NULL: no device needed


def test_mode_names_and_environment(monkeypatch):
    assert ops.coarse_mode_id("fp16x2") == 0 and ops.coarse_mode_id("fp16") == 1
    for bad in ("fp32", "FP16", "", None, 1):
        with pytest.raises(ValueError):
            ops.coarse_mode_id(bad)
    monkeypatch.delenv("P2P_COARSE_MODE", raising=False)
    assert ops.default_coarse_mode() == "fp16x2"
    monkeypatch.setenv("P2P_COARSE_MODE", "fp16")
    assert ops.default_coarse_mode() == "fp16"
    monkeypatch.setenv("P2P_COARSE_MODE", "half")             # an unknown name fails where a handle would take it
    with pytest.raises(ValueError):
        ops.coarse_mode_id(ops.default_coarse_mode())
    assert callable(ops.NcnWeights.set_mode) and isinstance(ops.NcnWeights.mode, property)
    assert callable(patch2pix.Patch2Pix.set_coarse_mode) and isinstance(patch2pix.Patch2Pix.coarse_mode, property)


def test_generic_handles_refuse_the_mode():
    """NcnWeights.set_mode on a generic handle raises before the library is asked; a wrong name is a ValueError first."""
    w = ops.NcnWeights.__new__(ops.NcnWeights)
    w.handle, w.generic = None, True
    w.layout = ops.ncn_layout(dict(kernel_sizes=[3, 3, 3], channels=[10, 10, 1]))
    assert w.layout != ops.RELEASED_NCN_LAYOUT
    with pytest.raises(NotImplementedError):
        w.set_mode("fp16")
    with pytest.raises(ValueError):
        w.set_mode("half")


def _round_fp16(t, scale):
    return (t * scale).to(torch.float16).double() / scale


def test_correlation_bound_against_single_rounded_operands():
    """corr_bound (no normalisation error: enorm = 0) covers the exact fp64 correlation of operands rounded once to fp16 under
    2^12, subnormal operands and exact zeros included."""
    gen = torch.Generator().manual_seed(5)
    for tiny in (1.0, 2.0 ** -20):
        na = torch.randn(32, 3, 4, generator=gen, dtype=torch.float64) * 0.2 * tiny
        nb = torch.randn(32, 2, 5, generator=gen, dtype=torch.float64) * 0.2
        na[:, 0, 1] = 0.0
        got = orc.correlation(_round_fp16(na, 4096.0), _round_fp16(nb, 4096.0))
        err = (got - orc.correlation(na, nb)).abs()
        bound = cm.corr_bound(na.abs(), nb.abs(), "fp16", enorm=0.0)
        assert bool((err <= bound).all()) and float(err.max()) > 0
        assert float((err / bound.clamp_min(1e-300)).max()) > 1e-3          # not vacuous: within three decades of the bound
        assert bool((bound[0, 1] == 0).all())                               # dead cell: exact


def test_conv4d_bound_against_single_rounded_operands():
    gen = torch.Generator().manual_seed(6)
    x = torch.rand(1, 3, 4, 3, 5, generator=gen, dtype=torch.float64)
    x[0, 1] = 0.0
    w = torch.randn(3, 4, 1, 3, 3, 3, generator=gen, dtype=torch.float64) * 0.3
    b = torch.randn(4, generator=gen, dtype=torch.float64) * 0.1
    ws = cm.pow2_to_top(w.abs().amax(dim=(0, 2, 3, 4, 5), keepdim=True))
    got = orc.conv4d(_round_fp16(x, 4096.0), _round_fp16(w, ws), b)
    err = (got - orc.conv4d(x, w, b)).abs()
    bound = cm.conv_bound(x.abs(), torch.zeros_like(x), w, b, ws, 4096.0, "fp16", 81)
    assert bool((err <= bound).all()) and float(err.max()) > 0
    assert float((err / bound).max()) > 1e-3


def test_mutual_matching_bound_keeps_every_order():
    """mm_bound covers a perturbation as large as the value itself (the first-order form does not)."""
    gen = torch.Generator().manual_seed(7)
    p = torch.rand(3, 4, 3, 4, generator=gen, dtype=torch.float64)
    p[0, 0] *= 1e-3
    ep = torch.full_like(p, 2e-3)
    x, ex = cm.mm_bound(p, ep)
    for sign in (1.0, -1.0):
        q = p + sign * ep * (torch.rand(p.shape, generator=gen, dtype=torch.float64) * 2 - 1).sign()
        assert bool(((orc.mutual_matching(q) - x).abs() <= ex).all())


def test_default_bound_is_much_smaller():
    fa, fb = cm.case_inputs("c32_6x8_k1")
    na, nb = orc.l2_normalize(fa[0].double(), 0).abs(), orc.l2_normalize(fb[0].double(), 0).abs()
    assert float((cm.corr_bound(na, nb, "fp16") / cm.corr_bound(na, nb, "fp16x2")).min()) > 50
