"""The operator kernels (csrc/operators.hip, the PLANAR form of csrc/consensus_generic.hip) compiled for the host and run on the
CPU (tests/hipemu) on the smallest case of each operator, against the bars of tests/operators_reference.py."""
import ctypes
import os
import sys

import pytest
import torch

import operators_reference as orf

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402

P = emu_lib.ptr


@pytest.fixture(scope="module")
def emu():
    lib = emu_lib.load()
    assert "p2p_correlation_batch" in emu_lib.real.EXPORTS
    return lib


def correlation(emu, fa, fb):
    b, c, ha, wa = fa.shape
    hb, wb = fb.shape[2:]
    out = torch.full((b, ha * wa, hb * wb), float("nan"))
    assert emu.p2p_correlation_batch(P(fa), P(fb), b, c, ha, wa, hb, wb, P(out), None) == 0, emu.p2p_last_error()
    return out


def maxpool(emu, x, k):
    b, h1, w1, h2, w2 = x.shape
    shape = (b, h1 // k, w1 // k, h2 // k, w2 // k)
    pooled, code = torch.full(shape, float("nan")), torch.full(shape, 255, dtype=torch.uint8)
    assert emu.p2p_maxpool4d_batch(P(x), b, h1, w1, h2, w2, k, P(pooled), P(code), None) == 0, emu.p2p_last_error()
    return pooled, code


def mutual(emu, x):
    b, ha, wa, hb, wb = x.shape
    y = torch.full_like(x, float("nan"))
    n = emu.p2p_mutual_matching_workspace_bytes(b, ha, wa, hb, wb)
    ws = torch.empty(n, dtype=torch.uint8)
    assert emu.p2p_mutual_matching_batch(P(x), b, ha, wa, hb, wb, P(y), P(ws), n, None) == 0, emu.p2p_last_error()
    assert emu.p2p_mutual_matching_batch(P(x), b, ha, wa, hb, wb, P(y), P(ws), n - 4, None) == -4
    return y


def conv4d(emu, x, w, bias):
    h = ctypes.c_void_p()
    assert emu.p2p_conv4d_create(P(w), P(bias), w.shape[2], w.shape[1], w.shape[0], ctypes.byref(h)) == 0, emu.p2p_last_error()
    b, _, h1, w1, h2, w2 = x.shape
    y = torch.full((b, w.shape[1], h1, w1, h2, w2), float("nan"))
    assert emu.p2p_conv4d_forward_batch(h, P(x), b, h1, w1, h2, w2, P(y), None) == 0, emu.p2p_last_error()
    emu.p2p_conv4d_destroy(h)
    return y


def l2(emu, x, dim):
    import math
    y = torch.full_like(x, float("nan"))
    assert emu.p2p_l2_normalize(P(x), math.prod(x.shape[:dim]), x.shape[dim], math.prod(x.shape[dim + 1:]), P(y), None) == 0
    return y


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_correlation(case, emu):
    fa, fb = orf.corr_inputs(case)
    orf.check_measured(correlation(emu, fa, fb), orf.correlation64(fa, fb), f"corr_{case}", "emulated")


def test_correlation_item_alone(emu):
    fa, fb = orf.corr_inputs("B")
    fa, fb = fa[:, :24, :5, :7].contiguous(), fb[:, :24, :3, :6].contiguous()
    both = correlation(emu, fa, fb)
    assert torch.equal(correlation(emu, fa[1:2].contiguous(), fb[1:2].contiguous())[0], both[1])


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_maxpool4d(k, emu):
    x, g = orf.pool_input(k), orf.golden("pool_mm_l2")
    pooled, code = maxpool(emu, x, k)
    assert torch.equal(pooled, torch.from_numpy(g[f"pooled_{k}"]))
    d = torch.from_numpy(g[f"delta_{k}"]).long()
    assert torch.equal(code.long(), ((d[0] * k + d[1]) * k + d[2]) * k + d[3])
    assert torch.equal(maxpool(emu, x[1:2].contiguous(), k)[1][0], code[1])


def test_maxpool4d_propagates_nan(emu):
    x, pooled, code = orf.pool_nan_case()
    got, got_code = maxpool(emu, x, 2)
    assert torch.equal(got.isnan(), pooled.isnan()) and torch.equal(got[~pooled.isnan()], pooled[~pooled.isnan()])
    assert torch.equal(got_code.long(), code)


def test_mutual_matching(emu):
    x = orf.mm_input()
    y = mutual(emu, x)
    orf.check_mutual(y, x, "emulated")
    assert torch.equal(mutual(emu, x[1:2].contiguous())[0], y[1])


@pytest.mark.parametrize("case", list(orf.CONV_CASES))
def test_conv4d(case, emu):
    w, bias = orf.conv_weights(case)
    x = orf.conv_input(case, "v2392")
    y = conv4d(emu, x, w, bias)
    orf.check_measured(y, orf.conv4d64(x, w, bias), f"conv_{case}_v2392", "emulated")
    assert torch.equal(conv4d(emu, x[1:2].contiguous(), w, bias)[0], y[1])


@pytest.mark.parametrize("case", list(orf.L2_CASES))
def test_l2_normalize(case, emu):
    x, dim = orf.l2_input(case), orf.L2_CASES[case][1]
    orf.check_l2(l2(emu, x, dim), x, dim, f"{case} emulated")
