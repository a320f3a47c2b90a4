"""The operator layer without a GPU: the reference's goldens against the float64 restatements (the inputs are well conditioned
before any kernel runs), argument errors of the new entry points before any device use, state_dict round trips, the import
route, and the refusal of CPU tensors."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import operators_reference as orf
from patch2pix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def test_version_and_exports():
    assert _lib.p2p_version() & ~_lib.VERSION_EXPERIMENT >= 110
    for name in ("p2p_correlation_batch", "p2p_maxpool4d_batch", "p2p_mutual_matching_workspace_bytes", "p2p_mutual_matching_batch",
                 "p2p_conv4d_create", "p2p_conv4d_destroy", "p2p_conv4d_forward_batch", "p2p_l2_normalize"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)


def test_goldens_against_restatements():
    g = orf.golden("corr")
    for case in orf.CORR_CASES:
        fa, fb = orf.corr_inputs(case)
        if case != "B":
            assert torch.equal(T(g[f"a_{case}"]), fa) and torch.equal(T(g[f"b_{case}"]), fb)
        else:
            assert str(g["digest_B"]) == orf.input_digest(fa, fb), ("the seeded inputs of correlation case B differ from those the "
                                                                     "fixture was made from: this torch draws another random stream")
        err = orf.rel_err(T(g[f"out_{case}"]), orf.correlation64(fa, fb))
        print(f"corr_{case}: golden {err:.3g}, REF_ERR {orf.REF_ERR[f'corr_{case}']:.3g}")
        assert err <= orf.REF_ERR[f"corr_{case}"]
    g = orf.golden("conv4d")
    for case in orf.CONV_CASES:
        w, bias = orf.conv_weights(case)
        assert torch.equal(T(g[f"w_{case}"]), w)
        for vol in orf.CONV_VOLUMES:
            x = orf.conv_input(case, vol)
            assert torch.equal(T(g[f"x_{case}_{vol}"]), x)
            assert orf.rel_err(T(g[f"y_{case}_{vol}"]), orf.conv4d64(x, w, bias)) <= orf.REF_ERR[f"conv_{case}_{vol}"]
    g = orf.golden("nc")
    assert torch.equal(T(g["x"]), orf.nc_input())
    for case in orf.NC_CASES:
        y64 = orf.neigh_consensus64(orf.nc_input(), case)
        assert float((y64 > 0).double().mean()) >= 0.25
        assert orf.rel_err(T(g[f"y_{case}"]), y64) <= orf.REF_ERR[f"nc_{case}"]


def test_exact_goldens_against_restatements():
    g = orf.golden("pool_mm_l2")
    for k in orf.POOL_CASES:
        x = orf.pool_input(k)
        assert torch.equal(T(g[f"x_{k}"]), x)
        pooled, code = orf.maxpool4d_restated(x, k)
        d = T(g[f"delta_{k}"]).long()
        assert torch.equal(pooled, T(g[f"pooled_{k}"])) and torch.equal(code, ((d[0] * k + d[1]) * k + d[2]) * k + d[3])
        windows = x.shape[0] * pooled[0].numel()
        ties = int((torch.stack([x[:, i::k, j::k, a::k, b::k] for i in range(k) for j in range(k) for a in range(k) for b in range(k)], 1)
                    == pooled.unsqueeze(1)).sum(1).gt(1).sum())
        assert k == 1 or ties > windows // 2, (k, ties, windows)
    orf.check_mutual(T(g["mm_y"]), orf.mm_input(), "golden")
    for case, (_, dim) in orf.L2_CASES.items():
        orf.check_l2(T(g[f"l2_y_{case}"]), orf.l2_input(case), dim, f"{case} golden")


def test_argument_errors_before_any_device_use():
    L, one = _lib, 1
    h = ctypes.c_void_p()
    assert L.p2p_correlation_batch(None, one, 1, 8, 2, 2, 2, 2, one, None) == -1 and b"null" in L.p2p_last_error()
    assert L.p2p_correlation_batch(one, one, 0, 8, 2, 2, 2, 2, one, None) == -1
    assert L.p2p_correlation_batch(one, one, 1, 0, 2, 2, 2, 2, one, None) == -1
    assert L.p2p_correlation_batch(one, one, 1, 8, 4096, 4096, 2, 2, one, None) == -3
    assert L.p2p_maxpool4d_batch(None, 1, 4, 4, 4, 4, 2, one, None, None) == -1
    assert L.p2p_maxpool4d_batch(one, 1, 4, 4, 4, 4, 0, one, None, None) == -1
    assert L.p2p_maxpool4d_batch(one, 1, 4, 4, 4, 6, 4, one, None, None) == -1 and b"multiples" in L.p2p_last_error()
    assert L.p2p_maxpool4d_batch(one, 1, 5, 5, 5, 5, 5, one, None, None) == -3
    assert L.p2p_mutual_matching_workspace_bytes(0, 2, 2, 2, 2) == 0 and L.p2p_mutual_matching_workspace_bytes(2, 5, 6, 4, 7) == 2 * (32 + 28) * 4
    assert L.p2p_mutual_matching_batch(None, 1, 2, 2, 2, 2, one, one, 64, None) == -1
    assert L.p2p_mutual_matching_batch(one, 1, 2, 0, 2, 2, one, one, 64, None) == -1
    assert L.p2p_mutual_matching_batch(one, 1, 2, 2, 2, 2, one, 4, 8, None) == -4
    assert L.p2p_mutual_matching_batch(one, 1, 256, 256, 128, 256, one, one, 1 << 40, None) == -3      # 2^31 cells per item
    assert L.p2p_mutual_matching_batch(one, 1, 256, 256, 128, 255, one, 4, 8, None) == -4             # just below: the next check
    assert L.p2p_conv4d_create(None, None, 1, 1, 3, ctypes.byref(h)) == -1
    assert L.p2p_conv4d_create(one, None, 0, 1, 3, ctypes.byref(h)) == -1
    assert L.p2p_conv4d_create(one, None, 1, 17, 3, ctypes.byref(h)) == -3
    assert L.p2p_conv4d_create(one, None, 1, 1, 7, ctypes.byref(h)) == -3 and b"kernel" in L.p2p_last_error()
    assert L.p2p_conv4d_forward_batch(None, one, 1, 2, 2, 2, 2, one, None) == -1
    assert L.p2p_l2_normalize(None, 1, 1, 1, one, None) == -1
    assert L.p2p_l2_normalize(one, 1, 0, 1, one, None) == -1
    assert L.p2p_l2_normalize(one, 1 << 40, 4, 1, one, None) == -3
    with pytest.raises(NotImplementedError):
        L.check(-3, "p2p_conv4d_create")


def test_state_dict_round_trips():
    from patch2pix_amd.networks.ncn.conv4d import Conv4d
    from patch2pix_amd.networks.ncn.model import NeighConsensus
    g = orf.golden("nc")
    for case, c in orf.NC_CASES.items():
        net = NeighConsensus(use_cuda=False, **c)
        sd = {k[len(case) + 1:]: T(v) for k, v in g.items() if k.startswith(case + ".")}
        net.load_state_dict(sd, strict=True)
        back = net.state_dict()
        assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    default = NeighConsensus(use_cuda=False)
    assert default.kernel_sizes == [3, 3, 3] and default.channels == [10, 10, 1] and default.symmetric_mode
    assert tuple(default.state_dict()["conv.2.weight"].shape) == (3, 10, 10, 3, 3, 3)
    for case, (ci, co, k, has_bias) in orf.CONV_CASES.items():
        w, bias = orf.conv_weights(case)
        layer = Conv4d(ci, co, k, bias=has_bias)
        assert tuple(layer.weight.shape) == (k, co, ci, k, k, k) and (layer.bias is not None) == has_bias
        layer.load_state_dict({"weight": w} if bias is None else {"weight": w, "bias": bias}, strict=True)
        assert torch.equal(layer.state_dict()["weight"], w)
    assert tuple(Conv4d(2, 3, 3, pre_permuted_filters=False).weight.shape) == (3, 2, 3, 3, 3, 3)
    with pytest.raises(NotImplementedError):
        NeighConsensus(use_cuda=False, kernel_sizes=[7], channels=[1])
    with pytest.raises(NotImplementedError):
        NeighConsensus(use_cuda=False, kernel_sizes=[3, 3], channels=[32, 1])


def test_import_route_names(tmp_path):
    pkg = os.path.join(ROOT, "patch2pix_amd")
    code = f"""
import sys
sys.path.append({pkg!r})
from networks.modules import L2Normalize, cal_conv_out_size, maxpool4d, FeatCorrelation
from networks.ncn.model import MutualMatching, NeighConsensus
from networks.ncn.conv4d import Conv4d, conv4d
from networks.ncn.extract_ncmatches import corr_to_matches, corr_to_matches_topk
import inspect, networks.ncn.model as m, patch2pix_amd.networks.ncn.model as q
assert m is q and NeighConsensus.__module__ == 'patch2pix_amd.networks.ncn.model'
sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != 'self']
E = inspect.Parameter.empty
assert sig(maxpool4d) == [('corr4d_hres', E), ('k_size', 4)] and cal_conv_out_size(16, 3, 2, 1) == 8
assert sig(FeatCorrelation.__init__) == [('shape', '4D')]
assert sig(NeighConsensus.__init__) == [('use_cuda', True), ('kernel_sizes', [3, 3, 3]), ('channels', [10, 10, 1]), ('symmetric_mode', True)]
assert sig(Conv4d.__init__) == [('in_channels', E), ('out_channels', E), ('kernel_size', E), ('bias', True), ('pre_permuted_filters', True)]
assert sig(conv4d) == [('data', E), ('filters', E), ('bias', None), ('permute_filters', True), ('use_half', False)]
assert sig(corr_to_matches) == [('corr4d', E), ('delta4d', None), ('ksize', 1), ('do_softmax', True), ('scale', 'positive'),
                                ('invert_matching_direction', False), ('return_indices', True)]
assert sig(corr_to_matches_topk) == [('corr4d', E), ('delta4d', None), ('topk', 1), ('ksize', 1), ('do_softmax', True),
                                     ('invert_matching_direction', False)]
try:
    from networks.modules import FeatRegressNet
except NotImplementedError as e:
    assert 'materialised patches' in str(e)
    print("ROUTE_OK")
"""
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0 and "ROUTE_OK" in res.stdout, res.stderr[-3000:]


def test_cpu_tensors_are_refused():
    from patch2pix_amd.networks import modules
    from patch2pix_amd.networks.ncn import conv4d, extract_ncmatches, model
    x6 = torch.zeros(1, 1, 2, 2, 2, 2)
    calls = [lambda: modules.L2Normalize(torch.zeros(2, 3), 1), lambda: modules.maxpool4d(x6, 2),
             lambda: modules.FeatCorrelation()(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)),
             lambda: model.MutualMatching(x6), lambda: model.NeighConsensus(use_cuda=False)(x6),
             lambda: conv4d.Conv4d(1, 2, 3)(x6), lambda: conv4d.conv4d(x6, torch.zeros(2, 1, 3, 3, 3, 3)),
             lambda: extract_ncmatches.corr_to_matches(x6), lambda: extract_ncmatches.corr_to_matches_topk(x6, topk=2)]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(NotImplementedError):
        conv4d.conv4d(x6, torch.zeros(2, 1, 3, 3, 3, 3), use_half=True)
