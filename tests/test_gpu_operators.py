"""The operator layer on the GPU: every case of tests/operators_reference.py through the real library behind the Python names
(networks.modules, networks.ncn.*), an item alone against the item in its batch, and the operators chained by hand on the
pyramids of one seeded pair against Patch2Pix.forward / cal_coarse_matches of the same model."""
import os
import subprocess
import sys

import pytest
import torch

import ncn_reference as nr
import operators_reference as orf
import regressor_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def names():
    from patch2pix_amd.networks import modules
    from patch2pix_amd.networks.ncn import conv4d, extract_ncmatches, model
    import types
    return types.SimpleNamespace(modules=modules, conv4d=conv4d, extract=extract_ncmatches, model=model)


@pytest.mark.parametrize("case", list(orf.CORR_CASES))
def test_correlation(case, dev, names):
    fa, fb = orf.corr_inputs(case)
    out = names.modules.FeatCorrelation()(fa.to(dev), fb.to(dev))
    b, _, ha, wa = fa.shape
    assert out.shape == (b, 1, ha, wa) + tuple(fb.shape[2:])
    flat = out.reshape(b, ha * wa, -1)
    orf.check_measured(flat.cpu(), orf.correlation64(fa, fb), f"corr_{case}", "gpu")
    out3 = names.modules.FeatCorrelation(shape='3D')(fa.to(dev), fb.to(dev))
    assert out3.shape == (b, flat.shape[2], ha, wa) and torch.equal(out3.reshape(b, -1, ha * wa).transpose(1, 2), flat)
    alone = names.modules.FeatCorrelation()(fa[-1:].to(dev), fb[-1:].to(dev))
    assert torch.equal(alone[0], out[-1])


@pytest.mark.parametrize("k", list(orf.POOL_CASES))
def test_maxpool4d(k, dev, names):
    x, g = orf.pool_input(k).to(dev), orf.golden("pool_mm_l2")
    pooled, mi, mj, mk, ml = names.modules.maxpool4d(x.unsqueeze(1), k)
    assert pooled.shape == mi.shape == (x.shape[0], 1) + tuple(s // k for s in x.shape[1:]) and mi.dtype == torch.int64
    assert torch.equal(pooled[:, 0].cpu(), T(g[f"pooled_{k}"]))
    assert torch.equal(torch.stack([mi, mj, mk, ml])[:, :, 0].cpu(), T(g[f"delta_{k}"]).long())
    alone = names.modules.maxpool4d(x[1:2].unsqueeze(1), k)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(alone, (pooled, mi, mj, mk, ml)))


def test_maxpool4d_default_and_bad_sides(dev, names):
    x = orf.pool_input(4).to(dev).unsqueeze(1)
    assert torch.equal(names.modules.maxpool4d(x)[0], names.modules.maxpool4d(x, 4)[0])
    with pytest.raises(RuntimeError):
        names.modules.maxpool4d(x, 3)            # 8 is no multiple of 3
    with pytest.raises(NotImplementedError):
        names.modules.maxpool4d(torch.zeros(1, 1, 5, 5, 5, 5, device=dev), 5)


def test_maxpool4d_propagates_nan_and_takes_an_empty_batch(dev, names):
    x, pooled, code = orf.pool_nan_case()
    got, mi, mj, mk, ml = names.modules.maxpool4d(x.to(dev).unsqueeze(1), 2)
    got = got[:, 0].cpu()
    assert torch.equal(got.isnan(), pooled.isnan()) and torch.equal(got[~pooled.isnan()], pooled[~pooled.isnan()])
    assert torch.equal((((mi * 2 + mj) * 2 + mk) * 2 + ml)[:, 0].cpu(), code)
    empty = names.modules.maxpool4d(torch.zeros(0, 1, 4, 4, 4, 4, device=dev), 2)
    assert empty[0].shape == empty[1].shape == (0, 1, 2, 2, 2, 2)


def test_functional_conv4d_with_temporary_filters(dev, names):
    """Different filters of one shape, each a temporary that is freed before the next call: every result is that of its own
    filters (a Conv4d module holding them), and the results differ."""
    x = orf.conv_input("1to16k3", "v2392").to(dev)
    g = torch.Generator().manual_seed(4450)
    outs = []
    with torch.no_grad():
        for _ in range(6):
            w = torch.randn(16, 1, 3, 3, 3, 3, generator=g) * 0.1           # [c_out, c_in, k, k, k, k]
            layer = names.conv4d.Conv4d(1, 16, 3, bias=False)
            layer.load_state_dict({"weight": w.permute(2, 0, 1, 3, 4, 5).contiguous()}, strict=True)
            want = layer.to(dev)(x)
            got = names.conv4d.conv4d(x, (w * 1.0).to(dev))                 # a temporary
            assert torch.equal(got, want)
            got_stored = names.conv4d.conv4d(x, w.permute(2, 0, 1, 3, 4, 5).contiguous().to(dev), permute_filters=False)
            assert torch.equal(got_stored, want)
            outs.append(got)
            del w, layer, want, got, got_stored
    assert all(not torch.equal(outs[i], outs[j]) for i in range(6) for j in range(i))


def test_mutual_matching(dev, names):
    x = orf.mm_input()
    y = names.model.MutualMatching(x.to(dev).unsqueeze(1))
    assert y.shape == (2, 1) + tuple(x.shape[1:])
    orf.check_mutual(y[:, 0].cpu(), x, "gpu")
    assert torch.equal(names.model.MutualMatching(x[1:2].to(dev).unsqueeze(1))[0], y[1])


@pytest.mark.parametrize("case", list(orf.L2_CASES))
def test_l2_normalize(case, dev, names):
    x, dim = orf.l2_input(case), orf.L2_CASES[case][1]
    y = names.modules.L2Normalize(x.to(dev), dim)
    orf.check_l2(y.cpu(), x, dim, f"{case} gpu")
    assert torch.equal(names.modules.L2Normalize(x[1:2].to(dev), dim)[0], y[1]) or dim == 0


@pytest.mark.parametrize("vol", list(orf.CONV_VOLUMES))
@pytest.mark.parametrize("case", list(orf.CONV_CASES))
def test_conv4d(case, vol, dev, names):
    ci, co, k, has_bias = orf.CONV_CASES[case]
    w, bias = orf.conv_weights(case)
    x = orf.conv_input(case, vol)
    layer = names.conv4d.Conv4d(ci, co, k, bias=has_bias)
    layer.load_state_dict({"weight": w} if bias is None else {"weight": w, "bias": bias}, strict=True)
    layer.to(dev)
    with torch.no_grad():
        y = layer(x.to(dev))
        assert y.shape == (x.shape[0], co) + tuple(x.shape[2:])
        orf.check_measured(y.cpu(), orf.conv4d64(x, w, bias), f"conv_{case}_{vol}", "gpu")
        assert torch.equal(layer(x[1:2].to(dev))[0], y[1])
        # the functional form, filters in the [c_out, c_in, k, k, k, k] layout
        f = names.conv4d.conv4d(x.to(dev), w.permute(1, 2, 0, 3, 4, 5).contiguous().to(dev), bias.to(dev) if has_bias else None)
        assert torch.equal(f, y)
        layer.weight.mul_(2.0)                   # the packed handle follows the parameter's version counter
        assert not torch.equal(layer(x.to(dev)), y)
    with pytest.raises(NotImplementedError):
        layer(x.to(dev).requires_grad_())


@pytest.mark.parametrize("case", list(orf.NC_CASES))
def test_neigh_consensus(case, dev, names):
    c = orf.NC_CASES[case]
    net = names.model.NeighConsensus(use_cuda=False, **c)
    net.load_state_dict(orf.nc_weights(case), strict=True)
    net.to(dev)
    x = orf.nc_input()
    with torch.no_grad():
        y = net(x.to(dev).unsqueeze(1))
    assert y.shape == (x.shape[0], 1) + tuple(x.shape[1:])
    assert net._hip.generic == (case != "R")     # the released stack runs the tuned kernel
    orf.check_measured(y[:, 0].cpu(), orf.neigh_consensus64(x, case), f"nc_{case}", "gpu")
    with torch.no_grad():
        handle = net._hip
        assert torch.equal(net(x[1:2].to(dev).unsqueeze(1))[0], y[1]) and net._hip is handle


def _same(out, g, name, score_tol=None):
    for i in range(4):
        ref = T(g[f"{name}.{i}"])
        assert out[i].dtype == ref.dtype and out[i].shape == ref.shape and torch.equal(out[i].cpu(), ref), (name, i)
    ref = T(g[f"{name}.4"])
    assert out[4].shape == ref.shape
    if score_tol is None:
        assert torch.equal(out[4].cpu(), ref), name
    else:
        err = (out[4].cpu() - ref).abs().max().item()
        assert err <= score_tol, (name, err)


def test_corr_to_matches(dev, names):
    g = orf.golden("matches")
    from patch2pix_amd import ops
    for name, ksize, kw in orf.match_cases() + orf.coord_cases():
        x, delta = orf.match_inputs(ksize)
        d = None if delta is None else tuple(t.to(dev) for t in delta)
        out = names.extract.corr_to_matches(x.to(dev), delta4d=d, **kw)
        _same(out, g, name, orf.SOFTMAX_TOL if kw["do_softmax"] else None)
        if kw["do_softmax"]:      # the scores of cal_coarse_matches on the same volume, bit for bit
            packed = None if d is None else (((d[0] * ksize + d[1]) * ksize + d[2]) * ksize + d[3])[:, 0].to(torch.uint8)
            _, s = ops.coarse_matches_batch(x.to(dev)[:, 0], packed, ksize, 1, False)
            nb = x.shape[4] * x.shape[5]
            assert torch.equal(out[4], s[:, nb:] if kw["invert_matching_direction"] else s[:, :nb])
        alone = names.extract.corr_to_matches(x[1:2].to(dev), delta4d=None if d is None else tuple(t[1:2] for t in d), **kw)
        assert all(torch.equal(a[0], b[1]) for a, b in zip(alone, out))


def test_corr_to_matches_topk(dev, names):
    g = orf.golden("matches")
    for name, ksize, kw in orf.topk_cases():
        x, delta = orf.match_inputs(ksize)
        d = None if delta is None else tuple(t.to(dev) for t in delta)
        out = names.extract.corr_to_matches_topk(x.to(dev), delta4d=d, **kw)
        _same(out, g, name, orf.SOFTMAX_TOL if kw["do_softmax"] else None)
    with pytest.raises(NotImplementedError):
        names.extract.corr_to_matches_topk(orf.match_inputs(1)[0].to(dev), topk=9)


def test_chain_reproduces_the_fused_coarse_stage(dev, names):
    """L2Normalize -> FeatCorrelation -> maxpool4d -> MutualMatching -> NeighConsensus -> MutualMatching -> corr_to_matches
    twice, on the layer-3 features of one seeded 128x160 pair at ksize 2, against Patch2Pix.forward and cal_coarse_matches."""
    from oracle import error_model
    from patch2pix_amd.utils.eval import model_helper
    ck = rr.checkpoint("R")
    net = model_helper.load_model(ck, lprint=lambda *a: None)
    a, b = synthetic.make_image_pair(31, 128, 160)
    norm = lambda x: (T(x).permute(2, 0, 1).float() / 255.0 - 0.45)[None].to(dev) / 0.225
    ksize = 2
    with torch.no_grad():
        corr4d, delta4d, f1s, f2s = net.forward(norm(a), norm(b), ksize=ksize, return_feats=True)
        rows, scores = net.cal_coarse_matches(corr4d, delta4d, ksize=ksize, upsample=1, center=False)
        f1, f2 = f1s[-1], f2s[-1]
        ncn = names.model.NeighConsensus(use_cuda=False, kernel_sizes=[3, 3], channels=[16, 1])
        ncn.load_state_dict({k[4:]: v for k, v in ck["state_dict"].items() if k.startswith("ncn.")}, strict=True)
        ncn.to(dev)
        hres = names.modules.FeatCorrelation()(names.modules.L2Normalize(f1, 1), names.modules.L2Normalize(f2, 1))
        pooled, mi, mj, mk, ml = names.modules.maxpool4d(hres, ksize)
        vol = names.model.MutualMatching(ncn(names.model.MutualMatching(pooled)))
        ba = names.extract.corr_to_matches(vol, delta4d=(mi, mj, mk, ml), ksize=ksize)
        ab = names.extract.corr_to_matches(vol, delta4d=(mi, mj, mk, ml), ksize=ksize, invert_matching_direction=True)
    chain_rows = torch.cat([torch.stack(ba[:4], -1), torch.stack(ab[:4], -1)], 1)
    fused_delta = torch.stack([t for t in delta4d])
    differ = int((fused_delta != torch.stack([mi, mj, mk, ml])).sum())
    scale = corr4d.abs().max().item()
    err = (vol - corr4d).abs().max().item()
    print(f"chain vs fused: {differ} relocalisation entries differ; volume {err:.3g} of max {scale:.3g}, bar {nr.CORR_RTOL * scale:.3g}")
    assert differ == 0
    assert err <= nr.CORR_RTOL * scale
    model = error_model.ErrorModel(f1[0].cpu(), f2[0].cpu(), ck["state_dict"], ksize=ksize)
    _, ok = model.decidable()
    print(f"{int(ok.sum())} of {ok.numel()} rows decidable")
    assert int(ok.sum()) > ok.numel() // 2
    assert torch.equal(chain_rows[0].cpu()[ok], rows[0].cpu()[ok])


def test_import_route_resolves_to_this_package(tmp_path):
    code = f"""
import sys
sys.path.append({os.path.join(ROOT, 'patch2pix_amd')!r})
import torch
from networks.ncn.model import NeighConsensus, MutualMatching
assert NeighConsensus.__module__ == 'patch2pix_amd.networks.ncn.model'
y = MutualMatching(torch.rand(1, 1, 3, 4, 2, 5, device='cuda'))
assert y.shape == (1, 1, 3, 4, 2, 5) and bool(torch.isfinite(y).all())
print("ROUTE_GPU_OK")
"""
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0 and "ROUTE_GPU_OK" in res.stdout, res.stderr[-3000:]
