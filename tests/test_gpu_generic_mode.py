"""MI355X: the generic regressor in mode 'generic_fp16x2' (csrc/regress_generic_h2.hip) on the "gpu" inputs of
tests/regressor_reference.py (96x128, 61 proposals, the four corner pairs among them): all six cases against the fp32
restatement at the project's bars, launch invariance and the round trip between the modes bit for bit, a chunk whose proposal
count is no multiple of 8, the range variants of tests/generic_mode_reference.py, a ResNet50 feat_idx [0, 1] model end to end
under Patch2Pix.set_fine_mode, and P2P_REGRESS_GENERIC_MODE in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import generic_mode_reference as gm
import regressor_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = "generic_fp16x2"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_regs = {}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    _regs.clear()          # the handles go while the library is still loaded


def _handles(case, dev, mode=MODE, sd=None, key=None):
    """(mid, fine) generic RegressorWeights of a case (fine is mid for shared=True) in `mode`, built once per (case, mode, key)."""
    from patch2pix_amd import ops
    k = (case, mode, key)
    if k not in _regs:
        ck = rr.checkpoint(case)
        sd = ck["state_dict"] if sd is None else sd
        kw = dict(config=ck["regressor_config"], feat_idx=ck["feat_idx"], generic=True)
        mid = ops.RegressorWeights(rr.sub_params(sd, "regress_mid."), dev, **kw)
        fine = mid if rr.CASES[case]["shared"] else ops.RegressorWeights(rr.sub_params(sd, "regress_fine."), dev, **kw)
        for reg in (mid, fine):
            assert reg.generic and reg.mode in ("generic", mode)
            reg.set_mode(mode)
            assert reg.mode == mode
        _regs[k] = (mid, fine)
    return _regs[k]


def _on(dev, pyr):
    return [t.to(dev) for t in pyr[:4]]


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "R"])
def test_cases_against_restatement(case, dev):
    from patch2pix_amd import ops
    p1, p2, props = rr.inputs("gpu")
    mid, fine = _handles(case, dev)
    out = ops.regress(mid, fine, _on(dev, p1), _on(dev, p2), props.to(dev), want_raw=True)
    rr.check_levels(out, p1, p2, props, case, "gpu generic_fp16x2")


@pytest.mark.parametrize("case", ["A", "C"])
def test_outputs_do_not_depend_on_the_launch(case, dev):
    """A proposal's raw outputs, bit for bit: alone, inside a ragged 3-item batch with images of different sizes, through
    regress_batch_dev with a stride of 64 and counts (61, 0, 17), and with a workspace of one 8-proposal unit."""
    from patch2pix_amd import ops, _lib
    p1, p2, props = rr.inputs("gpu")
    mid, fine = _handles(case, dev)
    a1, a2, pd = _on(dev, p1), _on(dev, p2), props.to(dev)
    base = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
    for i in (0, 17, 60):
        one = ops.regress(mid, fine, a1, a2, pd[i:i + 1], want_raw=True)
        assert torch.equal(one["raw1"][0], base["raw1"][i]) and torch.equal(one["raw2"][0], base["raw2"][i])
    q1, q2 = synthetic.make_pyramid(51, 64, 80), synthetic.make_pyramid(52, 64, 80)
    b1, b2 = _on(dev, q1), _on(dev, q2)
    small = torch.tensor([[5, 6, 70, 50], [40, 30, 41, 31], [79, 63, 0, 0]], dtype=torch.int64, device=dev)
    outs = ops.regress_batch(mid, fine, [b1, a1, b1], [b2, a2, b2], [small, pd, small[:2]], want_raw=True)
    for k in ("raw1", "raw2", "matches2", "probs2"):
        assert torch.equal(outs[1][k], base[k]), k
    assert torch.equal(outs[0]["raw2"][:2], outs[2]["raw2"])
    stride, counts = 64, (61, 0, 17)
    padded = torch.zeros((3, stride, 4), dtype=torch.int64, device=dev)
    for b, c in enumerate(counts):
        padded[b, :c] = pd[:c]
    sentinel = -7.5
    bufs = {k: torch.full((3, stride) + shp, sentinel, device=dev)
            for k, shp in (("matches1", (4,)), ("probs1", ()), ("raw1", (5,)), ("matches2", (4,)), ("probs2", ()), ("raw2", (5,)))}
    dout = ops.regress_batch_dev(mid, fine, [a1] * 3, [a2] * 3, padded, torch.tensor(counts, dtype=torch.int32, device=dev),
                                 want_raw=True, out=bufs)
    for b, c in enumerate(counts):
        for k in ("raw1", "raw2", "matches1", "matches2", "probs1", "probs2"):
            assert torch.equal(dout[k][b, :c], base[k][:c]), (k, b)
            assert bool((dout[k][b, c:] == sentinel).all()), (k, b)
    unit = _lib.p2p_regress_workspace_bytes_for(mid.handle, 8)
    assert _lib.p2p_regress_workspace_bytes_for(mid.handle, 61) == 8 * unit
    ops.generic_scratch_limit = unit
    try:
        chunked = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
    finally:
        ops.generic_scratch_limit = None
    for k in base:
        assert torch.equal(chunked[k], base[k]), k


def test_chunks_that_are_no_multiple_of_8(dev):
    """61 proposals in chunks of 24 (24 + 24 + 13): the last chunk's 13 proposals leave 3 rows of a unit of 8 empty, and with case
    D's 25-pixel maps its row tiles straddle samples and end inside a tile.  Bit for bit the one-chunk result."""
    from patch2pix_amd import ops, _lib
    p1, p2, props = rr.inputs("gpu")
    a1, a2, pd = _on(dev, p1), _on(dev, p2), props.to(dev)
    for case in ("D", "A"):
        mid, fine = _handles(case, dev)
        base = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
        ops.generic_scratch_limit = 3 * _lib.p2p_regress_workspace_bytes_for(mid.handle, 8)
        try:
            chunked = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
            odd = ops.regress(mid, fine, a1, a2, pd[:13], want_raw=True)
        finally:
            ops.generic_scratch_limit = None
        for k in base:
            assert torch.equal(chunked[k], base[k]) and torch.equal(odd[k], base[k][:13]), (case, k)


def test_round_trip_between_the_modes(dev):
    from patch2pix_amd import ops
    case = "A"
    p1, p2, props = rr.inputs("gpu")
    a1, a2, pd = _on(dev, p1), _on(dev, p2), props.to(dev)
    mid, fine = _handles(case, dev, mode="generic", key="round trip")
    run = lambda: {k: v.clone() for k, v in ops.regress(mid, fine, a1, a2, pd, want_raw=True).items()}

    def select(mode):
        for reg in (mid, fine):
            reg.set_mode(mode)
            assert reg.mode == mode
    first = run()
    select(MODE)
    second = run()
    select("generic")
    third = run()
    select(MODE)
    fourth = run()
    for k in first:
        assert torch.equal(first[k], third[k]) and torch.equal(second[k], fourth[k]), k
    assert not torch.equal(first["raw2"], second["raw2"])
    # a handle that never left the new mode computes the same bits
    again = ops.regress(*_handles(case, dev), a1, a2, pd, want_raw=True)
    for k in second:
        assert torch.equal(again[k], second[k]), k


@pytest.mark.parametrize("variant", gm.VARIANTS)
def test_range_variants(variant, dev):
    from patch2pix_amd import ops
    case = "A"
    p1, p2, props = rr.inputs("gpu")
    mid, fine = _handles(case, dev, sd=gm.variant_state_dict(case, variant), key=variant)
    out = ops.regress(mid, fine, _on(dev, p1), _on(dev, p2), props.to(dev), want_raw=True)
    gm.check_variant(out, p1, p2, props, case, variant, "gpu")


def test_resnet50_feat_idx_01_end_to_end(dev):
    """The committed ResNet50 / stride 8 / feat_idx [0, 1] fixture: the model in set_fine_mode('generic_fp16x2') makes the
    comparison tests/test_gpu_bottleneck.py makes for predict_fine on the reference's own features (the oracle on the same
    pyramids, every link; the reference's records for every proposal both sides hold), at the same bars; the same model in mode
    'generic' beside it; the choice survives load_state_dict."""
    import bottleneck_reference as br
    import test_gpu_bottleneck as tb
    from patch2pix_amd.networks.patch2pix import Patch2Pix
    name = "bottleneck_r50_fi01"
    g, ck = tb._golden(name), tb._ckpt(name)
    sd = ck["state_dict"]
    net = Patch2Pix(br.model_config(name, ck, dev))               # a model of its own: the shared one keeps its mode
    assert net.fine_mode == "generic" and net._weights()[1].generic and net._weights()[1].mode == "generic"
    with pytest.raises(NotImplementedError):
        net.set_fine_mode("fp16x2w")
    with pytest.raises(ValueError):
        net.set_fine_mode("generic_fp16")
    assert net._weights()[1].mode == "generic"
    p32, _ = tb._cpu_pyramids(name)
    fa, fb = tb._ref_feats(name)
    f1 = [t.to(dev) for t in p32[0][:4]] + [fa.to(dev)]
    f2 = [t.to(dev) for t in p32[1][:4]] + [fb.to(dev)]
    with torch.no_grad():
        exact = [t[0].cpu().clone() for t in net.predict_fine_from_feats(f1, f2, ksize=2, return_all=True)]
    net.set_fine_mode(MODE)
    assert net.fine_mode == MODE and all(r.mode == MODE for r in net._weights()[1:])
    net.load_state_dict(net.state_dict())                         # a re-pack: new handles, the model's choice applied again
    assert net._packed is None
    assert all(r.mode == MODE for r in net._weights()[1:])
    with torch.no_grad():
        out = net.predict_fine_from_feats(f1, f2, ksize=2, return_all=True)
    tb._against_the_oracle(net, sd, f1, f2, out, f"{name} generic_fp16x2")
    fine, fs, mid, ms, coarse = (t[0].cpu() for t in out)
    assert torch.equal(coarse, exact[4])
    dc = max(float((fine - exact[0]).abs().max()), float((mid - exact[2]).abs().max()))
    ds = max(float((fs - exact[1]).abs().max()), float((ms - exact[3]).abs().max()))
    print(f"{name}: generic_fp16x2 against generic: coord {dc:.3g} px score {ds:.3g} on {coarse.shape[0]} proposals")
    # the reference's records, as test_predict_fine_against_the_reference: every proposal both sides hold
    ref_c = [tuple(r) for r in g["coarse"].astype(np.int64).tolist()]
    where = {r: i for i, r in enumerate(ref_c)}
    got_c = [tuple(r) for r in coarse.tolist()]
    gi = torch.tensor([i for i, r in enumerate(got_c) if r in where], dtype=torch.int64)
    ri = torch.tensor([where[got_c[i]] for i in gi.tolist()], dtype=torch.int64)
    assert gi.numel() > 0
    unstable = tb._near_integer_rows(torch.from_numpy(g["mid"])[ri])
    assert int(unstable.sum()) <= 2
    for got, key, tol, rowsel in ((mid, "mid", tb.COORD_TOL, None), (ms, "mid_scores", tb.SCORE_TOL, None),
                                  (fine, "fine", tb.COORD_TOL, ~unstable), (fs, "fine_scores", tb.SCORE_TOL, ~unstable)):
        a, b = got[gi], torch.from_numpy(g[key])[ri]
        if rowsel is not None:
            a, b = a[rowsel], b[rowsel]
        err = float((a - b).abs().max())
        print(f"{name} generic_fp16x2: max |d {key}| against the reference {err:.2e} on {a.shape[0]} rows")
        assert err <= tol, f"{name}: {key} {err:.2e} from the reference"


CHILD = """
import torch
import regressor_reference as rr
from patch2pix_amd import ops
ck = rr.checkpoint("B")
kw = dict(config=ck["regressor_config"], feat_idx=ck["feat_idx"], generic=True)
reg = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_mid."), torch.device("cuda", 0), **kw)
print("mode:", reg.mode)
"""


def test_environment_sets_the_starting_mode_of_generic_handles():
    """P2P_REGRESS_GENERIC_MODE in a fresh child process (started with subprocess; nothing replaces a process that has the GPU open)."""
    env = dict(os.environ, P2P_REGRESS_GENERIC_MODE=MODE, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("P2P_REGRESS_MODE", None)
    res = subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and f"mode: {MODE}" in res.stdout, res.stdout
