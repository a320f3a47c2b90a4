"""The generic regressor on the GPU: every case of tests/regressor_reference.py against the fp32 restatement at the project's
bars (mid and fine level), the released configuration beside the tuned f32 mode and the reference's golden, bit-invariance of
a proposal's outputs under batching / device-side counts / chunk size, handle mismatches, and a non-released checkpoint end
to end (file -> load_model -> refine_matches / predict_fine_device / GraphedMatcher)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import regressor_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_regs = {}


def _handles(case, dev):
    """(mid, fine) generic RegressorWeights of a case (fine is mid for shared=True), built once."""
    from patch2pix_amd import ops
    if case not in _regs:
        ck = rr.checkpoint(case)
        kw = dict(config=ck["regressor_config"], feat_idx=ck["feat_idx"], generic=True)
        mid = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_mid."), dev, **kw)
        fine = mid if rr.CASES[case]["shared"] else ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_fine."), dev, **kw)
        assert mid.generic and mid.mode == "generic"
        _regs[case] = (mid, fine)
    return _regs[case]


def _on(dev, pyr):
    return [t.to(dev) for t in pyr[:4]]


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "R"])
def test_cases_against_restatement(case, dev):
    from patch2pix_amd import ops
    p1, p2, props = rr.inputs("gpu")
    mid, fine = _handles(case, dev)
    out = ops.regress(mid, fine, _on(dev, p1), _on(dev, p2), props.to(dev), want_raw=True)
    rr.check_levels(out, p1, p2, props, case, "gpu")


def test_released_configuration_beside_tuned_f32_and_golden(dev):
    """Case R through the generic handle and through the tuned f32 mode: both within the bars of the reference's
    forward_fine_match golden (no bit-equality between them is claimed)."""
    from patch2pix_amd import ops
    sd = gu.state_dict(0)
    g = gu.load("fine_96x128")
    p1, p2 = gu.fine_inputs(g)
    for tag, prefix in (("int_mid", "regress_mid."), ("float_fine", "regress_fine.")):
        sub = rr.sub_params(sd, prefix)
        tuned = ops.RegressorWeights(sub, dev)
        tuned.set_mode("f32")
        generic = ops.RegressorWeights(sub, dev, generic=True)
        assert not tuned.generic and generic.generic
        props = torch.from_numpy(g[tag + "_in"]).to(dev)
        for name, reg in (("tuned f32", tuned), ("generic", generic)):
            out = ops.regress(reg, None, _on(dev, p1), _on(dev, p2), props)
            dc = (out["matches1"].cpu() - torch.from_numpy(g[tag + "_matches"])).abs().max().item()
            ds = (out["probs1"].cpu() - torch.from_numpy(g[tag + "_probs"])).abs().max().item()
            print(f"case R {tag} {name}: coord {dc:.3g} px score {ds:.3g}")
            assert dc <= rr.COORD_TOL and ds <= rr.SCORE_TOL
        with pytest.raises(NotImplementedError):
            generic.set_mode("f32")
        with pytest.raises(NotImplementedError):
            from patch2pix_amd import _lib
            _lib.check(_lib.p2p_regressor_set_mode(tuned.handle, _lib.REGRESS_GENERIC), "p2p_regressor_set_mode")


@pytest.mark.parametrize("case", ["A", "C"])
def test_outputs_do_not_depend_on_the_launch(case, dev):
    """A proposal's raw outputs, bit for bit: alone, inside a ragged 3-item batch with images of different sizes, through
    regress_batch_dev with a stride of 64 and counts (61, 0, 17), and with a workspace of one 8-proposal unit."""
    from patch2pix_amd import ops, _lib
    p1, p2, props = rr.inputs("gpu")
    mid, fine = _handles(case, dev)
    a1, a2, pd = _on(dev, p1), _on(dev, p2), props.to(dev)
    base = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
    # alone
    for i in (0, 17, 60):
        one = ops.regress(mid, fine, a1, a2, pd[i:i + 1], want_raw=True)
        assert torch.equal(one["raw1"][0], base["raw1"][i]) and torch.equal(one["raw2"][0], base["raw2"][i])
    # ragged batch: another pair of another size in front and behind
    q1, q2 = synthetic.make_pyramid(51, 64, 80), synthetic.make_pyramid(52, 64, 80)
    b1, b2 = _on(dev, q1), _on(dev, q2)
    small = torch.tensor([[5, 6, 70, 50], [40, 30, 41, 31], [79, 63, 0, 0]], dtype=torch.int64, device=dev)
    outs = ops.regress_batch(mid, fine, [b1, a1, b1], [b2, a2, b2], [small, pd, small[:2]], want_raw=True)
    for k in ("raw1", "raw2", "matches2", "probs2"):
        assert torch.equal(outs[1][k], base[k]), k
    assert torch.equal(outs[0]["raw2"][:2], outs[2]["raw2"])
    # device-side counts, stride 64: slots past the counts keep their sentinel
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
    # chunks of 8 against one chunk
    unit = _lib.p2p_regress_workspace_bytes_for(mid.handle, 8)
    assert _lib.p2p_regress_workspace_bytes_for(mid.handle, 61) == 8 * unit
    assert _lib.p2p_regress_workspace_bytes_for(mid.handle, 100000) == 32 * unit          # the cap of 256 proposals
    ops.generic_scratch_limit = unit
    try:
        chunked = ops.regress(mid, fine, a1, a2, pd, want_raw=True)
    finally:
        ops.generic_scratch_limit = None
    for k in base:
        assert torch.equal(chunked[k], base[k]), k
    # n = 0
    empty = ops.regress(mid, fine, a1, a2, pd[:0], want_raw=True)
    assert empty["matches2"].shape == (0, 4) and empty["probs2"].shape == (0,)


def test_mismatched_handles_are_refused(dev):
    from patch2pix_amd import ops
    p1, p2, props = rr.inputs("gpu")
    a1, a2, pd = _on(dev, p1), _on(dev, p2), props.to(dev)
    gen_r = ops.RegressorWeights(rr.sub_params(gu.state_dict(0), "regress_mid."), dev, generic=True)
    tuned = ops.RegressorWeights(rr.sub_params(gu.state_dict(0), "regress_fine."), dev)
    with pytest.raises(RuntimeError, match="generic and a tuned"):
        ops.regress(gen_r, tuned, a1, a2, pd[:4])
    with pytest.raises(RuntimeError, match="generic and a tuned"):
        ops.regress(tuned, gen_r, a1, a2, pd[:4])
    with pytest.raises(RuntimeError, match="different configurations"):
        ops.regress(_handles("A", dev)[0], _handles("C", dev)[0], a1, a2, pd[:4])


def test_non_released_checkpoint_end_to_end(dev, tmp_path):
    """Case C from a checkpoint FILE: load_model, refine_matches on an image pair against the restatement chain on the same
    pyramids, predict_fine_device == predict_fine_from_feats, and a GraphedMatcher replay."""
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    case = "C"
    path = str(tmp_path / "case_c.pth")
    torch.save(rr.checkpoint(case), path)
    net = model_helper.load_model(path, lprint=lambda *a: None)
    assert net.feat_idx == [0, 2] and net._weights()[1].generic
    assert set(net.state_dict()) >= {"regress_mid.conv.2.weight", "regress_fine.fc.3.bias"}
    assert tuple(net.state_dict()["regress_mid.conv.0.weight"].shape) == (128, 67, 3, 3)
    H, W = 96, 128
    a, b = synthetic.make_image_pair(7, H, W)
    norm = lambda x: (torch.from_numpy(x).permute(2, 0, 1).float() / 255.0 - 0.45)[None].to(dev) / 0.225
    ia, ib = norm(a), norm(b)
    gen = torch.Generator().manual_seed(3)
    coarse = torch.stack([torch.randint(0, W, (40,), generator=gen), torch.randint(0, H, (40,), generator=gen),
                          torch.randint(0, W, (40,), generator=gen), torch.randint(0, H, (40,), generator=gen)], dim=1)
    with torch.no_grad():
        f1, f2 = net._pyramids(ia, ib)
        fine, fscores, mid, mscores = net._fine_chain(f1, f2, [coarse.to(dev)])
        refined, scores, kept = net.refine_matches(ia, ib, coarse.numpy(), io_thres=0.0)
    out = {"matches1": mid[0], "probs1": mscores[0], "matches2": fine[0], "probs2": fscores[0]}
    # the restatement reads the checkpoint of the case: the same weights the file holds
    rr.check_levels(out, [t[0].cpu() for t in f1[:4]], [t[0].cpu() for t in f2[:4]], coarse, case, "end to end")
    # two backbone runs may differ in the last bits (the convolution library picks its algorithm per call): the bars, not bits
    assert np.abs(refined - fine[0].cpu().numpy()).max() <= rr.COORD_TOL and np.abs(scores - fscores[0].cpu().numpy()).max() <= rr.SCORE_TOL
    assert np.array_equal(kept, coarse.numpy())
    # the device path and its graph, on pyramids that give the coarse stage something to match
    p1, p2 = synthetic.make_correlated_pyramids(905, H, W)
    g1, g2 = [t[None].to(dev) for t in p1], [t[None].to(dev) for t in p2]
    fine_l, scores_l, coarse_l = net.predict_fine_from_feats(g1, g2, ksize=2)
    dfine, dscores, dcoarse = net.unpad(*net.predict_fine_device(g1, g2, ksize=2))
    assert coarse_l[0].shape[0] > 0
    assert torch.equal(dcoarse[0], coarse_l[0]) and torch.equal(dfine[0], fine_l[0]) and torch.equal(dscores[0], scores_l[0])
    gm = GraphedMatcher(net, H, W, with_backbone=False)
    gfine, gscores, gcoarse = gm(g1, g2)
    assert torch.equal(gcoarse[0], coarse_l[0]) and torch.equal(gfine[0], fine_l[0]) and torch.equal(gscores[0], scores_l[0])
