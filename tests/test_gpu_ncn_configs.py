"""The generic consensus net on the GPU, through the real library: every case x volume of tests/ncn_reference.py against the
fp64 restatement and the reference's golden, bit-identity under batching and workspace size, the released stack through the
generic handle beside the tuned kernel in the coarse stage, and checkpoints with non-released stacks end to end (NC-only
through load_model / predict_coarse; a Patch2Pix one through predict_fine and a GraphedMatcher replay)."""
import copy

import pytest
import torch

import ncn_reference as nr
import regressor_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_handles = {}


def _handle(case, dev):
    from patch2pix_amd import ops
    if case not in _handles:
        h = ops.NcnWeights.from_state_dict(nr.weights(case), dev, symmetric_mode=nr.CASES[case]["symmetric_mode"], generic=True)
        assert h.generic and h.layout == nr.CASES[case]
        _handles[case] = h
    return _handles[case]


@pytest.mark.parametrize("vol", list(nr.VOLUMES))
@pytest.mark.parametrize("case", list(nr.CASES))
def test_cases_against_fp64_and_golden(case, vol, dev):
    from patch2pix_amd import ops
    x, y64 = nr.expected(case, vol)
    y = ops.neigh_consensus_batch(x.to(dev), _handle(case, dev)).cpu()
    nr.check(y, case, vol, "gpu")
    g = torch.from_numpy(nr.load_golden(case)[f"y_{vol}"])
    scale = y64.abs().max().item()
    err = (y - g).abs().max().item()
    print(f"case {case} volume {vol} against the golden: {err:.3g}, bar {nr.BAR_GOLDEN * nr.REF_ERR[case] * scale:.3g}")
    assert err <= nr.BAR_GOLDEN * nr.REF_ERR[case] * scale


@pytest.mark.parametrize("case", list(nr.CASES))
def test_a_volume_does_not_depend_on_the_launch(case, dev):
    """Pair 1 of the batch of 3: alone, and with a workspace of one volume (three groups) handed to the C entry point, bit for
    bit."""
    from patch2pix_amd import ops, _lib
    h = _handle(case, dev)
    x = nr.expected(case, "big")[0].to(dev)
    full = ops.neigh_consensus_batch(x, h)
    alone = ops.neigh_consensus_batch(x[1:2], h)
    per = _lib.p2p_neigh_consensus_workspace_bytes(h.handle, *x.shape[1:])
    ws = torch.empty(per, dtype=torch.uint8, device=dev)
    chunked = torch.full_like(x, float("nan"))
    _lib.check(_lib.p2p_neigh_consensus_batch(x.data_ptr(), x.shape[0], *x.shape[1:], h.handle, chunked.data_ptr(), ws.data_ptr(),
                                              per, ops._stream()), "p2p_neigh_consensus_batch")
    assert torch.equal(alone[0], full[1]) and torch.equal(chunked, full)


def test_generic_handle_kinds(dev):
    from patch2pix_amd import ops, _lib
    sd = nr.weights("R")
    tuned = ops.NcnWeights.from_state_dict(sd, dev)
    assert not tuned.generic and _lib.p2p_ncn_is_generic(tuned.handle) == 0 and tuned.layout == ops.RELEASED_NCN_LAYOUT
    tuned.set_tile(0, 5, 8)
    gen = _handle("R", dev)
    assert _lib.p2p_ncn_is_generic(gen.handle) == 1
    with pytest.raises(NotImplementedError):
        gen.set_tile(0, 5, 8)
    with pytest.raises(NotImplementedError):
        _lib.check(_lib.p2p_ncn_set_tile(gen.handle, 0, 5, 8), "p2p_ncn_set_tile")
    one_branch = ops.NcnWeights.from_state_dict(sd, dev, symmetric_mode=False)          # released shapes, not the released stack
    assert one_branch.generic and not one_branch.layout["symmetric_mode"]
    assert _lib.p2p_neigh_consensus_workspace_bytes(tuned.handle, 6, 7, 5, 8) == 4
    assert _lib.p2p_coarse_workspace_bytes_for(tuned.handle, 256, 8, 12, 8, 12, 2) == _lib.p2p_coarse_workspace_bytes(256, 8, 12, 8, 12, 2)
    assert _lib.p2p_coarse_workspace_bytes_for(gen.handle, 256, 8, 12, 8, 12, 2) > _lib.p2p_coarse_workspace_bytes(256, 8, 12, 8, 12, 2)
    x = nr.expected("M", "big")[0].to(dev)
    m_sym = ops.NcnWeights.from_state_dict(nr.weights("M"), dev, symmetric_mode=True)
    assert not torch.equal(ops.neigh_consensus_batch(x, m_sym), ops.neigh_consensus_batch(x, _handle("M", dev)))


@pytest.mark.parametrize("ksize,sides", [(1, (6, 8, 8, 6)), (2, (12, 16, 16, 12))])
def test_released_stack_generic_beside_tuned_in_the_coarse_stage(ksize, sides, dev):
    """ops.coarse_forward_batch on 48x64-pixel features (6x8 cells; at ksize 2 twice the side): the two handles agree within the
    sum of both bars and extract the same match rows wherever the fp64 pipeline's top-two gap exceeds twice the bar."""
    from patch2pix_amd import ops
    sd, lay = nr.weights("R"), nr.CASES["R"]
    fa, fb = nr.features(nr.COARSE_SEEDS[ksize], (2,) + sides, channels=32, shift=nr.COARSE_SHIFT)
    tuned = ops.NcnWeights.from_state_dict(sd, dev)
    cg, dg = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), ksize, _handle("R", dev))
    ct, dt = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), ksize, tuned)
    assert dg is None or torch.equal(dg, dt)
    mg, _ = ops.coarse_matches_batch(cg, dg, ksize, 8)
    mt, _ = ops.coarse_matches_batch(ct, dt, ksize, 8)
    left_out = total = 0
    for b in range(2):
        corr64, y64, _ = nr.pipeline(fa[b], fb[b], ksize, sd, lay)
        both = nr.handles_bar("R", y64)
        diff = (cg[b] - ct[b]).abs().max().item()
        print(f"ksize {ksize} pair {b}: generic - tuned {diff:.3g}, sum of bars {both:.3g}")
        assert diff <= both
        ok = nr.decidable(corr64, nr.coarse_bar("R", y64))
        assert torch.equal(mg[b].cpu()[ok], mt[b].cpu()[ok])
        left_out += int((~ok).sum())
        total += ok.numel()
    assert left_out <= nr.UNDECIDED_CAP * total


def _images(dev, seed, H, W):
    a, b = synthetic.make_image_pair(seed, H, W)
    norm = lambda x: (torch.from_numpy(x).permute(2, 0, 1).float() / 255.0 - 0.45)[None].to(dev) / 0.225
    return norm(a), norm(b)


def test_nc_only_checkpoint_of_the_default_stack(dev):
    """Layout N as an NC-only checkpoint (a bare state_dict) through load_model(method='nc') -> predict_coarse, against the
    fp64 pipeline on the library's own layer-3 features: the best cell of every decidable row, the rows left out under the
    cap.  predict_coarse returns the distinct rows in sorted order (filter_coarse merges a B->A and an A->B match of the
    same two cells), so the per-cell check reads the unfiltered list of the same forward pass and predict_coarse must
    return exactly its distinct rows."""
    from patch2pix_amd.utils.eval import model_helper
    sd = {k: v for k, v in rr.checkpoint("R")["state_dict"].items() if k.startswith("extract.")}
    sd.update({"ncn." + k: v for k, v in nr.weights("N").items()})
    net = model_helper.load_model({"state_dict": sd}, method="nc", lprint=lambda *a: None)
    assert net._ncn_layout == nr.CASES["N"] and net._weights()[0].generic
    assert tuple(net.state_dict()["ncn.conv.2.weight"].shape) == (3, 10, 10, 3, 3, 3) and "ncn.conv.4.bias" in net.state_dict()
    H, W, ksize = 64, 96, 2
    ia, ib = _images(dev, nr.NC_IMAGE_SEED, H, W)
    with torch.no_grad():
        rows, scores = net.predict_coarse(ia, ib, ksize=ksize, ncn_thres=0.0, mutual=False)
        f1, f2 = net._pyramids(ia, ib)
        raw, raw_scores = net.cal_coarse_matches(*net.forward_coarse_match(f1[-1], f2[-1], ksize=ksize), ksize=ksize,
                                                 upsample=net.upsample)
    corr64, y64, _ = nr.pipeline(f1[-1][0].cpu(), f2[-1][0].cpu(), ksize, nr.weights("N"), nr.CASES["N"])
    ha, wa, hb, wb = corr64.shape
    assert raw[0].shape == (ha * wa + hb * wb, 4) and bool((raw_scores[0] > 0).all())
    assert torch.equal(rows[0].cpu(), torch.unique(raw[0].cpu(), dim=0)) and bool((scores[0] > 0).all())
    cell = raw[0].cpu() // net.upsample // ksize                           # (xA, yA, xB, yB) -> pooled cells
    got = torch.cat([cell[:hb * wb, 1] * wa + cell[:hb * wb, 0], cell[hb * wb:, 3] * wb + cell[hb * wb:, 2]])
    bar = nr.coarse_bar("N", y64) + nr.CORR_RTOL * corr64.abs().max().item()
    ok = nr.decidable(corr64, bar)
    want = nr.best_cells(corr64)[0]
    print(f"NC-only N: {int(ok.sum())} of {ok.numel()} rows decidable at bar {bar:.3g}")
    assert int((~ok).sum()) <= nr.UNDECIDED_CAP * ok.numel()
    assert torch.equal(got[ok], want[ok])


def test_patch2pix_checkpoint_over_the_pf_pascal_stack(dev):
    """Layout P with the released regressors: load_model infers the stack from the checkpoint's shapes; predict_fine against the
    fine-level restatement fed with the library's own proposals; one GraphedMatcher replay equals the eager result."""
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    ck = copy.copy(rr.checkpoint("R"))
    ck["regressor_config"] = copy.deepcopy(ck["regressor_config"])
    ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if not k.startswith("ncn.")}
    ck["state_dict"].update({"ncn." + k: v for k, v in nr.weights("P").items()})
    net = model_helper.load_model(ck, lprint=lambda *a: None)
    assert net._ncn_layout == nr.CASES["P"] and net._weights()[0].generic and not net._weights()[1].generic
    assert tuple(net.state_dict()["ncn.conv.2.weight"].shape) == (5, 16, 16, 5, 5, 5)
    H, W = 64, 96
    ia, ib = _images(dev, 12, H, W)
    with torch.no_grad():
        f1, f2 = net._pyramids(ia, ib)
        fine, fscores, mid, mscores, coarse = net.predict_fine_from_feats(f1, f2, ksize=2, return_all=True)
    assert coarse[0].shape[0] > 0
    out = {"matches1": mid[0], "probs1": mscores[0], "matches2": fine[0], "probs2": fscores[0]}
    rr.check_levels(out, [t[0].cpu() for t in f1[:4]], [t[0].cpu() for t in f2[:4]], coarse[0].cpu(), "R", "stack P end to end")
    with torch.no_grad():
        dfine, dscores, dcoarse = net.unpad(*net.predict_fine_device(f1, f2, ksize=2))
        gm = GraphedMatcher(net, H, W, with_backbone=False)
        gfine, gscores, gcoarse = gm(f1, f2)
    assert torch.equal(dcoarse[0], coarse[0])
    assert torch.equal(gcoarse[0], dcoarse[0]) and torch.equal(gfine[0], dfine[0]) and torch.equal(gscores[0], dscores[0])
