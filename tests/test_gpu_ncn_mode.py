"""P2P_COARSE_GENERIC_FP16X2 on the GPU, through the real library: every case x volume of tests/ncn_mode_reference.py against the
fp64 restatement and the reference's fp32 outputs per pair, the single-layer case and the default mode's bits, invariance under
batching and workspace size, the mixed-magnitude batch, the range variants, the released stack forced generic in the mode beside
the tuned kernel in the coarse stage, and a Patch2Pix checkpoint over the PF-Pascal stack with set_coarse_mode('generic_fp16x2')
(decidable rows, load_state_dict, GraphedMatcher)."""
import copy

import pytest
import torch

import ncn_mode_reference as nm
import ncn_reference as nr
import regressor_reference as rr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_handles = {}


def _handle(case, dev, mode, variant=None):
    from patch2pix_amd import ops
    key = (case, variant)
    if key not in _handles:
        _handles[key] = ops.NcnWeights.from_state_dict(nm.weights(case, variant), dev, symmetric_mode=nr.CASES[case]["symmetric_mode"], generic=True)
    _handles[key].set_mode(mode)
    return _handles[key]


def _run(x, h, dev):
    from patch2pix_amd import ops
    return ops.neigh_consensus_batch(x.to(dev), h).cpu()


@pytest.mark.parametrize("vol", list(nm.VOLUMES))
@pytest.mark.parametrize("case", list(nr.CASES))
def test_cases_against_fp64_and_golden(case, vol, dev):
    x, y64 = nm.expected(case, vol)
    h = _handle(case, dev, "generic_fp16x2")
    assert h.mode == "generic_fp16x2"
    y = _run(x, h, dev)
    nm.check_pairs(y, y64, case, vol, "gpu fp16x2")
    g = torch.from_numpy(nm.load_golden(case)[f"y_{vol}"] if vol == nm.TILE else nr.load_golden(case)[f"y_{vol}"])
    nm.check_pairs(y, y64, case, vol, "gpu fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=g)


@pytest.mark.parametrize("case", ["S", "N", "P"])
def test_default_bits_and_the_two_modes(case, dev):
    """Mode 17 -> 0 gives the default's earlier bits; the single-layer stack computes the same bits in both modes, a multi-layer one
    different bits within nr.handles_bar per pair."""
    x, y64 = nm.expected(case, nm.TILE)
    before = _run(x, _handle(case, dev, "generic"), dev)
    h2 = _run(x, _handle(case, dev, "generic_fp16x2"), dev)
    after = _run(x, _handle(case, dev, "generic"), dev)
    assert torch.equal(before, after)
    if case == "S":
        assert torch.equal(before, h2)
        return
    assert not torch.equal(before, h2)
    for z, bar in enumerate(nm.handles_bar_pairs(case, y64)):
        diff = (before[z] - h2[z]).abs().max().item()
        print(f"case {case} pair {z}: generic - generic_fp16x2 {diff:.3g}, bar {bar:.3g}")
        assert diff <= bar


@pytest.mark.parametrize("case", ["R", "N", "P", "M"])
def test_a_pair_does_not_depend_on_the_launch(case, dev):
    from patch2pix_amd import ops, _lib
    h = _handle(case, dev, "generic_fp16x2")
    x = nm.expected(case, "big")[0].to(dev)
    full = ops.neigh_consensus_batch(x, h)
    alone = ops.neigh_consensus_batch(x[1:2], h)
    moved = ops.neigh_consensus_batch(torch.stack([x[1], x[0]]), h)
    per = _lib.p2p_neigh_consensus_workspace_bytes(h.handle, *x.shape[1:])
    ws = torch.empty(per, dtype=torch.uint8, device=dev)
    chunked = torch.full_like(x, float("nan"))
    _lib.check(_lib.p2p_neigh_consensus_batch(x.data_ptr(), x.shape[0], *x.shape[1:], h.handle, chunked.data_ptr(), ws.data_ptr(),
                                              per, ops._stream()), "p2p_neigh_consensus_batch")
    assert torch.equal(alone[0], full[1]) and torch.equal(chunked, full) and torch.equal(moved[0], full[1]) and torch.equal(moved[1], full[0])
    assert _lib.p2p_neigh_consensus_batch(x.data_ptr(), x.shape[0], *x.shape[1:], h.handle, chunked.data_ptr(), ws.data_ptr(),
                                          per - 1, ops._stream()) == nm.ENOMEM


@pytest.mark.parametrize("case", nm.HIDDEN_CASES)
def test_mixed_magnitude_batch(case, dev):
    x, y64 = nm.mixed(case)
    y = _run(x, _handle(case, dev, "generic_fp16x2"), dev)
    nm.check_pairs(y, y64, case, "mixed", "gpu fp16x2")
    nm.check_pairs(y, y64, case, "mixed", "gpu fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=torch.from_numpy(nm.load_golden(case)["y_mixed"]))


def test_zero_and_inf_pairs(dev):
    case = "N"
    h = _handle(case, dev, "generic_fp16x2")
    x = nm.expected(case, "big")[0].clone()
    base = _run(x, h, dev)
    x[1] = 0.0
    y = _run(x, h, dev)
    y64 = nr.restate(x, nr.weights(case), nr.CASES[case])
    assert torch.isfinite(y).all() and torch.equal(y[0], base[0]) and torch.equal(y[2], base[2])
    assert (y[1].double() - y64[1]).abs().max().item() <= nr.BAR_F64 * nr.REF_ERR[case] * max(y64[1].abs().max().item(), 1e-30)
    x[1, 2, 3, 1, 4] = float("inf")        # what the inf does inside its own pair: tests/test_ncn_mode_emulated.py
    y = _run(x, h, dev)
    assert torch.equal(y[0], base[0]) and torch.equal(y[2], base[2])


@pytest.mark.parametrize("vol", ["big", nm.TILE])
@pytest.mark.parametrize("variant", nm.VARIANTS)
@pytest.mark.parametrize("case", nm.HIDDEN_CASES)
def test_range_variants(case, variant, vol, dev):
    x, y64 = nm.expected(case, vol, variant)
    key = nm.input_key(vol, variant)
    y = _run(x, _handle(case, dev, "generic_fp16x2", variant), dev)
    nm.check_pairs(y, y64, case, key, "gpu fp16x2")
    nm.check_pairs(y, y64, case, key, "gpu fp16x2 against the golden", bar=nr.BAR_GOLDEN, ref=torch.from_numpy(nm.load_golden(case)[f"y_{key}"]))


@pytest.mark.parametrize("ksize,sides", [(1, (6, 8, 8, 6)), (2, (12, 16, 16, 12))])
def test_released_stack_generic_fp16x2_beside_tuned_in_the_coarse_stage(ksize, sides, dev):
    """The sizes and seeds of test_released_stack_generic_beside_tuned_in_the_coarse_stage (tests/test_gpu_ncn_configs.py)."""
    from patch2pix_amd import ops
    sd, lay = nr.weights("R"), nr.CASES["R"]
    fa, fb = nr.features(nr.COARSE_SEEDS[ksize], (2,) + sides, channels=32, shift=nr.COARSE_SHIFT)
    tuned = ops.NcnWeights.from_state_dict(sd, dev)
    cg, dg = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), ksize, _handle("R", dev, "generic_fp16x2"))
    ct, dt = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), ksize, tuned)
    assert dg is None or torch.equal(dg, dt)
    mg, _ = ops.coarse_matches_batch(cg, dg, ksize, 8)
    mt, _ = ops.coarse_matches_batch(ct, dt, ksize, 8)
    left_out = total = 0
    for b in range(2):
        corr64, y64, _ = nr.pipeline(fa[b], fb[b], ksize, sd, lay)
        both = nr.handles_bar("R", y64)
        diff = (cg[b] - ct[b]).abs().max().item()
        print(f"ksize {ksize} pair {b}: generic_fp16x2 - tuned {diff:.3g}, sum of bars {both:.3g}")
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


def test_patch2pix_checkpoint_over_the_pf_pascal_stack_in_the_mode(dev):
    """The checkpoint, size (64 x 96, ksize 2) and image seed of test_patch2pix_checkpoint_over_the_pf_pascal_stack: with
    set_coarse_mode('generic_fp16x2') every decidable row of the coarse matches names the fp64 pipeline's winner on the library's own
    features, the undecidable share stays under nr.UNDECIDED_CAP, the mode survives load_state_dict, and a GraphedMatcher captured
    after the choice equals the eager result."""
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    ck = copy.copy(rr.checkpoint("R"))
    ck["regressor_config"] = copy.deepcopy(ck["regressor_config"])
    ck["state_dict"] = {k: v for k, v in ck["state_dict"].items() if not k.startswith("ncn.")}
    ck["state_dict"].update({"ncn." + k: v for k, v in nr.weights("P").items()})
    net = model_helper.load_model(ck, lprint=lambda *a: None)
    assert net._ncn_layout == nr.CASES["P"] and net._weights()[0].generic
    with pytest.raises(NotImplementedError):
        net.set_coarse_mode("fp16")
    with pytest.raises(ValueError):
        net.set_coarse_mode("half")
    net.set_coarse_mode("generic_fp16x2")
    assert net.coarse_mode == "generic_fp16x2" and net._weights()[0].mode == "generic_fp16x2"
    net.load_state_dict(net.state_dict())
    assert net._packed is None and net._weights()[0].mode == "generic_fp16x2" and net.coarse_mode == "generic_fp16x2"
    H, W, ksize = 64, 96, 2
    ia, ib = _images(dev, 12, H, W)
    with torch.no_grad():
        f1, f2 = net._pyramids(ia, ib)
        raw, _ = net.cal_coarse_matches(*net.forward_coarse_match(f1[-1], f2[-1], ksize=ksize), ksize=ksize, upsample=net.upsample)
    corr64, y64, _ = nr.pipeline(f1[-1][0].cpu(), f2[-1][0].cpu(), ksize, nr.weights("P"), nr.CASES["P"])
    ha, wa, hb, wb = corr64.shape
    cell = raw[0].cpu() // net.upsample // ksize                           # (xA, yA, xB, yB) -> pooled cells
    got = torch.cat([cell[:hb * wb, 1] * wa + cell[:hb * wb, 0], cell[hb * wb:, 3] * wb + cell[hb * wb:, 2]])
    bar = nr.coarse_bar("P", y64) + nr.CORR_RTOL * corr64.abs().max().item()
    ok = nr.decidable(corr64, bar)
    print(f"stack P in generic_fp16x2: {int(ok.sum())} of {ok.numel()} rows decidable at bar {bar:.3g}")
    assert int((~ok).sum()) <= nr.UNDECIDED_CAP * ok.numel()
    assert torch.equal(got[ok], nr.best_cells(corr64)[0][ok])
    with torch.no_grad():
        dfine, dscores, dcoarse = net.unpad(*net.predict_fine_device(f1, f2, ksize=2))
        gm = GraphedMatcher(net, H, W, with_backbone=False)
        gfine, gscores, gcoarse = gm(f1, f2)
    assert dcoarse[0].shape[0] > 0
    assert torch.equal(gcoarse[0], dcoarse[0]) and torch.equal(gfine[0], dfine[0]) and torch.equal(gscores[0], dscores[0])
