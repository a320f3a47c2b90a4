"""Mode 'fp16' (P2P_REGRESS_FP16) on the MI355X: the case table of tests/fast_mode_reference.py through the real library against
the model's bars, the launch invariants by bytes, predict_fine in all four modes, and a GraphedMatcher replay."""
import pytest
import torch

import fast_mode_reference as fm
import golden_util as gu
import range_reference as rr
from oracle import p2p_oracle as orc
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from patch2pix_amd import ops
    return ops


def _weights(ops, sd, dev, mode=fm.MODE):
    mid = ops.RegressorWeights(fm.sub_sd(sd, "regress_mid."), dev)
    fine = ops.RegressorWeights(fm.sub_sd(sd, "regress_fine."), dev)
    mid.set_mode(mode)
    fine.set_mode(mode)
    return mid, fine


def _run(ops, w, p1, p2, props, dev):
    out = ops.regress(w[0], w[1], [t.to(dev) for t in p1[:4]], [t.to(dev) for t in p2[:4]], props.to(dev), want_mid=True, want_raw=True)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_mode_is_selectable(ops, dev):
    mid, _ = _weights(ops, gu.state_dict(0), dev, "fp16x2w")
    assert mid.mode == "fp16x2w"
    mid.set_mode("fp16")
    assert mid.mode == "fp16"
    with pytest.raises(ValueError, match="fp16"):
        mid.set_mode("fp8")


@pytest.mark.parametrize("name", list(fm.CASES))
def test_case_table_within_the_model(name, ops, dev):
    sd, p1, p2, props = fm.case_inputs(name)
    out = _run(ops, _weights(ops, sd, dev), p1, p2, props, dev)
    res = rr.measure(out, sd, p1, p2, props, with_f32=True)
    coord_bar, score_bar, score_b, p64 = fm.bounds(sd, p1, p2, props, out["matches1"])
    with torch.no_grad():
        p32 = orc.fine_level(p1, p2, out["matches1"], orc.split_params(sd)[2])[1]
    nflip, cap = fm.flips(out["probs2"], p64), fm.flip_cap(p32, p64, score_b)
    print(f"\nfp16[MI355X] {name:>20s}: coord {res['coord']:.2e} px (model {coord_bar:.2e})  score {res['score']:.2e} "
          f"(model {score_bar:.2e})  | fp32 oracle {res['o32_coord']:.2e} px {res['o32_score']:.2e} | io_thres flips {nflip} (cap {cap})")
    assert res["coord"] <= coord_bar and res["score"] <= score_bar, res
    assert nflip <= cap


@pytest.mark.parametrize("tag", ["int_mid", "float_fine"])
def test_against_the_reference_golden(tag, ops, dev):
    """The reference's own fp32 outputs (fine_48x64.npz): mode fp16 within the model's per-proposal bound of them, and the side
    of io_thres against the golden's scores (cap: the proposals whose score lies within the bound of the threshold)."""
    golden = fm.golden_level(tag, 8)
    p1, p2, props, gm, gp, par = golden
    w = _weights(ops, gu.state_dict(0), dev)[0 if tag == "int_mid" else 1]
    out = ops.regress(w, None, [t.to(dev) for t in p1], [t.to(dev) for t in p2], props.to(dev), want_raw=True)
    torch.cuda.synchronize()
    fm.assert_against_golden(tag, out["matches1"].cpu(), out["probs1"].cpu(), golden, "MI355X")
    sb = fm.level_bounds(par, p1, p2, props)[1] + rr.SCORE_TOL
    assert fm.flips(out["probs1"].cpu(), gp.double()) <= int(((gp.double() - fm.IO_THRES).abs() <= sb).sum())


def test_more_proposals_than_a_chunk(ops, dev):
    """Chunks are cut from the proposal count (whole units of 256, at most 3328): 3403 proposals run as [0, 1792) + [1792, 3403),
    the half-size U buffer is reused by the second round and its last row block is partly filled; 3329 is the smallest two-chunk
    call.  Every proposal's bytes are those of a small launch of its own; then more items than a launch holds AND more
    proposals than a chunk in the first launch (tests/test_gpu_parity.py has the same call for the other modes)."""
    sd = gu.state_dict(0)
    w = _weights(ops, sd, dev)
    H, W = 48, 64
    g = torch.Generator().manual_seed(12)
    rnd = lambda c: torch.stack([torch.randint(0, W + 1, (c,), generator=g), torch.randint(0, H + 1, (c,), generator=g),
                                 torch.randint(0, W + 1, (c,), generator=g), torch.randint(0, H + 1, (c,), generator=g)], 1).to(dev)
    pyr = lambda seed: [t.to(dev) for t in synthetic.make_pyramid(seed, H, W)[:4]]
    p1, p2, props = pyr(500), pyr(600), rnd(3403)
    keys = ("matches1", "probs1", "matches2", "probs2")
    full = ops.regress(w[0], w[1], p1, p2, props)
    for n in (3329, 3403):
        out = full if n == 3403 else ops.regress(w[0], w[1], p1, p2, props[:n].contiguous())
        for k in keys:
            assert bool(torch.isfinite(out[k]).all()), (n, k)
            assert torch.equal(out[k], full[k][:n]), (n, k)
    for lo, hi in ((0, 9), (1785, 1800), (3320, 3336), (3395, 3403)):          # around both chunk edges, and the partly filled last block
        part = ops.regress(w[0], w[1], p1, p2, props[lo:hi].contiguous())
        for k in keys:
            assert torch.equal(part[k], full[k][lo:hi]), (lo, hi, k)
    counts = [1500, 1500] + [40] * 16
    pyr1, pyr2 = [pyr(500 + i) for i in range(18)], [pyr(600 + i) for i in range(18)]
    plist = [rnd(c) for c in counts]
    outs = ops.regress_batch(w[0], w[1], pyr1, pyr2, plist)
    for i in (0, 1, 2, 15, 16, 17):
        single = ops.regress(w[0], w[1], pyr1[i], pyr2[i], plist[i])
        for k in keys:
            assert torch.equal(outs[i][k], single[k]), (i, k)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, rows_a, rows_b, what):
    for k in ("matches1", "probs1", "raw1", "matches2", "probs2", "raw2"):
        assert torch.equal(_bits(a[k])[rows_a], _bits(b[k])[rows_b]), f"{what}: {k}"


@pytest.fixture(scope="module")
def big(ops, dev):
    """17 proposals (four on image corners) on a 64 x 96 pair, both levels; and the same on an unrounded 100 x 140 pair."""
    sd = gu.state_dict(0)
    w = _weights(ops, sd, dev)
    res = {}
    for hh, ww in ((64, 96), (100, 140)):
        p1, p2 = fm.unrounded_pair(hh, ww) if hh % 8 else (synthetic.make_pyramid(7, hh, ww)[:4], synthetic.make_pyramid(8, hh, ww)[:4])
        props = rr.proposals(hh, ww, 17)
        props[3] = torch.tensor([ww, 0, 0, hh])
        props[4] = torch.tensor([0, hh, ww, 0])
        props[5] = torch.tensor([ww, hh, 0, 0])
        res[(hh, ww)] = (p1, p2, props, _run(ops, w, p1, p2, props, dev))
    return sd, w, res


@pytest.mark.parametrize("size", [(64, 96), (100, 140)])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_alone_and_in_batches(n, size, big, ops, dev):
    sd, w, res = big
    p1, p2, props, ref = res[size]
    for lo in ((0, 3, 5, 16) if n == 1 else (0, 17 - n)):
        out = _run(ops, w, p1, p2, props[lo:lo + n], dev)
        _same(out, ref, slice(0, n), slice(lo, lo + n), f"{size}: proposals [{lo}, {lo + n})")
    assert bool(torch.isfinite(ref["raw2"]).all())


def test_accuracy_of_the_unrounded_pair(big):
    sd, w, res = big
    p1, p2, props, ref = res[(100, 140)]
    sub = slice(3, 6)                                           # the corner proposals: clamped border patches
    out = {k: v[sub] for k, v in ref.items()}
    r = rr.measure(out, sd, p1, p2, props[sub])
    cb, sb, _, _ = fm.bounds(sd, p1, p2, props[sub], out["matches1"])
    assert r["coord"] <= cb and r["score"] <= sb, (r, cb, sb)


def test_device_counts_with_an_empty_item_and_a_poisoned_workspace(big, ops, dev):
    """Device-side counts (7, 0, 9 of stride 9) leave the bytes of the host-count launches and do not touch empty slots; the
    launch of ops.regress_batch_dev sizes its workspace with the mode's own query."""
    sd, w, res = big
    p1, p2, props, ref = res[(64, 96)]
    g = lambda p: [t.to(dev) for t in p]
    stride = 9
    slots = torch.zeros(3, stride, 4, dtype=torch.int64)
    slots[0, :7], slots[2, :9] = props[:7], props[8:17]
    counts = torch.tensor([7, 0, 9], dtype=torch.int32, device=dev)
    mark = 4242.0
    bufs = {k: torch.full((3, stride, c) if c > 1 else (3, stride), mark, device=dev)
            for k, c in (("matches1", 4), ("probs1", 1), ("matches2", 4), ("probs2", 1))}
    out = ops.regress_batch_dev(w[0], w[1], [g(p1)] * 3, [g(p2)] * 3, slots.to(dev), counts, out=bufs)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    for k in ("matches1", "probs1", "matches2", "probs2"):
        assert torch.equal(_bits(out[k][0, :7]), _bits(ref[k][:7])) and torch.equal(_bits(out[k][2, :9]), _bits(ref[k][8:17])), k
        assert bool((out[k][1] == mark).all()) and bool((out[k][0, 7:] == mark).all()), f"{k}: an empty slot was written"


def test_exact_poisoned_workspace(big, ops, dev):
    """p2p_regress_batch with a NaN-filled workspace of exactly p2p_regress_workspace_bytes_mode bytes and a guard behind it."""
    import ctypes
    from patch2pix_amd import _lib
    sd, w, res = big
    p1, p2, props, ref = res[(64, 96)]
    n = 9
    need = _lib.p2p_regress_workspace_bytes_mode(n, fm.MODE_ID)
    assert 0 < need <= _lib.p2p_regress_workspace_bytes_mode(n, 4)
    ws = torch.full((need // 4 + 64,), float("nan"), device=dev)
    lv = [[t.to(dev).contiguous() for t in p] for p in (p1, p2)]
    pyr = []
    for levels in lv:
        q = _lib.Pyramid()
        for j in range(4):
            q.level[j] = levels[j].data_ptr()
        q.height, q.width = levels[0].shape[-2:]
        pyr.append((_lib.Pyramid * 1)(q))
    o = {k: torch.full((n, c) if c > 1 else (n,), float("nan"), device=dev)
         for k, c in (("matches1", 4), ("probs1", 1), ("raw1", 5), ("matches2", 4), ("probs2", 1), ("raw2", 5))}
    pr = props[:n].to(dev).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    st = _lib.p2p_regress_batch(w[0].handle, w[1].handle, 1, pyr[0], pyr[1], (ctypes.c_int * 1)(n), pr.data_ptr(), 0,
                                o["matches1"].data_ptr(), o["probs1"].data_ptr(), o["raw1"].data_ptr(),
                                o["matches2"].data_ptr(), o["probs2"].data_ptr(), o["raw2"].data_ptr(), ws.data_ptr(), need, stream)
    assert st == 0, _lib.p2p_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need // 4:]).all()), "the launch wrote behind the queried size"
    _same({k: v.cpu() for k, v in o.items()}, ref, slice(0, n), slice(0, n), "a poisoned workspace of exactly the queried size")


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


def test_predict_fine_in_all_four_modes(net, dev):
    """128 x 160 synthetic pair end to end: the fp32-equivalent modes agree at the project's bars, 'fp16' lies within the model's
    bar of 'f32' (both evaluations are within their own bound of fp64: the model's bar plus the bars of the fp32 modes)."""
    a, b = synthetic.make_image_pair(5, 128, 160)
    norm = lambda x: (torch.from_numpy(x).permute(2, 0, 1).float() / 255.0 - 0.45)[None].to(dev) / 0.225
    ia, ib = norm(a), norm(b)
    _, mid, fine = net._weights()
    got = {}
    try:
        for mode in ("f32", "fp16x2", "fp16x2w", "fp16"):
            mid.set_mode(mode)
            fine.set_mode(mode)
            assert mid.mode == mode
            with torch.no_grad():
                got[mode] = [t[0].cpu() for t in net.predict_fine(ia, ib, ksize=2, return_all=True)]      # fine, scores, mid, mid scores, coarse
    finally:
        mid.set_mode("fp16x2w")
        fine.set_mode("fp16x2w")
    ref = got["f32"]
    nrow = min(12, ref[0].shape[0])
    assert nrow > 0
    # the bars are derived for THESE inputs: the model's per-proposal bounds on the pyramids the backbone made, the mid level at
    # the coarse matches, the fine level at mode f32's mid matches, for the first rows; plus twice the fp32 floor (both modes)
    with torch.no_grad():
        feats1, feats2 = net._pyramids(ia, ib)
    p1, p2 = [t[0].cpu() for t in feats1[:4]], [t[0].cpu() for t in feats2[:4]]
    mid_p, fine_p = rr.params64(synthetic.make_checkpoint(0)["state_dict"])
    cb_mid, sb_mid, _ = fm.level_bounds(mid_p, p1, p2, ref[4][:nrow].double())
    cb_fine, sb_fine, _ = fm.level_bounds(fine_p, p1, p2, ref[2][:nrow].double())
    zero = torch.zeros(nrow, dtype=torch.float64)
    for mode, bars in (("fp16x2", (zero, zero, zero, zero)), ("fp16x2w", (zero, zero, zero, zero)), ("fp16", (cb_mid, sb_mid, cb_fine, sb_fine))):
        fine_m, fine_s, mid_m, mid_s, coarse = got[mode]
        assert torch.equal(coarse, ref[4]), f"{mode}: the coarse matches differ"
        dm, dms = (mid_m - ref[2]).abs().amax(1).double(), (mid_s - ref[3]).abs().double()
        df, dfs = (fine_m - ref[0]).abs().amax(1).double(), (fine_s - ref[1]).abs().double()
        # a mid match on the other side of an integer moves the whole fine patch (networks/utils.py:19): the fine level is compared
        # where both modes regressed the same patch, and a row that did not must have a mid coordinate within its bound of an integer
        same = (mid_m.long() == ref[2].long()).all(1)
        print(f"\npredict_fine[MI355X] {mode:>8s} vs f32: mid {dm.max().item():.2e} px {dms.max().item():.2e}  fine {df[same].max().item():.2e} px "
              f"{dfs[same].max().item():.2e}  ({int(same.sum())} of {same.numel()} matches on the same fine patch)")
        r = slice(0, nrow)
        assert bool((dm[r] <= bars[0] + 2 * rr.COORD_TOL).all()) and bool((dms[r] <= bars[1] + 2 * rr.SCORE_TOL).all()), (mode, dm[r], bars[0])
        ok = same[r]
        assert bool((df[r][ok] <= bars[2][ok] + 2 * rr.COORD_TOL).all()) and bool((dfs[r][ok] <= bars[3][ok] + 2 * rr.SCORE_TOL).all()), (mode, df[r], bars[2])
        to_int = (ref[2][r] - ref[2][r].round()).abs().amin(1).double()
        assert bool((to_int[~ok] <= bars[0][~ok] + 2 * rr.COORD_TOL).all()), f"{mode}: a fine patch moved without a mid coordinate near an integer"


def test_predict_fine_against_the_reference_golden(net, dev):
    """predict_fine_128x160.npz, the reference's own fp32 run (tests/test_gpu_parity.py holds the other modes to it at the
    project's bars): in mode fp16 the coarse matches are its bits, the mid matches lie within the model's per-proposal bound, the
    fine matches too where the fine patch is the golden's."""
    g = gu.load("predict_fine_128x160")
    p1, p2 = gu.pair_inputs(g)
    f1, f2 = [t[None].to(dev) for t in p1], [t[None].to(dev) for t in p2]
    _, mid, fine = net._weights()
    try:
        mid.set_mode("fp16")
        fine.set_mode("fp16")
        fine_m, fine_s, mid_m, mid_s, coarse = [t[0].cpu() for t in net.predict_fine_from_feats(f1, f2, return_all=True)]
    finally:
        mid.set_mode("fp16x2w")
        fine.set_mode("fp16x2w")
    assert torch.equal(coarse, torch.from_numpy(g["coarse"]))
    n = 12
    gmid, gfine = torch.from_numpy(g["mid"]), torch.from_numpy(g["fine"])
    mid_p, fine_p = rr.params64(gu.state_dict(0))
    cb_mid, sb_mid, _ = fm.level_bounds(mid_p, p1[:4], p2[:4], coarse[:n].double())
    cb_fine, sb_fine, _ = fm.level_bounds(fine_p, p1[:4], p2[:4], gmid[:n].double())
    dm, dms = (mid_m - gmid).abs().amax(1).double(), (mid_s - torch.from_numpy(g["mid_scores"])).abs().double()
    df, dfs = (fine_m - gfine).abs().amax(1).double(), (fine_s - torch.from_numpy(g["fine_scores"])).abs().double()
    same = (mid_m.long() == gmid.long()).all(1)
    print(f"\npredict_fine[MI355X] fp16 vs golden: mid {dm.max().item():.2e} px {dms.max().item():.2e}  fine {df[same].max().item():.2e} px "
          f"{dfs[same].max().item():.2e}  ({int(same.sum())} of {same.numel()} on the golden's fine patch); "
          f"bounds of the first {n}: mid {cb_mid.max().item():.2e} fine {cb_fine.max().item():.2e}")
    assert bool((dm[:n] <= cb_mid + rr.COORD_TOL).all()) and bool((dms[:n] <= sb_mid + rr.SCORE_TOL).all()), (dm[:n], cb_mid)
    ok = same[:n]
    assert bool((df[:n][ok] <= cb_fine[ok] + rr.COORD_TOL).all()) and bool((dfs[:n][ok] <= sb_fine[ok] + rr.SCORE_TOL).all()), (df[:n], cb_fine)
    to_int = (gmid[:n] - gmid[:n].round()).abs().amin(1).double()
    assert bool((to_int[~ok] <= cb_mid[~ok] + rr.COORD_TOL).all())


def test_graphed_matcher_replay_equals_eager(net, dev):
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    _, mid, fine = net._weights()
    H, W = 128, 160
    try:
        mid.set_mode("fp16")
        fine.set_mode("fp16")
        g = GraphedMatcher(net, H, W, with_backbone=False)
        for seed in (910, 911):
            p1, p2 = synthetic.make_correlated_pyramids(seed, H, W)
            f1, f2 = [t[None].to(dev) for t in p1], [t[None].to(dev) for t in p2]
            fine_m, scores, coarse = net.predict_fine_from_feats(f1, f2, ksize=2)
            gfine, gscores, gcoarse = g(f1, f2)
            assert torch.equal(gcoarse[0], coarse[0]) and torch.equal(gfine[0], fine_m[0]) and torch.equal(gscores[0], scores[0])
    finally:
        mid.set_mode("fp16x2w")
        fine.set_mode("fp16x2w")
