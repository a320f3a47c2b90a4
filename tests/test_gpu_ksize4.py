"""ksize = 4 on the MI355X: the coarse stage with the 4x4x4x4 max-pool / relocalisation on the MFMA accumulators
(corr_pool_kernel<4>, csrc/coarse.hip) against the unmodified reference's outputs (tests/golden/coarse_*_k4.npz) and the
CPU oracle, and end to end through Patch2Pix / model_helper / the streaming and graphed entry points.  Bars are those of
the ksize = 2 tests in tests/test_gpu_parity.py.  Needs an MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

import cabi_example_io as io
import golden_util as gu
from adjudicate import ErrorModel, U, _eps, differing_rows_are_near_ties, differing_rows_are_near_ties_local
from oracle import p2p_oracle as orc
from oracle.error_model import NEAR_TIE_TOL
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu

COORD_TOL = 1e-3
SCORE_TOL = 1e-5
K = 4
K4_CASES = ["coarse_256x320_k4", "coarse_160x352_k4"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from patch2pix_amd import ops
    return ops


@pytest.fixture(scope="module")
def cweights(dev, ops):
    sd = gu.state_dict(0)
    return sd, ops.NcnWeights(sd["ncn.conv.0.weight"], sd["ncn.conv.0.bias"], sd["ncn.conv.2.weight"], sd["ncn.conv.2.bias"], dev)


def _model(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


def _pack(planes, k=K):
    return ((planes[0] * k + planes[1]) * k + planes[2]) * k + planes[3]


def _near_tie_flips(fa, fb, got, ref_code, k=K):
    """Every pooled cell whose relocalisation code differs from the fp32 oracle's, re-evaluated in fp64 (the general-k form
    of test_gpu_parity._adjudicate_delta_flips): the two candidates' correlations must be closer than NEAR_TIE_TOL x the
    fp32 error bound of the two dot products (oracle/error_model.py).  Returns the number of differing cells."""
    na = fa.double() / (fa.double().pow(2).sum(0, keepdim=True) + 1e-6).sqrt()
    nb = fb.double() / (fb.double().pow(2).sum(0, keepdim=True) + 1e-6).sqrt()
    eps_c = _eps(fa.shape[0], 1.0) + 2 * (0.5 * _eps(fa.shape[0], 1.0) + 3 * U)
    flips = np.argwhere(got != ref_code)
    for a, b, c, d in flips:
        def corr_of(code):
            di, dj, dk, dl = code // (k * k * k), (code // (k * k)) % k, (code // k) % k, code % k
            va, vb = na[:, k * a + di, k * b + dj], nb[:, k * c + dk, k * d + dl]
            return float((va * vb).sum()), eps_c * float((va * vb).abs().sum())
        (g, eg), (r, er) = corr_of(int(got[a, b, c, d])), corr_of(int(ref_code[a, b, c, d]))
        print(f"  cell {(a, b, c, d)}: kernel {int(got[a, b, c, d])}, oracle {int(ref_code[a, b, c, d])}, fp64 gap {abs(g - r):.3e} "
              f"(fp32 error bound {eg + er:.1e})")
        assert abs(g - r) <= NEAR_TIE_TOL * (eg + er), f"cell {(a, b, c, d)}: the relocalisation differs and is not a near-tie"
    return len(flips)


# ------------------------------------------------------------------------------------------ coarse stage
@pytest.mark.parametrize("name", K4_CASES)
def test_k4_coarse_golden(name, dev, ops, cweights):
    """The unmodified reference's corr4d / delta4d / matches at ksize 4: 0 differing relocalisation codes."""
    sd, ncn = cweights
    g = gu.load(name)
    assert int(g["ksize"]) == K
    p1, p2 = gu.coarse_inputs(g)
    corr, delta = ops.coarse_forward(p1[4].to(dev), p2[4].to(dev), K, ncn)
    np.testing.assert_allclose(corr.cpu().numpy(), g["corr4d"], rtol=2e-4, atol=1e-7)
    assert delta.dtype == torch.uint8
    ref_code = _pack(g["delta4d"].astype(np.int64))
    flips = int((delta.cpu().numpy().astype(np.int64) != ref_code).sum())
    assert flips == 0, f"{flips} relocalisation argmax differ from the reference"
    m, s = ops.coarse_matches(corr, delta, K, 8, True)
    assert np.array_equal(m.cpu().numpy(), g["all_matches"])
    np.testing.assert_allclose(s.cpu().numpy(), g["all_scores"], rtol=2e-4)
    planes = ops.delta_unpack(delta, K)
    assert np.array_equal(torch.stack(planes).cpu().numpy().astype(np.int8), g["delta4d"])


@pytest.mark.parametrize("hw", [(128, 160), (256, 320), (224, 352), (480, 640)])
def test_k4_coarse_vs_oracle(hw, dev, ops, cweights):
    """Assertions of test_coarse_vs_oracle; at most 2 differing relocalisation codes per case, each a near-tie.
    (The fp32 oracle itself differs from its fp64 evaluation in 0 / 0 / 0 / 1 cells on these inputs.)"""
    sd, ncn = cweights
    H, W = hw
    p1, p2 = synthetic.make_correlated_pyramids(100 + H + K, H, W)
    o_ncn, _, _ = orc.split_params(sd)
    rc, rd = orc.coarse_forward(p1[4], p2[4], K, o_ncn)
    corr, delta = ops.coarse_forward(p1[4].to(dev), p2[4].to(dev), K, ncn)
    np.testing.assert_allclose(corr.cpu().numpy(), rc.numpy(), rtol=2e-4, atol=1e-7)
    flips = _near_tie_flips(p1[4], p2[4], delta.cpu().numpy().astype(np.int64), _pack(rd).numpy())
    print(f"\n{hw}: {flips} of {delta.numel()} relocalisation codes differ from the fp32 oracle")
    assert flips <= 2, f"{flips} relocalisation flips"
    rm, rs = orc.cal_coarse_matches(rc, rd, K, 8)
    # match extraction on identical inputs must be bit-exact: feed the oracle's volume (codes up to 255) to the kernel
    k_delta = _pack(rd).to(torch.uint8).to(dev)
    m, s = ops.coarse_matches(rc.to(dev), k_delta, K, 8, True)
    assert torch.equal(m.cpu(), rm)
    assert torch.allclose(s.cpu(), rs, rtol=1e-5)


def test_k4_images_of_different_sizes(dev, ops, cweights):
    """Ragged pair: 128x96 against 64x160 (4x3 x 2x5 cells; 192 / 160 GEMM rows: partial tiles on both sides)."""
    sd, ncn = cweights
    p1, p2 = synthetic.make_pyramid(71, 128, 96), synthetic.make_pyramid(72, 64, 160)
    o_ncn, _, _ = orc.split_params(sd)
    rc, rd = orc.coarse_forward(p1[4], p2[4], K, o_ncn)
    corr, delta = ops.coarse_forward(p1[4].to(dev), p2[4].to(dev), K, ncn)
    assert tuple(corr.shape) == tuple(rc.shape) == (4, 3, 2, 5)
    np.testing.assert_allclose(corr.cpu().numpy(), rc.numpy(), rtol=2e-4, atol=1e-7)
    assert _near_tie_flips(p1[4], p2[4], delta.cpu().numpy().astype(np.int64), _pack(rd).numpy()) == 0
    rm, rs = orc.cal_coarse_matches(rc, rd, K, 8)
    m, s = ops.coarse_matches(corr, delta, K, 8, True)
    assert torch.equal(m.cpu(), rm) and torch.allclose(s.cpu(), rs, rtol=2e-4)


def test_k4_large_image_vs_oracle(dev, ops, cweights):
    """960x1280 with ksize 4: the 19200 x 19200 correlation of config E pooled to 30x40x30x40 cells (the volume of a
    480x640 / ksize 2 pair) against the CPU oracle: all 2400 coarse rows equal or fp32 near-ties, differing relocalisation
    codes (of 1.44 M) near-ties and few."""
    sd, ncn = cweights
    p1, p2 = synthetic.make_correlated_pyramids(31, 960, 1280)
    o_ncn, _, _ = orc.split_params(sd)
    with torch.no_grad():
        rc, rd = orc.coarse_forward(p1[4], p2[4], K, o_ncn)
        rm, rs = orc.cal_coarse_matches(rc, rd, K, 8)
    corr, delta = ops.coarse_forward(p1[4].to(dev), p2[4].to(dev), K, ncn)
    assert tuple(corr.shape) == (30, 40, 30, 40)
    m, s = ops.coarse_matches(corr, delta, K, 8, True)
    np.testing.assert_allclose(corr.cpu().numpy(), rc.numpy(), rtol=2e-4, atol=1e-7)
    flips = _near_tie_flips(p1[4], p2[4], delta.cpu().numpy().astype(np.int64), _pack(rd).numpy())
    print(f"\n960x1280, ksize 4: {flips} of {delta.numel()} relocalisation codes differ from the fp32 oracle")
    # Every differing cell was held to the near-tie criterion above; their number is capped at the rate the 480x640 case
    # allows (2 per 90000 cells, where the fp32 oracle alone is 1 cell away from its own fp64 evaluation): 32 for 1.44 M
    # cells of 256 candidates each.
    assert flips <= 32
    ndiff, worst = differing_rows_are_near_ties_local(m.cpu(), rm, p1[4], p2[4], sd, K, volume_got=corr.cpu())
    assert ndiff <= 2, f"{ndiff} of {rm.shape[0]} coarse rows differ"
    if ndiff == 0:
        assert torch.allclose(s.cpu(), rs, rtol=2e-4)


def test_k4_coarse_batch_equals_per_pair(dev, ops, cweights, monkeypatch):
    """Batch of pairs == per-pair calls, bit for bit, also when the workspace holds two of the five pairs at a time."""
    sd, ncn = cweights
    H, W, B = 224, 352, 5
    pairs = [synthetic.make_correlated_pyramids(500 + i, H, W) for i in range(B)]
    fa = torch.stack([p[0][4] for p in pairs]).to(dev)
    fb = torch.stack([p[1][4] for p in pairs]).to(dev)
    singles = [ops.coarse_forward(fa[i], fb[i], K, ncn) for i in range(B)]
    per_pair = ops._lib.p2p_coarse_workspace_bytes(fa.shape[1], fa.shape[2], fa.shape[3], fb.shape[2], fb.shape[3], K)
    for limit in (ops.COARSE_WORKSPACE_LIMIT, 2 * per_pair + 1):
        monkeypatch.setattr(ops, "COARSE_WORKSPACE_LIMIT", limit)
        corr, delta = ops.coarse_forward_batch(fa, fb, K, ncn)
        m, sc = ops.coarse_matches_batch(corr, delta, K, 8, True)
        for i in range(B):
            assert torch.equal(corr[i], singles[i][0]) and torch.equal(delta[i], singles[i][1]), (limit, i)
            m1, s1 = ops.coarse_matches(singles[i][0], singles[i][1], K, 8, True)
            assert torch.equal(m[i], m1) and torch.equal(sc[i], s1), (limit, i)


def test_k4_argument_errors(dev, ops, cweights):
    """ksize 3 and 5 stay NotImplementedError (status -3); a 6x8 map with ksize 4 is the library's P2P_EINVAL message."""
    sd, ncn = cweights
    f = torch.randn(32, 12, 60, device=dev)
    for ksize in (3, 5):
        with pytest.raises(NotImplementedError, match="1, 2 or 4"):
            ops.coarse_forward(f, f, ksize, ncn)
    with pytest.raises(RuntimeError, match="multiples of ksize"):
        ops.coarse_forward(torch.randn(32, 6, 8, device=dev), torch.randn(32, 8, 8, device=dev), K, ncn)


def test_k4_plain_c_host_matches_python_host(dev, ops, cweights, tmp_path):
    """examples/cabi_coarse.c with ksize 4 in its input file against the ctypes front end on the same inputs."""
    import subprocess
    from patch2pix_amd import build
    sd, ncn = cweights
    exe = build.build_examples(verbose=False, trust_existing=True)
    pairs = [synthetic.make_correlated_pyramids(700 + i, 96, 128) for i in range(3)]
    fa = torch.stack([p[0][4] for p in pairs]).contiguous()
    fb = torch.stack([p[1][4] for p in pairs]).contiguous()
    io.write_input(tmp_path / "in.bin", sd, fa, fb, K)
    res = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    corr, delta = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), K, ncn)
    m, sc = ops.coarse_matches_batch(corr, delta, K, 8, True)
    c_corr, c_delta, c_m, c_s = io.read_output(tmp_path / "out.bin", corr.numel(), sc.numel(), K)
    np.testing.assert_allclose(c_corr, corr.cpu().numpy().ravel(), rtol=1e-6, atol=1e-9)
    assert np.array_equal(c_delta, delta.cpu().numpy().ravel())
    assert np.array_equal(c_m, m.cpu().numpy().ravel())
    np.testing.assert_allclose(c_s, sc.cpu().numpy().ravel(), rtol=1e-6)


# ------------------------------------------------------------------------------------------ end to end
def _check_against_oracle(sd, p1, p2, all_rows, coarse, mid, fine, fine_scores, mid_scores=None):
    """p1, p2: CPU pyramids of one pair.  all_rows: the product's unfiltered coarse rows; coarse / mid / fine: what the
    product returned.  Coarse rows that fp32 can decide equal the oracle's; both regressors on the product's own
    proposals within 1e-3 px / 1e-5."""
    o_ncn, mid_p, fine_p = orc.split_params(sd)
    with torch.no_grad():
        rc, rd = orc.coarse_forward(p1[4], p2[4], K, o_ncn)
        rm, rs = orc.cal_coarse_matches(rc, rd, K, 8)
        if not torch.equal(all_rows, rm):
            em = ErrorModel(p1[4], p2[4], sd, K)
            em.check(rc, "oracle fp32 volume")
            nd, gap = differing_rows_are_near_ties(all_rows, rm, em)
            print(f"\n{nd} of {rm.shape[0]} coarse rows differ from the fp32 oracle, fp64 gap {gap:.3f} of the fp32 error bound")
            assert nd <= 2
            rm = all_rows
        ref_sel, _ = orc.filter_coarse(rm, torch.ones(rm.shape[0]), 0.0, True)
        assert torch.equal(coarse, ref_sel), "the mutual coarse matches differ from the oracle's filter_coarse"
        assert coarse.shape[0] > 0
        ref_mid, ref_mp, _ = orc.fine_level(p1[:4], p2[:4], coarse, mid_p)
        if mid is None:            # entry points that do not return the mid level: the oracle's chain, unstable truncations apart
            frac = ref_mid - ref_mid.floor()
            ok = ~((((frac > 0) & (frac < 2e-4)) | (frac > 1 - 2e-4)).any(dim=1))
            assert int((~ok).sum()) <= 2
            mid = ref_mid
        else:
            ok = torch.ones(coarse.shape[0], dtype=torch.bool)
            assert (mid - ref_mid).abs().max() <= COORD_TOL
            if mid_scores is not None:
                assert (mid_scores - ref_mp).abs().max() <= SCORE_TOL
        ref_fine, ref_fp, _ = orc.fine_level(p1[:4], p2[:4], mid, fine_p)
    assert (fine - ref_fine)[ok].abs().max() <= COORD_TOL
    assert (fine_scores - ref_fp)[ok].abs().max() <= SCORE_TOL


def _normalised_pair(seed, H, W, dev):
    a, b = synthetic.make_image_pair(seed, H, W)
    norm = lambda x: (torch.from_numpy(x).permute(2, 0, 1).float() / 255.0 - 0.45)[None].to(dev) / 0.225
    return norm(a), norm(b)


def test_k4_predict_fine_vs_oracle(dev):
    """Patch2Pix.predict_fine(ksize=4) on synthetic weights against oracle.p2p_oracle (fed with the product's pyramids)."""
    net = _model(dev)
    sd = gu.state_dict(0)
    ia, ib = _normalised_pair(21, 256, 320, dev)
    with torch.no_grad():
        f1, f2 = net._pyramids(ia, ib)
        fine, fine_s, mid, mid_s, coarse = net.predict_fine(ia, ib, ksize=K, return_all=True)
        corr4d, delta4d = net.forward_coarse_match(f1[4], f2[4], ksize=K)
        assert corr4d.shape == (1, 1, 8, 10, 8, 10) and int(delta4d.packed.max()) > 127
        rows, _ = net.cal_coarse_matches(corr4d, delta4d, ksize=K, upsample=net.upsample, center=True)
    p1, p2 = [t[0].cpu() for t in f1], [t[0].cpu() for t in f2]
    _check_against_oracle(sd, p1, p2, rows[0].cpu(), coarse[0].cpu(), mid[0].cpu(), fine[0].cpu(), fine_s[0].cpu(), mid_s[0].cpu())
    # from correlated pyramids as well (more mutual matches), through the device-side filter too
    q1, q2 = synthetic.make_correlated_pyramids(45, 256, 320)
    g1, g2 = [t[None].to(dev) for t in q1], [t[None].to(dev) for t in q2]
    with torch.no_grad():
        fine, fine_s, mid, mid_s, coarse = net.predict_fine_from_feats(g1, g2, ksize=K, return_all=True)
        rows, _ = net.cal_coarse_matches(*net.forward_coarse_match(g1[4], g2[4], ksize=K), ksize=K, upsample=8)
        dfine, dscores, dcoarse = net.unpad(*net.predict_fine_device(g1, g2, ksize=K))
    _check_against_oracle(sd, q1, q2, rows[0].cpu(), coarse[0].cpu(), mid[0].cpu(), fine[0].cpu(), fine_s[0].cpu(), mid_s[0].cpu())
    assert torch.equal(dcoarse[0], coarse[0]) and torch.equal(dfine[0], fine[0]) and torch.equal(dscores[0], fine_s[0])


def test_k4_estimate_matches_vs_oracle(dev, tmp_path):
    """model_helper.estimate_matches(ksize=4), both eval_types, on image files (loaded to multiples of upsample * ksize = 32
    pixels) against the oracle on the same pyramids (backbone evaluated on the CPU on both sides)."""
    import copy
    from PIL import Image
    from patch2pix_amd.utils.datasets.preprocess import load_im_pixels, normalise_pixels
    from patch2pix_amd.utils.eval import model_helper
    net = _model(dev)
    sd = gu.state_dict(0)
    a, b = synthetic.make_image_pair(53, 300, 400)
    Image.fromarray(a).save(tmp_path / "1.png")
    Image.fromarray(b).save(tmp_path / "2.png")
    files = (str(tmp_path / "1.png"), str(tmp_path / "2.png"))
    cpu_extract = copy.deepcopy(net.extract).to("cpu")
    loaded = [load_im_pixels(f, K, net.upsample) for f in files]
    assert tuple(loaded[0][0].shape) == (288, 384, 3)
    with torch.no_grad():          # both images as one batch, like Patch2Pix._pyramids
        feats = cpu_extract.pyramid(torch.cat([normalise_pixels(px.unsqueeze(0)) for px, _ in loaded]))
    p1, p2 = [f[0] for f in feats], [f[1] for f in feats]
    to_original = np.array([tuple(loaded[0][1]) + tuple(loaded[1][1])])
    gpu_pyramid = net.extract.pyramid
    net.extract.pyramid = lambda im: [f.to(dev) for f in cpu_extract.pyramid(im.cpu())]
    try:
        m, s, c = model_helper.estimate_matches(net, *files, ksize=K, io_thres=0.0, eval_type="fine")
        mc, sc, cc = model_helper.estimate_matches(net, *files, ksize=K, ncn_thres=0.0, eval_type="coarse")
    finally:
        net.extract.pyramid = gpu_pyramid
    with torch.no_grad():
        rows, _ = net.cal_coarse_matches(*net.forward_coarse_match(p1[4][None].to(dev), p2[4][None].to(dev), ksize=K),
                                         ksize=K, upsample=net.upsample)
    assert m.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64 and m.shape == c.shape
    assert np.array_equal(mc, cc)
    unscale = lambda x: torch.from_numpy(x / to_original)
    coarse = unscale(c).round().long()
    assert np.abs(coarse.numpy() * to_original - c).max() < 1e-9
    # io_thres = 0 keeps every row (the confidences are positive): the product's rows are the whole filtered list
    _check_against_oracle(sd, p1, p2, rows[0].cpu(), coarse, None, unscale(m).float(), torch.from_numpy(s))
    # eval_type 'coarse' with mutual=True: filter_coarse of the same rows, scaled
    assert np.array_equal(unscale(mc).round().long().numpy(), coarse.numpy())


def test_k4_stream_equals_per_pair_calls(dev, tmp_path):
    """estimate_matches_stream(ksize=4) returns what estimate_matches(ksize=4) returns pair by pair (rows matched by their
    coarse match: the batched backbone may differ from the un-batched one in the last bits)."""
    from PIL import Image
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    net = _model(dev)
    pairs = []
    for i, (h, w) in enumerate([(256, 320), (256, 320), (256, 320), (192, 256), (192, 256), (256, 320)]):
        a, b = synthetic.make_image_pair(300 + i, h, w)
        pa, pb = tmp_path / f"{i}a.jpg", tmp_path / f"{i}b.jpg"
        Image.fromarray(a).save(pa, quality=95)
        Image.fromarray(b).save(pb, quality=95)
        pairs.append((str(pa), str(pb)))
    streamed = list(estimate_matches_stream(net, pairs, ksize=K, io_thres=0.25, batch=3, workers=3))
    assert len(streamed) == len(pairs)
    for (m, s, c), (pa, pb) in zip(streamed, pairs):
        rm, rs, rc = model_helper.estimate_matches(net, pa, pb, ksize=K, io_thres=0.25)
        assert m.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64
        ref = {tuple(np.round(r, 6)): i for i, r in enumerate(rc)}
        hits = [(i, ref[tuple(np.round(r, 6))]) for i, r in enumerate(c) if tuple(np.round(r, 6)) in ref]
        assert len(hits) >= 0.9 * max(len(rc), 1), (len(hits), len(rc))
        if hits:
            gi = np.array([h[0] for h in hits]); ri = np.array([h[1] for h in hits])
            assert np.median(np.abs(m[gi] - rm[ri]).max(axis=1)) < 0.02


def test_k4_graphed_matcher_equals_eager_path(dev):
    """GraphedMatcher(ksize=4): the captured device path replays to what the eager calls return."""
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    net = _model(dev)
    H, W = 256, 320
    g = GraphedMatcher(net, H, W, ksize=K, with_backbone=False)
    for seed in (910, 911):
        p1, p2 = synthetic.make_correlated_pyramids(seed, H, W)
        f1, f2 = [t[None].to(dev) for t in p1], [t[None].to(dev) for t in p2]
        fine, scores, coarse = net.predict_fine_from_feats(f1, f2, ksize=K)
        gfine, gscores, gcoarse = g(f1, f2)
        assert coarse[0].shape[0] > 0
        assert torch.equal(gcoarse[0], coarse[0]) and torch.equal(gfine[0], fine[0]) and torch.equal(gscores[0], scores[0])
    g2 = GraphedMatcher(net, H, W, ksize=K, with_backbone=True)
    for seed in (5, 6):
        ia, ib = _normalised_pair(seed, H, W, dev)
        with torch.no_grad():
            fine, scores, coarse = net.predict_fine(ia, ib, ksize=K)
        gfine, gscores, gcoarse = g2(ia, ib)
        assert torch.equal(gcoarse[0], coarse[0])
        if coarse[0].shape[0]:
            assert (gfine[0] - fine[0]).abs().max() <= COORD_TOL and (gscores[0] - scores[0]).abs().max() <= SCORE_TOL


def test_k4_nc_only_model_and_predict_coarse(dev):
    """load_model(method='nc') + forward_coarse_match / cal_coarse_matches / predict_coarse at ksize 4 against the reference's
    fixture; the reference-format delta4d (four int64 planes, values up to 3 -> code 255) is accepted like the packed one."""
    from patch2pix_amd.networks.utils import filter_coarse
    from patch2pix_amd.utils.eval import model_helper
    sd = gu.state_dict(0)
    nc_sd = {k: v for k, v in sd.items() if k.startswith(("extract.", "ncn."))}
    net = model_helper.load_model({"state_dict": nc_sd}, method="nc", lprint=lambda *a: None)
    assert net.regress_mid is None and net.upsample == 8
    g = gu.load("coarse_256x320_k4")
    p1, p2 = gu.coarse_inputs(g)
    corr4d, delta4d = net.forward_coarse_match(p1[4][None].to(dev), p2[4][None].to(dev), ksize=K)
    assert corr4d.shape == (1, 1, 8, 10, 8, 10) and len(delta4d) == 4
    assert delta4d[0].dtype == torch.int64 and delta4d[0].shape == corr4d.shape
    assert np.array_equal(torch.stack([d[0, 0] for d in delta4d]).cpu().numpy().astype(np.int8), g["delta4d"])
    m, s = net.cal_coarse_matches(corr4d, delta4d, ksize=K, upsample=net.upsample, center=True)
    assert np.array_equal(m[0].cpu().numpy(), g["all_matches"])
    planes = tuple(t.clone() for t in delta4d)
    assert max(int(t.max()) for t in planes) == 3
    m2, _ = net.cal_coarse_matches(corr4d, planes, ksize=K, upsample=net.upsample, center=True)
    assert torch.equal(m, m2)
    fm, _ = filter_coarse(m, s, 0.0, True)
    assert np.array_equal(fm[0].cpu().numpy(), g["mutual_matches"])
    fu, _ = filter_coarse(m, s, 0.0, False)
    assert np.array_equal(fu[0].cpu().numpy(), g["unique_matches"])
    # predict_coarse from images: the rows of forward + cal_coarse_matches + filter_coarse on the same pyramids
    ia, ib = _normalised_pair(22, 256, 320, dev)
    with torch.no_grad():
        pm, ps = net.predict_coarse(ia, ib, ksize=K, ncn_thres=0.0, mutual=True)
        f1, f2 = net._pyramids(ia, ib)
        rows, sc = net.cal_coarse_matches(*net.forward_coarse_match(f1[-1], f2[-1], ksize=K), ksize=K, upsample=net.upsample)
    o_ncn, _, _ = orc.split_params(sd)
    rc, rd = orc.coarse_forward(f1[-1][0].cpu(), f2[-1][0].cpu(), K, o_ncn)
    rm, rs = orc.cal_coarse_matches(rc, rd, K, 8)
    if not torch.equal(rows[0].cpu(), rm):
        em = ErrorModel(f1[-1][0].cpu(), f2[-1][0].cpu(), sd, K)
        nd, _ = differing_rows_are_near_ties(rows[0].cpu(), rm, em)
        assert nd <= 2
        rm, rs = rows[0].cpu(), sc[0].cpu()
    ref_sel, _ = orc.filter_coarse(rm, rs, 0.0, True)
    assert torch.equal(pm[0].cpu(), ref_sel)
