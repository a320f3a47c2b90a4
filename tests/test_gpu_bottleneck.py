"""MI355X: ResNet50 / ResNet101 pyramid producers, stride-16 models and 1024-channel matching against the reference's
fixtures (tests/golden/bottleneck_*.npz, made by tests/make_golden_bottleneck.py) and the project's own oracle.  Cases, seeded
checkpoints and images: tests/bottleneck_reference.py.  The reference tree is not needed here."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bottleneck_reference as br  # noqa: E402
import golden_util as gu  # noqa: E402
from oracle import error_model as em  # noqa: E402
from oracle import p2p_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
COORD_TOL, SCORE_TOL = 1e-3, 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _golden(name):
    g = dict(np.load(br.golden_path(name)))
    im1, im2 = br.images(name)
    assert abs(gu.checksum([im1, im2]) - float(g["image_checksum"])) <= 1e-9 * float(g["image_checksum"]), "the seeded images drifted"
    return g


@functools.lru_cache(maxsize=None)
def _ckpt(name):
    g = _golden(name)
    ckpt = br.checkpoint(name, torch.from_numpy(g["contrast_shift"]))
    got = gu.checksum([v for v in ckpt["state_dict"].values() if v.is_floating_point()])
    assert abs(got - float(g["weights_checksum"])) <= 1e-9 * float(g["weights_checksum"]), "the seeded checkpoint drifted"
    return ckpt


@functools.lru_cache(maxsize=None)
def _model(name):
    from patch2pix_amd.networks.patch2pix import Patch2Pix
    return Patch2Pix(br.model_config(name, _ckpt(name), torch.device("cuda", 0)))


@functools.lru_cache(maxsize=None)
def _cpu_pyramids(name):
    """This implementation's torch path on the CPU (the reference's module arithmetic): fp32 and fp64 pyramids of both images."""
    net = _model(name)
    import copy
    cpu = copy.deepcopy(net.extract).cpu()
    im1, im2 = br.images(name)
    with torch.no_grad():
        p32 = [cpu.pyramid(im) for im in (im1, im2)]
        cpu = cpu.double()
        p64 = [cpu.pyramid(im.double()) for im in (im1, im2)]
    return p32, p64


def _ref_feats(name):
    """The reference's own level-4 features of both images ([1,C,h,w] fp32): what its recorded volumes, rows and scores were
    computed from.  The coarse stage is compared on THESE inputs; this machine's CPU path differs from them in the last bits."""
    g = _golden(name)
    return torch.from_numpy(g["feat1_l4"])[None], torch.from_numpy(g["feat2_l4"])[None]


PYRAMID_CASES = ["bottleneck_r50_s8", "bottleneck_r50_s16", "bottleneck_r101_s8", "bottleneck_r34_s16"]


@pytest.mark.parametrize("name", PYRAMID_CASES)
def test_pyramid_vs_fp64_golden_and_library(name, dev, monkeypatch):
    """Every level against the fp64 walk of the same module at the ResNet34 bar (tests/test_gpu_parity.py:
    test_backbone_pyramid_vs_fp64: no farther than max(3e-6, 2.5 x the MIOpen path's error) of the image's largest value),
    against the reference's recorded levels, and an image alone against the image in a batch, bit for bit."""
    net, g = _model(name), _golden(name)
    _, p64 = _cpu_pyramids(name)
    ims = br.images(name)
    for i, im in enumerate(ims):
        with torch.no_grad():
            monkeypatch.setenv("P2P_BACKBONE", "hip")
            got = net.extract.pyramid(im.to(dev))
            monkeypatch.setenv("P2P_BACKBONE", "miopen")
            lib = net.extract.pyramid(im.to(dev))
        assert len(got) == 5 and torch.equal(got[0].cpu(), im)
        for lv in range(1, 5):
            ref = p64[i][lv]
            assert got[lv].shape == ref.shape and got[lv].dtype == torch.float32 and got[lv].is_contiguous()
            scale = ref.abs().amax()
            e_hip = float((got[lv].cpu().double() - ref).abs().max() / scale)
            e_lib = float((lib[lv].cpu().double() - ref).abs().max() / scale)
            bar = max(3e-6, 2.5 * e_lib)
            print(f"{name} image {i + 1} level {lv}: HIP {e_hip:.2e}, MIOpen {e_lib:.2e} of the largest value")
            assert e_hip <= bar, f"{name} image {i + 1} level {lv}: HIP {e_hip:.2e} vs MIOpen {e_lib:.2e}"
            step = int(g[f"pyr{i + 1}_l{lv}_step"])
            want = torch.from_numpy(g[f"pyr{i + 1}_l{lv}"]).double()
            e_ref = float((got[lv][0, ::step].cpu().double() - want).abs().max() / scale)
            assert e_ref <= 2 * bar, f"{name} image {i + 1} level {lv}: {e_ref:.2e} from the reference's recorded level"
    if ims[0].shape == ims[1].shape:
        monkeypatch.setenv("P2P_BACKBONE", "hip")
        with torch.no_grad():
            both = net.extract.pyramid(torch.cat([ims[0], ims[1] * 40.0]).to(dev))        # a batch mate on another scale
            one = net.extract.pyramid(ims[0].to(dev))
        for lv in range(1, 5):
            assert torch.equal(one[lv][0], both[lv][0]), f"{name} level {lv}: the image alone differs from the image in a batch"


def test_resnet101_stride16_pyramid(dev, monkeypatch):
    """The one backbone / stride combination without a fixture: fp64 walk and the library path, level-4 shape of stride 16."""
    from patch2pix_amd.networks import resnet
    from patch2pix_amd.utils import synthetic
    sd = synthetic.make_backbone_checkpoint(506, "ResNet101", False)["state_dict"]
    net = resnet.ResNet101()
    net.load_state_dict({k[len("extract."):]: v for k, v in sd.items() if k.startswith("extract.")}, strict=False)
    net.eval()
    x = br.images("bottleneck_r50_s16")[0]
    with torch.no_grad():
        ref = net.double().pyramid(x.double())
        net = net.float().to(dev)
        monkeypatch.setenv("P2P_BACKBONE", "hip")
        got = net.pyramid(x.to(dev))
        monkeypatch.setenv("P2P_BACKBONE", "miopen")
        lib = net.pyramid(x.to(dev))
    assert tuple(got[4].shape) == (1, 1024, 8, 12) and tuple(got[3].shape) == (1, 512, 16, 24)
    for lv in range(1, 5):
        scale = ref[lv].abs().amax()
        e_hip = float((got[lv].cpu().double() - ref[lv]).abs().max() / scale)
        e_lib = float((lib[lv].cpu().double() - ref[lv]).abs().max() / scale)
        assert e_hip <= max(3e-6, 2.5 * e_lib), f"level {lv}: HIP {e_hip:.2e} vs MIOpen {e_lib:.2e}"


def _adjudicate(rows, scores, delta, g, k, model, upsample, what):
    """Rows of cal_coarse_matches against the fp64 model and the reference's recorded rows: decidable rows exact, differing rows
    near-ties, decidable relocalisation codes exact (the scores: test_nc_scores_against_the_reference)."""
    rows, scores = rows.cpu(), scores.cpu()
    want_rows, want_scores = torch.from_numpy(g[f"k{k}_rows"].astype(np.int64)), torch.from_numpy(g[f"k{k}_scores"])
    ndec, nrows = em.assert_decidable_rows(rows, model, upsample)
    ndiff, worst = em.differing_rows_are_near_ties(rows, want_rows, model, upsample)
    if delta is not None:
        flips = delta.cpu() != torch.from_numpy(g[f"k{k}_delta"])
        assert not bool((flips & model.reloc_decidable).any()), f"{what}: a decidable relocalisation code differs from the reference's"
    print(f"{what} ksize {k}: {ndec} of {nrows} rows decidable in fp32, {ndiff} differ from the reference (worst gap {worst:.3f} of the bound)")
    return ndiff


@pytest.mark.parametrize("name", list(br.CASES))
def test_nc_path_against_the_reference(name, dev):
    """Patch2Pix.forward, cal_coarse_matches and predict_coarse on every fixture: (1) on the reference's own level-4 features
    (identical inputs on both sides), (2) from the images through the HIP producer."""
    from patch2pix_amd.networks.utils import filter_coarse
    net, g, ckpt = _model(name), _golden(name), _ckpt(name)
    assert net.upsample == int(g["upsample"]) == (8 if br.CASES[name][1] else 16)
    p32, _ = _cpu_pyramids(name)
    for lv in range(1, 5):           # the CPU path reproduces the reference's features (same module arithmetic; thread counts may differ)
        drift = abs(gu.checksum([p32[0][lv]]) - float(g[f"pyr1_l{lv}_checksum"])) / float(g[f"pyr1_l{lv}_checksum"])
        assert drift <= 1e-5, f"{name} level {lv}: the CPU path's features drifted {drift:.1e} from the reference's"
    im1, im2 = (t.to(dev) for t in br.images(name))
    fa, fb = _ref_feats(name)
    assert fa.shape == p32[0][4].shape and fb.shape == p32[1][4].shape
    for k in br.CASES[name][4]:
        model = em.ErrorModel(fa[0], fb[0], ckpt["state_dict"], ksize=k)
        with torch.no_grad():
            corr, delta = net.forward_coarse_match(fa.to(dev), fb.to(dev), ksize=k)
            rows, scores = net.cal_coarse_matches(corr, delta, ksize=k, upsample=net.upsample, center=True)
        model.check(corr[0, 0].cpu(), f"{name} HIP volume")
        model.check(torch.from_numpy(g[f"k{k}_corr4d"]), f"{name} reference volume")
        _adjudicate(rows[0], scores[0], delta.packed[0] if delta is not None else None, g, k, model, net.upsample, f"{name} (identical pyramids)")
        with torch.no_grad():
            corr2, delta2 = net.forward(im1, im2, ksize=k)
            rows2, scores2 = net.cal_coarse_matches(corr2, delta2, ksize=k, upsample=net.upsample, center=True)
            assert corr2.shape == corr.shape
            em.assert_decidable_rows(rows2[0].cpu(), model, net.upsample)
            em.differing_rows_are_near_ties(rows2[0].cpu(), torch.from_numpy(g[f"k{k}_rows"].astype(np.int64)), model, net.upsample)
            # the same path against the error model of the features it read (the HIP producer's own level-4 maps): the volume,
            # every decidable row and every decidable relocalisation code
            h1, h2 = net.extract.pyramid(im1)[4][0].cpu(), net.extract.pyramid(im2)[4][0].cpu()
            own = em.ErrorModel(h1, h2, ckpt["state_dict"], ksize=k)
            own.check(corr2[0, 0].cpu(), f"{name} HIP volume on HIP features")
            em.assert_decidable_rows(rows2[0].cpu(), own, net.upsample)
            if delta2 is not None:
                flips = delta2.packed[0].cpu() != own.reloc_code
                assert not bool((flips & own.reloc_decidable).any()), f"{name}: a decidable relocalisation code on HIP features is not the fp64 one"
            pc, ps = net.predict_coarse(im1, im2, ksize=k, ncn_thres=0.0, mutual=False)
            fc, fs = filter_coarse(rows2, scores2, 0.0, False)
        assert torch.equal(pc[0], fc[0]) and torch.equal(ps[0], fs[0])


@pytest.mark.parametrize("name", list(br.CASES))
def test_nc_scores_against_the_reference(name, dev):
    """cal_coarse_matches scores on the reference's own level-4 features within 1e-5 of the reference's recorded scores, on every
    row both lists agree on.  Both sides are fp32 evaluations of the same inputs; the fixtures' own scores are 4e-6 ... 7e-6 from
    the fp64 ones (a fixture's condition, tests/make_golden_bottleneck.py).  Measured on an MI355X: 6.6e-6 ... 9.2e-6 over the six
    cases; before corr_pool_kernel cut its accumulation chains at 1024 channels: up to 3.9e-5."""
    net, g = _model(name), _golden(name)
    fa, fb = _ref_feats(name)
    for k in br.CASES[name][4]:
        with torch.no_grad():
            corr, delta = net.forward_coarse_match(fa.to(dev), fb.to(dev), ksize=k)
            rows, scores = net.cal_coarse_matches(corr, delta, ksize=k, upsample=net.upsample, center=True)
        want_rows, want_scores = torch.from_numpy(g[f"k{k}_rows"].astype(np.int64)), torch.from_numpy(g[f"k{k}_scores"])
        same = (rows[0].cpu() == want_rows).all(dim=1)
        err = float((scores[0].cpu()[same] - want_scores[same]).abs().max())
        print(f"{name} ksize {k}: max |d score| {err:.2e} on {int(same.sum())} of {same.numel()} rows; largest volume value {float(corr.max()):.2f}")
        assert err <= SCORE_TOL, f"{name} ksize {k}: scores {err:.2e} from the reference's"


FINE_CASES = ["bottleneck_r34_s16", "bottleneck_r50_fi01"]      # ResNet34 at stride 16, released regressors; ResNet50 at stride 8, feat_idx [0, 1]


def _near_integer_rows(mid, eps=2e-4):
    """tests/test_gpu_parity.py: rows with a coordinate within eps of an integer without being one -- trunc() of a value that
    differs in the last bits may land on the other side, and the fine level then reads another patch."""
    frac = mid - mid.floor()
    return (((frac > 0) & (frac < eps)) | (frac > 1 - eps)).any(dim=1)


def _coarse_of(net, f1, f2):
    """The coarse stage on the level-4 maps of the pyramids f1, f2: volume, packed relocalisation codes, rows and scores of
    cal_coarse_matches -- what predict_fine_from_feats computes inside (the kernels are deterministic)."""
    with torch.no_grad():
        corr, delta = net.forward_coarse_match(f1[4], f2[4], ksize=2)
        rows, scores = net.cal_coarse_matches(corr, delta, ksize=2, upsample=net.upsample, center=True)
    return corr[0, 0].cpu(), delta.packed[0].cpu(), rows[0].cpu(), scores[0].cpu()


def _against_the_oracle(net, sd, f1, f2, out, what):
    """`out` = (fine, fine_scores, mid, mid_scores, coarse) of predict_fine*(..., return_all=True) on the device pyramids f1, f2.
    Every link of the chain is held to the project's oracle on THOSE pyramids, every row of it:
      * the volume within the fp32 error model, every decidable row of cal_coarse_matches the fp64 winner, at the model's stride;
      * the proposals exactly the mutual filter (oracle/p2p_oracle.py: filter_coarse) of the kernel's rows;
      * mid = the oracle's fine_level on the kernel's proposals, fine = the oracle's fine_level on the kernel's mid (the same
        truncated patch centres on both sides): coordinates within 1e-3 px, scores within 1e-5.
    -> the oracle's (fine, fine_scores)."""
    fine, fs, mid, ms, coarse = (t[0].cpu() for t in out)
    c1, c2 = [t.cpu() for t in f1], [t.cpu() for t in f2]
    volume, _, rows, scores = _coarse_of(net, f1, f2)
    model = em.ErrorModel(c1[4][0], c2[4][0], sd, ksize=2)
    model.check(volume, f"{what} HIP volume")
    ndec, nrows = em.assert_decidable_rows(rows, model, net.upsample)
    want, _ = orc.filter_coarse(rows, scores, 0.0, True)
    assert coarse.dtype == torch.int64 and coarse.shape[0] > 0 and torch.equal(coarse, want), f"{what}: the proposals are not the mutual rows"
    assert fine.shape == mid.shape == (coarse.shape[0], 4) and fs.shape == ms.shape == (coarse.shape[0],)
    n = max(net.feat_idx) + 1                           # the oracle gathers every level it is given
    p1, p2 = [t[0] for t in c1[:n]], [t[0] for t in c2[:n]]
    _, mid_p, fine_p = orc.split_params(sd)
    omid, oms, _ = orc.fine_level(p1, p2, coarse, mid_p)
    ofine, ofs, _ = orc.fine_level(p1, p2, mid, fine_p)
    print(f"{what}: {ndec} of {nrows} rows decidable, {coarse.shape[0]} proposals")
    for got, ref, key, tol in ((mid, omid, "mid", COORD_TOL), (ms, oms, "mid_scores", SCORE_TOL),
                               (fine, ofine, "fine", COORD_TOL), (fs, ofs, "fine_scores", SCORE_TOL)):
        err = float((got - ref).abs().max())
        print(f"{what}: max |d {key}| against the oracle {err:.2e}")
        assert err <= tol, f"{what}: {key} {err:.2e} from the oracle"
    return ofine, ofs


@pytest.mark.parametrize("name", FINE_CASES)
def test_predict_fine_against_the_reference(name, dev):
    """predict_fine_from_feats on the pyramids the reference's records were computed from (its own level-4 features; levels 0..3
    from the same module arithmetic on the CPU), against those records and against the oracle (_against_the_oracle).
    Proposals: the rows of cal_coarse_matches are adjudicated like the NC path's; a proposal that only one side holds must be
    one of the rows the adjudication accepted as a near-tie (a mutual row appears or disappears only with one of its two
    directional rows); with no differing row the list equals the reference's, in its order.  Every proposal both sides hold:
    mid within 1e-3 px / 1e-5; fine too, except rows whose mid coordinate is within 2e-4 of an integer (at most 2, as
    tests/test_gpu_parity.py: test_predict_fine_golden) -- those are held by the oracle on the kernel's own mid."""
    net, g, sd = _model(name), _golden(name), _ckpt(name)["state_dict"]
    p32, _ = _cpu_pyramids(name)
    fa, fb = _ref_feats(name)
    f1 = [t.to(dev) for t in p32[0][:4]] + [fa.to(dev)]
    f2 = [t.to(dev) for t in p32[1][:4]] + [fb.to(dev)]
    with torch.no_grad():
        out = net.predict_fine_from_feats(f1, f2, ksize=2, return_all=True)
    _against_the_oracle(net, sd, f1, f2, out, f"{name} (identical pyramids)")
    fine, fs, mid, ms, coarse = (t[0].cpu() for t in out)
    _, delta, rows, scores = _coarse_of(net, f1, f2)
    model = em.ErrorModel(fa[0], fb[0], sd, ksize=2)
    _adjudicate(rows, scores, delta, g, 2, model, net.upsample, f"{name} (identical pyramids)")
    want_rows = torch.from_numpy(g["k2_rows"].astype(np.int64))
    moved = (rows != want_rows).any(dim=1)
    near_ties = {tuple(r) for r in rows[moved].tolist()} | {tuple(r) for r in want_rows[moved].tolist()}
    got_c, ref_c = [tuple(r) for r in coarse.tolist()], [tuple(r) for r in g["coarse"].astype(np.int64).tolist()]
    one_sided = set(got_c) ^ set(ref_c)
    print(f"{name}: {len(got_c)} proposals, the reference {len(ref_c)}, {int(moved.sum())} near-tie rows, {len(one_sided)} proposals on one side only")
    assert one_sided <= near_ties, f"{name}: {len(one_sided - near_ties)} proposals differ from the reference's without a near-tie row"
    if not bool(moved.any()):
        assert got_c == ref_c
    where = {r: i for i, r in enumerate(ref_c)}
    gi = torch.tensor([i for i, r in enumerate(got_c) if r in where], dtype=torch.int64)
    ri = torch.tensor([where[got_c[i]] for i in gi.tolist()], dtype=torch.int64)
    assert gi.numel() > 0
    ref_mid = torch.from_numpy(g["mid"])[ri]
    unstable = _near_integer_rows(ref_mid)
    assert int(unstable.sum()) <= 2
    for got, key, tol, rowsel in ((mid, "mid", COORD_TOL, None), (ms, "mid_scores", SCORE_TOL, None),
                                  (fine, "fine", COORD_TOL, ~unstable), (fs, "fine_scores", SCORE_TOL, ~unstable)):
        a, b = got[gi], torch.from_numpy(g[key])[ri]
        if rowsel is not None:
            a, b = a[rowsel], b[rowsel]
        err = float((a - b).abs().max())
        print(f"{name}: max |d {key}| against the reference {err:.2e} on {a.shape[0]} rows")
        assert err <= tol, f"{name}: {key} {err:.2e} from the reference"


def _pair_files():
    d = os.path.join(gu.GOLDEN, "images", "pair_1")
    return os.path.join(d, "1.jpg"), os.path.join(d, "2.jpg")


@pytest.mark.parametrize("name", FINE_CASES)
def test_estimate_matches_against_the_oracle(name, dev):
    """From image files through the HIP producer: predict_fine on the loaded images is predict_fine_from_feats on the
    producer's pyramids, those results are held to the oracle on the same pyramids (_against_the_oracle: the stride enters
    through the rows' cells and the proposals' pixel positions), and estimate_matches is exactly that with the factors back to
    original pixels (1e-3 px of the network's image, i.e. times the factor, and 1e-5 against the oracle).  Image sizes follow
    upsample x ksize; the two images differ in size."""
    from patch2pix_amd.networks import resnet
    from patch2pix_amd.utils.datasets.preprocess import load_im_flexible
    from patch2pix_amd.utils.eval import model_helper
    net, sd = _model(name), _ckpt(name)["state_dict"]
    pa, pb = _pair_files()
    (t1, s1), (t2, s2) = (load_im_flexible(p, 2, net.upsample, imsize=256) for p in (pa, pb))
    for t in (t1, t2):
        assert t.shape[-1] % (2 * net.upsample) == 0 and t.shape[-2] % (2 * net.upsample) == 0
    assert t1.shape != t2.shape
    to_original = np.array([tuple(s1) + tuple(s2)])
    im1, im2 = t1[None].to(dev), t2[None].to(dev)
    with torch.no_grad():
        f1, f2 = resnet.pair_pyramids(net.extract, im1, im2)
        out = net.predict_fine(im1, im2, ksize=2, return_all=True)
        again = net.predict_fine_from_feats(f1, f2, ksize=2, return_all=True)
    assert tuple(f1[4].shape[-2:]) == (t1.shape[-2] // net.upsample, t1.shape[-1] // net.upsample)
    for a, b in zip(out, again):
        assert torch.equal(a[0], b[0])
    ofine, ofs = _against_the_oracle(net, sd, f1, f2, out, f"{name} (HIP producer)")
    fine, fs, coarse = out[0][0].cpu().numpy(), out[1][0].cpu().numpy(), out[4][0].cpu().numpy()
    m, s, c = model_helper.estimate_matches(net, pa, pb, ksize=2, io_thres=0.0, eval_type="fine", imsize=256)
    assert m.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64
    assert bool((fs > 0.0).all())                       # io_thres 0: every row is kept
    assert np.array_equal(c, to_original * coarse) and np.array_equal(m, to_original * fine) and np.array_equal(s, fs)
    err_m = float((np.abs(m - to_original * ofine.numpy()) / to_original).max())
    err_s = float(np.abs(s - ofs.numpy()).max())
    print(f"{name}: estimate_matches against the oracle: {err_m:.2e} px of the network's image, scores {err_s:.2e}")
    assert err_m <= COORD_TOL and err_s <= SCORE_TOL
    mc, sc, cc = model_helper.estimate_matches(net, pa, pb, ksize=2, ncn_thres=0.0, eval_type="coarse", imsize=256)
    assert np.array_equal(mc, to_original * coarse) and np.array_equal(mc, cc) and sc.shape == (mc.shape[0],)


@pytest.mark.parametrize("name", FINE_CASES)
def test_graph_and_stream_equal_the_eager_path(name, dev, tmp_path):
    """GraphedMatcher (backbone inside the graph) and estimate_matches_stream against the eager path of the same model, itself
    held to the oracle above: the same proposals in the same order, coordinates within 1e-3 px, scores within 1e-5.  The stream
    gets a batch of two pairs of equal sizes and different content, then a pair of other sizes."""
    from PIL import Image
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    net = _model(name)
    pa, pb = _pair_files()
    qa, qb = str(tmp_path / "1.png"), str(tmp_path / "2.png")
    Image.open(pa).transpose(Image.FLIP_LEFT_RIGHT).save(qa)
    Image.open(pb).transpose(Image.FLIP_TOP_BOTTOM).save(qb)
    pairs = [(pa, pb), (qa, qb), (pb, pa)]
    streamed = list(estimate_matches_stream(net, pairs, ksize=2, io_thres=0.0, batch=2, workers=2, imsize=256))
    assert len(streamed) == len(pairs)
    for (sm, ss, sc), (a, b) in zip(streamed, pairs):
        m, s, c = model_helper.estimate_matches(net, a, b, ksize=2, io_thres=0.0, eval_type="fine", imsize=256)
        assert c.shape[0] > 0 and np.array_equal(sc, c), f"{name}: the stream's proposals differ from the eager path's"
        assert np.array_equal(sm, m) and np.array_equal(ss, s), f"{name}: the stream's matches differ from the eager path's"
    im1, im2 = (t.to(dev) for t in br.images(name))
    g = GraphedMatcher(net, im1.shape[-2], im1.shape[-1], with_backbone=True)
    with torch.no_grad():
        fine, scores, coarse = net.predict_fine(im1, im2, ksize=2)
    gfine, gscores, gcoarse = g(im1, im2)
    assert coarse[0].shape[0] > 0 and torch.equal(gcoarse[0], coarse[0])
    assert (gfine[0] - fine[0]).abs().max() <= COORD_TOL and (gscores[0] - scores[0]).abs().max() <= SCORE_TOL


def test_single_plane_modes_on_resnet50(dev, monkeypatch):
    """set_mode('fp16') reaches every packed layer of a Bottleneck trunk and moves the pyramid only within the propagated
    single-plane bound; set_coarse_mode('fp16') at 1024 channels stays within the stage bound of tests/coarse_mode_reference.py."""
    import backbone_mode_reference as bm
    import coarse_mode_reference as cm
    name = "bottleneck_r50_s8"
    net = _model(name)
    monkeypatch.setenv("P2P_BACKBONE", "hip")
    im = br.images(name)[0]
    import copy
    cpu = copy.deepcopy(net.extract).cpu()
    try:
        net.extract.set_mode("fp16")
        with torch.no_grad():
            fast = net.extract.pyramid(im.to(dev))
        stem, trunk = net.extract._hip_trunk(dev)
        assert stem.mode == "fp16" and all(l.mode == "fp16" for blocks in trunk for layers in blocks for l in layers if l is not None)
    finally:
        net.extract.set_mode("fp16x2")
    with torch.no_grad():
        default = net.extract.pyramid(im.to(dev))
    levels, bounds = pyramid_yardstick(cpu, im, "fp16")
    for lv in range(1, 5):
        err = (fast[lv].cpu().double() - levels[lv]).abs()
        ratio = float((err / bounds[lv].clamp_min(1e-300)).max())
        print(f"mode fp16 level {lv}: max err / bound {ratio:.3f}")
        assert ratio <= 1.0
        assert not torch.equal(fast[lv], default[lv])
    p32, _ = _cpu_pyramids(name)
    fa, fb = p32[0][4], p32[1][4]
    sd = _ckpt(name)["state_dict"]
    try:
        net.set_coarse_mode("fp16")
        with torch.no_grad():
            corr, _ = net.forward_coarse_match(fa.to(dev), fb.to(dev), ksize=2)
    finally:
        net.set_coarse_mode("fp16x2")
    yd = cm.Yardstick(fa[0], fb[0], 2, sd, "fp16")
    ratio = float(((corr[0, 0].cpu().double() - yd.z).abs() / yd.e_z.clamp_min(1e-300)).max())
    print(f"coarse mode fp16 at 1024 channels: max err / bound {ratio:.4f}")
    assert ratio <= 1.0


def pyramid_yardstick(extract, image, mode):
    """tests/backbone_mode_reference.py's fp64 walk with the propagated bound of `mode`, over a block's own list of
    convolutions (BasicBlock: two, Bottleneck: three): -> (levels [5], bounds [5])."""
    import backbone_mode_reference as bm
    import torch.nn.functional as F

    def step(x, e, conv, bn, skip=None, e_skip=None, relu=True):
        wt, b, st, pad = conv.weight.data, bm._bn_of(bn), conv.stride[0], conv.padding[0]
        a, beta, mean = bm._fold(b)
        y = F.conv2d(x, wt.double(), None, st, pad) * a.view(1, -1, 1, 1) + (beta - mean * a).view(1, -1, 1, 1)
        sk_abs = None if skip is None else skip.abs() + e_skip
        eo = bm.layer_bound(x.abs() + e, wt, b, st, mode, sk_abs, pad) + bm.propagate(e, wt, b, st, pad)
        if skip is not None:
            y, eo = y + skip, eo + e_skip
        return (y.relu() if relu else y), eo

    x = image.double()
    e = torch.zeros_like(x)
    levels, bounds = [x], [e]
    x, e = step(x, e, extract.conv1, extract.bn1)
    levels.append(x); bounds.append(e)
    x, e = F.max_pool2d(x, 3, 2, 1), F.max_pool2d(e, 3, 2, 1)
    for name, _, _, _ in extract.stages:
        for blk in getattr(extract, name):
            skip, e_skip = x, e
            if blk.downsample is not None:
                skip, e_skip = step(x, e, blk.downsample[0], blk.downsample[1], relu=False)
            y, ey = x, e
            for c, b in blk.convs[:-1]:
                y, ey = step(y, ey, getattr(blk, c), getattr(blk, b))
            c, b = blk.convs[-1]
            x, e = step(y, ey, getattr(blk, c), getattr(blk, b), skip, e_skip)
        levels.append(x); bounds.append(e)
    return levels, bounds
