"""The epipolar evaluation on the MI355X: the case table of tests/epipolar_reference.py through the real library at the bars
of tests/test_epipolar_emulated.py, the batch / slot / stride bit-identity, the reference's names (networks.utils.sampson_dist /
sym_epi_dist on device tensors, utils.eval.measure with numpy in and out, check_inliers_distr), and the two entry points that
carry a fundamental matrix (estimate_matches_device, estimate_matches_stream).
Needs an MI355X:  pytest -m gpu"""
import os

import numpy as np
import pytest
import torch

import epipolar_reference as er
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu

GRID = [(c, k, e, dt, out) for c in er.CASES for k, e in er.CONFIGS for dt in er.IN_DTYPES for out in er.OUT_DTYPES]
IDS = [f"{c}-{k}-eps{e:g}-{dt}-{out}" for c, k, e, dt, out in GRID]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from patch2pix_amd import _lib
    return er.bind(_lib.lib)


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """Three 96x128 synthetic pairs on disk and a fundamental matrix each (any 3x3 matrix serves: the distances are compared
    with the yardstick under the same matrix)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("epipolar_pairs")
    out = []
    for i in range(3):
        a, b = synthetic.make_image_pair(500 + i, 96, 128)
        pa, pb = str(root / f"{i}a.png"), str(root / f"{i}b.png")
        Image.fromarray(a).save(pa)
        Image.fromarray(b).save(pb)
        F = er.inputs("P")["F"] * (1.0 + i)
        F[2, 2] += 0.01 * i
        out.append((pa, pb, F))
    return out


@pytest.mark.parametrize("case,kind,eps,dt,out", GRID, ids=IDS)
def test_case_table(case, kind, eps, dt, out, lib, dev):
    er.check_case(lib, case, kind, eps, dt, out, device=dev)


def test_batch_slot_and_stride_identity(lib, dev):
    er.check_batch_identity(lib, device=dev)


def test_minus_one_and_zero_counts(lib, dev):
    a = er.inputs("P")
    dist, hist = er.run(lib, [(None, a["F"]), (a["rows"]["f64"][:0], a["F"]), (a["rows"]["f64"][:70], a["F"])], "sampson", 1e-8,
                        bins=er.DEFAULT_BINS, stride=80, device=dev, in_dtype=np.float64)
    assert bool((dist[:2] == er.FILL).all()) and bool((dist[2, 70:] == er.FILL).all()) and hist.sum(axis=1).tolist() == [0, 0, 70]


@pytest.mark.parametrize("dt", er.IN_DTYPES)
def test_networks_utils_names(dt, dev):
    """networks.utils.sampson_dist / sym_epi_dist on device tensors of the three input types: float32 [N] on the device, the
    kernel's fp64 result rounded once -- within E (with its half fp32 ulp) of the yardstick.  The reference's own fp32 torch
    result (the fixture; F as float32) is printed beside it: its error is larger and is not the bar.  sym_epi_dist ignores
    `sqrt` like the reference (networks/utils.py:88)."""
    from patch2pix_amd.networks import utils as nutils
    for case in er.POSE_CASES:
        inp, g = er.inputs(case), np.load(er.golden_name(case))
        rows = torch.from_numpy(inp["rows"][dt]).to(dev)
        F = torch.from_numpy(inp["F"]).to(dev)
        for name, kind, fn in (("sampson", "sampson", nutils.sampson_dist), ("sym", "sym", nutils.sym_epi_dist)):
            got = fn(rows, F)
            assert got.dtype == torch.float32 and got.is_cuda and got.shape == (len(rows),)
            d, e = er.yardstick(inp["rows"][dt], inp["F"], kind, 1e-8, out="f32")
            er.within(f"networks.utils {name} {case} {dt}", got.cpu().numpy(), d, e)
            ref = g[f"t_{name}_{dt}"].astype(np.longdouble)
            big = inp["noise"] >= 1.0
            print(f"    the reference's fp32 result: max relative error {float((abs(ref - d)[big] / d[big]).max()):.3g} on the >= 1 px rows, "
                  f"ours {float((abs(got.cpu().numpy().astype(np.longdouble) - d)[big] / d[big]).max()):.3g}")
        assert torch.equal(nutils.sym_epi_dist(rows, F, sqrt=True), nutils.sym_epi_dist(rows, F, sqrt=False))
        assert torch.equal(nutils.sym_epi_dist(rows, inp["F"]), nutils.sym_epi_dist(rows, F))          # F from the host
    empty = nutils.sampson_dist(rows[:0], F)
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda


def test_measure_names_numpy_and_tensors(dev):
    """utils.eval.measure: numpy in -> float64 numpy out, device tensors in -> float64 device tensor out, both within E of the
    yardstick and equal to each other bit for bit; homos=False with ones; check_inliers_distr on arrays == the reference's
    string and ratios (tests/golden/epipolar_distr.npz) where no row is undecidable."""
    from patch2pix_amd.utils.eval import measure
    sampson = {}
    for case in er.CASES:
        inp = er.inputs(case)
        rows, F = inp["rows"]["f64"], inp["F"]
        for kind, eps in er.NUMPY_CONFIGS:
            fn = {"sampson": lambda a, b, F, **k: measure.sampson_distance(a, b, F, **k),
                  "sym": lambda a, b, F, **k: measure.symmetric_epipolar_distance(a, b, F, **k),
                  "sym_sqrt": lambda a, b, F, **k: measure.symmetric_epipolar_distance(a, b, F, sqrt=True, **k)}[kind]
            got = fn(rows[:, 0:2], rows[:, 2:4], F)
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (len(rows),)
            d, e = er.yardstick(rows, F, kind, eps)
            er.within(f"measure {kind} {case}", got, d, e)
            t = torch.from_numpy(rows).to(dev)
            dev_got = fn(t[:, 0:2], t[:, 2:4], torch.from_numpy(F).to(dev))
            assert dev_got.is_cuda and dev_got.dtype == torch.float64
            assert np.array_equal(dev_got.cpu().numpy().view(np.int64), got.view(np.int64))
            homo = fn(measure.expand_homo_ones(rows[:, 0:2]), measure.expand_homo_ones(rows[:, 2:4]), F, homos=False)
            assert np.array_equal(homo.view(np.int64), got.view(np.int64))
            if kind == "sampson":
                sampson[case] = got
    g = np.load(os.path.join(er.GOLDEN_DIR, "epipolar_distr.npz"))
    order = [str(c) for c in g["order"]]
    dists = [sampson[c] for c in order]
    dists.insert(int(g["empty_at"]), np.empty(0))
    for name, bins in (("default", er.DEFAULT_BINS), ("eval", er.EVAL_BINS)):
        for c in order:
            inp = er.inputs(c)
            d, e = er.yardstick(inp["rows"]["f64"], inp["F"], "sampson", 1e-8)
            assert bool(er.decidable(d, e, bins).all())
        ratios, text = measure.check_inliers_distr(dists, bins=bins, tag=str(g[f"tag_{name}"]), return_ratios=True)
        assert text == str(g[f"text_{name}"]), (text, str(g[f"text_{name}"]))
        assert np.array_equal(np.array(ratios), g[f"ratios_{name}"])
        assert measure.check_inliers_distr([torch.from_numpy(x).to(dev) for x in dists], bins=bins, tag=str(g[f"tag_{name}"])) == text


def _check_report(rep, m, c, F, bins):
    """fdist / cdist within E of the yardstick on the returned rows; counts np.histogram's of them, summing to the rows when no
    distance falls outside the bins."""
    assert rep.n == len(m) == len(c) and list(rep.bins) == list(bins)
    for dist, hist, rows, what in ((rep.fdist, rep.fhist, m, "fdist"), (rep.cdist, rep.chist, c, "cdist")):
        assert dist.dtype == np.float64 and dist.shape == (len(rows),) and hist.dtype == np.int64 and hist.shape == (len(bins) - 1,)
        d, e = er.yardstick(rows, F, "sampson", 1e-8)
        er.within(what, dist, d, e)
        assert np.array_equal(hist, np.histogram(dist, bins)[0])
        inside = int(((dist >= bins[0]) & (dist <= bins[-1])).sum())
        assert hist.sum() <= len(rows) and hist.sum() == inside


def test_estimate_matches_device_with_fundamental(net, pairs, dev):
    """With a [3,3] F the call returns a fourth value, the EpipolarReport; the first three equal the call without it bit for bit
    (both calls get the SAME pyramids through a memo: MIOpen may pick another convolution algorithm from one call to the next)."""
    from patch2pix_amd.utils.eval import measure, model_helper
    pa, pb, F = pairs[0]
    memo, real_pyramid = {}, net.extract.pyramid

    def pyramid(im):
        key = (tuple(im.shape), float(im.double().sum()))
        if key not in memo:
            memo[key] = real_pyramid(im)
        return memo[key]
    net.extract.pyramid = pyramid
    try:
        plain = model_helper.estimate_matches_device(net, pa, pb, ksize=2, io_thres=0.25)
        with_f = model_helper.estimate_matches_device(net, pa, pb, ksize=2, io_thres=0.25, fundamental=F)
        custom = model_helper.estimate_matches_device(net, pa, pb, ksize=2, io_thres=0.25, fundamental=torch.from_numpy(F), bins=[0, 1, 1e12])
    finally:
        net.extract.pyramid = real_pyramid
    assert len(plain) == 3 and len(with_f) == 4 and plain[0].shape[0] > 0
    for x, y in zip(plain, with_f):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    rep = with_f[3]
    assert isinstance(rep, measure.EpipolarReport)
    _check_report(rep, with_f[0], with_f[2], F, er.EVAL_BINS)
    _check_report(custom[3], custom[0], custom[2], F, [0, 1, 1e12])
    assert custom[3].fhist.sum() == len(custom[0])          # nothing falls outside [0, 1e12]
    # the report is what the numpy route gives on the returned rows, bit for bit
    again = measure.sampson_distance(with_f[0][:, 0:2], with_f[0][:, 2:4], F)
    assert np.array_equal(again.view(np.int64), rep.fdist.view(np.int64))
    text = measure.check_inliers_distr([rep], bins=er.EVAL_BINS, tag="fdist")
    assert text == measure.check_inliers_distr([rep.fdist], bins=er.EVAL_BINS, tag="fdist")
    assert measure.check_inliers_distr([rep], bins=er.EVAL_BINS, tag="cdist") == measure.check_inliers_distr([rep.cdist], bins=er.EVAL_BINS, tag="cdist")


def test_estimate_matches_stream_with_fundamentals(net, pairs, dev):
    """Three small pairs in batches of two: every item carries the report of its own rows -- equal, bit for bit, to the
    per-pair evaluation of those rows (a pair's distances do not depend on its batch, slot or stride); without `fundamentals`
    the items stay triples."""
    from patch2pix_amd.utils.eval import measure
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    items = list(estimate_matches_stream(net, [(a, b) for a, b, _ in pairs], ksize=2, io_thres=0.25, batch=2, workers=2,
                                         fundamentals=[F for _, _, F in pairs]))
    assert len(items) == 3
    for (m, s, c, rep), (_, _, F) in zip(items, pairs):
        assert m.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64 and len(m) > 0
        _check_report(rep, m, c, F, er.EVAL_BINS)
        for rows, dist in ((m, rep.fdist), (c, rep.cdist)):
            alone = measure.sampson_distance(rows[:, 0:2], rows[:, 2:4], F)
            assert np.array_equal(alone.view(np.int64), dist.view(np.int64))
    plain = list(estimate_matches_stream(net, [(a, b) for a, b, _ in pairs[:1]], ksize=2, io_thres=0.25, batch=2, workers=2))
    assert len(plain) == 1 and len(plain[0]) == 3
    with pytest.raises(ValueError, match="device path"):
        next(estimate_matches_stream(net, [(a, b) for a, b, _ in pairs], device_filter=False, fundamentals=[F for _, _, F in pairs]))
