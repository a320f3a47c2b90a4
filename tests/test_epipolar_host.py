"""The epipolar evaluation (p2p_epipolar_batch, utils/eval/measure.py, networks/utils.py) without a GPU: the test
infrastructure against the unmodified reference's fixtures (tests/golden/epipolar_*.npz), the two conditions that keep the
error bound E honest, the argument checks of the Python layer and of the real library (none touches a device), the host
formatting of check_inliers_distr, and the documented import route."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import epipolar_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "patch2pix_amd")
GRID = [(c, dt) for c in er.CASES for dt in er.IN_DTYPES]


@pytest.fixture(scope="module")
def real_lib():
    """The real library, built if need be (importing the package needs it); nothing here launches a kernel."""
    from patch2pix_amd import build
    build.build(verbose=False)
    from patch2pix_amd import _lib
    return _lib


@pytest.mark.parametrize("case,dt", GRID, ids=[f"{c}-{dt}" for c, dt in GRID])
def test_restatement_equals_the_reference_and_condition_1(case, dt):
    """The fixture's inputs are the generator's; the literal numpy restatement equals the reference's distances bit for bit;
    condition 1: the reference's own result lies within E of the yardstick on every row; its counts are np.histogram's, and
    the reference has no undecidable row."""
    g, inp = np.load(er.golden_name(case)), er.inputs(case)
    assert np.array_equal(g["F"], inp["F"]) and np.array_equal(g[f"rows_{dt}"], inp["rows"][dt]), "the generator no longer gives the fixture's inputs"
    assert g[f"rows_{dt}"].dtype == inp["rows"][dt].dtype
    for kind, eps in er.NUMPY_CONFIGS:
        ref = g[f"np_{kind}_{dt}"]
        assert np.array_equal(er.restate_numpy(inp["rows"][dt], inp["F"], kind, eps).view(np.int64), ref.view(np.int64)), (kind, "restatement")
        d, e = er.yardstick(inp["rows"][dt], inp["F"], kind, eps)
        er.within(f"reference {case} {kind} {dt}", ref, d, e)
        with np.errstate(all="ignore"):
            assert np.array_equal(g[f"hist_{kind}_{dt}"], np.histogram(ref, er.DEFAULT_BINS)[0])
        assert bool(er.decidable(d, e, er.DEFAULT_BINS).all()) and bool(er.decidable(d, e, er.EVAL_BINS).all()), (kind, "undecidable rows")


@pytest.mark.parametrize("case", er.POSE_CASES)
def test_condition_2_and_bin_coverage(case):
    """Condition 2: E <= 1e-9 d on the rows with >= 1 px noise, for every configuration, input and output type (fp32 output:
    the half ulp of fp32 is the format's, 2^-24 d, and is left out of this comparison).  The Sampson distances of a pose case
    cover every default bin, and the zero-noise rows sit on the cancellation of dd (d below 1e-20)."""
    inp = er.inputs(case)
    big = inp["noise"] >= 1.0
    assert big.sum() == len(big) // 2
    for dt in er.IN_DTYPES:
        for kind, eps in er.CONFIGS:
            d, e = er.yardstick(inp["rows"][dt], inp["F"], kind, eps)
            worst = float((e[big] / d[big]).max())
            print(f"case {case} {kind} eps {eps:g} {dt}: max E / d on the >= 1 px rows {worst:.3g}")
            assert worst <= er.E_CAP
    d, _ = er.yardstick(inp["rows"]["f64"], inp["F"], "sampson", 1e-8)
    assert bool((np.histogram(d.astype(np.float64), er.DEFAULT_BINS)[0] > 0).all())
    assert float(d[inp["noise"] == 0].max()) < 1e-20


def test_ops_and_measure_argument_validation(real_lib):
    """ValueError for a malformed call, NotImplementedError for what the kernel does not do; CPU tensors, no device."""
    from patch2pix_amd import ops
    from patch2pix_amd.utils.eval import measure, model_helper
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    m, F = torch.zeros(1, 5, 4, dtype=torch.float64), np.eye(3)
    with pytest.raises(ValueError, match="monotonically"):
        ops.epipolar_batch(m, None, F, bins=[0, 5, 1])
    with pytest.raises(ValueError, match="monotonically"):
        ops.epi_edges([0, float("nan"), 1])
    with pytest.raises(ValueError, match="edges"):
        ops.epi_edges([1.0])
    with pytest.raises(NotImplementedError, match="bins"):
        ops.epi_edges(list(range(18)))
    assert ops.epi_edges(er.DEFAULT_BINS).dtype == np.float64 and ops.EPI_BINS_MEASURE == er.DEFAULT_BINS and ops.EPI_BINS_EVAL == er.EVAL_BINS
    for bad_F in (np.eye(4), np.zeros((2, 3, 3)), np.zeros(9)):
        with pytest.raises(ValueError, match="F must"):
            ops.epipolar_batch(m, None, bad_F)
    with pytest.raises(ValueError, match="kind"):
        ops.epipolar_batch(m, None, F, kind="sampson2")
    with pytest.raises(ValueError, match="eps"):
        ops.epipolar_batch(m, None, F, eps=-1.0)
    with pytest.raises(ValueError, match="matches"):
        ops.epipolar_batch(torch.zeros(5, 4), None, F)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.epipolar_batch(m, None, F, out_dtype=torch.float16)
    assert [ops.epi_kind(k) for k in ("sampson", "sym", "sym_sqrt")] == [er.KIND_CODE[k] for k in ("sampson", "sym", "sym_sqrt")] == [0, 1, 2]
    assert real_lib.DTYPES == {"float32": 0, "float64": 1, "int64": 2} == {f"{'float' if k[0] == 'f' else 'int'}{k[1:]}": v for k, v in er.DTYPE_CODE.items()}
    # measure: shapes, and homos=False with a third coordinate other than 1
    p = np.zeros((4, 2))
    with pytest.raises(ValueError, match="F must"):
        measure.sampson_distance(p[:0], p[:0], np.eye(4))
    with pytest.raises(ValueError, match="shape"):
        measure.sampson_distance(np.zeros((4, 3)), p, F)
    with pytest.raises(ValueError, match="points"):
        measure.symmetric_epipolar_distance(p, p[:3], F)
    h = np.concatenate([p, np.full((4, 1), 2.0)], axis=1)
    with pytest.raises(NotImplementedError, match="third coordinate"):
        measure.sampson_distance(h, h, F, homos=False)
    with pytest.raises(NotImplementedError, match="third coordinate"):
        measure.symmetric_epipolar_distance(torch.from_numpy(h), torch.from_numpy(h), F, homos=False, sqrt=True)
    assert np.array_equal(measure.expand_homo_ones(p), np.concatenate([p, np.ones((4, 1))], axis=1))
    assert measure.expand_homo_ones(p.T, axis=0).shape == (3, 4)
    assert measure.sampson_distance(p[:0], p[:0], F).shape == (0,) and measure.check_inliers_distr([]) == ''
    assert measure.check_inliers_distr([], return_ratios=True) == (None, '')
    # entry points: a fundamental matrix of the wrong shape, a sequence of the wrong length -- before any work
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        model_helper.estimate_matches_device(None, "a.jpg", "b.jpg", fundamental=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="2 matrices for 1 pairs"):
        next(estimate_matches_stream(None, [("a.jpg", "b.jpg")], fundamentals=[np.eye(3), np.eye(3)]))
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        next(estimate_matches_stream(None, [("a.jpg", "b.jpg")], fundamentals=[np.zeros(9)]))


def test_entry_point_argument_errors(real_lib):
    """The argument checks of the REAL library: P2P_EINVAL (-1) / P2P_EUNSUPPORTED (-3) before the device is touched
    (placeholder addresses, no GPU here)."""
    lib = er.bind(real_lib.lib)
    p = ctypes.c_void_p(256)

    def call(matches=p, mdt=1, counts=p, F=p, batch=2, stride=4, kind=0, eps=1e-8, edges=None, nbins=0, dist=p, ddt=1, hist=None):
        return lib.p2p_epipolar_batch(matches, mdt, counts, F, batch, stride, kind, eps, edges, nbins, dist, ddt, hist, None)

    for null in ("matches", "counts", "F", "dist"):
        assert call(**{null: None}) == -1 and b"null" in lib.p2p_last_error()
    assert call(batch=0) == -1 and call(batch=65536) == -1 and call(stride=0) == -1
    assert call(mdt=3) == -1 and call(ddt=2) == -1 and call(kind=4) == -1 and call(kind=-1) == -1
    assert call(eps=-1.0) == -1 and call(eps=float("nan")) == -1
    assert call(hist=p, nbins=3) == -1 and call(edges=p, nbins=3) == -1 and call(edges=p, hist=p, nbins=0) == -1
    assert call(edges=p, hist=p, nbins=17) == -3 and b"17 bins" in lib.p2p_last_error()
    assert real_lib.p2p_version() & ~real_lib.VERSION_EXPERIMENT >= 109 and "p2p_epipolar_batch" in real_lib.EXPORTS


def test_check_inliers_distr_string_from_golden_histograms(real_lib):
    """Host formatting only: the reference's strings and ratios (tests/golden/epipolar_distr.npz), character for character,
    from the per-pair counts stored beside them -- as arrays, and as the EpipolarReport list an evaluation loop collects."""
    from patch2pix_amd.utils.eval import measure
    g = np.load(os.path.join(er.GOLDEN_DIR, "epipolar_distr.npz"))
    order = [str(c) for c in g["order"]]
    npts = [len(er.inputs(c)["noise"]) for c in order]
    for name in ("default", "eval"):
        bins = er.DEFAULT_BINS if name == "default" else er.EVAL_BINS
        assert np.array_equal(g[f"bins_{name}"], np.array(bins, dtype=np.float64))
        ratios, text = measure.format_inliers_distr(g[f"hists_{name}"], npts, len(order) + 1, bins, tag=str(g[f"tag_{name}"]), return_ratios=True)
        assert text == str(g[f"text_{name}"]), (text, str(g[f"text_{name}"]))
        assert np.array_equal(np.array(ratios), g[f"ratios_{name}"])
        # the same through check_inliers_distr with reports that carry these counts (no launch: the stored counts are used)
        reports = [measure.EpipolarReport(np.zeros(n), np.zeros(n), h, h, bins, n) for n, h in zip(npts, g[f"hists_{name}"])]
        reports.insert(int(g["empty_at"]), measure.EpipolarReport(np.empty(0), np.empty(0), np.zeros(len(bins) - 1, np.int64),
                                                                  np.zeros(len(bins) - 1, np.int64), bins, 0))
        assert measure.check_inliers_distr(reports, bins=bins, tag=str(g[f"tag_{name}"])) == str(g[f"text_{name}"])
        assert measure.check_inliers_distr(reports, bins=bins, tag="cdist", return_ratios=True)[0] == ratios


def test_measure_imports_through_the_documented_route(tmp_path):
    """utils.eval.measure and the two new names of networks.utils through <repo>/patch2pix_amd on sys.path, in a fresh
    interpreter; the reference's signatures."""
    code = f"""
import sys
sys.path.append({PKG!r})
from utils.eval.measure import expand_homo_ones, sampson_distance, symmetric_epipolar_distance, check_inliers_distr
from networks.utils import sym_epi_dist, sampson_dist, filter_coarse
import utils.eval.measure as m, patch2pix_amd.utils.eval.measure as q
import inspect
assert m is q
assert list(inspect.signature(sampson_distance).parameters) == ['pts1', 'pts2', 'F', 'homos', 'eps']
assert list(inspect.signature(symmetric_epipolar_distance).parameters) == ['pts1', 'pts2', 'F', 'homos', 'sqrt']
assert list(inspect.signature(check_inliers_distr).parameters)[:4] == ['inlier_dists', 'bins', 'tag', 'return_ratios']
assert inspect.signature(check_inliers_distr).parameters['bins'].default == [0, 1e-2, 1, 5, 10, 25, 50, 100, 400, 2500, 1e5]
assert list(inspect.signature(sym_epi_dist).parameters) == ['matches', 'F', 'sqrt', 'eps']
assert list(inspect.signature(sampson_dist).parameters) == ['matches', 'F', 'eps']
assert not hasattr(m, 'eval_matches_relapose')
assert {ROOT!r} not in sys.path
print("IMPORT_OK")
"""
    res = subprocess.run([sys.executable, "-W", "error::ImportWarning", "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0 and "IMPORT_OK" in res.stdout, res.stderr[-3000:]
