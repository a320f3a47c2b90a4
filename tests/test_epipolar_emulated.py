"""The epipolar evaluation (epipolar_kernel of csrc/epipolar.hip behind p2p_epipolar_batch) executed on the CPU by the
test-suite's HIP stand-in (tests/hipemu) over every case x kind x input type x output type of tests/epipolar_reference.py:
distances within the derived bound E of the np.longdouble yardstick, bin counts equal to np.histogram's and, on the decidable
rows, to those of the unmodified reference's distances (tests/golden/epipolar_*.npz); the smallest shapes at which the kernel
can go wrong; a pair alone equal to the pair in any batch, slot and stride, bit for bit; every argument error of the header."""
import ctypes
import os
import sys

import numpy as np
import pytest

import epipolar_reference as er

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402

GRID = [(c, k, e, dt, out) for c in er.CASES for k, e in er.CONFIGS for dt in er.IN_DTYPES for out in er.OUT_DTYPES]
IDS = [f"{c}-{k}-eps{e:g}-{dt}-{out}" for c, k, e, dt, out in GRID]


@pytest.fixture(scope="module")
def emu():
    return er.bind(emu_lib.load())


@pytest.mark.parametrize("case,kind,eps,dt,out", GRID, ids=IDS)
def test_case_table(case, kind, eps, dt, out, emu):
    er.check_case(emu, case, kind, eps, dt, out)


def test_batch_slot_and_stride_identity(emu):
    er.check_batch_identity(emu)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts(n, emu):
    """n rows in a stride of n + 5 (stride > n; n = 0 in a stride of 5): the first n distances within E, the others untouched,
    the counts np.histogram's of those n."""
    inp = er.inputs("Q")
    rows, F = inp["rows"]["f64"][::5][:n], inp["F"]          # every fifth row: all four noise levels
    dist, hist = er.run(emu, [(rows, F)], "sampson", 1e-8, bins=er.DEFAULT_BINS, stride=n + 5, in_dtype=np.float64)
    assert bool((dist[0, n:] == er.FILL).all()) and hist.sum() <= n
    if n:
        d, e = er.yardstick(rows, F, "sampson", 1e-8)
        er.within(f"n = {n}", dist[0, :n], d, e)
        assert np.array_equal(hist[0], np.histogram(dist[0, :n], er.DEFAULT_BINS)[0]) and hist.sum() == n
    else:
        assert bool((hist == 0).all())


def test_batch_of_three_with_counts_0_1_300(emu):
    a = er.inputs("P")
    rows, F = a["rows"]["f64"], a["F"]
    dist, hist = er.run(emu, [(rows[:0], F), (rows[200:201], F), (rows, F)], "sym", 1e-8, bins=er.DEFAULT_BINS, in_dtype=np.float64)
    assert dist.shape == (3, 300) and bool((dist[0] == er.FILL).all()) and bool((dist[1, 1:] == er.FILL).all())
    assert hist.sum(axis=1).tolist() == [0, 1, 300]
    d, e = er.yardstick(rows, F, "sym", 1e-8)
    er.within("count 300", dist[2], d, e)
    er.within("count 1", dist[1, :1], d[200:201], e[200:201])


def test_minus_one_passes_through(emu):
    """counts[b] = -1: the hist row is zeros and the dist row keeps what it held; with and without a histogram."""
    a = er.inputs("P")
    for bins in (er.DEFAULT_BINS, None):
        dist, hist = er.run(emu, [(None, a["F"]), (a["rows"]["i64"][:5], a["F"])], "sampson", 1e-8, bins=bins, stride=7, in_dtype=np.int64)
        assert bool((dist[0] == er.FILL).all()) and bool((dist[1, :5] != er.FILL).all()) and bool((dist[1, 5:] == er.FILL).all())
        if bins is not None:
            assert bool((hist[0] == 0).all()) and hist[1].sum() == 5


def _values_as_rows(values):
    """Rows whose symmetric square-root distance under F = [e_x]x is exactly the given value v >= 0: l1 = (0, 1, -y2), l2 =
    (0, -1, y1), dd = y1 - y2, d = |y1 - y2| (1 / 1 + 1 / 1) = 2 |v / 2| with eps = 0 -- every step exact."""
    rows = np.zeros((len(values), 4))
    rows[:, 1] = np.asarray(values, dtype=np.float64) / 2
    return rows, np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])


def test_values_on_edges_nan_and_out_of_range(emu):
    """A value exactly on an inner edge opens the bin to its right, a value exactly on the last edge belongs to the last bin;
    NaN, infinity and values beyond the edges are in no bin.  nbins 1 and 16."""
    edges16 = [0.5 * i for i in range(1, 18)]          # 0.5 .. 8.5: 16 bins, every edge an exact distance
    values = [0.25, 0.5, 0.75, 1.0, 4.0, 8.25, 8.5, 8.75, 1e9]
    rows, F = _values_as_rows(values)
    dist, hist = er.run(emu, [(rows, F)], "sym_sqrt", 0.0, bins=edges16, in_dtype=np.float64)
    assert np.array_equal(dist[0], np.array(values)), "the probe distances are not exact"
    want = np.histogram(np.array(values), edges16)[0]
    assert hist.shape == (1, 16) and np.array_equal(hist[0], want) and hist.sum() == 6
    assert hist[0, 0] == 2 and hist[0, 1] == 1 and hist[0, 7] == 1 and hist[0, 15] == 2          # 0.5, 0.75 | 1.0 | 4.0 | 8.25, 8.5
    dist, hist = er.run(emu, [(rows, F)], "sym_sqrt", 0.0, bins=[0.5, 8.5], in_dtype=np.float64)
    assert hist.shape == (1, 1) and hist[0, 0] == 6
    # NaN: F = 0 without eps
    dist, hist = er.run(emu, [(rows, np.zeros((3, 3)))], "sym_sqrt", 0.0, bins=edges16, in_dtype=np.float64)
    assert bool(np.isnan(dist).all()) and hist.sum() == 0
    # the value-only kind stores and bins the first column
    values += [np.inf, -1.0, np.nan]
    probe = np.zeros((len(values), 4))
    probe[:, 0] = values
    dist, hist = er.run(emu, [(probe, F)], "value", 0.0, bins=edges16, in_dtype=np.float64)
    assert np.array_equal(dist[0], np.array(values), equal_nan=True) and np.array_equal(hist[0], want)


def test_argument_errors(emu):
    """Every P2P_EINVAL (-1) / P2P_EUNSUPPORTED (-3) of the header, before a kernel runs (placeholder addresses)."""
    p = ctypes.c_void_p(256)

    def call(matches=p, mdt=1, counts=p, F=p, batch=2, stride=4, kind=0, eps=1e-8, edges=None, nbins=0, dist=p, ddt=1, hist=None):
        return emu.p2p_epipolar_batch(matches, mdt, counts, F, batch, stride, kind, eps, edges, nbins, dist, ddt, hist, None)

    for null in ("matches", "counts", "F", "dist"):
        assert call(**{null: None}) == -1 and b"null" in emu.p2p_last_error()
    for batch in (0, -1, 65536):
        assert call(batch=batch) == -1 and b"bad sizes" in emu.p2p_last_error()
    assert call(stride=0) == -1 and call(stride=-3) == -1
    for mdt in (-1, 3):
        assert call(mdt=mdt) == -1 and b"matches dtype" in emu.p2p_last_error()
    for ddt in (-1, 2, 3):
        assert call(ddt=ddt) == -1 and b"dist dtype" in emu.p2p_last_error()
    for kind in (-1, 4, 16):
        assert call(kind=kind) == -1 and b"kind" in emu.p2p_last_error()
    for eps in (-1e-8, float("nan"), -float("inf")):
        assert call(eps=eps) == -1 and b"eps" in emu.p2p_last_error()
    assert call(hist=p, nbins=3) == -1 and b"go together" in emu.p2p_last_error()
    assert call(edges=p, nbins=3) == -1 and b"go together" in emu.p2p_last_error()
    assert call(edges=p, hist=p, nbins=0) == -1 and call(nbins=2) == -1
    assert call(edges=p, hist=p, nbins=17) == -3 and b"17 bins" in emu.p2p_last_error()
