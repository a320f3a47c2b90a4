"""TEST INFRASTRUCTURE: what the tests of the epipolar evaluation (p2p_epipolar_batch; utils/eval/measure.py and
networks/utils.py of the package) share -- the case table, the seeded inputs, the yardstick (the three formulas of reference
utils/eval/measure.py:18-71 / networks/utils.py:74-110 restated in np.longdouble), the error bound E that is carried beside it,
a literal restatement of the reference's numpy expressions, a ctypes binding of the entry point that works on either library
handle (the real one with device tensors, the CPU emulator's with host tensors) and the checks the emulated and the GPU test
both run.

The bound E (a derivation; nothing in it is measured).  u = 2^-53.  Inputs are exact: F is fp64, and every coordinate type
widens to fp64 without rounding (|int64| < 2^53 here).  First-order running error analysis, every quantity taken at the
yardstick's value; a bound is stated for ANY evaluation order with or without fused operations, so that it holds for the
library's documented order (include/p2p_hip.h) and for the reference's numpy expression (np.dot, left-to-right sums) alike:
  * a sum of k products, each product or term passing through at most n roundings (its own multiplication and the additions
    that follow it), has |error| <= n u sum|terms| + sum |factor| E(other factor).  A line coordinate l = a x + b y + c: n = 3,
    E_l = 3u (|a x| + |b y| + |c|).  dd = x2 l2_0 + y2 l2_1 + l2_2: n = 3 plus the inherited |x2| E(l2_0) + |y2| E(l2_1) + E(l2_2)
    -- this is where the zero-noise rows live: dd cancels to nothing while its terms are of order |F| 10^6;
  * a denominator eps + (sum of m squares), m = 2 or 4: each square is rounded once and then passes through at most m
    additions (the reference adds left to right, eps first): n = m + 1, E_den = (m + 1) u den + sum 2 |l| E_l;
  * sq = dd^2: (dd + t)^2 - dd^2 = 2 dd t + t^2 exactly, and on the zero-noise rows |dd| is SMALLER than E_dd, so the square of
    the inherited error is the leading term there and is kept: E_sq = u (|dd| + E_dd)^2 + 2 |dd| E_dd + E_dd^2 (the one place
    where first order is not enough);   a quotient q = a / b: E_q = u |q| + E_a / |b| + |q| E_b / |b|;   a sum or product of
    two results: u |result| + the propagated terms;   sqrt (within one ulp in the device library's documentation, correctly
    rounded in numpy): E = 2u sqrt(e) + E_e / (2 sqrt(e));
  * an fp32 result adds half an fp32 ulp, <= 2^-24 |d| (+ 2^-150 for the subnormal range).
The total is multiplied by 1 + 2^-10 for the second-order terms and for the yardstick's own roundings (2^-64 on x86, 2^-11 of
each term above).  Where the yardstick is not finite (0 / 0, x / 0 with eps = 0) there is no bound: the result must be the same
NaN / the same infinity.

Two conditions keep E honest; tests/test_epipolar_host.py checks both:
  1. the REFERENCE'S OWN numpy result (tests/golden/epipolar_*.npz) lies within E of the yardstick on every row of every case;
  2. on the rows of the pose cases with >= 1 px noise, E <= 1e-9 d (E_CAP).  Coordinates of order 1e3 times a few dozen u give
     about 1e-12 relative to a distance of a pixel, so the cap is loose by three orders -- for rows that are not by chance on
     their epipolar line: dd -> 0 makes 2 E_dd / |dd| unbounded.  The family therefore redraws the noise of a >= 1 px row until
     both of its points are at least NOISE_FLOOR = 0.05 px from their epipolar lines, in all three input types.

Histogram decidability: a row whose yardstick distance is within E of a bin edge may fall on either side; such rows are
removed before counts are compared (an edge <= 0 decides every row: each kind is a square or an absolute value times a
non-negative factor, >= +0 in any arithmetic), at most 1 % (MAX_UNDECIDABLE) of a case's rows may be such, and with these families the
reference has none."""
import ctypes
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble
U = LD(2.0) ** -53
E_CAP = 1e-9
NOISE_FLOOR = 0.05
MAX_UNDECIDABLE = 0.01
NOISES = (0.0, 1e-3, 1.0, 30.0)
DEFAULT_BINS = [0, 1e-2, 1, 5, 10, 25, 50, 100, 400, 2500, 1e5]          # measure.py:116
EVAL_BINS = [0, 1e-2, 1, 5, 10, 25, 50, 100, 2500, 1e5]                  # eval_epoch_immatch.py:85

KIND_CODE = {"sampson": 0, "sym": 1, "sym_sqrt": 2, "value": 3}           # P2P_EPI_* of include/p2p_hip.h
DTYPE_CODE = {"f32": 0, "f64": 1, "i64": 2}                               # P2P_F32 / _F64 / _I64
TORCH_DTYPE = {"f32": torch.float32, "f64": torch.float64, "i64": torch.int64}
IN_DTYPES = ("f64", "f32", "i64")
OUT_DTYPES = ("f64", "f32")
# (kind, eps): the four reference functions -- measure.sampson_distance, measure.symmetric_epipolar_distance without and with
# sqrt (no eps), networks.utils.sym_epi_dist / sampson_dist (eps 1e-8) -- and the square-root form with eps, which only the
# dead branch of networks/utils.py:90 spells
CONFIGS = (("sampson", 1e-8), ("sym", 0.0), ("sym_sqrt", 0.0), ("sym", 1e-8), ("sym_sqrt", 1e-8))
NUMPY_CONFIGS = CONFIGS[:3]                                               # what utils/eval/measure.py computes

# id -> family, rows per noise level, seed.  Row counts: 300 = 4 x 75 (one work-group, two waves used), 1300 > the 1024 threads
# of a work-group (a second round of the row loop)
CASES = {
    "P": dict(family="pose", per_noise=75, seed=2301, unit_norm=False),          # F = K2^-T [t]x R K1^-1 as it comes (|F| ~ 1e-6)
    "Q": dict(family="pose", per_noise=325, seed=2302, unit_norm=True),          # scaled to |F| = 1
    "Z0": dict(family="zero", per_noise=8, seed=2303),                           # F = 0: d = 0 with eps, NaN without
    "Z1": dict(family="row0", per_noise=8, seed=2304),                           # first row of F zero: l2_0 = 0
    "Z2": dict(family="row2", per_noise=8, seed=2305),                           # only the last row: l2 = (0, 0, c), x / 0 without eps
}
POSE_CASES = ("P", "Q")

_inputs = {}


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _rotation(w):
    th = np.linalg.norm(w)
    k = _skew(w / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def _variants(rows):
    """The three input types of one set of rows: as they are, rounded to float32, truncated to int64."""
    return {"f64": rows, "f32": rows.astype(np.float32), "i64": np.trunc(rows).astype(np.int64)}


def _offsets(F, rows):
    """Distance (px) of each row's second point from l2 = F x1 and of its first point from l1 = F^T x2, plain fp64 (the
    generator's own acceptance test; not the yardstick)."""
    rows = rows.astype(np.float64)
    p1 = np.concatenate([rows[:, 0:2], np.ones((len(rows), 1))], axis=1)
    p2 = np.concatenate([rows[:, 2:4], np.ones((len(rows), 1))], axis=1)
    l2, l1 = p1 @ F.T, p2 @ F
    dd = np.abs((l2 * p2).sum(axis=1))
    return np.minimum(dd / np.hypot(l2[:, 0], l2[:, 1]), dd / np.hypot(l1[:, 0], l1[:, 1]))


def inputs(case):
    """dict(F [3,3] fp64, rows {f64, f32, i64: [n,4]}, noise [n] px) of a case, built once from its seed and never modified.
    Pose families: a relative pose (rotation of up to 0.35 rad, unit baseline), intrinsics with focal lengths in [500, 1200]
    and the principal point of a 480x640 frame, 3-D points 3 to 8 baselines in front of the first camera, their projections
    plus Gaussian noise of 0, 1e-3, 1 and 30 px per coordinate (redrawn for the >= 1 px rows until both points are
    NOISE_FLOOR from their epipolar lines in all three input types)."""
    if case in _inputs:
        return _inputs[case]
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    R, t = _rotation(rng.uniform(-0.2, 0.2, 3)), rng.normal(size=3)
    t /= np.linalg.norm(t)
    K1, K2 = (np.array([[rng.uniform(500, 1200), 0, 320.0], [0, rng.uniform(500, 1200), 240.0], [0, 0, 1]]) for _ in range(2))
    F = np.linalg.inv(K2).T @ _skew(t) @ R @ np.linalg.inv(K1)
    if c.get("unit_norm"):
        F = F / np.linalg.norm(F)
    n = 4 * c["per_noise"]
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n), rng.uniform(3, 8, n)], axis=1)
    X2 = X @ R.T + t
    clean = np.concatenate([(X @ K1.T)[:, :2] / X[:, 2:], (X2 @ K2.T)[:, :2] / X2[:, 2:]], axis=1)
    noise = np.repeat(np.array(NOISES), c["per_noise"])
    rows = clean + noise[:, None] * rng.normal(size=(n, 4))
    if c["family"] == "zero":
        F = np.zeros((3, 3))
    elif c["family"] == "row0":
        F = F.copy(); F[0] = 0.0
    elif c["family"] == "row2":
        F = F.copy(); F[:2] = 0.0
    if c["family"] == "pose":
        for _ in range(100):
            bad = (noise >= 1.0) & (np.min([_offsets(F, v) for v in _variants(rows).values()], axis=0) < NOISE_FLOOR)
            if not bad.any():
                break
            rows[bad] = clean[bad] + noise[bad, None] * rng.normal(size=(int(bad.sum()), 4))
        assert not bad.any(), f"case {case}: rows left within {NOISE_FLOOR} px of their epipolar line"
    _inputs[case] = dict(F=np.ascontiguousarray(F), rows=_variants(rows), noise=noise)
    return _inputs[case]


def yardstick(rows, F, kind, eps, out="f64"):
    """(d, E): the formula in np.longdouble and the bound of the module docstring, per row.  Where d is not finite E is NaN."""
    with np.errstate(all="ignore"):
        r, f, eps = rows.astype(LD), F.astype(LD), LD(eps)
        x1, y1, x2, y2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]

        def line(a, b, c, x, y):
            return a * x + b * y + c, 3 * U * (abs(a * x) + abs(b * y) + abs(c))

        l20, e20 = line(f[0, 0], f[0, 1], f[0, 2], x1, y1)
        l21, e21 = line(f[1, 0], f[1, 1], f[1, 2], x1, y1)
        l22, e22 = line(f[2, 0], f[2, 1], f[2, 2], x1, y1)
        l10, e10 = line(f[0, 0], f[1, 0], f[2, 0], x2, y2)
        l11, e11 = line(f[0, 1], f[1, 1], f[2, 1], x2, y2)
        dd = x2 * l20 + y2 * l21 + l22
        e_dd = 3 * U * (abs(x2 * l20) + abs(y2 * l21) + abs(l22)) + abs(x2) * e20 + abs(y2) * e21 + e22
        s1, s2 = l10 * l10 + l11 * l11, l20 * l20 + l21 * l21
        p1, p2 = 2 * (abs(l10) * e10 + abs(l11) * e11), 2 * (abs(l20) * e20 + abs(l21) * e21)      # inherited by s1, s2
        sq, e_sq = dd * dd, U * (abs(dd) + e_dd) ** 2 + 2 * abs(dd) * e_dd + e_dd * e_dd
        if kind == "sampson":
            den = eps + s1 + s2
            e_den = 5 * U * den + p1 + p2
            d = sq / den
            e = U * abs(d) + e_sq / den + abs(d) * e_den / den
        else:
            d1, d2 = eps + s1, eps + s2
            e_d1, e_d2 = 3 * U * d1 + p1, 3 * U * d2 + p2
            if kind == "sym":
                r1, r2 = 1 / d1, 1 / d2
                e_r1, e_r2 = U * r1 + r1 * e_d1 / d1, U * r2 + r2 * e_d2 / d2
                rr = r1 + r2
                e_rr = U * rr + e_r1 + e_r2
                d = sq * rr
                e = U * abs(d) + e_sq * rr + sq * e_rr
            elif kind == "sym_sqrt":
                q1, q2 = np.sqrt(d1), np.sqrt(d2)
                e_q1, e_q2 = 2 * U * q1 + e_d1 / (2 * q1), 2 * U * q2 + e_d2 / (2 * q2)
                r1, r2 = 1 / q1, 1 / q2
                e_r1, e_r2 = U * r1 + r1 * e_q1 / q1, U * r2 + r2 * e_q2 / q2
                rr = r1 + r2
                e_rr = U * rr + e_r1 + e_r2
                d = abs(dd) * rr
                e = U * abs(d) + e_dd * rr + abs(dd) * e_rr
            else:
                raise ValueError(kind)
        if out == "f32":
            e = e + LD(2.0) ** -24 * abs(d) + LD(2.0) ** -150
        e = e * (1 + LD(2.0) ** -10)
        e = np.where(np.isfinite(d), e, LD("nan"))
    return d, e


def restate_numpy(rows, F, kind, eps):
    """The reference's own numpy expressions (measure.py:30-40, 55-71), fp64: what the fixtures must equal bit for bit."""
    with np.errstate(all="ignore"):
        rows = rows.astype(np.float64)
        pts1 = np.concatenate([rows[:, 0:2], np.ones((rows.shape[0], 1))], axis=1)
        pts2 = np.concatenate([rows[:, 2:4], np.ones((rows.shape[0], 1))], axis=1)
        l2 = np.dot(F, pts1.T)
        l1 = np.dot(F.T, pts2.T)
        dd = np.sum(l2.T * pts2, 1)
        if kind == "sampson":
            return dd ** 2 / (eps + l1[0, :] ** 2 + l1[1, :] ** 2 + l2[0, :] ** 2 + l2[1, :] ** 2)
        assert eps == 0.0
        if kind == "sym_sqrt":
            return np.abs(dd) * (1.0 / np.sqrt(l1[0, :] ** 2 + l1[1, :] ** 2) + 1.0 / np.sqrt(l2[0, :] ** 2 + l2[1, :] ** 2))
        return dd ** 2 * (1.0 / (l1[0, :] ** 2 + l1[1, :] ** 2) + 1.0 / (l2[0, :] ** 2 + l2[1, :] ** 2))


def golden_name(case):
    return os.path.join(GOLDEN_DIR, f"epipolar_{case}.npz")


def golden_key(kind, eps, dt):
    return f"np_{kind}_{dt}" if eps == 0.0 or kind == "sampson" else None


def within(what, got, d, e):
    """got against the yardstick (d, E) row by row: inside E where d is finite, the same NaN / infinity where it is not.
    Prints the figure first; returns the largest |error| / E."""
    got = np.asarray(got).astype(LD)
    fin = np.isfinite(d)
    same = np.where(np.isnan(d), np.isnan(got), got == d)
    assert bool(same[~fin].all()), f"{what}: a non-finite yardstick value is not reproduced"
    err = np.abs(got[fin] - d[fin])
    ok = err <= e[fin]
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(e[fin] > 0, err / e[fin], np.where(err > 0, np.inf, 0)), initial=0.0))
    print(f"{what}: {int(fin.sum())} finite rows, max |error| {float(err.max(initial=0)):.3g}, {ratio:.3g} of E")
    assert bool(ok.all()), (what, ratio)
    return ratio


def decidable(d, e, bins):
    """Rows whose yardstick distance is further than E from every edge (non-finite distances are decidable: in no bin)."""
    fin = np.isfinite(d)
    near = np.zeros(len(d), dtype=bool)
    for edge in bins:
        if edge <= 0:          # no arithmetic crosses it: every kind is a square or an absolute value times a non-negative factor
            continue
        near |= fin & (np.abs(np.where(fin, d, 0) - LD(edge)) <= np.where(fin, e, 0))
    return ~near


# ---- ctypes: the entry point of the real library or of the emulator's ------------------------------------------------------
def bind(lib):
    """Prototype of p2p_epipolar_batch on a ctypes handle (AttributeError where the library lacks it)."""
    fn = lib.p2p_epipolar_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.p2p_last_error.restype = ctypes.c_char_p
    return lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


FILL = -7.0          # what run() pre-fills dist with: rows the kernel must not touch keep it


def run(lib, items, kind, eps, bins=None, out="f64", stride=None, device="cpu", in_dtype=None):
    """The entry point on a batch of items [(rows [n,4] numpy of one dtype, F [3,3]) or (None, F) for a count of -1] ->
    (dist [B,stride] numpy pre-filled with FILL, hist [B,nbins] numpy or None)."""
    ns = [(-1 if r is None else len(r)) for r, _ in items]
    stride = stride or max(1, max(ns))
    dt = in_dtype or next(r.dtype for r, _ in items if r is not None)
    dt = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32", np.dtype(np.int64): "i64"}[np.dtype(dt)]
    m = torch.zeros((len(items), stride, 4), dtype=TORCH_DTYPE[dt])
    for b, (r, _) in enumerate(items):
        if r is not None and len(r):
            m[b, :len(r)] = torch.from_numpy(np.ascontiguousarray(r))
    Fs = torch.from_numpy(np.stack([np.asarray(F, dtype=np.float64).reshape(9) for _, F in items]))
    counts = torch.tensor(ns, dtype=torch.int32)
    dist = torch.full((len(items), stride), FILL, dtype=TORCH_DTYPE[out])
    edges = torch.tensor(list(bins), dtype=torch.float64) if bins is not None else None
    hist = torch.full((len(items), len(bins) - 1), -1, dtype=torch.int32) if bins is not None else None
    m, Fs, counts, dist = m.to(device), Fs.to(device), counts.to(device), dist.to(device)
    edges, hist = (edges.to(device), hist.to(device)) if bins is not None else (None, None)
    st = lib.p2p_epipolar_batch(_ptr(m), DTYPE_CODE[dt], _ptr(counts), _ptr(Fs), len(items), stride, KIND_CODE[kind], float(eps),
                                _ptr(edges), len(bins) - 1 if bins is not None else 0, _ptr(dist), DTYPE_CODE[out], _ptr(hist), None)
    assert st == 0, f"p2p_epipolar_batch returned {st}: {lib.p2p_last_error().decode()}"
    return dist.cpu().numpy(), (hist.cpu().numpy() if hist is not None else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- the checks, shared by the emulated and the GPU test ----------------------------------------------------------------
def check_case(lib, case, kind, eps, dt, out, device="cpu", bins=DEFAULT_BINS):
    """One (case, kind, eps, input type, output type) through `lib`: distances within E of the yardstick, the bin counts equal
    to np.histogram of the stored distances, and on the decidable rows equal to the counts of the reference's distances
    (tests/golden/epipolar_*.npz) where the reference computes this configuration; rows beyond the count untouched."""
    inp = inputs(case)
    rows, F = inp["rows"][dt], inp["F"]
    n = len(rows)
    dist, hist = run(lib, [(rows, F)], kind, eps, bins=bins, out=out, stride=n + 3, device=device)
    tag = f"case {case} {kind} eps {eps:g} {dt}->{out}"
    assert dist.dtype == (np.float64 if out == "f64" else np.float32) and bool((dist[0, n:] == FILL).all()), f"{tag}: rows beyond the count"
    d, e = yardstick(rows, F, kind, eps, out)
    within(tag, dist[0, :n], d, e)
    with np.errstate(all="ignore"):
        assert np.array_equal(hist[0], np.histogram(dist[0, :n].astype(np.float64), bins)[0]), f"{tag}: counts are not np.histogram's"
    dec = decidable(d, e, bins)
    assert (~dec).sum() <= MAX_UNDECIDABLE * n, f"{tag}: {(~dec).sum()} undecidable rows of {n}"
    key = golden_key(kind, eps, dt)
    if key is not None:
        ref = np.load(golden_name(case))[key]
        with np.errstate(all="ignore"):
            want = np.histogram(ref[dec], bins)[0]
            got = np.histogram(dist[0, :n][dec].astype(np.float64), bins)[0]
        assert np.array_equal(got, want), f"{tag}: counts differ from the reference's on the decidable rows: {got} vs {want}"
        if dec.all() and bins is DEFAULT_BINS:
            assert np.array_equal(hist[0], np.load(golden_name(case))[f"hist_{kind}_{dt}"]), f"{tag}: counts differ from the fixture"


def check_batch_identity(lib, device="cpu"):
    """A pair's distances and counts alone == the same pair in a batch of three, in another slot, with another stride and beside
    a -1 item, bit for bit; for both output types."""
    a, b = inputs("P"), inputs("Q")
    ra, rb = a["rows"]["f64"], b["rows"]["f64"][:300]
    for kind, eps in CONFIGS:
        for out in OUT_DTYPES:
            d1, h1 = run(lib, [(ra, a["F"])], kind, eps, bins=DEFAULT_BINS, out=out, device=device)
            d2, h2 = run(lib, [(rb, b["F"])], kind, eps, bins=DEFAULT_BINS, out=out, device=device)
            d3, h3 = run(lib, [(rb, b["F"]), (None, a["F"]), (ra, a["F"])], kind, eps, bins=DEFAULT_BINS, out=out, stride=333, device=device)
            assert np.array_equal(_bits(d3[2, :300]), _bits(d1[0])) and np.array_equal(h3[2], h1[0]), (kind, out, "slot 2")
            assert np.array_equal(_bits(d3[0, :300]), _bits(d2[0])) and np.array_equal(h3[0], h2[0]), (kind, out, "slot 0")
            assert bool((d3[1] == FILL).all()) and bool((h3[1] == 0).all()), (kind, out, "the -1 item")
            assert bool((d3[:, 300:] == FILL).all())
