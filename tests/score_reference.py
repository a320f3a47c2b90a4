"""TEST INFRASTRUCTURE: what the tests of the pair score (p2p_coarse_score_batch, Patch2Pix.cal_coarse_score) share -- the
case table, the seeded inputs, a restatement of the reference's cal_coarse_score (networks/patch2pix.py:320-338) that is
evaluated in fp64 as the yardstick (and in fp32 as the reference's own arithmetic), the bars, a ctypes binding of the entry
point that works on either library handle (the real one with device tensors, the CPU emulator's with host tensors), and the
checks the emulated and the GPU test both run.

Bars.  SCORE_TOL = 1e-5 is the project's score bar (tests/test_gpu_parity.py, tests/topk_reference.py).  Scores in [0, 1]
(softmax; l1 on a non-negative volume): absolute.  Signed l1 and the means of raw maxima: 1e-5 * max(1, |value|).  The raw
(`None`) cell scores and the two bit-equalities (softmax cells == the one-candidate match scores; a pair alone == the pair in
its batch) are exact.

Signed l1 (case D).  x / (sum x + 1e-4) is as well conditioned as its denominator.  The generator asserts that every row and
every column of the signed volume has |sum x + 1e-4| >= 0.1 * sum |x|, which bounds the relative error of ANY fp32
summation order of the n <= 54 terms by 10 * n * 2^-24.  89 rows and columns of plain N(0, 1) values never all meet that
(|sum| ~ sqrt(n), sum |x| ~ 0.8 n), so the signed volume is torch.randn + 1 (a sixth of its values negative) with the
planted negative row and column at torch.randn - 1."""
import ctypes
import os

import numpy as np
import torch

SCORE_TOL = 1e-5                    # the project's bar (tests/test_gpu_parity.py, tests/topk_reference.py)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORMS = (None, "softmax", "l1")
NORM_CODE = {None: 0, "softmax": 1, "l1": 2}          # P2P_SCORE_* of include/p2p_hip.h
L1_CONDITION = 0.1

# id -> pooled volume (hA, wA, hB, wB), batch, seed
CASES = {
    # nB 54 < 64 lanes; nA 35 no multiple of the 16 row slices; the last block of 16 columns holds 6
    "S": dict(dims=(5, 7, 6, 9), batch=1, seed=1901),
    # batch strides; nB 65: a second round of the 64 lanes
    "W": dict(dims=(7, 10, 5, 13), batch=3, seed=1902),
    # nA 12 < the 16 row slices: four empty slices bring (-inf, +inf, 0) to the tree; nB 25 < one wave
    "N": dict(dims=(3, 4, 5, 5), batch=2, seed=1903),
    # planted (see inputs): zero row and column, negative row and column, maxima that occur twice; the signed l1 case
    "D": dict(dims=(5, 7, 6, 9), batch=2, seed=1904),
    # the pooled volume of a 240x320 pair at ksize 2: 19 blocks of 16 columns, 5 rounds of 64 lanes, 2 cells per thread of
    # the pair sum.  GPU only.
    "T": dict(dims=(15, 20, 15, 20), batch=2, seed=1905),
}
HOST_CASES = ("S", "W", "N", "D")          # emulated, and with a fixture from the unmodified reference
PLANTED = dict(neg_row=10, neg_col=20, zero_row=3, zero_col=5, twice_row=(7, (11, 40)), twice_col=((12, 30), 33))

_inputs = {}


def kind_of(case, normalize):
    """Which volume a (case, normalisation) runs on: 'rand' in [0, 1) for softmax and for l1 on a non-negative volume,
    'randn' for the raw maxima, 'signed' (randn + 1) for the l1 of case D."""
    if normalize == "softmax":
        return "rand"
    if normalize is None:
        return "randn"
    return "signed" if case == "D" else "rand"


def is_unit_range(case, normalize):
    return normalize == "softmax" or (normalize == "l1" and case != "D")


def bar(case, normalize, value):
    """The bar of one score (see the module docstring); `value`: the yardstick's."""
    value = torch.as_tensor(value, dtype=torch.float64)
    return SCORE_TOL * (torch.ones_like(value) if is_unit_range(case, normalize) else value.abs().clamp(min=1.0))


def l1_condition(corr):
    """min over every row and column of |sum x + 1e-4| / sum |x| (inf where a slice is all zero)."""
    B, nA = corr.shape[0], corr.shape[1] * corr.shape[2]
    X = corr.double().reshape(B, nA, -1)
    worst = float("inf")
    for dim in (1, 2):
        den = X.abs().sum(dim=dim)
        ratio = torch.where(den > 0, (X.sum(dim=dim) + 1e-4).abs() / den.clamp(min=1e-300), torch.full_like(den, float("inf")))
        worst = min(worst, ratio.min().item())
    return worst


def inputs(case, normalize):
    """corr [B,hA,wA,hB,wB] fp32 on the CPU, built once per (case, kind) and never modified.  Case D then gets, in every
    pair: row 10 and column 20 lowered by 2 (sums clearly negative), row 3 and column 5 all zero, the maximum of row 7
    twice (columns 11 and 40) and the maximum of column 33 twice (rows 12 and 30)."""
    kind = kind_of(case, normalize)
    key = (case, kind)
    if key not in _inputs:
        c = CASES[case]
        gen = torch.Generator().manual_seed(c["seed"] + {"rand": 0, "randn": 1000, "signed": 2000}[kind])
        shape = (c["batch"],) + c["dims"]
        corr = torch.rand(shape, generator=gen) if kind == "rand" else torch.randn(shape, generator=gen)
        if kind == "signed":
            corr += 1.0
        if case == "D":
            p = PLANTED
            nA = c["dims"][0] * c["dims"][1]
            X = corr.view(c["batch"], nA, -1)
            X[:, p["neg_row"], :] -= 2.0
            X[:, :, p["neg_col"]] -= 2.0
            r, cols = p["twice_row"]
            X[:, r, cols[0]] = X[:, r, cols[1]] = X[:, r].max(dim=1)[0] + 1.0
            rows, col = p["twice_col"]
            X[:, rows[0], col] = X[:, rows[1], col] = X[:, :, col].max(dim=1)[0] + 1.0
            X[:, p["zero_row"], :] = 0.0
            X[:, :, p["zero_col"]] = 0.0
            assert bool((X[:, p["neg_row"]].sum(dim=1) < -10).all() and (X[:, :, p["neg_col"]].sum(dim=1) < -10).all())
            assert bool((X[:, r] == X[:, r].max(dim=1, keepdim=True)[0]).sum(dim=1).eq(2).all()), "case D lost its double row maximum"
            assert bool((X[:, :, col] == X[:, :, col].max(dim=1, keepdim=True)[0]).sum(dim=1).eq(2).all()), "case D lost its double column maximum"
        if kind == "signed":
            assert bool((corr < 0).any()) and l1_condition(corr) >= L1_CONDITION, f"case {case}: signed l1 input ill-conditioned"
        if kind == "rand" and case != "D":
            assert bool((corr >= 0).all())
        _inputs[key] = corr
    return _inputs[key]


def restate(corr, normalize, dtype=torch.float64):
    """cal_coarse_score (patch2pix.py:320-338) on corr [B,hA,wA,hB,wB], evaluated in `dtype` on the CPU: the same views,
    normalisations, maxima, concatenation and mean -> (cells [B, nA+nB] A cells first, pair [B], the reference's scalar)."""
    x = corr.detach().cpu().to(dtype).unsqueeze(1)
    if normalize is None:
        norm = lambda t: t
    elif normalize == "softmax":
        norm = lambda t: torch.nn.functional.softmax(t, 1)
    elif normalize == "l1":
        norm = lambda t: t / (torch.sum(t, dim=1, keepdim=True) + 0.0001)
    else:
        raise ValueError(normalize)
    B, _, h1, w1, h2, w2 = x.shape
    nc_b_avec = norm(x.reshape(B, h1 * w1, h2, w2))
    nc_a_bvec = norm(x.reshape(B, h1, w1, h2 * w2).permute(0, 3, 1, 2))
    scores_b = torch.max(nc_b_avec, dim=1)[0]
    scores_a = torch.max(nc_a_bvec, dim=1)[0]
    cells = torch.cat([scores_a.reshape(-1, h1 * w1), scores_b.reshape(-1, h2 * w2)], dim=1)
    return cells, cells.mean(dim=1), cells.mean()


# ---- ctypes: the entry point of the real library or of the emulator's ------------------------------------------------------
def bind(lib):
    """Prototypes of p2p_coarse_score_batch and its workspace query on a ctypes handle (AttributeError where the library
    lacks them), and of p2p_coarse_matches_batch for the softmax identity."""
    fn = lib.p2p_coarse_score_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                            ctypes.c_void_p]
    lib.p2p_coarse_score_workspace_bytes.restype = ctypes.c_size_t
    lib.p2p_coarse_score_workspace_bytes.argtypes = [ctypes.c_int] * 5
    lib.p2p_last_error.restype = ctypes.c_char_p
    lib.p2p_coarse_matches_batch.restype = ctypes.c_int
    lib.p2p_coarse_matches_batch.argtypes = ([ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 +
                                             [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    return lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_score(lib, corr, normalize, with_cells=True):
    """The entry point on a tensor of either device (default stream) -> (cells [B, nA+nB] or None, pair [B]) on the CPU.
    with_cells=False: cell_scores = NULL and a workspace of exactly the queried size."""
    corr = corr.contiguous()
    B, hA, wA, hB, wB = corr.shape
    n = hA * wA + hB * wB
    pair = torch.full((B,), float("nan"), dtype=torch.float32, device=corr.device)
    cells = ws = None
    need = 0
    if with_cells:
        cells = torch.full((B, n), float("nan"), dtype=torch.float32, device=corr.device)
    else:
        need = lib.p2p_coarse_score_workspace_bytes(B, hA, wA, hB, wB)
        assert need == B * n * 4
        ws = torch.empty(need, dtype=torch.uint8, device=corr.device)
    st = lib.p2p_coarse_score_batch(_ptr(corr), B, hA, wA, hB, wB, NORM_CODE[normalize], _ptr(cells), _ptr(pair), _ptr(ws), need, None)
    assert st == 0, f"p2p_coarse_score_batch returned {st}: {lib.p2p_last_error().decode()}"
    return (cells.cpu() if with_cells else None), pair.cpu()


def run_match_scores(lib, corr):
    """The scores of p2p_coarse_matches_batch (ksize 1, no delta) on the same volume, reordered A cells first."""
    corr = corr.contiguous()
    B, hA, wA, hB, wB = corr.shape
    nA, nB = hA * wA, hB * wB
    m = torch.empty((B, nA + nB, 4), dtype=torch.int64, device=corr.device)
    s = torch.full((B, nA + nB), float("nan"), dtype=torch.float32, device=corr.device)
    st = lib.p2p_coarse_matches_batch(_ptr(corr), None, B, hA, wA, hB, wB, 1, 8, 1, _ptr(m), _ptr(s), None)
    assert st == 0, f"p2p_coarse_matches_batch returned {st}: {lib.p2p_last_error().decode()}"
    s = s.cpu()
    return torch.cat([s[:, nB:], s[:, :nB]], dim=1)          # that call lists the B cells first


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the checks, shared by the emulated and the GPU test ----------------------------------------------------------------
def golden_name(case):
    return os.path.join(GOLDEN_DIR, f"score_{case}.npz")


def norm_tag(normalize):
    return "none" if normalize is None else normalize


def assert_within(what, got, want, case, normalize):
    """got (fp32) against the yardstick want (fp64), each element at its bar; prints the figure first."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    err = (got - want).abs()
    ratio = (err / bar(case, normalize, want)).max().item()
    print(f"{what}: max |error| {err.max().item():.3g}, {ratio:.3g} of the bar")
    assert ratio <= 1.0, (what, err.max().item())


def check_case(lib, case, normalize, device="cpu"):
    """Cell scores and pair scores of one (case, normalisation) through `lib`: the exact statements for None and softmax,
    the bars against the fp64 yardstick for l1 cells and every pair score, a pair alone against the pair in its batch, and
    cell_scores = NULL."""
    corr = inputs(case, normalize)
    dcorr = corr.to(device)
    cells, pair = run_score(lib, dcorr, normalize)
    ycells, ypair, _ = restate(corr, normalize)
    B, nA = corr.shape[0], corr.shape[1] * corr.shape[2]
    tag = f"case {case} {norm_tag(normalize)}"
    assert cells.shape == ycells.shape and pair.shape == ypair.shape
    if normalize is None:
        X = corr.reshape(B, nA, -1)
        want = torch.cat([X.max(dim=2)[0], X.max(dim=1)[0]], dim=1)
        assert torch.equal(_bits(cells), _bits(want)), f"{tag}: cell scores not bit-equal to torch.max"
    elif normalize == "softmax":
        want = run_match_scores(lib, dcorr)
        assert torch.equal(_bits(cells), _bits(want)), f"{tag}: cell scores differ from the scores of p2p_coarse_matches_batch"
    assert_within(f"{tag} cells", cells, ycells, case, normalize)
    assert_within(f"{tag} pairs", pair, ypair, case, normalize)
    # a pair alone == the pair in its batch
    for b in range(B):
        c1, p1 = run_score(lib, dcorr[b:b + 1], normalize)
        assert torch.equal(_bits(c1[0]), _bits(cells[b])) and torch.equal(_bits(p1), _bits(pair[b:b + 1])), f"{tag}: pair {b} alone differs"
    # cell_scores = NULL: through the workspace
    _, p0 = run_score(lib, dcorr, normalize, with_cells=False)
    assert torch.equal(_bits(p0), _bits(pair)), f"{tag}: pair scores differ without cell_scores"


def check_against_golden(lib, case, normalize, device="cpu"):
    """The unmodified reference's scalar (tests/make_golden_score.py) on the inputs stored with it: the fp32 mean of the
    library's pair scores within the bar."""
    g = np.load(golden_name(case))
    corr = torch.from_numpy(g[f"corr_{kind_of(case, normalize)}"])
    _, pair = run_score(lib, corr.to(device), normalize)
    assert_within(f"case {case} {norm_tag(normalize)} against the reference", pair.mean(), float(g[f"score_{norm_tag(normalize)}"]),
                  case, normalize)
