"""TEST INFRASTRUCTURE: what the tests of the top-k match extraction share -- the case table, the seeded inputs, a plain
torch restatement of p2p_coarse_matches_topk_batch written from the row order of include/p2p_hip.h (a stable descending
sort along the axis, its first topk entries, softmax in fp32, relocalisation from the packed delta byte, pixel scaling),
and a ctypes binding of the entry point that works on either library handle (the real one with device tensors, the CPU
emulator's with host tensors)."""
import ctypes
import os

import numpy as np
import torch

SCORE_TOL = 1e-5                    # the project's bar (tests/test_gpu_parity.py)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# id -> pooled volume (hA, wA, hB, wB), batch, ksize, topk values, upsample, center, seed
CASES = {
    # nB 54 < 64 lanes; nA 35 no multiple of the 16 row slices; the last block of 16 columns holds 6
    "S": dict(dims=(5, 7, 6, 9), batch=1, ksize=1, topks=(1, 2, 3, 8), upsample=16, center=True, seed=901),
    # nB 65: a second round of the 64 lanes; batch strides; delta decode
    "W": dict(dims=(7, 10, 5, 13), batch=3, ksize=2, topks=(2, 5), upsample=8, center=True, seed=902),
    # ksize 4 codes up to byte 255; no centring
    "K": dict(dims=(4, 4, 6, 6), batch=2, ksize=4, topks=(4,), upsample=4, center=False, seed=903),
    # planted ties (see inputs)
    "T": dict(dims=(5, 7, 6, 9), batch=1, ksize=2, topks=(3,), upsample=8, center=True, seed=904),
    # nA 12 < the 16 row slices of the column kernels: four empty slices bring (-inf, 0x7fffffff) to the tree; nB 25 < one
    # wave: 39 empty lanes in the row kernels, and a last block of 16 columns that holds 9
    "N": dict(dims=(3, 4, 5, 5), batch=2, ksize=1, topks=(1, 3), upsample=16, center=True, seed=905),
}
GOLDEN_CASES = ("S", "W", "K")      # T has ties: torch.topk, which the reference calls, leaves their order open

_inputs = {}


def inputs(case, do_softmax):
    """(corr [B,hA,wA,hB,wB] fp32, delta uint8 of that shape or None) of a case, CPU, built once and never modified:
    torch.rand volumes for the softmax scores, torch.randn (negative values included) for the raw ones, delta bytes
    uniform in [0, ksize^4).  Case T then gets an all-zero row (3), an all-zero column (5), a row (10) whose 2nd to 4th
    values are equal and a column (20) whose maximum occurs twice."""
    key = (case, bool(do_softmax))
    if key not in _inputs:
        c = CASES[case]
        gen = torch.Generator().manual_seed(c["seed"] + (0 if do_softmax else 1000))
        shape = (c["batch"],) + c["dims"]
        corr = torch.rand(shape, generator=gen) if do_softmax else torch.randn(shape, generator=gen)
        k = c["ksize"]
        delta = torch.randint(0, k ** 4, shape, generator=gen).to(torch.uint8) if k > 1 else None
        if k == 4:
            assert int(delta.max()) == 255, "the ksize 4 case must reach the last code of the byte"
        if case == "T":
            nA, nB = c["dims"][0] * c["dims"][1], c["dims"][2] * c["dims"][3]
            X = corr.view(nA, nB)
            top = X[10].max()
            X[10, 13] = top + 1.0
            X[10, [40, 7, 22]] = top + 0.5
            X[[30, 4], 20] = X[:, 20].max() + 1.0
            X[3, :] = 0.0
            X[:, 5] = 0.0
            v, w = torch.sort(X[10], descending=True)[0], torch.sort(X[:, 20], descending=True)[0]
            assert v[0] > v[1] == v[2] == v[3] > v[4] and w[0] == w[1] > w[2], "case T lost its planted ties"
        _inputs[key] = (corr, delta)
    return _inputs[key]


def pixel_rows(ra, cb, delta, dims, ksize, upsample, center):
    """Cells (ra, cb) of one pair, any equal shape -> int64 rows (xA, yA, xB, yB) [..., 4]: relocalisation with the packed
    byte s = ((di*k+dj)*k+dk)*k+dl, then upsample * cell (+ upsample // 2 with centring)."""
    hA, wA, hB, wB = dims
    ia, ja, ib, jb = ra // wA, ra % wA, cb // wB, cb % wB
    if ksize > 1:
        k = ksize
        s = delta.reshape(hA * wA, hB * wB)[ra, cb].long()
        di, dj, dk, dl = s // (k * k * k), (s // (k * k)) % k, (s // k) % k, s % k
        ia, ja, ib, jb = ia * k + di, ja * k + dj, ib * k + dk, jb * k + dl
    off = upsample // 2 if center else 0
    return torch.stack([ja, ia, jb, ib], dim=-1) * upsample + off


def restate(corr, delta, ksize, upsample, center, topk, do_softmax):
    """-> (matches [B, topk*(nB+nA), 4] int64, scores [B, topk*(nB+nA)] fp32) on the CPU."""
    corr = corr.detach().cpu().float()
    delta = delta.detach().cpu() if delta is not None else None
    B, dims = corr.shape[0], tuple(corr.shape[1:])
    nA, nB = dims[0] * dims[1], dims[2] * dims[3]
    rows, scores = [], []
    for b in range(B):
        X = corr[b].reshape(nA, nB)
        d = delta[b] if delta is not None else None
        # B -> A: rank t of column c in row t*nB + c
        _, idx = torch.sort(X, dim=0, descending=True, stable=True)
        idx = idx[:topk]                                                      # [topk, nB] A cells
        cols = torch.arange(nB).expand(topk, nB)
        sc = (torch.softmax(X, dim=0) if do_softmax else X).gather(0, idx)
        m_ba, s_ba = pixel_rows(idx, cols, d, dims, ksize, upsample, center).reshape(-1, 4), sc.reshape(-1)
        # A -> B: rank t of row r in row topk*nB + r*topk + t
        _, idx = torch.sort(X, dim=1, descending=True, stable=True)
        idx = idx[:, :topk]                                                   # [nA, topk] B cells
        rws = torch.arange(nA)[:, None].expand(nA, topk)
        sc = (torch.softmax(X, dim=1) if do_softmax else X).gather(1, idx)
        m_ab, s_ab = pixel_rows(rws, idx, d, dims, ksize, upsample, center).reshape(-1, 4), sc.reshape(-1)
        rows.append(torch.cat([m_ba, m_ab]))
        scores.append(torch.cat([s_ba, s_ab]))
    return torch.stack(rows), torch.stack(scores)


# ---- ctypes: the entry point of the real library or of the emulator's ------------------------------------------------------
def bind(lib):
    """Prototype of p2p_coarse_matches_topk_batch on a ctypes handle (AttributeError where the library lacks it)."""
    fn = lib.p2p_coarse_matches_topk_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 10 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.p2p_last_error.restype = ctypes.c_char_p
    lib.p2p_coarse_matches_batch.restype = ctypes.c_int
    lib.p2p_coarse_matches_batch.argtypes = ([ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 +
                                             [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    return lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_topk(lib, corr, delta, ksize, upsample, center, topk, do_softmax):
    """The entry point on tensors of either device (default stream) -> (matches, scores) on the CPU."""
    corr = corr.contiguous()
    delta = delta.contiguous() if delta is not None else None
    B, hA, wA, hB, wB = corr.shape
    n = topk * (hA * wA + hB * wB)
    m = torch.full((B, n, 4), -1, dtype=torch.int64, device=corr.device)
    s = torch.full((B, n), float("nan"), dtype=torch.float32, device=corr.device)
    st = lib.p2p_coarse_matches_topk_batch(_ptr(corr), _ptr(delta), B, hA, wA, hB, wB, ksize, upsample, int(center), topk,
                                           int(do_softmax), _ptr(m), _ptr(s), None)
    assert st == 0, f"p2p_coarse_matches_topk_batch returned {st}: {lib.p2p_last_error().decode()}"
    return m.cpu(), s.cpu()


def run_top1(lib, corr, delta, ksize, upsample, center):
    """p2p_coarse_matches_batch, the existing one-candidate entry point, on the same tensors."""
    corr = corr.contiguous()
    delta = delta.contiguous() if delta is not None else None
    B, hA, wA, hB, wB = corr.shape
    n = hA * wA + hB * wB
    m = torch.full((B, n, 4), -1, dtype=torch.int64, device=corr.device)
    s = torch.full((B, n), float("nan"), dtype=torch.float32, device=corr.device)
    st = lib.p2p_coarse_matches_batch(_ptr(corr), _ptr(delta), B, hA, wA, hB, wB, ksize, upsample, int(center), _ptr(m), _ptr(s),
                                      None)
    assert st == 0, f"p2p_coarse_matches_batch returned {st}: {lib.p2p_last_error().decode()}"
    return m.cpu(), s.cpu()


# ---- the parity checks, shared by the emulated and the GPU test -------------------------------------------------------
def case_runs(case):
    c = CASES[case]
    return [(topk, sm) for topk in c["topks"] for sm in (True, False)]


def _assert_restated(what, m, s, rm, rs, sm):
    """Match rows exact (the tie rule of case T included), raw scores bit-equal, softmax scores within SCORE_TOL."""
    assert m.shape == rm.shape and s.shape == rs.shape
    bad = (m != rm).any(dim=-1)
    assert not bad.any(), f"{what} softmax {sm}: {int(bad.sum())} rows differ, first {bad.nonzero()[0].tolist()}"
    if sm:
        err = (s - rs).abs().max().item()
        print(f"{what}: softmax score error {err:.3g}")
        assert err <= SCORE_TOL, err
    else:
        assert torch.equal(s.view(torch.int32), rs.view(torch.int32)), f"{what}: raw scores not bit-equal"


def check_against_restatement(lib, case, device="cpu"):
    c = CASES[case]
    for topk, sm in case_runs(case):
        corr, delta = inputs(case, sm)
        rm, rs = restate(corr, delta, c["ksize"], c["upsample"], c["center"], topk, sm)
        m, s = run_topk(lib, corr.to(device), delta.to(device) if delta is not None else None, c["ksize"], c["upsample"],
                        c["center"], topk, sm)
        _assert_restated(f"case {case} topk {topk}", m, s, rm, rs, sm)


def check_one_candidate_against_restatement(lib, case, device="cpu"):
    """p2p_coarse_matches_batch against the restatement with one candidate and softmax, at the bars of topk = 1 above: the
    one-candidate kernels and the top-k kernels are one body, so their identity (check_top1_identity) compares that body
    with itself."""
    c = CASES[case]
    corr, delta = inputs(case, True)
    rm, rs = restate(corr, delta, c["ksize"], c["upsample"], c["center"], 1, True)
    m, s = run_top1(lib, corr.to(device), delta.to(device) if delta is not None else None, c["ksize"], c["upsample"], c["center"])
    _assert_restated(f"case {case} one candidate", m, s, rm, rs, True)


def golden_name(case):
    return os.path.join(GOLDEN_DIR, f"topk_{case}.npz")


def check_against_golden(lib, case, device="cpu"):
    """The unmodified reference's (jA, iA, jB, iB, score) of both directions (tests/make_golden_topk.py; tie-free by
    construction, so no row is left out): indices exact in every row, scores at the same bars."""
    c = CASES[case]
    g = np.load(golden_name(case))
    up, off = c["upsample"], (c["upsample"] // 2 if c["center"] else 0)
    for topk in c["topks"]:
        for sm in (True, False):
            tag = "soft" if sm else "raw"
            corr = torch.from_numpy(g[f"corr_{tag}"])
            delta = torch.from_numpy(g[f"delta_{tag}"]) if c["ksize"] > 1 else None
            m, s = run_topk(lib, corr.to(device), delta.to(device) if delta is not None else None, c["ksize"], up,
                            c["center"], topk, sm)
            want = torch.from_numpy(g[f"idx_{tag}_k{topk}"].astype(np.int64)) * up + off
            assert torch.equal(m, want), f"case {case} topk {topk} {tag}: rows differ from the reference"
            ref_s = torch.from_numpy(g[f"score_{tag}_k{topk}"])
            if sm:
                err = (s - ref_s).abs().max().item()
                print(f"case {case} topk {topk}: softmax score error against the reference {err:.3g}")
                assert err <= SCORE_TOL, err
            else:
                assert torch.equal(s.view(torch.int32), ref_s.view(torch.int32))
    # do_softmax=False of the one-candidate extractor (corr_to_matches): topk = 1 of the new entry
    corr = torch.from_numpy(g["corr_raw"])
    delta = torch.from_numpy(g["delta_raw"]) if c["ksize"] > 1 else None
    m, s = run_topk(lib, corr.to(device), delta.to(device) if delta is not None else None, c["ksize"], up, c["center"], 1, False)
    assert torch.equal(m, torch.from_numpy(g["idx_raw_top1"].astype(np.int64)) * up + off)
    assert torch.equal(s.view(torch.int32), torch.from_numpy(g["score_raw_top1"]).view(torch.int32))


def check_top1_identity(lib, case, device="cpu"):
    """topk = 1 with softmax == p2p_coarse_matches_batch on the same inputs, matches and scores bit for bit."""
    c = CASES[case]
    corr, delta = inputs(case, True)
    corr, delta = corr.to(device), (delta.to(device) if delta is not None else None)
    m, s = run_topk(lib, corr, delta, c["ksize"], c["upsample"], c["center"], 1, True)
    m1, s1 = run_top1(lib, corr, delta, c["ksize"], c["upsample"], c["center"])
    assert torch.equal(m, m1), f"case {case}: matches differ from the one-candidate kernels"
    assert torch.equal(s.view(torch.int32), s1.view(torch.int32)), f"case {case}: scores differ from the one-candidate kernels"
