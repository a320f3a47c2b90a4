"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/topk_*.npz by running the UNMODIFIED reference's
corr_to_matches_topk (and, for do_softmax=False with one candidate, corr_to_matches; ncn/extract_ncmatches.py) on the CPU
over cases S, W and K of tests/topk_reference.py, in both directions, concatenated B->A first then A->B the way
cal_coarse_matches concatenates them.

Run where the reference tree exists:   python tests/make_golden_topk.py
A fixture holds the inputs and, per topk, the reference's (jA, iA, jB, iB) as idx_* [B, n, 4] and its score [B, n].  The
generator refuses inputs in which the topk + 1 best values of a row or a column are not pairwise distinct: torch.topk
leaves the order of ties open, and without ties every row of the fixture is comparable.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import topk_reference as tr                          # noqa: E402


def assert_tie_free(corr, topk):
    B = corr.shape[0]
    nA = corr.shape[1] * corr.shape[2]
    X = corr.reshape(B, nA, -1)
    for dim in (1, 2):
        v = torch.sort(X, dim=dim, descending=True)[0].narrow(dim, 0, topk + 1)
        assert bool((v.narrow(dim, 0, topk) > v.narrow(dim, 1, topk)).all()), "ties among the best topk + 1 values"


def planes(delta, k):
    """packed byte -> the reference's delta4d: four int64 [B,1,hA,wA,hB,wB]."""
    s = delta.long().unsqueeze(1)
    return s // (k * k * k), (s // (k * k)) % k, (s // k) % k, s % k


def both_directions(fn, corr, delta4d, **kw):
    out = [fn(corr.unsqueeze(1), delta4d=delta4d, invert_matching_direction=inv, **kw) for inv in (False, True)]
    idx = torch.cat([torch.stack(o[:4], dim=-1) for o in out], dim=1)          # [B, n, 4] = (jA, iA, jB, iB)
    score = torch.cat([o[4] for o in out], dim=1)
    return idx.numpy().astype(np.int16), score.numpy().astype(np.float32)


def main():
    ext = ref_shim.load_reference().extract
    for case in tr.GOLDEN_CASES:
        c = tr.CASES[case]
        k, arrays = c["ksize"], {}
        for sm in (True, False):
            tag = "soft" if sm else "raw"
            corr, delta = tr.inputs(case, sm)
            assert_tie_free(corr, max(c["topks"]))
            arrays[f"corr_{tag}"] = corr.numpy()
            if delta is not None:
                arrays[f"delta_{tag}"] = delta.numpy()
            d4 = planes(delta, k) if delta is not None else None
            for topk in c["topks"]:
                arrays[f"idx_{tag}_k{topk}"], arrays[f"score_{tag}_k{topk}"] = both_directions(
                    ext.corr_to_matches_topk, corr, d4, topk=topk, ksize=k, do_softmax=sm)
        corr, delta = tr.inputs(case, False)
        arrays["idx_raw_top1"], arrays["score_raw_top1"] = both_directions(
            ext.corr_to_matches, corr, planes(delta, k) if delta is not None else None, ksize=k, do_softmax=False)
        np.savez_compressed(tr.golden_name(case), **arrays)
        print(f"{tr.golden_name(case)}: {os.path.getsize(tr.golden_name(case))} bytes")


if __name__ == "__main__":
    main()
