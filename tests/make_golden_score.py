"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/score_*.npz by running the UNMODIFIED reference's
Patch2Pix.cal_coarse_score (networks/patch2pix.py:320-338; the method reads nothing of `self`, so it is called unbound) on
the CPU over cases S, W, N and D of tests/score_reference.py with normalize None, 'softmax' and 'l1'.

Run where the reference tree exists:   python tests/make_golden_score.py
A fixture holds the inputs (one volume per kind of values the case uses) and the reference's scalar per normalisation."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import score_reference as sr                         # noqa: E402


def main():
    cal_coarse_score = ref_shim.load_reference().patch2pix.Patch2Pix.cal_coarse_score
    for case in sr.HOST_CASES:
        arrays = {}
        for normalize in sr.NORMS:
            corr = sr.inputs(case, normalize)
            arrays[f"corr_{sr.kind_of(case, normalize)}"] = corr.numpy()
            score = cal_coarse_score(None, corr.unsqueeze(1), normalize=normalize)
            assert score.dim() == 0 and score.dtype == corr.dtype
            arrays[f"score_{sr.norm_tag(normalize)}"] = np.float32(score.item())
        np.savez_compressed(sr.golden_name(case), **arrays)
        print(f"{sr.golden_name(case)}: {os.path.getsize(sr.golden_name(case))} bytes, "
              + ", ".join(f"{k} {float(v):.7g}" for k, v in arrays.items() if k.startswith("score_")))


if __name__ == "__main__":
    main()
