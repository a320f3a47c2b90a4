"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/epipolar_*.npz by running the UNMODIFIED reference's
utils.eval.measure.{sampson_distance, symmetric_epipolar_distance (sqrt False and True), check_inliers_distr} and
networks.utils.{sym_epi_dist, sampson_dist} on the CPU over the cases and input types of tests/epipolar_reference.py.

Run where the reference tree exists:   python tests/make_golden_epipolar.py
A case's fixture holds its inputs (F, the rows in the three input types), the reference's fp64 numpy distances np_<kind>_<type>,
the np.histogram counts of those over the default bins (hist_<kind>_<type>), and the fp32 torch distances t_<kind>_<type> (F as
a float32 tensor, the reference's usual arithmetic there).  epipolar_distr.npz holds check_inliers_distr on the list of the
cases' Sampson distances (with an empty pair in it): the strings and ratios for the default bins and for the bins of
eval_epoch_immatch.py:85, and the per-pair counts they were made from."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import epipolar_reference as er                      # noqa: E402


def main():
    ref = ref_shim.load_reference()
    measure = importlib.import_module("utils.eval.measure")          # resolves inside the reference's `utils.eval` package
    assert measure.__file__.startswith(ref_shim.REFERENCE_ROOT)
    np.seterr(all="ignore")
    sampson = {}
    for case in er.CASES:
        inp = er.inputs(case)
        F = inp["F"]
        arrays = {"F": F, "noise": inp["noise"]}
        for dt in er.IN_DTYPES:
            rows = inp["rows"][dt]
            arrays[f"rows_{dt}"] = rows
            p = rows.astype(np.float64)
            out = {"sampson": measure.sampson_distance(p[:, 0:2], p[:, 2:4], F),
                   "sym": measure.symmetric_epipolar_distance(p[:, 0:2], p[:, 2:4], F),
                   "sym_sqrt": measure.symmetric_epipolar_distance(p[:, 0:2], p[:, 2:4], F, sqrt=True)}
            for kind, d in out.items():
                assert d.dtype == np.float64 and d.shape == (len(rows),)
                arrays[f"np_{kind}_{dt}"] = d
                arrays[f"hist_{kind}_{dt}"] = np.histogram(d, er.DEFAULT_BINS)[0]
            F32 = torch.from_numpy(F).float()
            arrays[f"t_sampson_{dt}"] = ref.utils.sampson_dist(torch.from_numpy(rows), F32).numpy()
            arrays[f"t_sym_{dt}"] = ref.utils.sym_epi_dist(torch.from_numpy(rows), F32).numpy()
            assert arrays[f"t_sym_{dt}"].dtype == np.float32
        sampson[case] = arrays["np_sampson_f64"]
        np.savez_compressed(er.golden_name(case), **arrays)
        print(f"{er.golden_name(case)}: {os.path.getsize(er.golden_name(case))} bytes, {len(inp['noise'])} rows, "
              f"sampson counts {arrays['hist_sampson_f64'].tolist()}")
    order = list(er.CASES)
    dists = [sampson[c] for c in order[:2]] + [np.empty(0)] + [sampson[c] for c in order[2:]]
    distr = {"order": np.array(order), "empty_at": np.int64(2)}
    for name, bins, tag in (("default", er.DEFAULT_BINS, ""), ("eval", er.EVAL_BINS, "fdist")):
        ratios, text = measure.check_inliers_distr(dists, bins=bins, tag=tag, return_ratios=True)
        assert text == measure.check_inliers_distr(dists, bins=bins, tag=tag)
        distr[f"text_{name}"], distr[f"ratios_{name}"], distr[f"tag_{name}"] = np.array(text), np.array(ratios, dtype=np.float64), np.array(tag)
        distr[f"bins_{name}"] = np.array(bins, dtype=np.float64)
        distr[f"hists_{name}"] = np.stack([np.histogram(d, bins)[0] for d in dists if len(d)])
        print(text)
    path = os.path.join(er.GOLDEN_DIR, "epipolar_distr.npz")
    np.savez_compressed(path, **distr)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
