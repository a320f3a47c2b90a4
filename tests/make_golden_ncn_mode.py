"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/ncn_mode_<case>.npz by running the UNMODIFIED reference's
NeighConsensus (networks/ncn/model.py:124-155, use_cuda=False) on the CPU over the inputs tests/ncn_mode_reference.py adds
(the volume "tile", the range variants on "big" and "tile", the mixed-magnitude batch), and measure the reference's own fp32 error
PER PAIR against the fp64 restatement on them and on the volumes of tests/ncn_reference.py.

Run where the reference tree exists:   python tests/make_golden_ncn_mode.py
A fixture holds the reference's fp32 outputs y_<input> (inputs and weights are regenerated from their seeds).  The REF_ERR_MODE
table it prints goes into tests/ncn_mode_reference.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import ncn_reference as nr                           # noqa: E402
import ncn_mode_reference as nm                      # noqa: E402


def main():
    ref = ref_shim.load_reference().ncn_model
    table = {}

    def run(case, sd, x):
        c = nr.CASES[case]
        net = ref.NeighConsensus(use_cuda=False, kernel_sizes=c["kernel_sizes"], channels=c["channels"], symmetric_mode=c["symmetric_mode"])
        net.load_state_dict(sd, strict=True)
        net.eval()
        with torch.no_grad():
            return net(x.unsqueeze(1))[:, 0].contiguous()

    def measure(case, key, y, y64):
        rel = 0.0
        for z in range(y.shape[0]):
            scale = y64[z].abs().max().item()
            rel = max(rel, (y[z].double() - y64[z]).abs().max().item() / scale if scale else 0.0)
        share = float((y64 > 0).double().mean())
        print(f"case {case} input {key}: reference fp32 error per pair {rel:.3g} (table {nr.REF_ERR[case]:.3g}), non-zero cells {share:.3f}")
        if rel > nr.REF_ERR[case]:
            table[(case, key)] = rel

    for case in nr.CASES:
        arrays = {}
        for vol in nm.VOLUMES:
            x, y64 = nm.expected(case, vol)
            y = run(case, nr.weights(case), x)
            measure(case, vol, y, y64)
            if vol == nm.TILE:
                arrays[f"y_{vol}"] = y.numpy()
        if case in nm.HIDDEN_CASES:
            for variant in nm.VARIANTS:
                for vol in ("big", nm.TILE):
                    x, y64 = nm.expected(case, vol, variant)
                    y = run(case, nm.weights(case, variant), x)
                    key = nm.input_key(vol, variant)
                    measure(case, key, y, y64)
                    arrays[f"y_{key}"] = y.numpy()
            x, y64 = nm.mixed(case)
            y = run(case, nr.weights(case), x)
            measure(case, "mixed", y, y64)
            arrays["y_mixed"] = y.numpy()
            arrays["outlier_channel"] = np.array(nm.outlier_channel(case))
        np.savez_compressed(nm.golden_name(case), **arrays)
        print(f"{nm.golden_name(case)}: {os.path.getsize(nm.golden_name(case))} bytes")
    # rounded UP to three digits: the recorded bound must not fall below the measured error
    up = lambda v: float(f"{v:.2e}") if float(f"{v:.2e}") >= v else float(f"{v:.2e}") + 10 ** (np.floor(np.log10(v)) - 2)
    print("REF_ERR_MODE = {" + ", ".join(f'("{k[0]}", "{k[1]}"): {up(v):.3g}' for k, v in table.items()) + "}")


if __name__ == "__main__":
    main()
