"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/ncn_<case>.npz by running the UNMODIFIED reference's
NeighConsensus (networks/ncn/model.py:124-155, use_cuda=False) on the CPU over the cases and volumes of
tests/ncn_reference.py, and measure the reference's own fp32 error against the fp64 restatement.

Run where the reference tree exists:   python tests/make_golden_ncn.py
A fixture holds, per volume, the input x_<volume> and the reference's output y_<volume> (fp32), and the weights w<i> / b<i>
in the stored layout.  The REF_ERR table it prints goes into tests/ncn_reference.py.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import ncn_reference as nr                           # noqa: E402


def main():
    ref = ref_shim.load_reference().ncn_model
    table = {}
    for case, c in nr.CASES.items():
        sd = nr.weights(case)
        net = ref.NeighConsensus(use_cuda=False, kernel_sizes=c["kernel_sizes"], channels=c["channels"],
                                 symmetric_mode=c["symmetric_mode"])
        net.load_state_dict(sd, strict=True)
        net.eval()
        arrays, worst = {}, 0.0
        for i in range(len(c["kernel_sizes"])):
            arrays[f"w{i}"], arrays[f"b{i}"] = sd[f"conv.{2 * i}.weight"].numpy(), sd[f"conv.{2 * i}.bias"].numpy()
        for vol in nr.VOLUMES:
            x, y64 = nr.expected(case, vol)
            with torch.no_grad():
                y = net(x.unsqueeze(1))[:, 0].contiguous()
            scale = y64.abs().max().item()
            err = (y.double() - y64).abs().max().item()
            rel = err / scale if scale else 0.0
            worst = max(worst, rel)
            print(f"case {case} volume {vol}: max |f64| {scale:.4g}, reference fp32 error {err:.3g} (relative {rel:.3g}), "
                  f"share of non-zero cells {float((y64 > 0).double().mean()):.3f}")
            arrays[f"x_{vol}"], arrays[f"y_{vol}"] = x.numpy(), y.numpy()
        np.savez_compressed(nr.golden_name(case), **arrays)
        table[case] = worst
        print(f"{nr.golden_name(case)}: {os.path.getsize(nr.golden_name(case))} bytes")
    # rounded UP to three digits: the recorded bound must not fall below the measured error
    up = lambda v: float(f"{v:.2e}") if float(f"{v:.2e}") >= v else float(f"{v:.2e}") + 10 ** (np.floor(np.log10(v)) - 2)
    print("REF_ERR = {" + ", ".join(f'"{k}": {up(v):.3g}' for k, v in table.items()) + "}")


if __name__ == "__main__":
    main()
