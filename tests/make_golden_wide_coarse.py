"""Record tests/golden/wide_coarse_parent.npz: the operand buffers and outputs of the coarse stage at 32 and 256 channels as the
library computes them (the kernels' code on the CPU, tests/hipemu), in both coarse modes.

Run ONCE on the commit before the preparation kernel learnt more than 256 channels; tests/test_wide_coarse_emulated.py then
holds every later library to these bits (cases `GOLDEN_CASES` of tests/wide_coarse_reference.py).  The inputs are regenerated
from their seeds; the file stores an input checksum per case, the raw feature-plane bytes of both images, the first mutual
matching, the consensus output, the final volume, the relocalisation codes and the coarse rows and scores.

    python tests/make_golden_wide_coarse.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import golden_util as gu  # noqa: E402
import coarse_mode_reference as cm  # noqa: E402
import stage_reference as sr  # noqa: E402
import wide_coarse_reference as wc  # noqa: E402


def record(emu, sd, name, mode):
    """-> {key: array} of one case and mode."""
    fa, fb = wc.case_inputs(name)
    c, (ha, wa), (hb, wb), k, _, _ = wc.WIDE[name][0]
    out = wc.run(emu, sd, name, mode)
    ncn = cm.ncn_create(emu, sd)
    try:
        cm.set_mode(emu, ncn, mode)
        res = sr.run_coarse(emu, ncn, fa, fb, k, "cpu")
    finally:
        emu.p2p_ncn_destroy(ncn)
    off = sr.coarse_ws_offsets(c, ha, wa, hb, wb, k)
    half = 2 if mode == "fp16" else 1            # one plane: the blocks fill the first half of the buffers
    pre = f"{name}/{mode}/"
    return {pre + "input_checksum": np.float64(gu.checksum([fa, fb])),
            pre + "fnA": res["ws"][0][off["fnA"]:off["fnA"] + sr._up(ha * wa, 128) * c * 4 // half].numpy().copy(),
            pre + "fnB": res["ws"][0][off["fnB"]:off["fnB"] + sr._up(hb * wb, 128) * c * 4 // half].numpy().copy(),
            pre + "x": out["x"].numpy(), pre + "y": out["y"].numpy(), pre + "corr": out["corr"].numpy(),
            pre + "delta": out["delta"].numpy(), pre + "rows": out["rows"].numpy(), pre + "scores": out["scores"].numpy()}


def main():
    emu = cm.bind(emu_lib.load())
    sd = gu.state_dict(0)
    data = {}
    for name in wc.GOLDEN_CASES:
        for mode in ("fp16x2", "fp16"):
            data.update(record(emu, sd, name, mode))
    path = os.path.join(gu.GOLDEN, wc.GOLDEN_FILE + ".npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(data)} arrays")


if __name__ == "__main__":
    main()
