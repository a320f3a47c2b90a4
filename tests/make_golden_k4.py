"""TEST INFRASTRUCTURE ONLY -- generate the ksize = 4 fixtures tests/golden/coarse_*_k4.npz by running the UNMODIFIED
reference (through oracle/make_golden.py's own case_coarse) on seeded synthetic inputs, on CPU fp32.

Run where the reference tree exists:   python tests/make_golden_k4.py
The fixtures hold the reference's outputs, the seed recipe and a checksum of the inputs (see oracle/make_golden.py).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg                 # noqa: E402
from patch2pix_amd.utils import synthetic            # noqa: E402

# name, seed, H, W: 8x10x8x10 cells; 5x11x5x11 cells (880 positions per image: the last 32-row block of the
# correlation GEMM holds one cell and one cell of padding)
CASES = [("coarse_256x320_k4", 35, 256, 320), ("coarse_160x352_k4", 36, 160, 352)]


def main():
    ref = mg.load_reference()
    sd = synthetic.make_state_dict(mg.SD_SEED)
    net = mg.build_reference_net(sd, synthetic.default_regressor_config())
    for name, seed, H, W in CASES:
        mg.case_coarse(ref, net, sd, name, seed, H, W, 4)


if __name__ == "__main__":
    main()
