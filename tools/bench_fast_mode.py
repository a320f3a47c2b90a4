"""bench.py's measuring loop in the opt-in single-plane mode `fp16` (P2P_REGRESS_FP16).

bench.py labels its JSON line from its own table of modes (dtype text, kernel names, peak), which lists the three
fp32-equivalent modes only, so `P2P_REGRESS_MODE=fp16 python bench.py` ends in KeyError.  This tool adds the entry for `fp16`
to that table IN MEMORY and calls bench.main(): the workload, the timing and the parity leg are bench.py's, unchanged.

    python tools/bench_fast_mode.py [--steps 30 --warmup 10 ...]      (any bench.py argument; --gpus 1 by default)

The numbers of NOTES.md ("Single-plane mode fp16: raw numbers") and DESIGN.md section 4 ("Single-plane mode") are this tool's
line next to `python bench.py` on the same box."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["P2P_REGRESS_MODE"] = "fp16"

import bench  # noqa: E402

bench.MODES["fp16"] = dict(
    kernel="p2p_regress_batch", products=1, peak=bench.PEAK_BF16_MFMA_TFLOPS,
    kernels=["fp16x1::regress_h2_kernel<true>", "fp16x1::wino_gemm_kernel", "regress_fc_kernel"],
    dtype="single-plane fp16 operands under exact power-of-two scales (NOT f32-equivalent: relative operand rounding 2^-11), "
          "1 fp16 MFMA product per product, f32 accumulate; second convolution as Winograd F(2x2,3x3)",
    peak_note="peak = 2500 TFLOP/s dense fp16 MFMA, one product per product")

if __name__ == "__main__":
    if not any(a.startswith("--gpus") for a in sys.argv[1:]):
        sys.argv[1:1] = ["--gpus", "1"]
    bench.main()
