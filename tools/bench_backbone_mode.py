"""The pyramid producer in its two arithmetics, `fp16x2` (default) and the opt-in single-plane `fp16` (P2P_CONV_FP16), and what
the choice is worth end to end -- one process on one box, the modes alternating (a repetition of every mode before the next
repetition of any), so that drift of the box lands on all of them alike.

    python tools/bench_backbone_mode.py [--reps 5] [--iters 20] [--stream-pairs 160] [--no-stream]

  producer   ms per 480x640 image of extract.pyramid on a batch of 16, per repetition and the median;
  stream     pairs/s of estimate_matches_stream(batch=8, workers=4) over JPEG files for the four combinations of backbone mode
             (fp16x2 | fp16) and regressor mode (fp16x2w | fp16), per repetition and the median.

The numbers of DESIGN.md section 4 ("Single-plane mode of the producer") and of profiles/backbone_mode_bench.txt are this tool's
output."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from patch2pix_amd.utils import synthetic  # noqa: E402
from patch2pix_amd.utils.eval import model_helper  # noqa: E402

H, W, BATCH = 480, 640, 16
BACKBONE_MODES = ("fp16x2", "fp16")
REGRESS_MODES = ("fp16x2w", "fp16")


def producer_ms(net, x, iters):
    with torch.no_grad():
        for _ in range(3):
            net.extract.pyramid(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            net.extract.pyramid(x)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters / x.shape[0] * 1e3


def stream_rate(net, work, warm):
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    list(estimate_matches_stream(net, warm, batch=8, workers=4))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in estimate_matches_stream(net, work, batch=8, workers=4))
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="producer launches of the batch per timed window")
    ap.add_argument("--stream-pairs", type=int, default=160)
    ap.add_argument("--no-stream", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_backbone_mode: needs an MI355X; there is no CPU path and no number to report without one")
    torch.cuda.set_device(0)
    os.environ.pop("P2P_BACKBONE_MODE", None)
    os.environ["P2P_BACKBONE"] = "hip"
    net = model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)
    _, mid, fine = net._weights()
    x = torch.randn(BATCH, 3, H, W, device=net.device)

    print(f"producer: extract.pyramid, batch {BATCH} of {H}x{W}, {args.iters} launches per window, ms per image")
    times = {m: [] for m in BACKBONE_MODES}
    for _ in range(args.reps):
        for m in BACKBONE_MODES:
            net.extract.set_mode(m)
            times[m].append(producer_ms(net, x, args.iters))
    for m in BACKBONE_MODES:
        print(f"  {m:7s} " + " ".join(f"{t:.4f}" for t in times[m]) + f"   median {statistics.median(times[m]):.4f}")
    print(f"  fp16x2 / fp16 (medians): {statistics.median(times['fp16x2']) / statistics.median(times['fp16']):.3f}x")
    if args.no_stream:
        return

    from PIL import Image
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for i in range(8):
            a, b = synthetic.make_image_pair(100 + i, H, W)
            pa, pb = os.path.join(td, f"{i}a.jpg"), os.path.join(td, f"{i}b.jpg")
            Image.fromarray(a).save(pa, quality=95)
            Image.fromarray(b).save(pb, quality=95)
            paths.append((pa, pb))
        work = (paths * (args.stream_pairs // 8 + 1))[:args.stream_pairs]
        combos = [(b, r) for b in BACKBONE_MODES for r in REGRESS_MODES]
        rates = {c: [] for c in combos}
        print(f"stream: estimate_matches_stream(batch=8, workers=4), {len(work)} pairs of {H}x{W} JPEG files per window, pairs/s")
        try:
            for _ in range(args.reps):
                for b, r in combos:
                    net.extract.set_mode(b)
                    mid.set_mode(r)
                    fine.set_mode(r)
                    rates[(b, r)].append(stream_rate(net, work, paths * 3))
        finally:
            net.extract.set_mode("fp16x2")
            mid.set_mode("fp16x2w")
            fine.set_mode("fp16x2w")
        base = statistics.median(rates[("fp16x2", "fp16x2w")])
        for c in combos:
            med = statistics.median(rates[c])
            print(f"  backbone {c[0]:7s} regressors {c[1]:8s} " + " ".join(f"{v:7.1f}" for v in rates[c]) +
                  f"   median {med:7.1f}  ({med / base:.3f}x the default pair)")


if __name__ == "__main__":
    main()
