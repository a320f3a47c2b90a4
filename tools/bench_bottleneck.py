"""The ResNet50 / ResNet101 pyramid producers (HIP path and the all-PyTorch MIOpen path, both producer modes) and the coarse
stage at 1024 against 256 channels -- one process on one box, the variants alternating (a repetition of every variant before the
next repetition of any), so that drift of the box lands on all of them alike.

    python tools/bench_bottleneck.py [--reps 3] [--iters 5]

Prints one JSON line:
  producer_ms_per_image   {backbone: {"hip_fp16x2", "hip_fp16", "miopen"}}: ms per 480x640 image of extract.pyramid, batch 16,
                          stride 8 (change_stride), median of the repetitions (ResNet34 is there as the yardstick);
  coarse_ms_per_pair      {"c256", "c1024"}: ms per pair of forward_coarse_match at 60x80 cells (480x640, stride 8), ksize 2,
                          batch 16, both coarse modes.

The numbers of DESIGN.md section 4 ("Bottleneck backbones and 1024-channel matching") and of profiles/bottleneck_bench.txt are
this tool's output."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from patch2pix_amd import ops  # noqa: E402
from patch2pix_amd.networks import resnet  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402

H, W, BATCH = 480, 640, 16


def timed(fn, iters):
    with torch.no_grad():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters / BATCH * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5, help="launches of the batch per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bottleneck: needs an MI355X; there is no CPU path and no number to report without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    os.environ.pop("P2P_BACKBONE_MODE", None)
    x = torch.randn(BATCH, 3, H, W, device=dev)
    nets = {}
    for name in ("ResNet34", "ResNet50", "ResNet101"):
        net = getattr(resnet, name)()
        net.change_stride("layer3")
        sd = synthetic.make_backbone_checkpoint(1, name)["state_dict"]
        net.load_state_dict({k[len("extract."):]: v for k, v in sd.items() if k.startswith("extract.")})
        nets[name] = net.eval().to(dev)
    variants = [("hip_fp16x2", "hip", "fp16x2"), ("hip_fp16", "hip", "fp16"), ("miopen", "miopen", "fp16x2")]
    prod = {n: {v[0]: [] for v in variants} for n in nets}
    for _ in range(args.reps):
        for name, net in nets.items():
            for key, path, mode in variants:
                os.environ["P2P_BACKBONE"] = path
                net.set_mode(mode)
                prod[name][key].append(timed(lambda: net.pyramid(x), args.iters))
            net.set_mode("fp16x2")
    os.environ["P2P_BACKBONE"] = "hip"

    sd0 = synthetic.make_state_dict(0, backbone=False)
    ncn = ops.NcnWeights.from_state_dict({k[len("ncn."):]: v for k, v in sd0.items() if k.startswith("ncn.")}, dev)
    coarse = {f"c{c}": {m: [] for m in ("fp16x2", "fp16")} for c in (256, 1024)}
    feats = {c: (torch.relu(torch.randn(BATCH, c, H // 8, W // 8, device=dev)), torch.relu(torch.randn(BATCH, c, H // 8, W // 8, device=dev)))
             for c in (256, 1024)}
    for _ in range(args.reps):
        for c, (fa, fb) in feats.items():
            for m in ("fp16x2", "fp16"):
                ncn.set_mode(m)
                coarse[f"c{c}"][m].append(timed(lambda: ops.coarse_forward_batch(fa, fb, 2, ncn), args.iters))
    ncn.set_mode("fp16x2")
    med = lambda d: {k: (med(v) if isinstance(v, dict) else round(statistics.median(v), 4)) for k, v in d.items()}
    print(json.dumps({"tool": "bench_bottleneck", "image": [H, W], "batch": BATCH, "reps": args.reps, "iters": args.iters,
                      "device": torch.cuda.get_device_name(0), "producer_ms_per_image": med(prod), "coarse_ms_per_pair": med(coarse)}))


if __name__ == "__main__":
    main()
