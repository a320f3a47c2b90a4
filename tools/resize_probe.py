"""Bicubic resize on the device (csrc/preprocess.hip) against Pillow on one host core, per image size:
  * Pillow's Image.resize(..., BICUBIC) on one core (the resize="host" path on this machine),
  * the device time of the two launches (resize + normalise) from events, after warm-up,
  * bytes moved / that time, against the HBM rate (NOTES.md: check every "HBM-bound" label),
  * the time of the upload of the original pixels (pinned memory, events).
`--stream N`: pairs/s of estimate_matches_stream with resize="host" and resize="device" on N copies of the example pairs.
    python tools/resize_probe.py [--stream 24]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from patch2pix_amd.utils.datasets import preprocess  # noqa: E402

HBM_TBS = 8.0
SIZES = [((1200, 1600), (480, 640)), ((768, 1024), (480, 640))]


def probe(in_hw, out_hw, reps=50):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, in_hw + (3,), dtype=np.uint8)
    pil = Image.fromarray(img, "RGB")
    torch.set_num_threads(1)
    pil.resize((out_hw[1], out_hw[0]), Image.BICUBIC)
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        want = pil.resize((out_hw[1], out_hw[0]), Image.BICUBIC)
        t.append(time.perf_counter() - t0)
    host_ms = 1e3 * float(np.median(t))
    pinned = torch.from_numpy(img).pin_memory()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    up = []
    for _ in range(10):
        start.record()
        pixels = pinned.to(dev, non_blocking=True)
        stop.record()
        stop.synchronize()
        up.append(start.elapsed_time(stop))
    out = torch.empty((1, 3) + out_hw, device=dev)
    for _ in range(5):
        preprocess.resize_pixels_device(pixels, out_hw, normalise=True, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start.record()
        preprocess.resize_pixels_device(pixels, out_hw, normalise=True, out=out)
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    dev_ms = float(np.median(times))
    assert torch.equal(out[0].cpu(), preprocess._normalised(want)), "device resize differs from Pillow"
    # read the source, write + read the intermediate (in_h rows of out_w pixels), write the float planes
    moved = in_hw[0] * in_hw[1] * 3 + 2 * in_hw[0] * out_hw[1] * 3 + out_hw[0] * out_hw[1] * 12
    rate = moved / (dev_ms * 1e-3) / 1e12
    print(f"resize {in_hw[1]}x{in_hw[0]} -> {out_hw[1]}x{out_hw[0]}: Pillow on one core {host_ms:.2f} ms | device (two launches, "
          f"table upload included) {1e3 * dev_ms:.1f} us, {moved / 1e6:.1f} MB moved = {rate:.2f} TB/s ({100 * rate / HBM_TBS:.0f} % of "
          f"{HBM_TBS:.0f} TB/s) | upload of {img.nbytes / 1e6:.1f} MB {1e3 * float(np.median(up)):.0f} us | device + upload "
          f"{dev_ms + float(np.median(up)):.2f} ms", flush=True)


def stream_rate(n):
    from patch2pix_amd.utils import synthetic
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.stream import estimate_matches_stream
    net = model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)
    d = os.path.join(ROOT, "tests", "golden", "images")
    pairs = [(os.path.join(d, "pair_3", "1.jpg"), os.path.join(d, "pair_3", "1.jpg"))] * n       # 1600x1200 -> 640x480
    for mode in ("host", "device", "host", "device"):
        list(estimate_matches_stream(net, pairs[:8], imsize=640, resize=mode))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = list(estimate_matches_stream(net, pairs, imsize=640, resize=mode))
        dt = time.perf_counter() - t0
        print(f"stream, {n} pairs of 1600x1200 photographs at imsize 640, resize={mode!r}: {len(got) / dt:.1f} pairs/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", type=int, default=0)
    args = ap.parse_args()
    for in_hw, out_hw in SIZES:
        probe(in_hw, out_hw)
    if args.stream:
        stream_rate(args.stream)
