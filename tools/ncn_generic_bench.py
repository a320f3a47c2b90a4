"""Time the generic consensus net (csrc/consensus_generic.hip, csrc/consensus_generic_h2.hip) in both of its arithmetics: one
neigh_consensus_batch call per configuration on random mutual-matched volumes of 30 x 40 x 30 x 40 cells (a 480 x 640 pair at
stride 16), batch 1 and 4 --
  * cases P (NCNet's published [5,5,5] / [16,16,1]), N (the class default [3,3,3] / [10,10,1]) and R (the released [3,3] / [16,1]
    forced generic) of tests/ncn_reference.py through one handle each in `generic` (exact fp32 MFMA) and `generic_fp16x2` (every
    layer behind the first on the fp16 matrix cores, two fp16 planes, three MFMA products), the two alternating in the same
    process, with the largest difference of the two modes' outputs relative to the largest output;
  * per layer kind (batch 1): the same events around prefix stacks of the case's own shapes -- [k] / [1] (the one-input-channel
    layer: its columns are padded to 16 whatever it stores), [k, k] / [c, 1] (+ a c -> 1 layer), [k, k, k] / [c, c, 1]
    (+ a c -> c layer) -- whose differences are the times of one c -> 1 and one c -> c layer (both branches).
HIP events around the call, WARMUP rounds first (default 2), the median, minimum and maximum of NITER timed calls (default 7).
Prints one line per measurement and, with --out FILE, writes them to FILE as well.  No GPU: fails."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from patch2pix_amd import ops  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402
import ncn_reference as nr  # noqa: E402

SHAPE = (30, 40, 30, 40)


def volumes(batch, dev):
    """mutual-matched correlations of random unit features, the magnitudes the pipeline feeds the net"""
    fa, fb = nr.features(4242 + batch, (batch,) + SHAPE)
    fa = fa / (fa.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    fb = fb / (fb.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    return nr.mutual_matching(torch.einsum("bcij,bckl->bijkl", fa.to(dev), fb.to(dev))).contiguous()


def flops(layout, batch):
    cells, cin, total = SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3], 1, 0
    for k, c in zip(layout["kernel_sizes"], layout["channels"]):
        total += k ** 4 * cin * c
        cin = c
    return 2 * total * cells * batch * (2 if layout["symmetric_mode"] else 1)


def main():
    if not torch.cuda.is_available():
        sys.exit("ncn_generic_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda:0")
    niter, warm = int(os.environ.get("NITER", "7")), int(os.environ.get("WARMUP", "2"))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def handle(sd, layout, mode):
        h = ops.NcnWeights.from_state_dict(sd, dev, symmetric_mode=layout["symmetric_mode"], generic=True)
        h.set_mode(mode)
        return h

    def timed(hs, x, rounds):
        ts = [[] for _ in hs]
        for _ in range(rounds):
            for i, h in enumerate(hs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.neigh_consensus_batch(x, h)
                e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1))
        return [sorted(t) for t in ts]

    def both(label, sd, layout, x, quiet=False):
        hs = [handle(sd, layout, "generic"), handle(sd, layout, "generic_fp16x2")]
        y = [ops.neigh_consensus_batch(x, h) for h in hs]
        diff = ((y[0] - y[1]).abs().max() / y[0].abs().max().clamp_min(1e-30)).item()
        timed(hs, x, warm)
        ts = timed(hs, x, niter)
        med = [t[len(t) // 2] for t in ts]
        if not quiet:
            for name, t, m in zip(("generic       ", "generic_fp16x2"), ts, med):
                say(f"{label} {name}: median {m:.3f} ms  min {t[0]:.3f} ms  max {t[-1]:.3f} ms  ({flops(layout, x.shape[0]) / m / 1e9:.1f} "
                    f"TFLOP/s of exact layer arithmetic, {len(t)} calls)")
            say(f"{label} generic / generic_fp16x2 = {med[0] / med[1]:.2f}x (ranges {ts[0][0]:.3f}-{ts[0][-1]:.3f} ms and "
                f"{ts[1][0]:.3f}-{ts[1][-1]:.3f} ms); largest difference of the two modes' outputs {diff:.3g} of the largest output")
        return med

    say(f"device: {torch.cuda.get_device_name(0)}; volume {'x'.join(map(str, SHAPE))}; WARMUP={warm} NITER={niter}")
    for case in ("P", "N", "R"):
        layout, sd = nr.CASES[case], nr.weights(case)
        for batch in (1, 4):
            both(f"case {case} batch {batch}", sd, layout, volumes(batch, dev))
        # layer kinds from prefix stacks of the case's shapes (batch 1)
        k, c, n = layout["kernel_sizes"][0], layout["channels"][0], len(layout["kernel_sizes"])
        x = volumes(1, dev)
        meds = []
        for depth in range(1, n + 1):
            ks, ch = [k] * depth, [c] * (depth - 1) + [1]
            psd = synthetic.make_ncn_state_dict(nr.SEEDS[case], ks, ch, gain=nr.GAINS[case], bias=0.02, prefix="")
            meds.append(both("", psd, dict(kernel_sizes=ks, channels=ch, symmetric_mode=layout["symmetric_mode"]), x, quiet=True))
        say(f"case {case} layer kinds, both branches, batch 1 (generic / generic_fp16x2): 1 -> any {meds[0][0]:.3f} / {meds[0][1]:.3f} ms (exact in both)"
            + (f"; {c} -> 1 {meds[1][0] - meds[0][0]:.3f} / {meds[1][1] - meds[0][1]:.3f} ms" if n > 1 else "")
            + (f"; {c} -> {c} {meds[2][0] - meds[1][0]:.3f} / {meds[2][1] - meds[1][1]:.3f} ms" if n > 2 else ""))
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
