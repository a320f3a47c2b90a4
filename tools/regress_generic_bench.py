"""Time the generic regressor (csrc/regress_generic.hip) beside the tuned exact-fp32 mode: one regress_batch call of
NPROP proposals (default 6400) x 2 levels on one 480x640 pair --
  * the released configuration (case R of tests/regressor_reference.py) through a generic handle and through the untouched
    tuned `f32` mode, alternating in the same process (the yardstick), with the largest coordinate / score difference of the two;
  * cases A and C (lighter configurations) through their generic handles.
HIP events around the call, WARMUP calls first (default 2), the median and minimum of NITER timed calls (default 7).
Prints one line per measurement and, with --out FILE, writes them to FILE as well.  No GPU: fails."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from patch2pix_amd import ops  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402
import regressor_reference as rr  # noqa: E402


def conv_flops(lay, n, levels=2):
    """Multiply-adds x 2 of the convolutions and FC layers of `levels` regressor levels over n proposals."""
    shapes, _ = ops.regressor_shapes(lay)
    spp = 2 if lay["feat_comb"] == "post" else 1
    side, total = 16, 0
    for i, (k, st) in enumerate(zip(lay["conv_kers"], lay["conv_strs"])):
        co, ci = shapes[f"conv.{2 * i}.weight"][:2]
        side = (side + 2 - k) // st + 1
        total += spp * side * side * co * ci * k * k
    total += sum(s[0] * s[1] for key, s in shapes.items() if key.startswith("fc.") and len(s) == 2)
    return 2 * total * n * levels


def main():
    if not torch.cuda.is_available():
        sys.exit("regress_generic_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda:0")
    n, niter, warm = int(os.environ.get("NPROP", "6400")), int(os.environ.get("NITER", "7")), int(os.environ.get("WARMUP", "2"))
    H, W = 480, 640
    p1, p2 = synthetic.make_pyramid(7, H, W), synthetic.make_pyramid(8, H, W)
    a1, a2 = [t.to(dev) for t in p1[:4]], [t.to(dev) for t in p2[:4]]
    g = torch.Generator().manual_seed(9)
    props = torch.stack([torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g),
                         torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g)], 1).to(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def handles(case, generic):
        ck = rr.checkpoint(case)
        kw = dict(config=ck["regressor_config"], feat_idx=ck["feat_idx"], generic=generic)
        mid = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_mid."), dev, **kw)
        fine = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_fine."), dev, **kw)
        return mid, fine

    def timed(regs, rounds):
        """rounds x one timed call per entry of regs, alternating -> list of times per entry"""
        ts = [[] for _ in regs]
        for _ in range(rounds):
            for i, (mid, fine) in enumerate(regs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.regress_batch(mid, fine, [a1], [a2], [props])
                e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1))
        return ts

    def report(name, lay, ts):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        say(f"{name}: n={n} x 2 levels  median {med:.2f} ms  min {ts[0]:.2f} ms  ({conv_flops(lay, n) / med / 1e9:.1f} TFLOP/s "
            f"of exact-fp32 layer arithmetic, {len(ts)} calls)")
        return med

    say(f"device: {torch.cuda.get_device_name(0)}; pair {H}x{W}; WARMUP={warm} NITER={niter}")
    tuned, generic = handles("R", False), handles("R", True)
    for r in tuned:
        r.set_mode("f32")
    both = [tuned, generic]
    outs = [ops.regress_batch(m, f, [a1], [a2], [props])[0] for m, f in both]
    dc = (outs[0]["matches2"] - outs[1]["matches2"]).abs().max().item()
    ds = (outs[0]["probs2"] - outs[1]["probs2"]).abs().max().item()
    timed(both, warm)
    t_tuned, t_gen = timed(both, niter)
    lay = ops.regressor_layout(None, None)
    m_t = report("case R tuned f32", lay, t_tuned)
    m_g = report("case R generic  ", lay, t_gen)
    say(f"case R generic / tuned f32 = {m_g / m_t:.2f}x; largest difference of the fine outputs {dc:.3g} px / {ds:.3g}")
    del tuned, generic, both
    for case in ("A", "C"):
        regs = [handles(case, True)]
        timed(regs, warm)
        report(f"case {case} generic  ", ops.regressor_layout(rr.regressor_config(case), rr.CASES[case]["feat_idx"]), timed(regs, niter)[0])
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
