"""Time the generic regressor (csrc/regress_generic.hip, csrc/regress_generic_h2.hip) in both of its arithmetics beside the tuned
modes: one regress_batch call of NPROP proposals (default 6400) x 2 levels on one 480x640 pair --
  * the released configuration (case R of tests/regressor_reference.py) through the untouched tuned `f32` and `fp16x2` modes and
    through a generic handle in `generic` (exact fp32 MFMA) and `generic_fp16x2` (two fp16 planes, three MFMA products), the four
    alternating in the same process (one box, one call: the spread of each is known from the same run), with the largest
    coordinate / score difference of generic against tuned f32 and of the two generic modes;
  * cases A and C (lighter configurations) and the ResNet50 feat_idx [0, 1] configuration (tests/bottleneck_reference.py:
    conv 64 / 64, fc 64 / 32 on 3 + 64 channels per image) in both generic modes.
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

    def handles(case, generic, mode=None, ck=None):
        ck = ck or rr.checkpoint(case)
        kw = dict(config=ck["regressor_config"], feat_idx=ck["feat_idx"], generic=generic)
        mid = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_mid."), dev, **kw)
        fine = ops.RegressorWeights(rr.sub_params(ck["state_dict"], "regress_fine."), dev, **kw)
        for r in (mid, fine):
            if mode:
                r.set_mode(mode)
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
            f"of exact-fp32 layer arithmetic, {len(ts)} calls, max {ts[-1]:.2f} ms)")
        return med, ts[0], ts[-1]

    def differences(ra, rb):
        """largest coordinate / score difference of two (mid, fine) handle pairs: the mid level on the proposals, the fine level
        of both started from ra's mid matches (so that no trunc() of a mid coordinate that differs in its last bits picks another patch)"""
        ma, mb = (ops.regress_batch(r[0], None, [a1], [a2], [props])[0] for r in (ra, rb))
        start = ma["matches1"].clone()
        fa, fb = (ops.regress_batch(r[1], None, [a1], [a2], [start])[0] for r in (ra, rb))
        dc = max((ma["matches1"] - mb["matches1"]).abs().max().item(), (fa["matches1"] - fb["matches1"]).abs().max().item())
        ds = max((ma["probs1"] - mb["probs1"]).abs().max().item(), (fa["probs1"] - fb["probs1"]).abs().max().item())
        return dc, ds

    def generic_pair(label, lay, ck=None, case=None):
        """both generic modes of one configuration, alternating; -> their (median, min, max) and the largest output difference"""
        regs = [handles(case, True, "generic", ck), handles(case, True, "generic_fp16x2", ck)]
        dc, ds = differences(*regs)
        timed(regs, warm)
        t_g, t_h = timed(regs, niter)
        r_g = report(f"{label} generic  ", lay, t_g)
        r_h = report(f"{label} generic_fp16x2", lay, t_h)
        say(f"{label} generic / generic_fp16x2 = {r_g[0] / r_h[0]:.2f}x (ranges {r_g[1]:.2f}-{r_g[2]:.2f} ms and {r_h[1]:.2f}-{r_h[2]:.2f} ms); "
            f"largest difference of the two modes' outputs (mid, and fine from the same mid) {dc:.3g} px / {ds:.3g}")
        return r_g, r_h

    say(f"device: {torch.cuda.get_device_name(0)}; pair {H}x{W}; WARMUP={warm} NITER={niter}")
    four = [handles("R", False, "f32"), handles("R", False, "fp16x2"), handles("R", True, "generic"), handles("R", True, "generic_fp16x2")]
    outs = [ops.regress_batch(m, f, [a1], [a2], [props])[0] for m, f in four]
    timed(four, warm)
    ts = timed(four, max(niter, 3))
    lay = ops.regressor_layout(None, None)
    r_t = report("case R tuned f32", lay, ts[0])
    r_t2 = report("case R tuned fp16x2", lay, ts[1])
    r_g = report("case R generic  ", lay, ts[2])
    r_h = report("case R generic_fp16x2", lay, ts[3])
    dc, ds = (outs[0]["matches2"] - outs[2]["matches2"]).abs().max().item(), (outs[0]["probs2"] - outs[2]["probs2"]).abs().max().item()
    say(f"case R generic / tuned f32 = {r_g[0] / r_t[0]:.2f}x; largest difference of the fine outputs {dc:.3g} px / {ds:.3g}")
    dc, ds = differences(four[2], four[3])
    say(f"case R generic / generic_fp16x2 = {r_g[0] / r_h[0]:.2f}x (ranges {r_g[1]:.2f}-{r_g[2]:.2f} ms and {r_h[1]:.2f}-{r_h[2]:.2f} ms; "
        f"generic_fp16x2 / tuned fp16x2 = {r_h[0] / r_t2[0]:.2f}x); largest difference of the two modes' outputs (mid, and fine from the same mid) {dc:.3g} px / {ds:.3g}")
    del four, outs
    for case in ("A", "C"):
        generic_pair(f"case {case}", ops.regressor_layout(rr.regressor_config(case), rr.CASES[case]["feat_idx"]), case=case)
    import bottleneck_reference as br  # noqa: E402
    rc = synthetic.default_regressor_config(**br.SMALL_RC)
    ck = synthetic.make_checkpoint(505, regressor_config=rc, feat_idx=[0, 1])
    generic_pair("ResNet50 feat_idx [0, 1]", ops.regressor_layout(rc, [0, 1]), ck=ck)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
