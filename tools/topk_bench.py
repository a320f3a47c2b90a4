"""Time the top-k match extraction (p2p_coarse_matches_topk_batch) beside the one-candidate kernels it extends: BATCH
(default 16) pooled volumes of a 480x640 pair at ksize 2 (30x40x30x40 cells, 5.8 MB each), seeded random values and delta
bytes.  p2p_coarse_matches_batch (the yardstick) and the new entry at topk 1, 2, 4 and 8 with softmax, and at topk 1 and 4
with raw scores, alternate in one process: HIP events around REPS (default 20) back-to-back calls, WARMUP rounds first
(default 2), the median and minimum of NITER rounds (default 7).  The timed calls go to the C entry points directly, on
outputs allocated once: no allocation and no tensor checks inside the events, so a figure is the two kernels of a call plus
their launches.  Also checks that topk = 1 returns the yardstick's bits.  ONLY_TOPK=k (1, 2, 4 or 8) times the yardstick and
that one softmax case alone: topk is a run-time argument, so a kernel-stats profile of the full run averages every topk.
Prints one line per measurement and, with --out FILE, writes them to FILE as well.  No GPU: fails."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from patch2pix_amd import _lib  # noqa: E402


def main():
    if not torch.cuda.is_available():
        sys.exit("topk_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda:0")
    env = lambda k, d: int(os.environ.get(k, d))
    batch, reps, niter, warm = env("BATCH", "16"), env("REPS", "20"), env("NITER", "7"), env("WARMUP", "2")
    ksize, up = 2, 8
    dims = (30, 40, 30, 40)
    gen = torch.Generator(device=dev).manual_seed(5)
    corr = torch.rand((batch,) + dims, generator=gen, device=dev)
    delta = torch.randint(0, ksize ** 4, (batch,) + dims, generator=gen, device=dev).to(torch.uint8)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ha, wa, hb, wb = dims
    n = ha * wa + hb * wb
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {k: (torch.empty((batch, k * n, 4), dtype=torch.int64, device=dev),
               torch.empty((batch, k * n), dtype=torch.float32, device=dev)) for k in (1, 2, 4, 8)}
    yard = (torch.empty_like(out[1][0]), torch.empty_like(out[1][1]))

    def one_candidate():
        _lib.check(_lib.p2p_coarse_matches_batch(corr.data_ptr(), delta.data_ptr(), batch, ha, wa, hb, wb, ksize, up, 1,
                                                 yard[0].data_ptr(), yard[1].data_ptr(), stream), "p2p_coarse_matches_batch")

    def topk_call(topk, sm):
        m, sc = out[topk]
        _lib.check(_lib.p2p_coarse_matches_topk_batch(corr.data_ptr(), delta.data_ptr(), batch, ha, wa, hb, wb, ksize, up, 1,
                                                      topk, int(sm), m.data_ptr(), sc.data_ptr(), stream),
                   "p2p_coarse_matches_topk_batch")

    runs = [("p2p_coarse_matches_batch     ", one_candidate, 2)]
    cases = ((1, True), (2, True), (4, True), (8, True), (1, False), (4, False))
    if "ONLY_TOPK" in os.environ:                # one softmax case beside the yardstick: the run to put under a profiler,
        cases = ((env("ONLY_TOPK", "4"), True),)  # whose per-kernel averages would otherwise mix every topk
    for topk, sm in cases:
        runs.append((f"topk {topk} {'softmax' if sm else 'raw    '}               ",
                     lambda topk=topk, sm=sm: topk_call(topk, sm), topk + (1 if sm else 0)))

    def timed(rounds):
        ts = [[] for _ in runs]
        for _ in range(rounds):
            for i, (_, fn, _) in enumerate(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1) / reps * 1e3)          # us per call
        return ts

    say(f"device: {torch.cuda.get_device_name(0)}; {batch} volumes of {'x'.join(map(str, dims))} cells, ksize {ksize}; "
        f"WARMUP={warm} NITER={niter} REPS={reps}")
    one_candidate()
    topk_call(1, True)
    same = torch.equal(yard[0], out[1][0]) and torch.equal(yard[1].view(torch.int32), out[1][1].view(torch.int32))
    say(f"topk 1 softmax == p2p_coarse_matches_batch bit for bit: {bool(same)}")
    timed(warm)
    ts = timed(niter)
    volume_bytes = corr.numel() * 4
    base = None
    for (name, _, passes), t in zip(runs, ts):
        t = sorted(t)
        med = t[len(t) // 2]
        base = base or med
        # every pass reads the volume once per direction
        say(f"{name}: median {med:8.1f} us  min {t[0]:8.1f} us  {med / base:5.2f}x the one-candidate kernels  "
            f"({2 * passes} volume reads, {2 * passes * volume_bytes / med / 1e6:.2f} TB/s)")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
