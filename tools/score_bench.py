"""Time the pair score (p2p_coarse_score_batch) beside the one-candidate match kernels, which read the same volume in the
same passes and write more: BATCH (default 16) pooled volumes of a 480x640 pair at ksize 2 (30x40x30x40 cells, 5.8 MB each),
seeded random values.  p2p_coarse_matches_batch (the yardstick) and the new entry with normalize none, softmax and l1 (cell
scores returned) and softmax without cell scores (through the workspace) alternate in one process: HIP events around REPS
(default 20) back-to-back calls, WARMUP rounds first (default 2), the median and minimum of NITER rounds (default 7).  The
timed calls go to the C entry points directly, on outputs allocated once.  Also checks that the softmax cell scores are the
yardstick's scores bit for bit.  Prints one line per measurement and, with --out FILE, writes them to FILE as well.
No GPU: fails."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from patch2pix_amd import _lib  # noqa: E402


def main():
    if not torch.cuda.is_available():
        sys.exit("score_bench: no GPU (this tool measures; it does not fall back)")
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
    na, nb = ha * wa, hb * wb
    n = na + nb
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    yard = (torch.empty((batch, n, 4), dtype=torch.int64, device=dev), torch.empty((batch, n), dtype=torch.float32, device=dev))
    cells = torch.empty((batch, n), dtype=torch.float32, device=dev)
    pair = torch.empty((batch,), dtype=torch.float32, device=dev)
    need = _lib.p2p_coarse_score_workspace_bytes(batch, ha, wa, hb, wb)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def one_candidate():
        _lib.check(_lib.p2p_coarse_matches_batch(corr.data_ptr(), delta.data_ptr(), batch, ha, wa, hb, wb, ksize, up, 1,
                                                 yard[0].data_ptr(), yard[1].data_ptr(), stream), "p2p_coarse_matches_batch")

    def score(norm, with_cells=True):
        _lib.check(_lib.p2p_coarse_score_batch(corr.data_ptr(), batch, ha, wa, hb, wb, _lib.SCORE_NORMS[norm],
                                               cells.data_ptr() if with_cells else None, pair.data_ptr(),
                                               None if with_cells else ws.data_ptr(), 0 if with_cells else need, stream),
                   "p2p_coarse_score_batch")

    # (name, call, passes over the volume per direction)
    runs = [("p2p_coarse_matches_batch     ", one_candidate, 2),
            ("score none                   ", lambda: score(None), 1),
            ("score softmax                ", lambda: score("softmax"), 2),
            ("score l1                     ", lambda: score("l1"), 1),
            ("score softmax, no cell_scores", lambda: score("softmax", False), 2)]

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

    say(f"device: {torch.cuda.get_device_name(0)}; {batch} volumes of {'x'.join(map(str, dims))} cells; "
        f"WARMUP={warm} NITER={niter} REPS={reps}")
    one_candidate()
    score("softmax")
    torch.cuda.synchronize()
    same = torch.equal(torch.cat([yard[1][:, nb:], yard[1][:, :nb]], dim=1).view(torch.int32), cells.view(torch.int32))
    say(f"softmax cell scores == the scores of p2p_coarse_matches_batch bit for bit: {bool(same)}")
    timed(warm)
    ts = timed(niter)
    volume_bytes = corr.numel() * 4
    base = None
    for (name, _, passes), t in zip(runs, ts):
        t = sorted(t)
        med = t[len(t) // 2]
        base = base or med
        say(f"{name}: median {med:8.1f} us  min {t[0]:8.1f} us  {med / base:5.2f}x the one-candidate kernels  "
            f"({2 * passes} volume reads, {2 * passes * volume_bytes / med / 1e6:.2f} TB/s)")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
