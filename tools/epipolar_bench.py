"""Time the epipolar evaluation on the device (p2p_epipolar_batch) beside the path a user has without it: BATCH (default 16)
pairs of ROWS (default 1200) float64 match rows -- the layout p2p_match_tail_batch leaves on the device --, Sampson distance,
the default bins of check_inliers_distr.
  * device: the C entry point on outputs allocated once, HIP events around REPS (default 20) back-to-back calls;
  * host:   the device-to-host copy of the same rows (pageable memory, as `tensor.cpu()` gives it) plus the reference's numpy
            expression (utils/eval/measure.py:30-40) and np.histogram per pair, wall clock around one pass.
WARMUP rounds first (default 2), the median and minimum of NITER rounds (default 7).  Also checks that the two paths count the
same rows per bin.  Prints one line per measurement and, with --out FILE, writes them to FILE as well.
No GPU: fails."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from patch2pix_amd import _lib, ops  # noqa: E402


def numpy_sampson(rows, F, eps=1e-8):
    """The reference's expression, restated (measure.py:30-40)."""
    pts1 = np.concatenate([rows[:, 0:2], np.ones((rows.shape[0], 1))], axis=1)
    pts2 = np.concatenate([rows[:, 2:4], np.ones((rows.shape[0], 1))], axis=1)
    l2 = np.dot(F, pts1.T)
    l1 = np.dot(F.T, pts2.T)
    dd = np.sum(l2.T * pts2, 1)
    return dd ** 2 / (eps + l1[0, :] ** 2 + l1[1, :] ** 2 + l2[0, :] ** 2 + l2[1, :] ** 2)


def main():
    if not torch.cuda.is_available():
        sys.exit("epipolar_bench: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda:0")
    env = lambda k, d: int(os.environ.get(k, d))
    batch, nrows, reps, niter, warm = env("BATCH", "16"), env("ROWS", "1200"), env("REPS", "20"), env("NITER", "7"), env("WARMUP", "2")
    bins = ops.EPI_BINS_MEASURE
    rng = np.random.default_rng(7)
    rows_h = rng.uniform(0, 640, (batch, nrows, 4))
    rows_h[:, :, 2:] = rows_h[:, :, :2] + rng.normal(scale=8.0, size=(batch, nrows, 2))
    F_h = np.stack([np.array([[0, -1e-3 * (1 + b), 0.3], [1e-3 * (1 + b), 0, -0.2], [-0.3, 0.2, 1e-2 * b]]) for b in range(batch)])
    rows, F = torch.from_numpy(rows_h).to(dev), torch.from_numpy(F_h.reshape(batch, 9)).to(dev)
    counts = torch.full((batch,), nrows, dtype=torch.int32, device=dev)
    edges = torch.tensor(bins, dtype=torch.float64, device=dev)
    dist = torch.empty((batch, nrows), dtype=torch.float64, device=dev)
    hist = torch.empty((batch, len(bins) - 1), dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def device_call():
        _lib.check(_lib.p2p_epipolar_batch(rows.data_ptr(), _lib.DTYPES["float64"], counts.data_ptr(), F.data_ptr(), batch, nrows,
                                           _lib.EPI_KINDS["sampson"], 1e-8, edges.data_ptr(), len(bins) - 1, dist.data_ptr(),
                                           _lib.DTYPES["float64"], hist.data_ptr(), stream), "p2p_epipolar_batch")

    def host_path():
        host = rows.cpu().numpy()
        return [np.histogram(numpy_sampson(host[b], F_h[b]), bins)[0] for b in range(batch)]

    def timed(rounds):
        td, th = [], []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                device_call()
            e1.record()
            torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1) / reps * 1e3)          # us per call
            t0 = time.perf_counter()
            host_path()
            th.append((time.perf_counter() - t0) * 1e6)
        return td, th

    say(f"device: {torch.cuda.get_device_name(0)}; {batch} pairs x {nrows} rows, Sampson distance, {len(bins) - 1} bins; "
        f"WARMUP={warm} NITER={niter} REPS={reps}")
    device_call()
    torch.cuda.synchronize()
    same = np.array_equal(hist.cpu().numpy(), np.stack(host_path()))
    say(f"bin counts of the device path == np.histogram of the reference's expression on the host: {bool(same)}")
    timed(warm)
    td, th = timed(niter)
    for name, t in (("p2p_epipolar_batch (device, HIP events)          ", td),
                    ("copy to the host + numpy + np.histogram (wall)   ", th)):
        t = sorted(t)
        say(f"{name}: median {t[len(t) // 2]:9.1f} us  min {t[0]:9.1f} us")
    say(f"ratio of the medians (host path / device call): {sorted(th)[len(th) // 2] / sorted(td)[len(td) // 2]:.1f}")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
