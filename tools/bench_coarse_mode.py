"""Coarse stage, default mode against the opt-in single-plane mode 'fp16' (NcnWeights.set_mode), alternating on one device.

    python tools/bench_coarse_mode.py [--rounds 3] [--iters 20] [--parent-lib /path/to/libp2p_hip.so]

Reports ms per pair of ops.coarse_forward_batch at 480x640 and 960x1280 (layer-3 maps 60x80 and 120x160, ksize 2), in a batch
of 16 (2 at 960x1280) and alone, `--rounds` times default / fp16 in turn.  --parent-lib: the default mode of this tree against
another build of the library (the parent commit's) through the C ABI on the same inputs, alternating: output bits and time.
The bench.py workload with the stages in fp16 is measured with bench.py itself under P2P_COARSE_MODE / P2P_BACKBONE_MODE /
P2P_REGRESS_FP16 (the environment variables the Python layer reads)."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from patch2pix_amd import _lib, ops  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def features(seed, batch, h, w, dev):
    gen = torch.Generator().manual_seed(seed)
    fa = torch.relu(torch.randn(batch, 256, h, w, generator=gen))
    fb = torch.relu(fa.roll((3, 5), (2, 3)) + 0.3 * torch.randn(batch, 256, h, w, generator=gen))
    return fa.to(dev), fb.to(dev)


def stage(ncn, fa, fb, ksize=2):
    b, _, h, w = fa.shape
    shape = (b, h // ksize, w // ksize, h // ksize, w // ksize)
    corr = torch.empty(shape, dtype=torch.float32, device=fa.device)
    delta = torch.empty(shape, dtype=torch.uint8, device=fa.device)
    return (lambda: ops.coarse_forward_batch(fa, fb, ksize, ncn, out_corr=corr, out_delta=delta)), corr


def c_abi_stage(lib, sd, fa, fb, ksize=2):
    """The default mode through the C ABI of `lib` (a ctypes.CDLL of any build) -> (callable, corr)."""
    keep = [sd[k].detach().float().contiguous() for k in ("ncn.conv.0.weight", "ncn.conv.0.bias", "ncn.conv.2.weight", "ncn.conv.2.bias")]
    lib.p2p_ncn_create.argtypes = [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_void_p)]
    lib.p2p_coarse_workspace_bytes.restype = ctypes.c_size_t
    lib.p2p_coarse_workspace_bytes.argtypes = [ctypes.c_int] * 6
    lib.p2p_coarse_forward_batch.argtypes = ([ctypes.c_void_p] * 2 + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p])
    h = ctypes.c_void_p()
    assert lib.p2p_ncn_create(*[t.data_ptr() for t in keep], ctypes.byref(h)) == 0
    b, c, hh, ww = fa.shape
    shape = (b, hh // ksize, ww // ksize, hh // ksize, ww // ksize)
    corr = torch.empty(shape, dtype=torch.float32, device=fa.device)
    delta = torch.empty(shape, dtype=torch.uint8, device=fa.device)
    need = b * lib.p2p_coarse_workspace_bytes(c, hh, ww, hh, ww, ksize)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=fa.device)
    base = (ws.data_ptr() + 255) & ~255

    def run():
        st = lib.p2p_coarse_forward_batch(fa.data_ptr(), fb.data_ptr(), b, c, hh, ww, hh, ww, ksize, h, corr.data_ptr(), delta.data_ptr(),
                                          base, need, torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
    run.keep = (ws, keep, delta)
    return run, corr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synthetic.make_state_dict(0)
    ncn = ops.NcnWeights.from_state_dict({k[len("ncn."):]: v for k, v in sd.items() if k.startswith("ncn.")}, dev)
    print(f"library version {_lib.p2p_version()}, device {torch.cuda.get_device_name(0)}")
    for (h, w, batches) in ((60, 80, (16, 1)), (120, 160, (2, 1))):
        for batch in batches:
            fa, fb = features(7, batch, h, w, dev)
            run, corr = stage(ncn, fa, fb)
            for r in range(args.rounds):
                ms = {}
                for mode in ("fp16x2", "fp16"):
                    ncn.set_mode(mode)
                    ms[mode] = timed(run, args.iters) / batch
                print(f"coarse stage {8 * h}x{8 * w} ksize 2 batch {batch:2d} round {r}: default {ms['fp16x2']:.4f} ms/pair, "
                      f"fp16 {ms['fp16']:.4f} ms/pair, ratio {ms['fp16x2'] / ms['fp16']:.3f}")
            ncn.set_mode("fp16x2")
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        fa, fb = features(7, 16, 60, 80, dev)
        run_new, corr_new = c_abi_stage(_lib.lib, sd, fa, fb)
        run_old, corr_old = c_abi_stage(parent, sd, fa, fb)
        for r in range(args.rounds):
            t_old, t_new = timed(run_old, args.iters) / 16, timed(run_new, args.iters) / 16
            print(f"default mode 480x640 batch 16 round {r}: parent build {t_old:.4f} ms/pair, this tree {t_new:.4f} ms/pair, "
                  f"output bits {'identical' if torch.equal(corr_old, corr_new) else 'DIFFER'}")


if __name__ == "__main__":
    main()
