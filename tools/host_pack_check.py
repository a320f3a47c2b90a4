#!/usr/bin/env python3
"""Do two trees pack the same bytes and compute the same results?  `python tools/host_pack_check.py OLD_TREE [NEW_TREE]`

Each tree builds its own emulated library (tests/hipemu/build_emu.py) and runs every constructor of the C ABI on the same
fixed-seed inputs, at the smallest shapes that walk every packing loop; every output array of the two trees must be equal
byte for byte (the emulator is deterministic: no tolerance).  One process per tree (`--dump FILE --tree TREE`), so that each
imports its own tests/hipemu and its own prototypes.  Exit status 1 on any difference."""
import os
import subprocess
import sys
import tempfile

import numpy as np


def dump(tree, out_file):
    sys.path[:0] = [tree, os.path.join(tree, "tests"), os.path.join(tree, "tests", "hipemu")]
    import ctypes
    import torch
    import emu_lib
    import ncn_reference as nr
    import regressor_reference as rr
    from patch2pix_amd.utils import synthetic
    emu = emu_lib.load()
    out = {}
    gen = torch.Generator().manual_seed(2024)
    rnd = lambda *s: torch.randn(*s, generator=gen)

    def bn(c):      # weight, bias, running_mean, running_var
        return [1.0 + 0.2 * rnd(c), 0.1 * rnd(c), 0.1 * rnd(c), 0.5 + torch.rand(c, generator=gen)]

    x = torch.relu(rnd(2, 64, 16, 16))
    for name, (co, ks, stride) in {"conv3x3s1": (64, 3, 1), "conv1x1s2": (128, 1, 2), "conv3x3s2": (128, 3, 2)}.items():
        y, ymax = emu_lib.conv_bn(emu, rnd(co, 64, ks, ks) * (2.0 / (64 * ks * ks)) ** 0.5, bn(co), stride, x)
        out[name], out[name + "_max"] = y, ymax
    for k, v in zip(("stem", "stem_pooled", "stem_nchw", "stem_max"), emu_lib.stem_pool(emu, rnd(64, 3, 7, 7) * 0.1, bn(64), rnd(1, 3, 16, 16))):
        out[k] = v

    def coarse(ncn, fa, fb, ksize):
        nb, c, ha, wa = fa.shape
        hb, wb = fb.shape[2:]
        shape = (nb, ha // ksize, wa // ksize, hb // ksize, wb // ksize)
        corr, delta = torch.empty(shape), torch.empty(shape, dtype=torch.uint8)
        n = nb * emu.p2p_coarse_workspace_bytes_for(ncn, c, ha, wa, hb, wb, ksize)
        ws = torch.empty(n + 256, dtype=torch.uint8)
        st = emu.p2p_coarse_forward_batch(emu_lib.ptr(fa), emu_lib.ptr(fb), nb, c, ha, wa, hb, wb, ksize, ncn, emu_lib.ptr(corr),
                                          emu_lib.ptr(delta), ctypes.c_void_p((ws.data_ptr() + 255) & ~255), n, None)
        assert st == 0, emu.p2p_last_error()
        return corr, delta

    fa, fb = nr.features(7, (1, 8, 8, 8, 8), channels=32)
    released = nr.weights("R")
    stacks = {"gen33": (released, nr.CASES["R"]),
              "gen53": (synthetic.make_ncn_state_dict(77, [5, 3], [8, 1], gain=2.0, bias=0.02, prefix=""),
                        dict(kernel_sizes=[5, 3], channels=[8, 1], symmetric_mode=False))}
    handles = {"tuned": emu_lib.ncn_create(emu, {"ncn." + k: v for k, v in released.items()})}
    for name, (sd, lay) in stacks.items():
        st, handles[name] = nr.create_config(emu, sd, lay)
        assert st == 0, emu.p2p_last_error()
    for name, h in handles.items():
        out["coarse_" + name], out["coarse_" + name + "_delta"] = coarse(h, fa, fb, 2)
        emu.p2p_ncn_destroy(h)

    sd = synthetic.make_state_dict(0, backbone=False)
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    p1, p2 = synthetic.make_pyramid(7, 32, 32), synthetic.make_pyramid(8, 32, 32)
    props = torch.tensor([[0, 0, 32, 32], [31, 17, 5, 20], [12, 30, 24, 9]])
    for mode in ("f32", "fp16x2", "fp16x2w"):
        pair = [emu_lib.regressor_create(emu, sub(p), mode) for p in ("regress_mid.", "regress_fine.")]
        for k, v in emu_lib.regress(emu, pair[0], pair[1], p1[:4], p2[:4], props).items():
            out[f"regress_{mode}_{k}"] = v
        for h in pair:
            emu.p2p_regressor_destroy(h)

    lay = dict(feat_idx=[0, 2], feat_comb="post", conv_dims=[32, 48], conv_kers=[3, 5], conv_strs=[2, 1], fc_dims=[64, 32])
    rc = synthetic.default_regressor_config(conv_dims=lay["conv_dims"], conv_kers=lay["conv_kers"], conv_strs=lay["conv_strs"],
                                            fc_dims=lay["fc_dims"], feat_comb="post", shared=False)
    gsd = synthetic.make_checkpoint(5, regressor_config=rc, feat_idx=lay["feat_idx"])["state_dict"]
    pair = []
    for prefix in ("regress_mid.", "regress_fine."):
        st, h = rr.create_config(emu, rr.sub_params(gsd, prefix), lay)
        assert st == 0, emu.p2p_last_error()
        pair.append(h)
    for k, v in rr.emu_regress(emu, pair[0], pair[1], p1, p2, props).items():
        out["regress_generic_" + k] = v
    for h in pair:
        emu.p2p_regressor_destroy(h)
    np.savez(out_file, **{k: v.numpy() for k, v in out.items()})


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(tmp, n + ".npz") for n in ("old", "new")]
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--dump", f, "--tree", os.path.abspath(t)])
                 for f, t in zip(files, (old, new))]
        if any(p.wait() for p in procs):
            sys.exit("a tree failed to run")
        a, b = (dict(np.load(f)) for f in files)
    ok = sorted(a) == sorted(b)
    for k in sorted(set(a) & set(b)):
        same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(np.frombuffer(a[k].tobytes(), np.uint8), np.frombuffer(b[k].tobytes(), np.uint8))
        print(f"{k:28s} {str(a[k].shape):18s} {a[k].nbytes:8d} bytes  {'identical' if same else 'DIFFERENT'}")
        ok &= same
    print("results identical" if ok else "RESULTS CHANGED")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--dump" and sys.argv[3] == "--tree":
        dump(sys.argv[4], sys.argv[2])
    elif len(sys.argv) in (2, 3):
        sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    else:
        sys.exit(__doc__)
