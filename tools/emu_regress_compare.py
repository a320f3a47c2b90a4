#!/usr/bin/env python3
"""Do two trees compute the same fine stage, bit for bit?  `python tools/emu_regress_compare.py OLD_TREE NEW_TREE`

Each tree's kernel sources are compiled for the host by its own tests/hipemu/build_emu.py and the regressor is run, in modes
fp16x2 and fp16x2w, on the inputs tests/test_kernels_emulated.py uses: the golden pair (integer proposals through the mid
regressor, float proposals through the fine one), mid -> fine with proposals on the image corners, an image size that is not
a multiple of 8, and device-side counts.  Every output array (matches, probabilities, raw) of one tree must equal the other
tree's byte for byte; exit status 1 otherwise.  The CPU half of the gate of a refactor of the fine-stage kernels whose device
assembly does not come out identical (tools/isa_diff.py); results: profiles/, see INDEX.md.  One process per tree: both
libraries export the same symbols."""
import os
import subprocess
import sys
import tempfile

import numpy as np


def dump(tree, out):
    for p in ("tests/hipemu", "tests", ""):
        sys.path.insert(0, os.path.join(tree, p))
    import ctypes
    import torch
    import emu_lib
    import golden_util as gu
    from patch2pix_amd import _lib as real
    from patch2pix_amd.utils import synthetic

    emu = emu_lib.load()
    sd = gu.state_dict(0)
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    res = {}

    def keep(tag, d, levels=2):
        for k, v in d.items():
            if int(k[-1]) <= levels:          # (one regressor: the second level's arrays are not written)
                res[f"{tag}/{k}"] = v.numpy().copy()

    for mode in ("fp16x2", "fp16x2w"):
        mid = emu_lib.regressor_create(emu, sub("regress_mid."), mode)
        fine = emu_lib.regressor_create(emu, sub("regress_fine."), mode)
        g = gu.load("fine_48x64")
        p1, p2 = gu.fine_inputs(g)
        for tag, reg in (("int_mid", mid), ("float_fine", fine)):
            keep(f"{mode}/golden_{tag}", emu_lib.regress(emu, reg, None, p1[:4], p2[:4], torch.from_numpy(g[tag + "_in"][:4])), 1)
        H, W = 48, 64
        p1, p2 = synthetic.make_pyramid(7, H, W), synthetic.make_pyramid(8, H, W)
        keep(f"{mode}/borders", emu_lib.regress(emu, mid, fine, p1[:4], p2[:4], torch.tensor([[0, 0, W, H], [W, H, 0, 0], [31, 17, 5, 40]])))
        H, W = 27, 37
        gen = torch.Generator().manual_seed(3)
        up = lambda d, j: (d + (1 << j) - 1) >> j
        pyr = lambda: [torch.randn(3, H, W, generator=gen)] + [torch.relu(torch.randn(c, up(H, j), up(W, j), generator=gen) + 0.3)
                                                               for c, j in ((64, 1), (64, 2), (128, 3))]
        p1, p2 = pyr(), pyr()
        keep(f"{mode}/odd_size", emu_lib.regress(emu, mid, None, p1, p2, torch.tensor([[W, H, 0, 0], [W - 1, H - 1, 3, 5], [18, 13, 30, 20], [0, H, W, 0]])), 1)
        # device counts: every item owns `stride` slots, the first counts[i] hold proposals
        sizes, stride, counts = [(16, 24), (24, 16), (8, 8)], 3, [2, -1 if mode == "fp16x2w" else 0, 1]
        gen = torch.Generator().manual_seed(4)
        props = torch.zeros(len(sizes), stride, 4, dtype=torch.int64)
        for i, ((h, w), c) in enumerate(zip(sizes, counts)):
            c = max(c, 0)
            props[i, :c] = torch.stack([torch.randint(0, w + 1, (c,), generator=gen), torch.randint(0, h + 1, (c,), generator=gen),
                                        torch.randint(0, w + 1, (c,), generator=gen), torch.randint(0, h + 1, (c,), generator=gen)], 1)
        arr_a, arr_b, alive = (real.Pyramid * len(sizes))(), (real.Pyramid * len(sizes))(), []
        for i, (h, w) in enumerate(sizes):
            for arr, seed in ((arr_a, 200 + i), (arr_b, 300 + i)):
                lv = [t.contiguous() for t in synthetic.make_pyramid(seed, h, w)[:4]]
                alive.append(lv)
                for j in range(4):
                    arr[i].level[j] = lv[j].data_ptr()
                arr[i].height, arr[i].width = lv[0].shape[-2:]
        n = len(sizes) * stride
        o = {k: torch.full((n, c) if c > 1 else (n,), -777.0) for k, c in (("matches1", 4), ("probs1", 1), ("matches2", 4), ("probs2", 1))}
        cnt = torch.tensor(counts, dtype=torch.int32)
        ws, wsp, wsn = emu_lib.regress_scratch(emu, n)
        emu_lib.check(emu, emu.p2p_regress_batch_dev(mid, fine, len(sizes), arr_a, arr_b, cnt.data_ptr(), stride, props.data_ptr(), 0,
                                                     o["matches1"].data_ptr(), o["probs1"].data_ptr(), None, o["matches2"].data_ptr(),
                                                     o["probs2"].data_ptr(), None, wsp, wsn, None), "p2p_regress_batch_dev")
        keep(f"{mode}/dev_counts", o)
    np.savez(out, **res)


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        outs = []
        for i, tree in enumerate((old, new)):
            outs.append(os.path.join(tmp, f"{i}.npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", os.path.abspath(tree), outs[-1]], check=True,
                           cwd=tree)
        a, b = np.load(outs[0]), np.load(outs[1])
        bad = sorted(set(a.files) ^ set(b.files))
        for k in sorted(set(a.files) & set(b.files)):
            same = a[k].tobytes() == b[k].tobytes()
            print(f"{k:40s} {str(a[k].shape):10s} {'byte-equal' if same else 'DIFFERENT'}")
            if not same:
                bad.append(k)
    print("fine stage byte-equal" if not bad else f"FINE STAGE CHANGED: {' '.join(bad)}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 3:
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
