#!/usr/bin/env python3
"""Is the gfx950 device code of two trees the same?  `python tools/isa_diff.py OLD_TREE NEW_TREE`

Every patch2pix_amd/csrc/*.hip of both trees is compiled to device assembly (hipcc --cuda-device-only -S, the flags of
patch2pix_amd/build.py) and compared line by line, without the lines that name `__hip_cuid_`: that symbol is a hash of the
source text, the one thing that differs when only host code or comments changed.  One verdict per file; exit status 1
unless every file both trees have is identical and every file only one of them has holds no kernel.  The gate of a
refactor that claims to leave the kernels alone (results: profiles/, see INDEX.md)."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def device_asm(path):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", path, "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def kernels(asm):
    return sorted(l.split()[1] for l in asm if l.lstrip().startswith(".amdhsa_kernel "))


def main(old, new):
    csrc = [os.path.join(t, "patch2pix_amd", "csrc") for t in (old, new)]
    names = [set(f for f in os.listdir(c) if f.endswith(".hip")) for c in csrc]
    jobs = [(f, c) for c, fs in zip(csrc, names) for f in sorted(fs)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        asm = dict(zip(jobs, ex.map(lambda j: device_asm(os.path.join(j[1], j[0])), jobs)))
    ok = True
    for f in sorted(names[0] | names[1]):
        if f in names[0] and f in names[1]:
            a, b = asm[(f, csrc[0])], asm[(f, csrc[1])]
            differ = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            verdict = "identical" if a == b else f"DIFFERENT ({differ} of {max(len(a), len(b))} lines)"
            print(f"{f:20s} {len(kernels(b)):2d} kernels, {len(b):6d} lines  {verdict}")
            ok &= a == b
        else:
            side = 0 if f in names[0] else 1
            k = kernels(asm[(f, csrc[side])])
            print(f"{f:20s} only in the {'old' if side == 0 else 'new'} tree, {len(k)} kernels {'' if not k else 'MOVED OR NEW: ' + ' '.join(k)}")
            ok &= not k
    print("device code identical" if ok else "DEVICE CODE CHANGED")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
