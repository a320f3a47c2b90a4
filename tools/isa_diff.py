#!/usr/bin/env python3
"""Is the gfx950 device code of two trees the same?  `python tools/isa_diff.py OLD_TREE NEW_TREE`

Every translation unit (SOURCES of patch2pix_amd/build.py) of both trees is compiled to device assembly (hipcc
--cuda-device-only -S, the flags of build.py) and compared line by line, without the lines that name `__hip_cuid_`: that
symbol is a hash of the source text, the one thing that differs when only host code or comments changed.  A .hip file that
is no unit is part of the units that include it (alone it need not compile) and is only listed.  One verdict per file, and
for a file that differs one per kernel: its code from its label to the end of the function and its .amdhsa_kernel block,
without comments and with the function numbers in local labels removed (they count the functions in front of it).  Text
is compared, nothing is looked for in it.  Exit status 1 unless every unit both trees have is identical and a unit only one
of them has holds no kernel.  The gate of a refactor that claims to leave the kernels alone (results: profiles/, see INDEX.md)."""
import ast
import os
import re
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


def kernel_text(asm, name):
    """The lines of one kernel: function body and kernel descriptor, local labels without their function number."""
    def part(first, last):
        lines = asm[next(i for i, l in enumerate(asm) if l.lstrip().startswith(first)):]
        return lines[:next(i for i, l in enumerate(lines) if l.lstrip().startswith(last)) + 1]
    body, desc = part(name + ":", ".Lfunc_end"), part(".amdhsa_kernel " + name, ".end_amdhsa_kernel")
    lines = [re.sub(r"\.L(BB|func_end)\d+", r".L\1", l.split(";")[0].rstrip()) for l in body + desc]      # (";": a comment)
    return [l for l in lines if l]


def units(tree):
    """SOURCES of the tree's build.py."""
    text = open(os.path.join(tree, "patch2pix_amd", "build.py")).read()
    return set(ast.literal_eval(re.search(r"^SOURCES = (\[.*?\])", text, re.M | re.S).group(1)))


def main(old, new):
    csrc = [os.path.join(t, "patch2pix_amd", "csrc") for t in (old, new)]
    files = [set(f for f in os.listdir(c) if f.endswith(".hip")) for c in csrc]
    names = [fs & units(t) for fs, t in zip(files, (old, new))]
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
            if a != b:
                ka, kb = kernels(a), kernels(b)
                for k in sorted(set(ka) | set(kb)):
                    if k in ka and k in kb:
                        ta, tb = kernel_text(a, k), kernel_text(b, k)
                        print(f"    {k}: {'identical' if ta == tb else f'DIFFERENT ({len(ta)} -> {len(tb)} lines)'}")
                    else:
                        print(f"    {k}: only in the {'old' if k in ka else 'new'} tree")
        else:
            side = 0 if f in names[0] else 1
            k = kernels(asm[(f, csrc[side])])
            print(f"{f:20s} only in the {'old' if side == 0 else 'new'} tree, {len(k)} kernels {'' if not k else 'MOVED OR NEW: ' + ' '.join(k)}")
            ok &= not k
    for side, (fs, us) in enumerate(zip(files, names)):
        if fs - us:
            print(f"no units of the {'old' if side == 0 else 'new'} tree (compiled with the units that include them): {' '.join(sorted(fs - us))}")
    print("device code identical" if ok else "DEVICE CODE CHANGED")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
