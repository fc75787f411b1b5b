#!/usr/bin/env python3
"""Per-kernel comparison of two sets of device assembly files (hipcc --cuda-device-only -S).

usage: isa_diff.py BASE_DIR NEW_DIR
Every *.s under each directory is read; kernels are matched by mangled name, whichever file they live in,
so a kernel that moved to another translation unit is compared with itself.  Comment and directive lines
are ignored, and so is the ordinal of the function inside its file that local labels carry (.LBB<ordinal>_<block>):
it changes when a kernel moves, the block numbers do not.  Exit status 0 only when both sides hold the same kernel names and every instruction stream
is identical; otherwise the differing / missing / duplicated names are listed.
"""
import collections
import glob
import os
import re
import sys


LOCAL_LABEL = re.compile(r"\.L([A-Za-z]+)\d+_(\d+)")


def kernels(d):
    out, dup = {}, []
    for fn in sorted(glob.glob(os.path.join(d, "*.s"))):
        cur = None
        names = set(re.findall(r"^\s+\.amdhsa_kernel\s+(\S+)", open(fn).read(), re.M))
        for ln in open(fn):
            m = re.match(r"^(_Z\w+):", ln)
            if m:
                cur = m.group(1) if m.group(1) in names else None
                if cur:
                    if cur in out:
                        dup.append(cur)
                    out[cur] = []
                continue
            if ln.startswith(".Lfunc_end"):
                cur = None
            if cur and not ln.lstrip().startswith((";", ".")):
                out[cur].append(LOCAL_LABEL.sub(r".L\1_\2", ln.split(";")[0].strip()))
    return out, dup


def main():
    a, da = kernels(sys.argv[1])
    b, db = kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) - set(b)):
        print("ONLY IN BASE", k); bad += 1
    for k in sorted(set(b) - set(a)):
        print("ONLY IN NEW ", k); bad += 1
    for k in da + db:
        print("DUPLICATE   ", k); bad += 1
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            same_mix = collections.Counter(x.split()[0] for x in a[k] if x) == collections.Counter(x.split()[0] for x in b[k] if x)
            print("DIFFERS     ", k, len(a[k]), "->", len(b[k]), "(same opcode mix)" if same_mix else "")
            bad += 1
    print(f"{len(a)} kernels in base, {len(b)} in new, {bad} findings")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
