#!/usr/bin/env python3
"""Compares the device code of two builds of csrc/wbcqp_api.hip, kernel by kernel.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -ffp-contract=on --cuda-device-only -S inria_wbc_amd/csrc/wbcqp_api.hip -o a.s
    python tools/device_asm_diff.py parent.s branch.s

The compilation-unit id (__hip_cuid_<hash of the source text>) is masked.  Prints the sha256 of both masked files, whether they are
identical as a whole, and -- the fallback where only the order of the instantiations moved -- the set of kernel symbols and every
kernel's body (from its `<symbol>: ; @<symbol>` label to its .Lfunc_end) compared by symbol.  Exit status 0: same device code.
"""
import hashlib
import re
import sys


def load(path):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())


def kernels(text):
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S):
        # local labels carry the function's position in the file (.LBB6_355, "Header=BB6_4", .LJTI6_0, .Lfunc_end6): that number is dropped
        # (and with it the column at which a label's trailing comment starts)
        body = re.sub(r"(BB|JTI|CPI)\d+_", r"\1_", m.group(2))
        body = re.sub(r"[ \t]+;", " ;", body)
        body = re.sub(r"func_(end|begin)\d+", r"func_\1", body)
        out[m.group(1)] = hashlib.sha256(body.encode()).hexdigest()
    return out


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    sa, sb = hashlib.sha256(a.encode()).hexdigest(), hashlib.sha256(b.encode()).hexdigest()
    print("masked sha256  %s  %s" % (sa, sys.argv[1]))
    print("masked sha256  %s  %s" % (sb, sys.argv[2]))
    print("whole files identical: %s" % (sa == sb))
    ka, kb = kernels(a), kernels(b)
    print("functions: %d and %d, same set of symbols: %s" % (len(ka), len(kb), set(ka) == set(kb)))
    bad = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
    for k in sorted(ka):
        print("%s  %s  %s" % ("same" if k not in bad else "DIFF", ka[k][:16], k))
    for k in bad:
        print("DIFFERS or missing on one side: %s" % k)
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())
