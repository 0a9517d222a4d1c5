#!/usr/bin/env python3
"""Are a kernel's instructions the same in two builds?

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -ffp-contract=on --cuda-device-only -S inria_wbc_amd/csrc/wbcqp_api.hip -o this.s
    (the same on a checkout of the other commit -> other.s)
    python tools/kernel_asm_diff.py other.s this.s observe_kernel [-v]

Compares, for every function of the two device assemblies whose mangled name contains the given text, the instructions and labels (comments,
.loc / .file / .cfi lines and blank lines dropped) and prints one line per function: IDENTICAL, or the number of unified-diff lines (-v: the
diff's head).  profiles/collision/observe_kernel_vs_parent.txt is its output for observe_kernel against the parent commit."""
import difflib
import re
import sys


def kernels(path, want):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s*;\s*@", ln)
        if m:
            cur = m.group(1) if want in m.group(1) else None
            if cur:
                out[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = ln.split(";")[0].rstrip()
        if s.strip() and not s.strip().startswith((".loc", ".file", ".cfi")):
            out[cur].append(s)
    return out


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1], sys.argv[3]), kernels(sys.argv[2], sys.argv[3])
    same = True
    for k in sorted(set(a) | set(b)):
        d = list(difflib.unified_diff(a.get(k, []), b.get(k, []), "other " + k, "this " + k, lineterm="", n=1))
        same = same and not d
        print(k, len(a.get(k, [])), "->", len(b.get(k, [])), "lines;", "IDENTICAL" if not d else "%d diff lines" % len(d))
        if d and "-v" in sys.argv:
            print("\n".join(d[:80]))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
