#!/usr/bin/env python3
"""Did a change of a HIP source move any instruction?  Compares, kernel by kernel, the device assembly of two builds of one source file:

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/sh23.hip -o commit.s        (and the same at the parent commit: parent.s)
    python tools/compare_kernel_bodies.py parent.s commit.s

A kernel's body is its instructions between its label and its end, comments dropped and the function number taken out of the local labels
(.LBB<n>_<m>: it changes when kernels are emitted in another order).  Prints how many kernels each file has, which are missing on either side
and which bodies differ, with the first differing lines of the first few; exit status 1 unless every body is equal.  No GPU needed.  A helper
function folded into several kernels can leave the LLVM IR with the same floating-point operations and still change which product of
a*b + c*d the backend rounds first, per kernel: equal bodies are the proof that results and speed are the parent's."""
import difflib
import re
import sys


def kernels(path, match):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\S+):", ln)
        if m:
            cur = m.group(1) if re.search(match, m.group(1)) else None
            if cur:
                out[cur] = []
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        if cur is not None:
            ln = re.sub(r";.*", "", re.sub(r"\.LBB\d+_", ".LBB_", ln)).rstrip()
            if ln.strip():
                out[cur].append(ln)
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    match = sys.argv[3] if len(sys.argv) > 3 else "."
    P, C = kernels(sys.argv[1], match), kernels(sys.argv[2], match)
    missing = sorted(set(P) ^ set(C))
    differ = [k for k in P if k in C and P[k] != C[k]]
    print("%d / %d kernels; on one side only: %d; bodies that differ: %d" % (len(P), len(C), len(missing), len(differ)))
    for k in missing[:10]:
        print("  one side only:", k)
    for k in differ[:5]:
        print("  differs:", k)
        for ln in list(difflib.unified_diff(P[k], C[k], lineterm="", n=0))[2:12]:
            print("    " + ln)
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main())
