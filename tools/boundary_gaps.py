#!/usr/bin/env python3
"""Idle time between dependent kernels, from a rocprofv3 --kernel-trace CSV:  tools/boundary_gaps.py <..._kernel_trace.csv> [min launches]

For every pair of consecutive dispatches of one queue, gap = begin(k+1) - end(k).  The pairs are grouped by (kernel k, kernel k+1); groups
with fewer than `min launches` (default 100) members — setup, the terminal condition, the gradient output — are left out, so what remains
is the steady time loop.  Prints one line per group (count, p10 / median / p90 / mean gap in us, mean duration of kernel k in us) and the
totals: gap time and kernel time of the listed pairs.  (A tuning aid: DESIGN.md section 5 quotes what was measured with it.)
"""
import csv
import re
import sys
from collections import defaultdict


def short(name):
    m = re.search(r"(kd\w*|kda\w*)<([^>]*)>", name)
    if not m:
        return re.sub(r"\(.*", "", name).split("::")[-1][:40]
    return "%s<%s>" % (m.group(1), m.group(2).replace(" ", ""))


def pct(v, q):
    return v[min(len(v) - 1, int(q * len(v)))]


def main():
    path = sys.argv[1]
    min_n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    per_queue = defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            per_queue[(r.get("Agent_Id"), r.get("Queue_Id"))].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    gaps, durs = defaultdict(list), defaultdict(list)
    for rows in per_queue.values():
        rows.sort()
        for (b0, e0, k0), (b1, e1, k1) in zip(rows, rows[1:]):
            gaps[(k0, k1)].append((b1 - e0) * 1e-3)
            durs[(k0, k1)].append((e0 - b0) * 1e-3)
    tot_gap = tot_dur = 0.0
    n_all = 0
    print("%-46s -> %-46s %7s %7s %7s %7s %7s %9s" % ("kernel k", "kernel k+1", "count", "p10", "median", "p90", "mean", "dur(k)"))
    for key in sorted(gaps, key=lambda k: -len(gaps[k])):
        v = sorted(gaps[key])
        if len(v) < min_n:
            continue
        mean = sum(v) / len(v)
        dmean = sum(durs[key]) / len(v)
        tot_gap += sum(v); tot_dur += sum(durs[key]); n_all += len(v)
        print("%-46s -> %-46s %7d %7.2f %7.2f %7.2f %7.2f %9.2f" % (key[0], key[1], len(v), pct(v, 0.1), pct(v, 0.5), pct(v, 0.9), mean, dmean))
    if n_all:
        print("listed boundaries: %d   gap time %.3f ms   kernel time %.3f ms   gaps / (gaps + kernels) = %.2f %%   mean gap %.2f us"
              % (n_all, tot_gap * 1e-3, tot_dur * 1e-3, 100.0 * tot_gap / (tot_gap + tot_dur), tot_gap / n_all))


if __name__ == "__main__":
    main()
