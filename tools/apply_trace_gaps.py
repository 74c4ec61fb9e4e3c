#!/usr/bin/env python3
"""Where an apply batch's time goes, from a rocprofv3 --kernel-trace CSV of tools/bench_apply.py: per batch (the kernels
from the list scatter to k_apply_top) the span on the GPU, the time inside kernels and the gaps between them; per
kernel the launches per batch and the median duration.

  python tools/apply_trace_gaps.py <..._kernel_trace.csv>"""
import csv
import statistics
import sys


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    batches, cur = [], None
    for a, b, name in rows:
        if "k_apply_scatter" in name:
            cur = []
        if cur is not None and ("k_apply" in name):
            cur.append((a, b, name))
            if "k_apply_top" in name:
                batches.append(cur)
                cur = None
    if not batches:
        print("no apply batches in the trace")
        return 1
    span = [(b[-1][1] - b[0][0]) / 1e6 for b in batches]
    busy = [sum(e - s for s, e, _ in b) / 1e6 for b in batches]
    print(f"apply batches: {len(batches)}; launches per batch (scatter .. top): median {statistics.median(len(b) for b in batches)}")
    print(f"span ms: median {statistics.median(span):.3f}  in kernels: {statistics.median(busy):.3f}  "
          f"gaps: {statistics.median(s - k for s, k in zip(span, busy)):.3f}")
    kinds = {}
    for b in batches:
        for s, e, name in b:
            key = next(k for k in ("k_apply_scatter", "k_apply_level_coop", "k_apply_level", "k_apply_top") if k in name)
            kinds.setdefault(key, []).append((e - s) / 1e3)
    for k, v in kinds.items():
        print(f"  {k:<20} {len(v) / len(batches):6.1f} per batch   median {statistics.median(v):8.1f} us   max {max(v):8.1f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
