#!/usr/bin/env python3
"""Medians and min-max of launch_table_ab.sh's runs, the parent's build beside this one: bench.py's
GB/s and the CLI's max total time per method, every run listed (parent | this).  usage: launch_table_ab_summary.py <outdir>"""
import csv
import os
import statistics as S
import sys

out = sys.argv[1]
print("bench.py (configs[1], one MI355X), GB/s, 5 runs each, the builds alternated in one session")
for b in ("parent", "this"):
    v = [float(line.split()[0]) for line in open(os.path.join(out, "bench_%s.txt" % b))]
    print("  %-6s median %.2f  min %.2f  max %.2f  runs %s" % (b, S.median(v), min(v), max(v), v))
print()
print("bin/test --procs 32 -a 14 -d 2048 -c 3 -m 0 -i 2 -k 1: max total time per method in us (the report")
print("prints whole us), 5 runs of 2 iterations each")
rows = {}
for b in ("parent", "this"):
    for r in csv.reader(open(os.path.join(out, "cli_%s.csv" % b))):
        if r[1] != "Method":
            rows.setdefault(r[1], {}).setdefault(b, []).append(round(float(r[-1]) * 1e6))
print("  %-30s %-20s %-20s %s" % ("method", "parent med (min-max)", "this med (min-max)", "this inside the parent's spread or better"))
outside = 0
for m, d in rows.items():
    p, t = d["parent"], d["this"]
    ok = max(t) <= max(p)
    outside += not ok
    f = lambda v: "%g (%d-%d)" % (S.median(v), min(v), max(v))  # noqa: E731
    print("  %-30s %-20s %-20s %-3s  runs %s | %s" % (m, f(p), f(t), "yes" if ok else "NO", " ".join(map(str, p)), " ".join(map(str, t))))
print("methods with a run of this build slower than the parent's slowest: %d of %d" % (outside, len(rows)))
