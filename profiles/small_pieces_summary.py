#!/usr/bin/env python3
"""Reducers of profiles/small_pieces_ab.sh.

  runs  <file>...                 each file holds one line per bench.py run of one arm ("value GB/s,
                                  ms per step, average launch us"): every run, the median and the
                                  min-max spread per arm, and CHOICE_RULE (bench.py) between the first
                                  file's arm and each of the others
  trace <run_kernel_trace.csv>    the copy launches of one bench.py process in start order; launch i sits
                                  at position i % 4 of its step (one launch per method, methods 1-4;
                                  the four verified runs in front keep the order): mean / median / p10 /
                                  p90 kernel time per position over the last `steps` steps
"""
import csv
import os
import statistics
import sys


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def runs(files):
    arms = {}
    for f in files:
        name = os.path.basename(f).rsplit(".", 1)[0]
        rows = [tuple(float(x) for x in line.split()[:3]) for line in open(f) if line.strip()]
        arms[name] = rows
        for i, r in enumerate(rows):
            print("%-16s run %d: %8.2f GB/s  %.4f ms per step  %.2f us per launch" % ((name, i + 1) + r))
    st = {}
    for name, rows in arms.items():
        ms = [r[1] for r in rows]
        st[name] = (statistics.median(ms), min(ms), max(ms))
        print("%-16s median %.4f ms per step (min %.4f max %.4f, spread %.4f), median %.2f GB/s"
              % (name, st[name][0], st[name][1], st[name][2], st[name][2] - st[name][1],
                 statistics.median(r[0] for r in rows)))
    base = os.path.basename(files[0]).rsplit(".", 1)[0]
    bm, blo, bhi = st[base]
    for name, (m, lo, hi) in st.items():
        if name == base:
            continue
        need = max(bhi - blo, hi - lo)
        print("%s vs %s: median %+.4f ms (%+.2f %%), larger spread %.4f ms -> %s"
              % (name, base, m - bm, (m - bm) / bm * 100, need,
                 "wins by the rule" if bm - m > need else "does not win by the rule"))


def trace(path, steps=50):
    rows = [r for r in csv.DictReader(open(path)) if "copy_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-4 * steps:] if len(rows) >= 4 * steps else rows[len(rows) % 4:]
    name = rows[0]["Kernel_Name"].split("(")[0].replace("void ", "").replace("xgk::", "")
    print("%d launches of %s, grid %s" % (len(rows), name, rows[0]["Grid_Size_X"]))
    tot = 0.0
    for p in range(4):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[p::4]]
        tot += statistics.mean(us)
        print("position %d: mean %.2f us  median %.2f  p10 %.2f  p90 %.2f  (%d launches)"
              % (p + 1, statistics.mean(us), statistics.median(us), pct(us, 0.1), pct(us, 0.9), len(us)))
    gaps = [(int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) / 1e3 for a, b in zip(rows, rows[1:])]
    print("sum of the four means %.2f us per step; gap between launches: mean %.2f us" % (tot, statistics.mean(gaps)))


if __name__ == "__main__":
    {"runs": runs, "trace": lambda a: trace(a[0])}[sys.argv[1]](sys.argv[2:])
