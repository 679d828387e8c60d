#!/usr/bin/env python3
"""Reduce the rocprofv3 kernel trace of launch_table_trace.py to what two builds that launch
alike must share.  Per plan, one line: the number of dispatches, a SHA-256 (first 32 hex digits)
over the dispatches in the order the host issued them -- kernel name with its template
arguments, grid size, workgroup size and queue (numbered by first use), one per line -- and the
count per kernel.  A plan's stretch runs from its first fill kernel to its last verify kernel.
With a second argument the sequences themselves are written there (a run of identical
dispatches as one line with its count), to diff when two builds' hashes part.
usage: launch_table_reduce.py <run_kernel_trace.csv> [full sequences file]"""
import collections
import csv
import hashlib
import itertools
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
queues, plans, verified = {}, [[]], False
for r in rows:
    name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("xgk::", "")
    if "fill_kernel" in name and verified:
        plans.append([])
        verified = False
    verified = verified or "verify_kernel" in name
    q = queues.setdefault(r["Queue_Id"], "q%d" % len(queues))
    plans[-1].append("%s grid %s wg %s %s" % (name, r["Grid_Size_X"], r["Workgroup_Size_X"], q))
full = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
for i, seq in enumerate(plans):
    names = collections.Counter(line.split(" grid ")[0] for line in seq)
    print("plan %2d: %4d dispatches %s  %s" % (
        i, len(seq), hashlib.sha256("\n".join(seq).encode()).hexdigest()[:32],
        ", ".join("%d %s" % (n, k) for k, n in sorted(names.items()))))
    if full:
        full.write("# plan %d\n" % i)
        for line, run in itertools.groupby(seq):
            n = len(list(run))
            full.write((line if n == 1 else "%d x %s" % (n, line)) + "\n")
