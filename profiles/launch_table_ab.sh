#!/bin/bash
# The launch table (host/plan_tables.cc: TableBuilder) against the commit before it.
#   trace: profiles/launch_table_trace.py under rocprofv3 --kernel-trace, one fresh process per
#          build, reduced by launch_table_reduce.py to one line per plan (a hash of its ordered
#          dispatches) and diffed; the sequences themselves (*.full.txt) stay only if they differ
#   ab:    bench.py and the README configuration through bin/test, five times each, the two
#          builds alternated in one session; launch_table_ab_summary.py reports medians and spreads
# usage: PARENT=<built checkout of the parent commit> profiles/launch_table_ab.sh trace|ab [outdir]
# (run from the root of this built checkout)
set -o pipefail
what=${1:?trace or ab}; root=$PWD; out=${2:-$root/profiles/r08/launch_table}; mkdir -p $out
parent=$(cd ${PARENT:?a built checkout of the parent commit} && pwd) || exit 1
export TMPDIR=/tmp
if [ $what = trace ]; then
  for b in parent this; do
    tree=$root; [ $b = parent ] && tree=$parent
    XG_TREE=$tree timeout -k 10 240 rocprofv3 --kernel-trace -d $out/$b.rocprof -o run --output-format csv -- \
      python3 profiles/launch_table_trace.py > $out/$b.out.txt 2>&1 || { tail -5 $out/$b.out.txt; exit 1; }
    python3 profiles/launch_table_reduce.py $(find $out/$b.rocprof -name run_kernel_trace.csv | head -1) \
      $out/$b.full.txt > $out/$b.trace.txt || exit 1
    rm -rf $out/$b.rocprof
  done
  grep "^plan" $out/this.out.txt > $out/plans.txt; rm -f $out/parent.out.txt $out/this.out.txt
  diff $out/parent.trace.txt $out/this.trace.txt > $out/trace.diff && cmp -s $out/parent.full.txt $out/this.full.txt &&
    rm -f $out/parent.full.txt $out/this.full.txt
  echo "diff: $(wc -l < $out/trace.diff) lines"
  exit 0
fi
rm -f $out/bench_parent.txt $out/bench_this.txt $out/cli_parent.csv $out/cli_this.csv
tmp=$(mktemp -d)
for i in 1 2 3 4 5; do
  for b in parent this; do
    tree=$root; [ $b = parent ] && tree=$parent
    cd $tree || exit 1
    timeout -k 10 150 python3 bench.py > $tmp/bench.json 2> $tmp/bench.err || { tail -5 $tmp/bench.err; exit 1; }
    python3 -c 'import json, sys; r = json.load(open(sys.argv[1])); print(r["value"], "GB/s", r["ms_per_step"], "ms per step")' \
      $tmp/bench.json >> $out/bench_$b.txt || exit 1
    cd $tmp || exit 1
    timeout -k 10 100 $tree/mpi-asynchronous-communication-test_amd/bin/test --procs 32 -a 14 -d 2048 -c 3 -m 0 -i 2 -k 1 \
      > report.txt 2> err.txt || { tail -5 err.txt; exit 1; }
    sed "s/^/run $i,/" results.csv | cut -d, -f1,2,16 >> $out/cli_$b.csv     # run, method, max total time
  done
done
cd $root && rm -rf $tmp && python3 profiles/launch_table_ab_summary.py $out | tee $out/summary.txt &&
  rm -f $out/bench_parent.txt $out/bench_this.txt $out/cli_parent.csv $out/cli_this.csv     # every run is in summary.txt
