#!/bin/bash
# The bench's large copy launches in small pieces (copy_kernel_q, one table row per copy) against
# the 32 KiB pieces of copy_kernel_g<4, true>.  Every mode runs bench.py arms ALTERNATED in one
# session on one box, five runs each, and reduces them with profiles/small_pieces_summary.py.
#   gate   on any build: bench.py --chunk 4096 | --chunk 16384 | default (copy_kernel_g at those
#          piece sizes), then rocprofv3 --kernel-trace --stats of --chunk 4096 and of the default,
#          kernel time per position in the step                       -> gate.txt
#   ab     PARENT=<built checkout of the parent commit>: the parent's bench.py against this build's
#          under each "NAME:ENV=VAL,ENV=VAL" arm of ARMS (default: the build as it stands);
#          BENCH_ARGS: arguments for every bench.py run (e.g. --size, for the launch-size sweep)
#                                                                     -> ab.txt
#   trace  rocprofv3 --kernel-trace --stats of this build's bench.py  -> kernel_stats.csv, trace.txt
#   pmc    FETCH_SIZE and WRITE_SIZE passes (separate runs, no tracing) -> pmc.txt, pmc_traffic.json
# usage: [PARENT=dir] [ARMS="..."] profiles/small_pieces_ab.sh gate|ab|trace|pmc [outdir]
# (run from the root of a built checkout)
set -o pipefail
what=${1:?gate, ab, trace or pmc}; root=$PWD; out=${2:-$root/profiles/r10/small_pieces}; mkdir -p $out
export TMPDIR=/tmp
tmp=$(mktemp -d)

# one bench.py run in tree $1 with environment assignments $2 (comma-separated) and arguments $3..:
# "GB/s  ms per step  us per launch" appended to $out/$arm.runs
bench() {
  local tree=$1 envs=$2; shift 2
  ( cd $tree && env $(echo $envs | tr , ' ') timeout -k 10 150 python3 bench.py ${BENCH_ARGS:-} "$@" > $tmp/bench.json 2> $tmp/bench.err ) ||
    { tail -5 $tmp/bench.err; return 1; }
  python3 -c 'import json, sys; r = json.load(open(sys.argv[1])); print(r["value"], r["ms_per_step"], r["roofline"]["avg_launch_us"])' \
    $tmp/bench.json >> $tmp/$arm.runs && tail -1 $tmp/$arm.runs | sed "s/^/$arm: /"
}

# rocprofv3 --kernel-trace --stats of one bench.py run -> per-position kernel times (stdout), $out/$1_kernel_stats.csv
trace() {
  local tag=$1; shift
  timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $tmp/kt_$tag -o run --output-format csv -- \
    python3 bench.py ${BENCH_ARGS:-} "$@" > $tmp/trace.json 2> $tmp/trace.err || { tail -5 $tmp/trace.err; return 1; }
  cp $(find $tmp/kt_$tag -name run_kernel_stats.csv | head -1) $out/${tag}_kernel_stats.csv
  python3 profiles/small_pieces_summary.py trace $(find $tmp/kt_$tag -name run_kernel_trace.csv | head -1)
}

case $what in
gate)
  for i in 1 2 3 4 5; do
    arm=chunk_default; bench $root "" || exit 1
    arm=chunk_4096; bench $root "" --chunk 4096 || exit 1
    arm=chunk_16384; bench $root "" --chunk 16384 || exit 1
  done
  { echo "# profiles/small_pieces_ab.sh gate: bench.py [--chunk N], arms alternated, one box"
    python3 profiles/small_pieces_summary.py runs $tmp/chunk_default.runs $tmp/chunk_4096.runs $tmp/chunk_16384.runs
    echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py (default pieces)"
    trace gate_default || exit 1
    echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --chunk 4096"
    trace gate_4096 --chunk 4096 || exit 1
  } | tee $out/gate.txt ;;
ab)
  parent=$(cd ${PARENT:?a built checkout of the parent commit} && pwd) || exit 1
  arms=${ARMS:-this:}
  for i in 1 2 3 4 5; do
    arm=parent; bench $parent "" || exit 1
    for a in $arms; do arm=${a%%:*}; bench $root "${a#*:}" || exit 1; done
  done
  { echo "# profiles/small_pieces_ab.sh ab: parent's bench.py against this build's, arms: $arms"
    python3 profiles/small_pieces_summary.py runs $tmp/parent.runs $(for a in $arms; do echo $tmp/${a%%:*}.runs; done)
  } | tee $out/ab.txt ;;
trace)
  { echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py (this build)"
    trace this || exit 1
  } | tee $out/trace.txt
  mv $out/this_kernel_stats.csv $out/kernel_stats.csv ;;
pmc)
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 150 rocprofv3 --pmc $c -d $tmp/$c -o run --output-format csv -- \
      python3 bench.py --steps 5 --warmup 1 > /dev/null 2> $tmp/pmc.err || { tail -5 $tmp/pmc.err; exit 1; }
  done
  f=$(find $tmp/FETCH_SIZE -name run_counter_collection.csv | head -1); w=$(find $tmp/WRITE_SIZE -name run_counter_collection.csv | head -1)
  python3 profiles/pmc_summary.py $(dirname $f) $(dirname $w) $out/pmc_traffic.json \
    "r10: bench.py --steps 5 --warmup 1 (rocprofv3 --pmc, separate passes)" > $tmp/pmc.json || exit 1
  python3 -c 'import json, sys
r = json.load(open(sys.argv[1]))
for k, v in r["kernels"].items():
    if "copy_kernel" in k:
        print("%s: read %.2f MB + write %.2f MB = %.2f MB per launch" % (k.split("(")[0], v["hbm_read_bytes"] / 1e6, v["hbm_write_bytes"] / 1e6, v["hbm_bytes"] / 1e6))' \
    $out/pmc_traffic.json | tee $out/pmc.txt ;;
*) echo "unknown mode $what"; exit 2 ;;
esac
rc=$?
rm -rf $tmp
exit $rc
