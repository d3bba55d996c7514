#!/bin/bash
# Developer helper (GPU box): everything profiles/ is built from.  Usage: tools/gpu_profiles.sh r05 [eval-only]
# Every GPU step runs under a time limit of its own; the first step that fails, aborts or runs out of time ends the script.
set -o pipefail
TAG=${1:-r05}
ONLY=${2:-all}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/profile_out}      # what tools/summarize_profiles.py reads (its OUT)
mkdir -p $OUT
exec 3>&1
stop() { echo "stopped at $1 (exit status $2)" >&3; exit "$2"; }
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --steps 400 --warmup 50 --full --no-cpu-baseline --no-kernel-timing --no-extras"
prof() {   # prof <dir> <command...>: rocprofv3 kernel stats of one command -> $OUT/<dir>/<TAG>_kernel_stats.csv
  local d=$1; shift
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$d -o $TAG -- "$@" > $OUT/$d.log 2>&1 || stop $d $?
  cut -d, -f1-4 $OUT/$d/${TAG}_kernel_stats.csv | head -5
}
prof prof_eager $CMD
# the two-launch form of the same evaluation (BXI_EVAL_TWO_LAUNCHES = 2: what larger instance counts, dilation 3 / 4
# and the head-fused call run); the shape real training runs, 128 and 64 instances (default form);
# the targets-ahead pair (bxi_boxinst_targets_f32 + BXI_EVAL_TARGETS_READY) at 32 and 128 instances
prof prof_two_launch $CMD --flags 2
prof prof_n128 $CMD --inst-per-box 4 --sets 6
prof prof_n64 $CMD --inst-per-box 2 --sets 6
prof prof_targets_n32 python $R/tools/ab_forms.py --ipb 1 --forms ready,targets_only --reps 1 --steps 300 --sets 6
prof prof_targets_n128 python $R/tools/ab_forms.py --ipb 4 --forms ready,targets_only --reps 1 --steps 300 --sets 6
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -o $TAG -- \
     python $R/bench.py --steps 100 --warmup 20 --full --no-cpu-baseline --no-kernel-timing --no-extras > $OUT/pmc_$c.log 2>&1 || stop pmc_$c $?
  ls $OUT/pmc_$c | head -3
done
for t in pairwise_op dynamic_head head_fused discobox levelset tree_filter; do
  [ "$ONLY" = eval-only ] && break
  # kernel durations under the profiler; the wall-clock JSON from a run WITHOUT it (a row of ~200 tiny launches is twice as slow under rocprofv3)
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$t -o $TAG -- python $R/tools/bench_$t.py > /dev/null 2> $OUT/${t}_bench.err || stop prof_$t $?
  timeout -k 10 300 python $R/tools/bench_$t.py > $OUT/${t}_bench.json 2>> $OUT/${t}_bench.err || stop bench_$t $?
  tail -c 300 $OUT/${t}_bench.json | tr '\n' ' '; echo
done
cd $R
# the per-wave trace needs the -DBXI_TRACE build of the library (tools/trace_forms.py's docstring); it is not kept in the tree
if [ -f boxinstseg_amd/lib/libboxinst_hip_trace.so ]; then
  (timeout -k 10 300 python tools/trace_forms.py && IPB=4 timeout -k 10 300 python tools/trace_forms.py &&
   IPB=4 BXI_FLAGS=34 timeout -k 10 300 python tools/trace_forms.py) 2>&1 | grep -v amdgpu.ids > $OUT/block_trace.txt || stop block_trace $?
  tail -3 $OUT/block_trace.txt | cut -c1-300
else
  rm -f $OUT/block_trace.txt; echo "no trace build: block trace skipped"
fi
timeout -k 10 600 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || stop bench_default $?
tail -c 600 $OUT/bench_default.json
