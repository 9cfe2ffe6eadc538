#!/bin/bash
# bench (the --full line) + rocprofv3 kernel stats on a GPU box; results under $OUT (default: bench_out/)
#   bash tools/gpu_bench.sh [steps] [prof|noprof]
R=$(pwd); O=$(realpath -m "${OUT:-bench_out}")
mkdir -p $O
export PYTHONDONTWRITEBYTECODE=1
python bench.py --gpus 1 --steps ${1:-10} --warmup 3 --full > $O/bench.json 2> $O/bench.err
echo "bench exit $?"; cat $O/bench.json; tail -5 $O/bench.err
if [ "${2:-prof}" = "prof" ]; then
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python $R/bench.py --gpus 1 --steps 5 --warmup 2 --full --no-cpu-baseline --no-profile --no-fp32-parity --no-dense-rows-ab > $O/prof_bench.json 2> $O/prof.err
  echo "rocprof exit $?"; cat $O/prof_bench.json
  find $O/prof -name "*stats*" | head
  f=$(find $O/prof -name "*kernel_stats.csv" | head -1); head -40 "$f"
  # keep only the small summaries
  find $O/prof -name "*kernel_trace.csv" -size +20M -delete
fi
