#!/bin/bash
# Runs ON the GPU box: kernel traces of the headline bench under the A/B switches of the round-6 kernel-map work
#   WARPCONVNET_AMD_KMAP_COMPACT=0|1 (compact table rows), WARPCONVNET_AMD_KMAP_COSCHED="0" | "s,h,c" (pair scatter inside the sort)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-tools/_tmp}  # traces, logs and summaries (relative to the repository root)
mkdir -p $OUT/prof
run() {
  TAG=$1; shift
  env "$@" rocprofv3 --kernel-trace --stats -d $OUT/prof -o t_${TAG} -- python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-secondary > $OUT/prof/t_${TAG}.log 2>&1
  python tools/rocpd_stats.py $OUT/prof/t_${TAG}_results.db > $OUT/trace_${TAG}.md
  rm -f $OUT/prof/t_${TAG}_results.db
  echo "== ${TAG}: $*"
  head -32 $OUT/trace_${TAG}.md
  grep -h '"metric"' $OUT/prof/t_${TAG}.log | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['phases_ms'])"
}
for spec in "$@"; do
  TAG=${spec%%:*}
  ENVS=${spec#*:}
  run "$TAG" $(echo "$ENVS" | tr ';' ' ')
done
