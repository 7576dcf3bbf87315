#!/bin/bash
# usage (on the GPU box, from the repo root): tools/round_profile.sh <tag>
# The evidence of a round in one call: bench line, rocprofv3 kernel stats + trace analyses of the same command, init(db) phase
# trace.  (PMC passes: tools/pmc_run.sh, a call of its own.)
set -e
tag=$1
root=${GRAFT_REPO_ROOT:-$(pwd)}
res=${KMX_OUT_DIR:-$root/tool_out}; mkdir -p "$res"
python bench.py --full --steps 5 --warmup 1 > $res/${tag}_bench100m.json 2> $res/${tag}_bench100m.err
python tools/show_bench.py $res/${tag}_bench100m.json > $res/${tag}_bench100m.txt 2>&1 || true
out=$res/prof_$tag
rm -rf "$out"; mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$out" -- python "$root/bench.py" --full --steps 1 --warmup 1 --no-init-db --no-query-strings --cpu-sample 0 --no-single-model --genome-bases 0 > "$res/${tag}_rocprof_run.json" 2> "$res/${tag}_rocprof.err"
cd "$root"
python tools/trace_rounds.py "$out" 5 k_round_detect > "$res/${tag}_round_timings.txt" 2>&1 || true
python tools/trace_block.py "$out" 167 > "$res/${tag}_block_timeline.txt" 2>&1 || true
python tools/trace_gaps.py "$out" > "$res/${tag}_build_gaps.txt" 2>&1 || true
f=$(ls "$out"/*/*kernel_stats.csv "$out"/*kernel_stats.csv 2>/dev/null | head -1)
[ -n "$f" ] && cp "$f" "$res/${tag}_bench100m_kernel_stats.csv"
rm -rf "$out"
KMX_INIT_TRACE=1 python tools/bench_init_trace.py > $res/${tag}_init_trace.txt 2>&1 || true
cat $res/${tag}_bench100m.txt $res/${tag}_build_gaps.txt
tail -30 $res/${tag}_init_trace.txt
