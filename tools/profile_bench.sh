#!/bin/bash
# usage (on the GPU box, from the repo root): tools/profile_bench.sh <tag> [bench.py args...]
# rocprofv3 --kernel-trace --stats of one bench.py run -> $KMX_OUT_DIR/<tag>_kernel_stats.csv, <tag>_rounds.txt (default tool_out/)
set -e
tag=$1; shift
root=${GRAFT_REPO_ROOT:-$(pwd)}
res=${KMX_OUT_DIR:-$root/tool_out}; mkdir -p "$res"
out=$res/prof_$tag
rm -rf "$out"; mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$out" -- python "$root/bench.py" --full --steps 1 --warmup 1 --no-init-db --cpu-sample 0 --no-single-model "$@" > "$res/${tag}_rocprof_run.json" 2> "$res/${tag}_rocprof.err"
cd "$root"
python tools/trace_rounds.py "$out" 5 k_round_detect > "$res/${tag}_rounds.txt" 2>&1 || true
python tools/trace_block.py "$out" 134 > "$res/${tag}_block_first.txt" 2>&1 || true      # first block of the last of 3 builds (10^8 k-mers: 67 blocks each)
python tools/trace_block.py "$out" 167 > "$res/${tag}_block_mid.txt" 2>&1 || true
f=$(ls "$out"/*/*kernel_stats.csv "$out"/*kernel_stats.csv 2>/dev/null | head -1)
[ -n "$f" ] && cp "$f" "$res/${tag}_kernel_stats.csv"
rm -rf "$out"
