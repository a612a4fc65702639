#!/bin/bash
# GPU idle time inside one proof: tools/gaps.sh <tag> [--list]   (env switches are inherited) -> $OUT/<tag>_gaps.txt
# OUT = output directory (default: measure_out/ in the repository root)
tag=$1; shift
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
out=${OUT:-measure_out}; mkdir -p "$out"
rm -rf $out/${tag}_tl
# --full: timeline_gaps.py analyses the last timed proof, the one before the verification proof that only --full makes
rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $out/${tag}_tl -- python bench.py --full --steps 3 --warmup 2 --pipelined 0 --no-kprof --no-cpu-baseline --no-end-to-end --alt-fib-n 0 --big-fib-n 0 --cached-setup-steps 0 --sharded-one-rank-blocks 0 > /dev/null 2> $out/${tag}_tl.err
k=$(ls $out/${tag}_tl/*/*_kernel_trace.csv | head -1); m=$(ls $out/${tag}_tl/*/*_memory_copy_trace.csv | head -1)
python tools/timeline_gaps.py $k $m "$@" > $out/${tag}_gaps.txt
head -${GAPS_HEAD:-14} $out/${tag}_gaps.txt
rm -rf $out/${tag}_tl
