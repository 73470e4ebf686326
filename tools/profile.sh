#!/bin/bash
# rocprofv3 kernel trace of one bench.py run -> $OUT/<tag>_summary.txt (+ raw stats csv)
# usage: tools/profile.sh <tag> [bench args...]
tag=$1; shift
root=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-out}   # output folder, relative to the repository root
out=$root/$OUT/${tag}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out -o prof -- python3 $root/bench.py --no-cpu-baseline "$@" > $out.log 2>&1
cd $root
python tools/prof_summary.py $out > $OUT/${tag}_summary.txt
find $out -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $OUT/${tag}_kernel_stats.csv
python tools/timeline.py $out > $OUT/${tag}_timeline.txt 2>&1
rm -rf $out
