#!/bin/bash
# The round's measurement set on a GPU box: tools/profile_round.sh <tag>   (raw outputs under $OUT, default prof_out/ in the
# repository root; summaries under profiles/ are written by the caller from the merged files)
tag=$1
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}
mkdir -p $OUT
cd $R && python bench.py --full > $OUT/bench_$tag.log 2> $OUT/bench_$tag.err
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_$tag $OUT/pmcF_$tag $OUT/pmcW_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -o run -- python $R/bench.py > $OUT/bench_${tag}_prof.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmcF_$tag -o f -- python $R/bench.py --steps 2 --warmup 1 --no-graph > $OUT/pmcF_$tag.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmcW_$tag -o w -- python $R/bench.py --steps 2 --warmup 1 --no-graph > $OUT/pmcW_$tag.log 2>&1
cd $R
tail -1 $OUT/bench_$tag.log | cut -c1-400
