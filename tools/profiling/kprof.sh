#!/bin/bash
# per-kernel timing of one bench run under rocprofv3 (GPU box): bash tools/profiling/kprof.sh <tag> [bench args]
# -> $OUT_DIR/prof_<tag>_kernel_stats.csv, default build/prof/ (copy the ones to be judged into profiles/)
export TMPDIR=/tmp
tag=$1; shift
R=$PWD
OUT_DIR=${OUT_DIR:-build/prof}
mkdir -p $OUT_DIR
rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT_DIR/prof_$tag -- python3 bench.py --steps 4 --warmup 2 "$@" > $OUT_DIR/prof_$tag.json 2> $OUT_DIR/prof_$tag.err
f=$(ls $OUT_DIR/prof_$tag/*/*kernel_stats.csv | head -1)
cp $f $OUT_DIR/prof_${tag}_kernel_stats.csv
rm -rf $OUT_DIR/prof_$tag
python3 tools/profiling/kstats.py $OUT_DIR/prof_${tag}_kernel_stats.csv
cat $OUT_DIR/prof_$tag.json
