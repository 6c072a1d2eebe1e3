# same-box A/B of the match stage: round-2 tree (_r02 worktree), current build
set -u
export TMPDIR=/tmp
ARGS="--steps 2 --warmup 1 --no-cpu-baseline --images-in-flight 1 --num-iter 20 --solo-images 2"
OUT=${OUT:-$PWD/out/ab}   # absolute: the old tree's leg runs from inside it
mkdir -p $OUT
if [ -d _r02 ]; then (cd _r02 && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r02 -- python3 bench.py $ARGS > $OUT/r02.log 2>&1); python3 tools/kstats.py $OUT/r02 match_kernel scatter fit_grad pixel_count; fi
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/cur -- python3 bench.py $ARGS --full > $OUT/cur.log 2>&1
python3 tools/kstats.py $OUT/cur match_kernel scatter fit_grad tile_cull
find $OUT -name "*kernel_trace.csv" -delete; find $OUT -name "*.db" -delete
