# parity + result digests + per-kernel times of the match / finalize stage, on the GPU box: bash tools/exp/run_match.sh <tag>
# (results under $OUT, default out/; $OUT/digest_before.txt, when present, is the digest run the new one must equal)
set -u
TAG=${1:-m}
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT/$TAG
python tools/exp/digest.py > $OUT/$TAG/digest.txt 2>&1
if [ -f $OUT/digest_before.txt ]; then diff <(grep DIGEST $OUT/digest_before.txt) <(grep DIGEST $OUT/$TAG/digest.txt) && echo "DIGESTS EQUAL"; else cat $OUT/$TAG/digest.txt; fi
python -m pytest tests/test_gpu_parity.py tests/test_gpu_api.py -x -q 2>&1 | tail -3
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG/trace -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --images-in-flight 1 --num-iter 20 --solo-images 2 > $OUT/$TAG/bench.log 2>&1
python3 tools/kstats.py $OUT/$TAG/trace
grep -o '"roofline_match".*' $OUT/$TAG/bench.log | cut -c1-330
find $OUT/$TAG -name "*kernel_trace.csv" -delete; find $OUT/$TAG -name "*.db" -delete
