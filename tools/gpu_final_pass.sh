# usage: sh tools/gpu_final_pass.sh OUT_DIR   (from the repository root, on a machine with the GPU; OUT_DIR should be kept out of git)
set -e
OUT=${1:?usage: sh tools/gpu_final_pass.sh OUT_DIR}
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -q -s > $OUT/gpu_tests.log 2>&1
tail -2 $OUT/gpu_tests.log
timeout -k 10 900 python tools/make_traffic_json.py profiles/r03 > $OUT/traffic.log 2>&1
cp profiles/r03/traffic.json $OUT/traffic.json
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err
tail -c 600 $OUT/bench.json
ROOT=$PWD
OUT=$(cd $OUT && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o b -- python3 $ROOT/bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > $OUT/bench_under_rocprof.json 2> $OUT/rocprof.err
cd $ROOT
find $OUT/prof -name "*kernel_stats.csv" -exec cp {} $OUT/bench_kernel_stats.csv \;
find $OUT/prof -name "*kernel_trace.csv" -delete
ls $OUT
