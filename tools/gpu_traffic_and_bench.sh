# usage: sh tools/gpu_traffic_and_bench.sh OUT_DIR   (from the repository root, on a machine with the GPU; OUT_DIR should be kept out of git)
set -e
OUT=${1:?usage: sh tools/gpu_traffic_and_bench.sh OUT_DIR}
mkdir -p $OUT
timeout -k 10 1000 python tools/make_traffic_json.py profiles/r03 > $OUT/traffic.log 2>&1
cp profiles/r03/traffic.json $OUT/traffic.json
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err
tail -c 1500 $OUT/bench.json
