# End-of-round check on the GPU box: GPU tests, bench (with CPU baseline), build+smoke in one process, stamp tools,
# rocprofv3 kernel statistics of the bench, and the micro-benchmarks that back DESIGN.md's next levers.
# bash tools/round_check.sh [tag]; the logs go to $OUT (default out/round_check under the repository root).
set -e
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/out/round_check}
mkdir -p "$OUT"; cd "$R"
V=${1:-19}
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/t$V.log" 2>&1
timeout -k 10 300 python bench.py --full > "$OUT/bench$V.log" 2>&1
timeout -k 10 100 python -c "import __graft_entry__ as g; g.build(); g.smoke(); print('smoke ok')" > "$OUT/smoke$V.log" 2>&1
timeout -k 10 120 python tools/ubench_attn.py > "$OUT/ua$V.log" 2>&1
timeout -k 10 120 python tools/stamps_bwd.py > "$OUT/stamps$V.log" 2>&1
if [ -x build/ubench_group_sync ]; then timeout -k 10 60 ./build/ubench_group_sync > "$OUT/group_sync$V.log" 2>&1; fi
cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof$V" -o r$V -- python3 "$R/bench.py" --steps 3 --warmup 2 --no-cpu-baseline --no-decode > "$OUT/prof$V.log" 2>&1
