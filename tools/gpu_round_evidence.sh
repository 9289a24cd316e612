# tools/gpu_round_evidence.sh <tag> <dir>: the end-of-round evidence on the GPU box: perf-guard record, the default bench line
# with --full (headline + the other configs + cpu_baseline) and the `--config` lines with --full, written to <dir>, then
# rocprofv3 stats + PMC passes of all four configs.  Afterwards: tools/collect_profiles.sh <tag>_c2 <tag>_c3 <tag>_c4 <tag>_c5,
# and copy <dir>/<tag>_bench_*.json and the perf-guard record into profiles/.
set -e
TAG=${1:-r03_b}
B=${2:?usage: tools/gpu_round_evidence.sh <tag> <directory for the bench lines>}
mkdir -p "$B"
mkdir -p gpurun_out
rm -f gpurun_out/perf_guard.json
FMCMC_PERF_GUARD_RECORD=1 timeout -k 10 600 python -m pytest tests/test_gpu_perf_guard.py -q -m gpu > gpurun_out/perf_guard_record.log 2>&1 || { tail -20 gpurun_out/perf_guard_record.log; exit 1; }
cat gpurun_out/perf_guard.json
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$B/${TAG}_bench_default.json" 2> "$B/${TAG}_bench_default.err" || { tail -5 "$B/${TAG}_bench_default.err"; exit 1; }
tail -c 900 "$B/${TAG}_bench_default.json"; echo
for c in c3 c4 c5; do
  timeout -k 10 600 python bench.py --full --config $c --steps 5 --warmup 1 > "$B/${TAG}_bench_$c.json" 2> "$B/${TAG}_bench_$c.err" || { tail -5 "$B/${TAG}_bench_$c.err"; exit 1; }
  tail -c 500 "$B/${TAG}_bench_$c.json"; echo
done
for c in c2 c3 c4 c5; do
  timeout -k 10 900 bash tools/profile_bench.sh ${TAG}_$c $c full > gpurun_out/prof_${TAG}_$c.log 2>&1 || true
  cat gpurun_out/prof_${TAG}_$c/passes.log | tr '\n' ' '; echo
done
echo evidence done
