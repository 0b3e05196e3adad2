# One parameterised GPU launcher (replaces the per-experiment gpu_r*.sh scripts).
# Usage: bash scripts/gpu_run.sh TAG STEPS...   where each step is one of
#   tests[=FILES]   pytest -m gpu on FILES (default: the whole suite)
#   smoke           __graft_entry__.smoke()
#   quick           bench.py --full --no-extras --no-cpu-baseline (headline line with its kernel / roofline figures)
#   bench           bench.py --full (all side lines, cpu baseline)
#   prof            rocprofv3 kernel-trace summary + PMC passes of the headline (scripts/gpu_prof_headline.sh)
#   sprof           rocprofv3 kernel stats of NerfRunner.train()-sized steps (scripts/gpu_small_prof.sh)
#   ab=LIBS         same-box A/B of library builds (scripts/gpu_ab.sh; FRAMES / ABL_ONLY from the env)
# Every GPU step runs under its own time limit; the script stops at the first failure.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
TAG=${1:?tag}
shift
for step in "$@"; do
  case "$step" in
    tests|tests=*)
      files=${step#tests}; files=${files#=}; files=${files:-tests}
      timeout -k 10 900 python -u -m pytest ${files//,/ } -m gpu -x -v --timeout 300 --timeout-method thread \
        > $OUT/tests_$TAG.log 2>&1 || { tail -40 $OUT/tests_$TAG.log; exit 2; }
      tail -3 $OUT/tests_$TAG.log ;;
    smoke)
      timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 \
        || { tail -20 $OUT/smoke_$TAG.log; exit 3; }
      tail -2 $OUT/smoke_$TAG.log ;;
    quick)
      timeout -k 10 400 python bench.py --full --no-extras --no-cpu-baseline > $OUT/bench_$TAG.json \
        2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 4; }
      python -c "import json; d=json.load(open('$OUT/bench_$TAG.json')); print(d['value'], d['ms_per_step'], {k: v['ms'] for k, v in d['kernels'].items()}, d['roofline']['frac'])" ;;
    bench)
      timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err \
        || { tail -20 $OUT/bench_$TAG.err; exit 5; }
      python -c "import json; d=json.load(open('$OUT/bench_$TAG.json')); print(d['value'], d['ms_per_step'], {k: v['ms'] for k, v in d['kernels'].items()}, d['roofline']['frac'], d['parity_mode']['ms_per_step'], d['config2']['ms_per_step'])" ;;
    prof)
      bash scripts/gpu_prof_headline.sh $TAG || exit 6 ;;
    sprof)
      bash scripts/gpu_small_prof.sh $TAG > $OUT/sprof_top_$TAG.txt 2>&1 || { tail -20 $OUT/sprof_top_$TAG.txt; exit 8; }
      cp $OUT/sprof_$TAG/run_kernel_stats.csv $OUT/kernel_stats_parity_$TAG.csv
      head -12 $OUT/sprof_top_$TAG.txt ;;
    ab=*)
      LIBS="${step#ab=}" bash scripts/gpu_ab.sh $TAG || exit 7 ;;
    *) echo "unknown step $step"; exit 9 ;;
  esac
done
echo "gpu_run $TAG done"
