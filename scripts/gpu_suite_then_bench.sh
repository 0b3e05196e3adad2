# Whole GPU suite without -x (every failure reported), then — only if pytest ended normally
# (0: green, 1: some tests failed; not a fault / abort / time limit) — smoke and the quick bench.
# Usage: bash scripts/gpu_suite_then_bench.sh TAG [pytest files...]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
TAG=${1:?tag}; shift
FILES=${*:-tests}
timeout -k 10 1000 python -u -m pytest $FILES -m gpu -v --timeout 300 --timeout-method thread \
  > $OUT/tests_$TAG.log 2>&1
rc=$?
grep -E "PASSED|FAILED|ERROR" $OUT/tests_$TAG.log | grep -v "^FAILED\|^ERROR" | awk '{print $NF, $1}' | sort | uniq -c | sort -rn | head -3
grep -E "^(FAILED|ERROR)" $OUT/tests_$TAG.log | head -20
tail -1 $OUT/tests_$TAG.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 \
  || { tail -20 $OUT/smoke_$TAG.log; exit 3; }
tail -2 $OUT/smoke_$TAG.log
timeout -k 10 400 python bench.py --full --no-extras --no-cpu-baseline > $OUT/bench_$TAG.json \
  2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 4; }
python -c "import json; d=json.load(open('$OUT/bench_$TAG.json')); print(d['value'], d['ms_per_step'], {k: v['ms'] for k, v in d['kernels'].items()}, d['roofline']['frac'])"
exit $rc
