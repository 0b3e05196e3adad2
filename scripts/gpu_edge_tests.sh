set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_gpu_step.py -m gpu -v -k "ragged" --timeout 200 --timeout-method thread > $OUT/tests_r6x.log 2>&1 || { tail -60 $OUT/tests_r6x.log; exit 2; }
tail -12 $OUT/tests_r6x.log
