# A/B timing of two library builds on the same box: scripts/ablate.py (variants in ABL_ONLY)
# with NOF_LIB = each of LIBS, at FRAMES frames (16: config 2, 64: headline pool).
# Usage: LIBS="libnof_prev.so libnof_ablate.so" FRAMES=64 bash scripts/gpu_ab.sh TAG
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
TAG=${1:-ab}
for L in ${LIBS:-libnof_prev.so libnof_ablate.so}; do
  for F in ${FRAMES:-16 64}; do
    FRAMES=$F NOF_LIB=$R/bundlesdf_amd/$L ONLY=${ABL_ONLY:-full} timeout -k 10 300 python scripts/ablate.py >> $OUT/ab_$TAG.jsonl 2> $OUT/ab_$TAG.err || { tail -20 $OUT/ab_$TAG.err; exit 1; }
  done
done
python -c "
import json
for l in open('$OUT/ab_$TAG.jsonl'):
    d = json.loads(l); print(d['lib'], d['frames'], d['variant'], d['field_ms_median'], d['kernels'])"
