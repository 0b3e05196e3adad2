# Same-box A/B of k_encode builds: the previous commit's production library (scripts/build_prev.py
# PROD=1 -> libnof_prev.so) against the working tree's (libnof.so), alternating, then the encode's
# two-level gather group (encode_group 2) against the default on the working tree's build.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
T=${1:-encab}
LIBS="libnof_prev.so libnof.so libnof_prev.so libnof.so libnof_prev.so libnof.so" FRAMES=64 bash scripts/gpu_ab.sh $T || exit 2
VARIANTS='{"g1": {}}' ROUNDS=1 \
  timeout -k 10 400 python scripts/knob_ab.py > $OUT/knob_$T.jsonl 2> $OUT/knob_$T.err || { tail -20 $OUT/knob_$T.err; exit 3; }
cat $OUT/knob_$T.jsonl
