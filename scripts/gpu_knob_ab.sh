# Same-box knob A/B on the working tree's build (scripts/knob_ab.py); VARIANTS from the environment.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
T=${1:-knob}
ROUNDS=${ROUNDS:-6} timeout -k 10 500 python scripts/knob_ab.py > $OUT/knob_$T.jsonl 2> $OUT/knob_$T.err || { tail -20 $OUT/knob_$T.err; exit 3; }
cat $OUT/knob_$T.jsonl
