# Same-box knob A/B on NerfRunner.train()'s 2048-ray step (scripts/parity_ab.py); VARIANTS from the env.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
T=${1:-pknob}
REPS=${REPS:-4} STEPS=${STEPS:-300} timeout -k 10 500 python scripts/parity_ab.py > $OUT/parity_$T.jsonl 2> $OUT/parity_$T.err || { tail -20 $OUT/parity_$T.err; exit 3; }
cat $OUT/parity_$T.jsonl
