# Upper bound of the scatter's input-gradient share: the headline field pass with frozen poses
# (skip_pose_grad: no corner re-gather, no slopes) against the default, same box, interleaved.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
VARIANTS='{"base": {}, "nodx": {"pose_grad": false}}' ROUNDS=6 \
  timeout -k 10 400 python scripts/knob_ab.py > $OUT/knob_nodx.jsonl 2> $OUT/knob_nodx.err || { tail -20 $OUT/knob_nodx.err; exit 3; }
cat $OUT/knob_nodx.jsonl
