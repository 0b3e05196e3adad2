# Final-build side shapes: BASELINE config 5 (global refine) per-GPU step and the 8-frame per-rank batch of N = 8.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
timeout -k 10 400 python bench.py --full --workload global_refine > $OUT/bench_global_refine_r6w.json 2> $OUT/bench_gr_r6w.err || { tail -20 $OUT/bench_gr_r6w.err; exit 3; }
python -c "import json; d=json.load(open('$OUT/bench_global_refine_r6w.json')); print(d['value'], d['ms_per_step'], {k: v['ms'] for k, v in d['kernels'].items()})"
timeout -k 10 300 python bench.py --full --pool-frames 8 --no-extras --no-cpu-baseline > $OUT/bench_8frames_per_rank_r6w.json 2> $OUT/bench_8f_r6w.err || { tail -20 $OUT/bench_8f_r6w.err; exit 4; }
python -c "import json; d=json.load(open('$OUT/bench_8frames_per_rank_r6w.json')); print(d['value'], d['ms_per_step'], {k: v['ms'] for k, v in d['kernels'].items()})"
