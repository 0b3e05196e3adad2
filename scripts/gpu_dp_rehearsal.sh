set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${NOF_OUT_DIR:-$R/out}   # results directory (NOF_OUT_DIR overrides)
cd $R && mkdir -p $OUT
NOF_BENCH_BACKEND=gloo NOF_BENCH_SHARE_GPU=1 timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/dp2.json 2> $OUT/dp2.err || { tail -30 $OUT/dp2.err; exit 3; }
cat $OUT/dp2.json
