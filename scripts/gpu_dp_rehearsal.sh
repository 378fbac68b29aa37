# N gloo ranks sharing ONE GPU: plumbing rehearsal of the N > 1 line (files under $OUT_DIR, default bench_out/)
export OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p "$OUT_DIR"
for n in 2 4; do
  TAVSR_DP_BACKEND=gloo timeout 900 python bench.py --full --gpus $n --steps 5 --warmup 2 --sustain-s 3 --no-roofline --no-cpu-baseline --no-fwd-encoder > "$OUT_DIR/dp_gloo$n.json" 2> "$OUT_DIR/dp_gloo$n.err"
  echo "gloo x$n rc=$?"; python -c "
import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['n_gpus'], d['value'], d['ms_per_step'], d.get('grad_exchange_exposed_ms_per_step'), d.get('sustained'), d['config']['grad_exchange'])" "$OUT_DIR/dp_gloo$n.json"
done
TAVSR_DP_BACKEND=gloo timeout 900 python bench.py --full --gpus 2 --steps 5 --warmup 2 --sustain-s 0 --no-roofline --no-cpu-baseline --no-fwd-encoder --no-graph > "$OUT_DIR/dp_gloo2_eager.json" 2> "$OUT_DIR/dp_gloo2_eager.err"; echo "gloo x2 eager rc=$?"; python -c "
import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['n_gpus'], d['value'], d['ms_per_step'], d.get('grad_exchange_exposed_ms_per_step'), d['config']['launch'])" "$OUT_DIR/dp_gloo2_eager.json"
# the N > 1 step as two hipGraphs (early buckets exchanged under the second) against one graph: per-phase host times
bash scripts/gpu_split_rehearsal.sh
