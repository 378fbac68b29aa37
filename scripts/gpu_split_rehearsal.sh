#!/bin/bash
# gloo world-2 rehearsal (both ranks on the one GPU) of the N > 1 step: two hipGraphs with early buckets leaving under the second,
# against one hipGraph with every bucket after it; per-phase host times on stderr (TAVSR_BENCH_TRACE).  Files under $OUT_DIR
# (default bench_out/).
cd "$(dirname "$0")/.." || exit 1
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p "$OUT_DIR"
for v in "" "--no-split-backward"; do
  tag=$([ -z "$v" ] && echo split || echo whole)
  TAVSR_BENCH_TRACE=1 TAVSR_DP_BACKEND=gloo timeout 900 python bench.py --full --gpus 2 --steps 4 --warmup 2 --sustain-s 0 --no-roofline --no-cpu-baseline --no-fwd-encoder $v > "$OUT_DIR/dp_gloo2_$tag.json" 2> "$OUT_DIR/dp_gloo2_$tag.err"
  echo "gloo x2 [$tag] rc=$?"; grep "two-graph\|rank 0\] step" "$OUT_DIR/dp_gloo2_$tag.err" | tail -8; python -c "
import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['n_gpus'], d['value'], d['ms_per_step'], d.get('grad_exchange_exposed_ms_per_step'), d['config']['launch'])" "$OUT_DIR/dp_gloo2_$tag.json"
done 2>&1 | tee "$OUT_DIR/split_rehearsal.txt"
