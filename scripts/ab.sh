# A/B inside ONE session on one GPU (GPUs of one pool differ by 1 - 2 %): bench.py under each environment given, twice, alternating.
# usage: bash scripts/ab.sh asr "TAVSR_WGRAD_BESIDE=0" "TAVSR_WGRAD_BESIDE=1" ...   (files under $OUT_DIR, default bench_out/)
#        bash scripts/ab.sh avsr "TAVSR_LIB=$PWD/lib_b/libtavsr_hip.so" "TAVSR_LIB=$PWD/tailored-avsr_amd/tavsr/lib/libtavsr_hip.so"   (two builds of the library)
OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p "$OUT_DIR"
W=$1; shift
for rep in 1 2; do
for cfg in "$@"; do
  env $cfg timeout 600 python bench.py --full --workload $W --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-decode --no-asr --no-fwd-encoder --no-box --sustain-s 3 > "$OUT_DIR/ab.json" 2> "$OUT_DIR/ab.err" || tail -5 "$OUT_DIR/ab.err"
  python - "$cfg" "$OUT_DIR/ab.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(f"{sys.argv[1]:40s}: {d['value']:8.1f} {d['unit']}  {d['ms_per_step']:.3f} ms/step  sustained {d.get('sustained', {}).get('value')}  eager {d.get('eager', {}).get('value')}  hbm_peak {d.get('hbm_peak_gb')} GB")
PY
done; done
