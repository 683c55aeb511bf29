export PIPER_HIP_TUNING=1  # the library honours PIPER_HIP_* switches only with this set
set -e
OUT=${1:?usage: collect_ab.sh OUT_DIR}
mkdir -p "$OUT"
for m in kernel dma kernel dma; do
  if [ $m = dma ]; then export PIPER_HIP_COLLECT_DMA=1; else unset PIPER_HIP_COLLECT_DMA; fi
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-scale-bench --steps 200 --warmup 20 > "$OUT/$m.json" 2>"$OUT/$m.err"
  python - <<PY
import json
d=json.load(open("$OUT/$m.json")); print("$m", d["ms_per_step"], d["gpu_ms_mean"], d["end_to_end_ms"])
PY
done
timeout -k 10 300 python -m pytest tests/test_gpu_voice.py -x -q -m gpu 2>&1 | tail -2
