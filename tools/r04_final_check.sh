set -u
OUT=${1:?usage: tools/r04_final_check.sh <output folder>}; mkdir -p "$OUT"
( time python -m pytest tests/ -x -q -m gpu ) > "$OUT/pytest_gpu.log" 2>&1; echo "pytest rc=$?"; tail -3 "$OUT/pytest_gpu.log"
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?"; tail -2 "$OUT/smoke.log"
( time python bench.py --full ) > "$OUT/bench_driver.json" 2> "$OUT/bench_driver.err"; echo "bench rc=$?"; tail -4 "$OUT/bench_driver.err"
OUT="$OUT" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ["OUT"], "bench_driver.json")).read().strip().splitlines()[-1])
print("value", d["value"], "with_inverse", d.get("value_with_inverse"), "literal", d["literal_loop"]["value"], d["literal_loop"]["fused_step_with_per_step_read_write"]["value"])
print({k: round(v["value"]/1e6,3) for k,v in d["configs"].items()})
print("roofline", {k:d["roofline"].get(k) for k in ["frac","achieved","kernel_ms","valu_issue_frac","valu_lane_util","traffic"]}, "cpu", d["cpu_baseline"]["value"], d["cpu_baseline"]["cores"])
PY
