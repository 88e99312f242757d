o=${1:-runs/final}; mkdir -p $o
python bench.py --full > $o/default.json 2> $o/default.err
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $o/driver_form.json 2>/dev/null
python bench.py --full --steps 40 --no-cpu-baseline > $o/window40.json 2>/dev/null
python bench.py --full --steps 40 --no-cpu-baseline --dtype f64_e32 > $o/window40_e32.json 2>/dev/null
python bench.py --full --steps 40 --no-cpu-baseline --single-label 3 > $o/single3.json 2>/dev/null
python bench.py --full --no-cpu-baseline --workload 8d > $o/w8d.json 2>/dev/null
python bench.py --full --no-cpu-baseline --images 7500 --steps 60 > $o/shard7500.json 2>/dev/null
python bench.py --full --no-cpu-baseline --maxm 300 --images 7500 --steps 20 --literal-steps 0 > $o/m300_shard.json 2>/dev/null
for f in default driver_form window40 window40_e32 single3 w8d shard7500 m300_shard; do python - $f $o <<'PY'
import json,sys
f=sys.argv[1]
try:
    d=json.load(open("%s/%s.json" % (sys.argv[2], f)))
    k=d["kernel_ms_per_step"]
    print(f, "%.1f/s %.3f ms lit %s | rf %.3f hbm %.3f step_exec %.3f alg %.3f | grad %.3f svd %.3f |" % (d["value"], d["ms_per_step"], d["value_literal_order"] and round(d["value_literal_order"],1), d["roofline"]["frac"], (d["roofline_hbm"] or {}).get("frac",0), d["roofline_step"]["frac_executed"], d["roofline_step"]["algorithmic_gflop_per_step"] / d["ms_per_step"] / 78.6, d["gradient_phase_ms"], d["svd_ms"]), {a:round(b,3) for a,b in k.items()}, d.get("cpu_baseline",{}).get("value"), d["device_gb"])
except Exception as e: print(f, "failed", e)
PY
done
