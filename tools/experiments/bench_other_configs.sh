cd $GRAFT_REPO_ROOT
T=$(mktemp -d)
for args in "--config stress16" "--config multiviewx --batch 4 --arch resnet50" "--config multiviewx"; do
  timeout 500 python bench.py $args --full --steps 3 --warmup 2 --no-cpu-baseline --no-gemm-tuning 2>$T/bench_cfg_err.log | tail -1 > $T/bench_cfg.json
  python - $T/bench_cfg.json <<'PY' || tail -3 $T/bench_cfg_err.log
import json, sys
d=json.load(open(sys.argv[1]))
g=lambda k: (d.get(k) or {}).get("frac")
print(d["config"]["workload"][:40], d["value"], g("roofline"), g("roofline_warp"), g("roofline_warp_bwd"), g("roofline_msda_bwd"), (d.get("roofline_msda_bwd") or {}).get("kernel","")[:48])
PY
done
rm -rf $T
