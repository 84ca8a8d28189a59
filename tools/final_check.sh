#!/bin/bash
# the round's last GPU check: the whole GPU suite, the bench line with --full (summary of its fields), the smoke entry
python -m pytest tests -x -q -m gpu > gpurun_out/t_full.log 2>&1; tail -4 gpurun_out/t_full.log
json=$(mktemp); python bench.py --full > $json 2> $json.err
python - $json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
print(d["value"], d["ms_per_rk_stage"], d["roofline"]["frac"], d["api_path_ms_per_rk_stage"], d["cpu_baseline"]["value"])
for k, v in d["also"].items():
    print(k, v.get("ms_per_rk_stage"), v.get("error"), v.get("leg_wall_s"))
PY
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')"
