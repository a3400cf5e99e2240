#!/bin/bash
# wall time of the full default line (`bench.py --full`: CPU baseline and secondary entries too) and a digest of it
# usage: tools/debug/default_line.sh [output directory, default: a new temporary one]
cd "$(dirname "$0")/../.."
O=${1:-$(mktemp -d)}
mkdir -p "$O"
S=$(date +%s.%N)
python bench.py --full > "$O/default_line.json" 2> "$O/default_line.err"
E=$(date +%s.%N)
echo "wall seconds: $(echo "$E - $S" | bc)"
LINE="$O/default_line.json" python - <<'PY'
import json, os
d = json.loads(open(os.environ["LINE"]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["traffic_source"])
print(d["cpu_baseline"]["value"], d["cpu_baseline"]["sample"][-40:], d["cpu_baseline"]["single_thread"]["value"])
for s in d["secondary"]:
    r = s.get("roofline") or {}
    print(s["config"], "%.4g" % s["value"], r.get("bound"), r.get("frac"), (r.get("hbm") or {}).get("frac"), r.get("traffic_source"))
PY
