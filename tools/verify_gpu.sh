#!/bin/bash
# full GPU test suite + config B / C bench lines in one call: bash tools/verify_gpu.sh [OUT_DIR] (default: a temporary directory)
set -o pipefail
O=${1:-$(mktemp -d)}
mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$O/pytest.log" 2>&1 || { tail -40 "$O/pytest.log"; exit 1; }
tail -3 "$O/pytest.log"
python bench.py --full --no-cpu-baseline > "$O/B.json" 2> "$O/B.err" || { tail -20 "$O/B.err"; exit 1; }
python bench.py --full --no-cpu-baseline --config C --steps 3 --warmup 1 > "$O/C.json" 2> "$O/C.err" || { tail -20 "$O/C.err"; exit 1; }
O="$O" python - <<'PY'
import json, os
for c in "BC":
    j=json.loads(open(os.path.join(os.environ["O"], "%s.json"%c)).read().strip().splitlines()[-1])
    print(c, "value %.3e ms %.2f its %s elem %s"%(j["value"],j["ms_per_step"],j["config"]["pcg_outer_iters_per_step"], j["element_stage"]["ms_per_step"]))
    print({k:(v["avg_us"],v["frac"]) for k,v in j["roofline_all"].items()})
PY
