#!/bin/bash
# usage: run_variants.sh name1 name2 ... ; "product" = product library
# (the bench lines and their stderr are kept in a fresh temporary folder, printed at the start)
R="$(cd "$(dirname "$0")/.." && pwd)"
O=$(mktemp -d) || exit 1
echo "bench lines: $O"
for v in "$@"; do
  if [ $v = product ]; then unset JELLO_HIP_LIB; else export JELLO_HIP_LIB=$R/jello_amd/libjello_hip_$v.so; fi
  timeout -k 10 200 python3 "$R/bench.py" --full --no-cpu-baseline > "$O/$v.json" 2> "$O/$v.err" || { tail -3 "$O/$v.err"; exit 1; }
  python3 - "$O/$v.json" $v <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[2], "frame", d["ms_per_step"], "one at a time", (d.get("one_frame_at_a_time") or {}).get("ms_per_step"), "fine", d["roofline"]["avg_ms"], "stages", {k:round(v,4) for k,v in d.get("stage_ms",{}).items()} if "stage_ms" in d else "")
PY
done
