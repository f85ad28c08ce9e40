#!/bin/bash
# usage: tools/exp_variants.sh <lib suffix>...   (experiment builds under tools/bin/)
tmp=$(mktemp -d)
for v in "$@"; do
  VPPX_LIB=$PWD/tools/bin/libvppx_$v.so python bench.py --full --steps 10 --warmup 3 --cpu-frames 0 > $tmp/$v.json 2> $tmp/$v.err
  python - "$v" "$tmp" <<'PY'
import sys, json
v, tmp = sys.argv[1], sys.argv[2]
try:
    d = json.loads(open(f"{tmp}/{v}.json").read().strip().splitlines()[-1])
    print(v, "ms/step", d["ms_per_step"], "agg in-pipeline", d["roofline"]["kernel_ms"], "agg back-to-back", d["roofline"]["kernel_ms_back_to_back"], "sum", d["stage_ms"]["sum_wta_left"])
except Exception as e:
    print(v, "failed", e, open(f"{tmp}/{v}.err").read()[-500:])
PY
done
