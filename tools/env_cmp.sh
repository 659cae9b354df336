#!/bin/bash
# Development aid: bench.py legs under two settings of one environment switch, interleaved.
#   usage (through gpurun): bash tools/env_cmp.sh GA3C_D1F_TILE 1 0 [extra bench args]
set -e -o pipefail
VAR=$1; A=$2; B=$3; shift 3
for round in 1 2; do
  for v in $A $B; do
    line=$(env $VAR=$v timeout -k 10 200 python bench.py --full --steps 300 --warmup 30 --cpu-seconds 0 --e2e-seconds 0 "$@" | tail -n 1)
    python - "$VAR=$v" "$line" <<'PY'
import json, sys
d = json.loads(sys.argv[2])
pl = d['predict_lanes']
print(sys.argv[1], 'lanes 1/2/3: %.2f %.2f %.2f M/s' % (pl['1'] / 1e6, pl['2'] / 1e6, pl['3'] / 1e6), 'train %.0f' % d['train']['value'],
      'u8 %.2f M/s' % (d['uint8_resident']['predictions_per_sec'] / 1e6))
PY
  done
done
