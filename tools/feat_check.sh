#!/bin/bash
# development aid: the feature tests, then tools/motion_check.sh's bench part and the headline
set -o pipefail
RESULTS=${RESULTS:-results}; export RESULTS  # where the logs and JSON lines go
mkdir -p "$RESULTS"
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_encoder.py -x -q -m gpu -k "features or window or motion or every_source or run_all or first_look or default_path" > $RESULTS/feat_tests.log 2>&1
rc=$?
tail -3 $RESULTS/feat_tests.log
[ $rc -ne 0 ] && { grep -n "Error\|error\|assert" $RESULTS/feat_tests.log | tail -20; exit $rc; }
for rep in 1 2; do
timeout -k 10 400 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-dense-extra --no-h2d-extra --no-kmodes-extra --no-frozen-extra --no-defaults-extra > $RESULTS/feat.json 2> $RESULTS/feat.err || { tail -5 $RESULTS/feat.err; exit 1; }
python - <<'PY'
import os
import json
j = json.loads(open(os.environ['RESULTS'] + '/feat.json').read().strip().splitlines()[-1])
print("value %.0f  %.2f ms" % (j["value"], j["ms_per_step"]), j["stage_ms"], "features %.2f ms" % j["stage_rooflines"]["features"]["ms"], j["parity_gate"])
k = "with_motion_prediction"
print("  ", k, round(j[k]["value"]), {a: b for a, b in j[k]["stage_ms"].items() if b > 20})
PY
done
