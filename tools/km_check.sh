#!/bin/bash
# development aid: k-means parity tests, then the headline bench (no extras) with the PreparePalettes timing lines
set -o pipefail
RESULTS=${RESULTS:-results}; export RESULTS  # where the logs and JSON lines go
mkdir -p "$RESULTS"
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_encoder.py -x -q -m gpu -k "kmeans or palett or quantize or run_all" > $RESULTS/km_tests.log 2>&1
rc=$?
tail -3 $RESULTS/km_tests.log
[ $rc -ne 0 ] && { grep -n "Error\|error\|assert" $RESULTS/km_tests.log | tail -20; exit $rc; }
for rep in 1 2; do
TM_PP_DEBUG=1 timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-motion-extra --no-defaults-extra --no-dense-extra --no-h2d-extra --no-frozen-extra --no-kmodes-extra > $RESULTS/km_bench.json 2> $RESULTS/km_bench.err || { tail -5 $RESULTS/km_bench.err; exit 1; }
python -c "
import json
j=json.loads(open('$RESULTS/km_bench.json').read().strip().splitlines()[-1])
print('fps=%.0f ms=%.2f'%(j['value'],j['ms_per_step']), j['stage_ms'], j['stage_rooflines']['kmeans']['tile_iters'], j['stage_rooflines']['kmeans']['pixel_iters'])"
grep "tm_pp" $RESULTS/km_bench.err | tail -8
done
