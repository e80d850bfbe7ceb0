#!/bin/bash
# development aid: the k-means parity tests, then the headline bench (no extras) with PreparePalettes' timing lines, a line of figures per run
#   tools/km_check.sh [-n REPS] [-g PATTERN] [--stamps] [--run-all] [--no-tests]
#   -n REPS      bench runs (default 2)
#   -g PATTERN   of the last [tm_pp] lines, show those that match (grep syntax, e.g. '192-D\|3-D\|colours'; default: the last 8, all of them)
#   --stamps     tools/kmr_stamps.sh between the tests and the bench: the resident launch's phase stamps (variant build "stamps")
#   --run-all    the tests take tests/test_gpu_encoder.py and `run_all` along
#   --no-tests   the bench alone
# The bench runs whatever library TM_LIB_VARIANT names (tools/build_variant.sh); RESULTS: where the logs and JSON lines go.
set -o pipefail
REPS=2; PATTERN=""; STAMPS=0; RUN_ALL=0; TESTS=1
while [ $# -gt 0 ]; do
  case "$1" in
    -n) REPS="$2"; shift 2 ;;
    -g) PATTERN="$2"; shift 2 ;;
    --stamps) STAMPS=1; shift ;;
    --run-all) RUN_ALL=1; shift ;;
    --no-tests) TESTS=0; shift ;;
    *) echo "km_check.sh: unknown argument $1" >&2; exit 2 ;;
  esac
done
RESULTS=${RESULTS:-results}; export RESULTS  # where the logs and JSON lines go
mkdir -p "$RESULTS"
if [ $TESTS -eq 1 ]; then
  FILES="tests/test_gpu_parity.py tests/test_gpu_fullsize.py"; SELECT="kmeans or palett or quantize"
  [ $RUN_ALL -eq 1 ] && { FILES="$FILES tests/test_gpu_encoder.py"; SELECT="$SELECT or run_all"; }
  timeout -k 10 900 python -m pytest $FILES -x -q -m gpu -k "$SELECT" > $RESULTS/km_tests.log 2>&1
  rc=$?
  tail -3 $RESULTS/km_tests.log
  [ $rc -ne 0 ] && { grep -n "Error\|error\|assert" $RESULTS/km_tests.log | tail -20; exit $rc; }
fi
if [ $STAMPS -eq 1 ]; then bash tools/kmr_stamps.sh || exit 1; fi
for rep in $(seq 1 "$REPS"); do
TM_PP_DEBUG=1 timeout -k 10 300 python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-motion-extra --no-defaults-extra --no-dense-extra --no-h2d-extra --no-frozen-extra --no-kmodes-extra > $RESULTS/km_bench.json 2> $RESULTS/km_bench.err || { tail -5 $RESULTS/km_bench.err; exit 1; }
python -c "
import json
j=json.loads(open('$RESULTS/km_bench.json').read().strip().splitlines()[-1])
print('lib=${TM_LIB_VARIANT:-build} fps=%.0f ms=%.2f'%(j['value'],j['ms_per_step']), j['stage_ms'], j['stage_rooflines']['kmeans']['tile_iters'], j['stage_rooflines']['kmeans']['pixel_iters'])"
if [ -n "$PATTERN" ]; then grep "tm_pp" $RESULTS/km_bench.err | tail -6 | grep "$PATTERN"; else grep "tm_pp" $RESULTS/km_bench.err | tail -8; fi
done
