#!/bin/bash
# tests/c/jpeg_decode.c and the host code it calls (tm_jpeg_in.hip: the container walk and the host twin of tm_jpeg.h's rule; tm_tables.hip)
# under AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program on the cases that tests/jpeg_cases.py writes and on
# seeded damages of them; CPU only, no device is touched.  usage: tools/asan_jpeg_in.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/jpeg_cases.py" "$OUT/jpeg_cases.bin"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/jpeg_decode.c" -o "$OUT/jpeg_decode.o"
objs=("$OUT/jpeg_decode.o")
pids=()
for f in tm_jpeg_in tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/jpeg_decode"
"$OUT/jpeg_decode" "$OUT/jpeg_cases.bin"
