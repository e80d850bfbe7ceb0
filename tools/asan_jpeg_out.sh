#!/bin/bash
# tests/c/jpeg_encode.c and the host code it calls (tm_jpeg_out.hip: the host twin of tm_jpeg_out.h's rule; tm_jpeg_in.hip: the reader the
# files go back through; tm_tables.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program on the pictures
# that tests/jpeg_out_cases.py writes with the restatement's files; CPU only, no device is touched.  usage: tools/asan_jpeg_out.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/jpeg_out_cases.py" "$OUT/jpeg_out_cases.bin"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/jpeg_encode.c" -o "$OUT/jpeg_encode.o"
objs=("$OUT/jpeg_encode.o")
pids=()
for f in tm_jpeg_out tm_jpeg_in tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/jpeg_encode"
"$OUT/jpeg_encode" "$OUT/jpeg_out_cases.bin"
