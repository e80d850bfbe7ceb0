#!/bin/bash
# tests/c/webp_encode.c and the host code it calls (tm_webp_out.hip: the host twin of tm_webp_out.h's rule; tm_deflate.hip: the code lengths, and tm_png.hip behind it;
# tm_gif_out.hip: the launches the device form shares; tm_tables.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as one
# stand-alone program on the cases that tests/webp_out_cases.py writes; CPU only, no device is touched.
# usage: tools/asan_webp_out.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/webp_out_cases.py" "$OUT/webp_out_cases.bin"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/webp_encode.c" -o "$OUT/webp_encode.o"
objs=("$OUT/webp_encode.o")
pids=()
for f in tm_webp_out tm_deflate tm_png tm_gif_out tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/webp_encode"
"$OUT/webp_encode" "$OUT/webp_out_cases.bin"
