#!/bin/bash
# tests/c/png_deflate.c and the host code it calls (tm_deflate.hip, tm_png.hip, tm_tables.hip) under AddressSanitizer and
# UndefinedBehaviorSanitizer, as one stand-alone program; CPU only, no device is touched.  usage: tools/asan_png_out.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/png_deflate.c" -o "$OUT/png_deflate.o"
objs=("$OUT/png_deflate.o")
pids=()
for f in tm_deflate tm_png tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/png_deflate"
"$OUT/png_deflate" "$OUT/png_deflate_tmp.png"
