#!/bin/bash
# tests/c/gif_encode.c and the host code it calls (tm_gif_out.hip: the host twin of tm_gif_out.h's rule; tm_gif_in.hip: the reader it is read
# back with; tm_tables.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program on the cases that
# tests/gif_out_cases.py writes; CPU only, no device is touched.  usage: tools/asan_gif_out.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/gif_out_cases.py" "$OUT/gif_out_cases.bin"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/gif_encode.c" -o "$OUT/gif_encode.o"
objs=("$OUT/gif_encode.o")
pids=()
for f in tm_gif_out tm_gif_in tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/gif_encode"
"$OUT/gif_encode" "$OUT/gif_out_cases.bin"
