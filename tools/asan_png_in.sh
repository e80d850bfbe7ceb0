#!/bin/bash
# tests/c/png_inflate.c and the host code it calls (tm_png_in.hip: the host twins of tm_inflate.h's rule; tm_png.hip: the reader they are
# held to; tm_tables.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program on the cases that
# tests/png_in_cases.py writes; CPU only, no device is touched.  usage: tools/asan_png_in.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/png_in_cases.py" "$OUT/png_in_cases.bin"  # (plain Python: the library it loads for two of the cases is the ordinary build)
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/png_inflate.c" -o "$OUT/png_inflate.o"
objs=("$OUT/png_inflate.o")
pids=()
for f in tm_png_in tm_png tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/png_inflate"
"$OUT/png_inflate" "$OUT/png_in_cases.bin" "$OUT/png_inflate_tmp.png"
