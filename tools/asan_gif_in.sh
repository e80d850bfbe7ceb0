#!/bin/bash
# tests/c/gif_decode.c and the host code it calls (tm_gif_in.hip: the container walk and the host twin of tm_gif.h's rule; tm_tables.hip)
# under AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program on the cases that tests/gif_cases.py writes and on
# seeded damages of them; CPU only, no device is touched.  usage: tools/asan_gif_in.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
PYTHON="${PYTHON:-python3}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$PYTHON" "$ROOT/tests/gif_cases.py" "$OUT/gif_cases.bin"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/gif_decode.c" -o "$OUT/gif_decode.o"
objs=("$OUT/gif_decode.o")
pids=()
for f in tm_gif_in tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  pids+=($!)
  objs+=("$OUT/$f.o")
done
for p in "${pids[@]}"; do wait "$p"; done  # (a failed compile ends the script here)
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/gif_decode"
"$OUT/gif_decode" "$OUT/gif_cases.bin"
