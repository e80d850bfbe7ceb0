#!/bin/bash
# tests/c/lz_matches.c and the host code it calls (tm_lzma.hip, tm_tables.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as one
# stand-alone program; CPU only, no device is touched.  usage: tools/asan_lz_matches.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/lz_matches.c" -o "$OUT/lz_matches.o"
objs=("$OUT/lz_matches.o")
for f in tm_lzma tm_tables; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  objs+=("$OUT/$f.o")
done
wait
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/lz_matches"
"$OUT/lz_matches" "$ROOT/tests/golden/football_cif_kf1.lzma"
