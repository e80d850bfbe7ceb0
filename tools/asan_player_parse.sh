#!/bin/bash
# tests/c/player_parse.c and the host code it calls (tm_player_parse.hip, tm_gtm.hip, tm_lzma.hip, tm_tables.hip) under AddressSanitizer and
# UndefinedBehaviorSanitizer, as one stand-alone program; CPU only, no device is touched.  usage: tools/asan_player_parse.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/player_parse.c" -o "$OUT/player_parse.o"
objs=("$OUT/player_parse.o")
for f in tm_player_parse tm_gtm tm_lzma tm_lz_matches tm_tables; do  # (tm_lz_matches: the key frames' coder threads behind the writer)
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  objs+=("$OUT/$f.o")
done
wait
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/player_parse"
"$OUT/player_parse" "$OUT" "$ROOT/tests/golden/football_cif_kf1.lzma" 44 36 83460
