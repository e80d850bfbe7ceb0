#!/bin/bash
# tests/c/rgb_clip_host.c and the host code it calls (tm_rgb_in.hip, tm_scale.hip, tm_resample.hip and what those link to) under
# AddressSanitizer and UndefinedBehaviorSanitizer, as one stand-alone program; CPU only, no device is touched.
# usage: tools/asan_rgb_clip.sh [BUILD_DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CLANG="${CLANG:-/opt/rocm/llvm/bin/clang}"
S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
mkdir -p "$OUT"
"$CLANG" -O1 -g $S -Wall -I"$ROOT/include" -c "$ROOT/tests/c/rgb_clip_host.c" -o "$OUT/rgb_clip_host.o"
objs=("$OUT/rgb_clip_host.o")
# tm_input_probe (scaled_size) brings the probes of the file inputs with it: the .gtm parser, the PNG reader, the YUV layouts
for f in tm_rgb_in tm_scale tm_resample tm_tables tm_input_probe tm_yuv_in tm_png tm_player_parse tm_gtm tm_lzma; do
  "$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -c "$ROOT/tiler_amd/csrc/$f.hip" -o "$OUT/$f.o" &
  objs+=("$OUT/$f.o")
done
wait
"$HIPCC" --offload-arch=gfx950 $S "${objs[@]}" -o "$OUT/rgb_clip_host"
"$OUT/rgb_clip_host"
