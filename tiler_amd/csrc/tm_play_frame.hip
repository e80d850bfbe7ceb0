// tm_play_frame.hip -- the player's kernel: one frame of a .gtm stream from its item records (tm_player.h: PlayRec), its launcher and the
// stage seam tm_stage_play_frame (the semantics are DESIGN.md section 16's "What is drawn", the design is section 19).
#include "tm_device.h"
#include "tm_player.h"

namespace tmx {
namespace {

// ---- the kernel: one frame.  A workgroup of 256 owns 16 consecutive items; an item is 64 pixels = 16 lanes x one 16-byte store.  Lanes are
// laid out row-major over the 16 items' common picture rows (8 rows x 32 lanes), so that the 32 lanes of a row store 512 contiguous bytes
// where the items lie in one tile row.  No LDS: a drawn lane reads 4 index bytes (one word) and 4 palette entries (the palettes stay in
// L2), a predicted lane gathers 4 pixels of the previous frame, each clamped on its own.
__global__ __launch_bounds__(256) void k_play_frame(const uint2 *__restrict__ recs, const uint8_t *__restrict__ intra, int64_t nintra,
                                                    const uint8_t *__restrict__ tiles, int64_t ntiles, const int32_t *__restrict__ palettes, int npal,
                                                    int pal_size, const uint32_t *prev, uint32_t *out, int tm_w, int tm_h) {
  const int t = threadIdx.x, row = t >> 5, half = t & 1;
  const int i = blockIdx.x * 16 + ((t & 31) >> 1);
  if (i >= tm_w * tm_h) return;
  const uint2 r = recs[i];
  const uint32_t a = r.x, pal = r.y & 0xffffu, fl = (r.y >> 16) & 0xffu;
  const int iy = i / tm_w, ix = i - iy * tm_w;
  const int W = tm_w * 8, H = tm_h * 8;
  const int y = iy * 8 + row, x = ix * 8 + half * 4;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (fl & REC_PRED) {
    if (prev) {  // (before frame 0 the picture is 0)
      const int ox = (int8_t)(a & 0xff), oy = (int8_t)((a >> 8) & 0xff);
      const uint32_t *src = prev + (int64_t)min(max(y + oy, 0), H - 1) * W;
      const int sx = x + ox;
      v.x = src[min(max(sx, 0), W - 1)];
      v.y = src[min(max(sx + 1, 0), W - 1)];
      v.z = src[min(max(sx + 2, 0), W - 1)];
      v.w = src[min(max(sx + 3, 0), W - 1)];
    }
  } else {
    const uint8_t *px = nullptr;
    if (fl & REC_INTRA) { if ((int64_t)a < nintra) px = intra + (int64_t)a * 64; }
    else if ((int64_t)a < ntiles) px = tiles + (int64_t)a * 64;
    if (px != nullptr && (int)pal < npal) {
      const int ty = (fl & 2) ? 7 - row : row, tx = (fl & 1) ? 4 - half * 4 : half * 4;  // DrawTile, tilingencoder.pas:3457-3503
      uint32_t w = *reinterpret_cast<const uint32_t *>(px + ty * 8 + tx);
      if (fl & 1) w = __builtin_bswap32(w);
      const int32_t *p = palettes + (int64_t)pal * pal_size;
      const int c0 = w & 0xff, c1 = (w >> 8) & 0xff, c2 = (w >> 16) & 0xff, c3 = w >> 24;
      v.x = c0 < pal_size ? swap_rb((uint32_t)p[c0]) : 0u;
      v.y = c1 < pal_size ? swap_rb((uint32_t)p[c1]) : 0u;
      v.z = c2 < pal_size ? swap_rb((uint32_t)p[c2]) : 0u;
      v.w = c3 < pal_size ? swap_rb((uint32_t)p[c3]) : 0u;
    }
  }
  *reinterpret_cast<uint4 *>(out + (int64_t)y * W + x) = v;
}

}  // namespace

int launch_play_frame(const void *recs, const void *intra, int64_t nintra, const void *tiles, int64_t ntiles, const void *palettes, int npal, int pal_size,
                      const void *prev, void *out, int tm_w, int tm_h, hipStream_t stream) {
  const int per = tm_w * tm_h;
  hipLaunchKernelGGL(k_play_frame, dim3((unsigned)((per + 15) / 16)), dim3(256), 0, stream, (const uint2 *)recs, (const uint8_t *)intra, nintra,
                     (const uint8_t *)tiles, ntiles, (const int32_t *)palettes, npal, pal_size, (const uint32_t *)prev, (uint32_t *)out, tm_w, tm_h);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" int tm_stage_play_frame(const void *records, const void *intra, int64_t nintra, const void *tiles, const void *palettes, const void *prev, void *out, int tm_w, int tm_h,
                        int pal_size, int64_t ntiles, int npal, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(records && out && tm_w > 0 && tm_h > 0 && tm_w <= 65535 && tm_h <= 65535 && pal_size >= 0 && ntiles >= 0 && npal >= 0 && nintra >= 0 && (intra || nintra == 0) &&
               (tiles || ntiles == 0) && (palettes || npal == 0), TM_E_INVAL, "play_frame: bad arguments");
  TM_CHECK((((uintptr_t)out | (uintptr_t)records) & 15) == 0 && (((uintptr_t)intra | (uintptr_t)tiles | (uintptr_t)palettes | (uintptr_t)prev) & 3) == 0, TM_E_INVAL,
           "play_frame: out and records must be 16-byte aligned, the other arrays 4-byte aligned");
  return launch_play_frame(records, intra, nintra, tiles, ntiles, palettes, npal, pal_size, prev, out, tm_w, tm_h, (hipStream_t)stream);
}
