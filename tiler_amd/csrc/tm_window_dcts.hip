// tm_window_dcts.hip -- the sliding-window features of motion prediction for gfx950: k_window_dcts<PACK>, every 8 x 8 window of a frame
// buffer by strips, as int16 rows or straight in the motion search's matrix layout.  tm_dct.h holds the arithmetic it shares with the tiles' kernels.
#include "tm_common.h"
#include "tm_dct.h"
#include "tm_internal.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// Every 8 x 8 window of a frame buffer (PredictMotion.DoDCTs / Reconstruct.DoDCTs, tilingencoder.pas:1157-1182, 1437-1462), weighted DCT on
// YUV: what k_features_i16<2> computes a window at a time -- 64 colour conversions, eight row transforms and a column transform per window
// and plane -- shares nearly all of it between windows: a pixel is converted once per strip (not 64 times), a row's transform at a
// horizontal position serves the eight windows that contain it (not one), and only the column transform and the rounding are a window's
// own.  The reference's order of summation shares nothing (DCTInner_asm, fixed order in Single and double), but only Round(z w) is stored:
// z the cheap way first, the reference's order when the rounding is in doubt, exactly as in k_features_i16 (same bound, same fallback).
// A workgroup takes strips of WD_RY x WD_CX windows: (1) the strip's pixels -> three planes of Singles in LDS; per plane: (2) the row
// transform of every (row, horizontal position) by an 8-point fast DCT in double (35 operations for eight outputs: any order of summation
// serves, the bound on |z_ref - z_fast| has nine decimal orders of room for it) and the row's sum of squares, (3) the windows' sums of
// squares, (4) a wave per window, lane = coefficient (u, v): eight multiply-adds down the column, weight, slack, Round.
constexpr int WD_RY = 8, WD_CX = 32, WD_PW = WD_CX + 8;  // window rows and columns of a strip; pitch of a plane row (WD_CX + 7 pixels)
// PACK: the coefficients leave in the motion search's matrix layout (tm_internal.h: launch_window_dcts_packed) instead of as int16 rows.  A strip's
// 32 columns are one block of that layout; lane (window j, piece u) holds block b = 8 c + u of the reference's 24 blocks of eight coefficients
// (CompareEuclideanDCTPtr_asm, utils.pas:559-725: two halves of twelve) and knows where its digits go: plain blocks (0-4, 7-11 of a half) to matrix
// block 10 half + (0..9), block 6 joined by block 5 (its lane neighbour) to matrix block 20 + half as b5 + b6, block 5's lane fills the padding
// (matrix blocks 22 / 23) with zeros; block 7 of the first half is stored raw as well; the squares of what went into the matrix are summed per window
// over the three planes.  Low digit = the int16's low byte, signed; high digit = its high byte + the low byte's top bit.
typedef short wd_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short wd_u16x2 __attribute__((ext_vector_type(2)));
template <bool PACK>
__global__ __launch_bounds__(256) void k_window_dcts(const uint32_t *__restrict__ fb, int w, int h, const float *__restrict__ lut, const double *__restrict__ weights,
                                                     const uint8_t *__restrict__ snake, const double *__restrict__ cosd, int16_t *__restrict__ out, int plain,
                                                     const int *__restrict__ only_if, uint8_t *__restrict__ packed, const int16_t *__restrict__ cur, int ntiles,
                                                     int *__restrict__ flag) {
  if (only_if && !*only_if) return;  // (the fallback's launch: the matrix search took this frame)
  __shared__ uint32_t s_nrm[PACK ? WD_RY : 1][WD_CX];  // PACK: the windows' sums of squares of what the matrix holds, over the planes
  bool bad = false;
  if constexpr (PACK) {  // the tile side's range check (its digits are made inside the search kernel)
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < (int64_t)ntiles * 24; i += (int64_t)gridDim.x * 256) {
      const int blk = (int)(i % 24) % 12;
      if (blk == 5) continue;  // never enters on the tile side
      const int lim = blk == 6 ? MM_LIMIT6 : MM_LIMIT;
      const uint4 v = reinterpret_cast<const uint4 *>(cur)[i];
      const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int lo = (int16_t)(wv[k] & 0xffff), hi = (int16_t)(wv[k] >> 16);
        bad |= lo > lim || lo < -lim || hi > lim || hi < -lim;
      }
    }
  }
  __shared__ float s_pl[3][WD_RY + 7][WD_PW];                                     // the strip's planes (Singles, as ConvertToCpnPixels leaves them)
  __shared__ __attribute__((aligned(16))) double s_r[WD_RY + 7][WD_CX][8];         // one plane's row transforms [row][horizontal position][u]
  __shared__ float s_rs[WD_RY + 7][WD_CX];                                          // ... and the rows' sums of squares
  __shared__ float s_ws[WD_RY][WD_CX];                                              // the windows' sums of squares
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = w - 7, wh = h - 7;
  const int nsx = (ww + WD_CX - 1) / WD_CX, nsy = (wh + WD_RY - 1) / WD_RY;
  // per coefficient cf = v * 8 + u: ratio x weight, the slack's factor, the zig-zag place (fill_coef_factors)
  // (read from LDS per coefficient: eight doubles, sixteen Singles and eight indices per lane in registers instead cost a wave per SIMD: 0.35 against 0.32 ms)
  __shared__ double s_cw[3][64];
  __shared__ float s_kw[3][64];
  __shared__ int s_zz[64];
  __shared__ __attribute__((aligned(16))) int16_t s_out[4][8 * 64];  // a wave's run of eight windows, one plane
  if (tid < 64) fill_coef_factors(tid, lut, true, weights, snake, s_cw, s_kw, s_zz);
  (void)cosd;
  for (int strip = blockIdx.x; strip < nsx * nsy; strip += gridDim.x) {
    const int sy = strip / nsx, sx = strip - sy * nsx;
    const int y0 = sy * WD_RY, x0 = sx * WD_CX;
    __syncthreads();  // the strip before is done with the planes
    for (int e = tid; e < (WD_RY + 7) * (WD_CX + 7); e += 256) {  // pixels beyond the frame repeat its edge: they only feed windows that are not stored
      const int py = e / (WD_CX + 7), px = e - py * (WD_CX + 7);
      const uint32_t col = fb[(int64_t)min(y0 + py, h - 1) * w + min(x0 + px, w - 1)];  // CopyRGBPixels(ABackBuffer, x, AIndex), 879-887
      float yy, uu, vv;
      rgb_to_yuv(col & 0xff, (col >> 8) & 0xff, (col >> 16) & 0xff, yy, uu, vv);
      s_pl[0][py][px] = yy; s_pl[1][py][px] = uu; s_pl[2][py][px] = vv;
    }
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
      __syncthreads();  // the planes are whole / the plane before is done with s_r
      if (!plain)
      for (int e = tid; e < (WD_RY + 7) * WD_CX; e += 256) {
        const int ry = e / WD_CX, rx = e - ry * WD_CX;
        const float *pp = &s_pl[c][ry][rx];
        float f[8];
        double p[8], r[8];
#pragma unroll
        for (int x = 0; x < 8; x++) { f[x] = pp[x]; p[x] = (double)f[x]; }
        s_rs[ry][rx] = ((f[0] * f[0] + f[1] * f[1]) + (f[2] * f[2] + f[3] * f[3])) + ((f[4] * f[4] + f[5] * f[5]) + (f[6] * f[6] + f[7] * f[7]));
        dct8(p, r);
#pragma unroll
        for (int uu = 0; uu < 8; uu++) s_r[ry][rx][uu] = r[uu];
      }
      __syncthreads();
      if (!plain) {
        const int wy = tid / WD_CX, wx = tid - wy * WD_CX;  // 256 threads = WD_RY x WD_CX windows
        float sq = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k++) sq += s_rs[wy + k][wx];
        s_ws[wy][wx] = sq;
      }
      __syncthreads();
      // (4) a wave per run of EIGHT consecutive windows of a strip row, lane = (window j, u): the lane's eight row transforms R[wy .. wy + 7][wx][u] go
      // through the same 8-point fast DCT down the column -- 35 double-precision operations for its eight coefficients v = 0..7 where a lane per
      // coefficient spent eight multiply-adds on ONE -- then weight, verdict, and the run's 8 x 64 coefficients of this plane leave through LDS as
      // eight 128-byte lines (a lane per 16 bytes; a lane per coefficient stored two bytes at a time).
      // (the lane's eight factors of this plane, and its zig-zag places, once per plane instead of once per coefficient)
      double cwr[8];
      float kwr[8];
      int zzr[8];
#pragma unroll
      for (int v = 0; v < 8; v++) { cwr[v] = s_cw[c][v * 8 + (lane & 7)]; kwr[v] = s_kw[c][v * 8 + (lane & 7)]; zzr[v] = (lane >> 3) * 64 + s_zz[v * 8 + (lane & 7)]; }  // (zzr: the place in the wave's run)
      // PACK: this lane's block of eight coefficients in this plane, where it goes, its range (see the kernel's head)
      const int pk_b = c * 8 + (lane & 7), pk_hf = pk_b >= 12 ? 1 : 0, pk_bi = pk_b - pk_hf * 12;
      const int pk_mb = pk_bi < 5 ? pk_hf * 10 + pk_bi : pk_bi == 5 ? 22 + pk_hf : pk_bi == 6 ? 20 + pk_hf : pk_hf * 10 + pk_bi - 2;
      const uint32_t pk_lim = ((pk_bi == 5 || pk_bi == 6) ? MM_LIMIT6 : MM_LIMIT) * 0x00010001u;
      const uint32_t keep_own = pk_bi == 5 ? 0u : 0xffffffffu, keep_left = pk_bi == 6 ? 0xffffffffu : 0u;
      const unsigned piece0 = (unsigned)(((pk_mb >> 2) * 64 + ((pk_mb >> 1) & 1) * 32 + (lane >> 3)) * 16 + (pk_mb & 1) * 8);
      for (int gi = wave; gi < WD_RY * (WD_CX / 8); gi += 4) {
        const int wy = gi / (WD_CX / 8), wx0 = (gi - wy * (WD_CX / 8)) * 8;
        if (y0 + wy >= wh || x0 + wx0 >= ww) continue;  // (uniform in the wave)
        const int j = lane >> 3, u = lane & 7, wx = wx0 + j;
        unsigned dmask = 0;  // bit v: coefficient (u, v) of window j is in doubt
        int16_t *so = s_out[wave];
        if (!plain) {
          const double *rp = &s_r[wy][wx][u];
          double p[8], z[8];
#pragma unroll
          for (int k = 0; k < 8; k++) p[k] = rp[k * WD_CX * 8];
          dct8(p, z);
          const float root = __builtin_amdgcn_sqrtf(s_ws[wy][wx]) * 1.00001f;
#pragma unroll
          for (int v = 0; v < 8; v++) {
            const double t = z[v] * cwr[v];  // cDCTUVRatio and the weight in one factor
            int o;
            const bool ok = first_look_rounds(t, kwr[v] * root, o);  // root x the LUT row's norm >= sum |pixel x LUT entry| (Cauchy-Schwarz)
            so[zzr[v]] = (int16_t)o;
            dmask |= ok ? 0u : (1u << v);
          }
        } else dmask = 0xffu;
        sum_in_doubt(dmask, lane, [&](int sj) { return s_pl[c][wy + (lane >> 3)][wx0 + sj + (lane & 7)]; }, lut, true, weights + c * 64, s_zz, so);  // (this lane's pixel of window sj)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (a wave's LDS operations are in order: its reads below see its writes above)
        if constexpr (!PACK) {
          if (x0 + wx < ww) {  // lane = (window j, 16-byte piece u) of the plane's 128 bytes
            const int64_t t_out = (int64_t)(y0 + wy) * ww + x0 + wx;
            *reinterpret_cast<uint4 *>(out + t_out * 192 + c * 64 + u * 8) = *reinterpret_cast<const uint4 *>(so + j * 64 + u * 8);
          }
        } else {
          const bool live = x0 + wx < ww;  // (a window position past the row's end is all zeros, as k_mo_pack_win leaves it)
          const uint4 raw = live ? *reinterpret_cast<const uint4 *>(so + j * 64 + u * 8) : make_uint4(0, 0, 0, 0);
          uint32_t x[4] = {raw.x, raw.y, raw.z, raw.w};
          // range: |v| <= lim  <=>  (uint16)(v + lim) <= 2 lim
          wd_u16x2 rg = __builtin_bit_cast(wd_u16x2, x[0]) + __builtin_bit_cast(wd_u16x2, pk_lim);
#pragma unroll
          for (int k = 1; k < 4; k++) rg = __builtin_elementwise_max(rg, __builtin_bit_cast(wd_u16x2, x[k]) + __builtin_bit_cast(wd_u16x2, pk_lim));
          bad |= __builtin_bit_cast(uint32_t, __builtin_elementwise_max(rg, __builtin_bit_cast(wd_u16x2, 2u * pk_lim))) != 2u * pk_lim;
          uint32_t sq = 0, hd[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x[k], 0x111, 0xf, 0xf, true);  // the lane before: block 5 beside block 6
            const uint32_t v = __builtin_bit_cast(uint32_t, __builtin_bit_cast(wd_u16x2, x[k] & keep_own) + __builtin_bit_cast(wd_u16x2, left & keep_left));
            sq = (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(wd_s16x2, v), __builtin_bit_cast(wd_s16x2, v), (int)sq, false);
            x[k] = v;
            hd[k] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(wd_u16x2, v) + __builtin_bit_cast(wd_u16x2, 0x00800080u));  // high digit = high byte of v + 128
          }
          uint8_t *obase = packed + ((int64_t)(y0 + wy) * nsx + sx) * MM_BLK_BYTES;  // (uniform in the wave)
          const unsigned piece = piece0 + (unsigned)wx0 * 16u;
          *reinterpret_cast<uint2 *>(obase + piece) = make_uint2(__builtin_amdgcn_perm(x[1], x[0], 0x06040200u), __builtin_amdgcn_perm(x[3], x[2], 0x06040200u));
          *reinterpret_cast<uint2 *>(obase + MM_CH * 1024 + piece) = make_uint2(__builtin_amdgcn_perm(hd[1], hd[0], 0x07050301u), __builtin_amdgcn_perm(hd[3], hd[2], 0x07050301u));
          if (pk_b == 7) *reinterpret_cast<uint4 *>(obase + MM_QUIRK + wx * 16) = raw;  // block 7 of the first half, raw: its pair sums are re-squared on the VALU
          sq = sum8_dpp(sq);  // over the window's eight lanes
          if (u == 0) {  // (the same wave has this run in every plane)
            const uint32_t tot = (c == 0 ? 0u : s_nrm[wy][wx]) + sq;
            if (c < 2) s_nrm[wy][wx] = tot;
            else reinterpret_cast<uint32_t *>(obase + MM_NORM)[wx] = tot;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next run's coefficients land after these reads)
      }
    }
  }
  if constexpr (PACK) { if (bad) atomicOr(flag, 1); }
}

int launch_window_dcts_packed(const void *fb, int w, int h, const void *cur, int ntiles, void *packed, int *flag, hipStream_t stream) {
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  TM_CHECK(w >= 8 && h >= 8, TM_E_INVAL, "frame buffer %dx%d smaller than a tile", w, h);
  const int strips = ((w - 7 + WD_CX - 1) / WD_CX) * ((h - 7 + WD_RY - 1) / WD_RY);
  hipLaunchKernelGGL(k_window_dcts<true>, dim3(std::min(strips, 256 * 4)), dim3(256), 0, stream, (const uint32_t *)fb, w, h, tab->dct_lut_f32[mode_special(TM_PVS_WEIGHTED_DCT)],
                     tab->weights, tab->snake, tab->dct_cos_f64[mode_special(TM_PVS_WEIGHTED_DCT)], (int16_t *)nullptr, knobs().features_plain ? 1 : 0, (const int *)nullptr,
                     (uint8_t *)packed, (const int16_t *)cur, ntiles, flag);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_window_dcts(const void *fb, int w, int h, void *out, hipStream_t stream, const int *only_if) {
  TM_CHECK(w >= 8 && h >= 8, TM_E_INVAL, "frame buffer %dx%d smaller than a tile", w, h);
  if (!knobs().window_dcts_by_tile) {
    const DeviceTables *tab;
    TM_TRY(get_tables(&tab));
    const int strips = ((w - 7 + WD_CX - 1) / WD_CX) * ((h - 7 + WD_RY - 1) / WD_RY);
    hipLaunchKernelGGL(k_window_dcts<false>, dim3(std::min(strips, 256 * 4)), dim3(256), 0, stream, (const uint32_t *)fb, w, h, tab->dct_lut_f32[mode_special(TM_PVS_WEIGHTED_DCT)],
                       tab->weights, tab->snake, tab->dct_cos_f64[mode_special(TM_PVS_WEIGHTED_DCT)], (int16_t *)out, knobs().features_plain ? 1 : 0, only_if, (uint8_t *)nullptr,
                       (const int16_t *)nullptr, 0, (int *)nullptr);
    TM_HIP(hipGetLastError());
    return TM_OK;
  }
  TM_CHECK(only_if == nullptr, TM_E_INVAL, "the window-at-a-time kernel has no conditional form");  // (launch_motion_search_fb takes the two-pass form under TM_WINDOW_DCTS_BY_TILE)
  return launch_features_windows_by_tile(fb, w, h, out, stream);
}

}  // namespace tmx
