// tm_features.hip -- the int16[192] features of tiles (A4 + A5) for gfx950: k_features_i16<SRC>, a tile at a time from every source, and
// k_features_tiles8, eight RGB tiles a wave.  tm_dct.h holds the arithmetic both share with the clustering's and the windows' kernels.
#include "tm_common.h"
#include "tm_dct.h"
#include "tm_internal.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// A4+A5: int16[192] features.  One wave per tile; lane = DCT position (v,u) and holds its 64-entry LUT row in
// registers; the 3x64 component planes live in LDS and are read as wave-wide broadcasts.
// SRC: 0 = RGB tiles, 1 = palette-index tiles through their palette, 2 = every 8x8 window of a frame buffer
// (PredictMotion.DoDCTs / Reconstruct.DoDCTs, tilingencoder.pas:1157-1182, 1437-1462: `tiles` is the buffer, pal_size its
// width in pixels, tile t = window at (t mod (width-7), t div (width-7))), 3 = every palette-index tile under every palette
// (row t = tile t div P under palette t mod P, P passed in use_lab: the vectors 1590-1591 recompute per query).
template <int SRC>
__global__ __launch_bounds__(256) void k_features_i16(const uint32_t *__restrict__ tiles, const uint8_t *__restrict__ pal_px,
                                                      const int32_t *__restrict__ pal_idx, const int32_t *__restrict__ palettes,
                                                      int pal_size, const uint8_t *__restrict__ mirror_flags, int64_t n,
                                                      int weighted, int use_lab, const float *__restrict__ lut,
                                                      const double *__restrict__ weights, const uint8_t *__restrict__ snake,
                                                      const float *__restrict__ srgb_lut, int16_t *__restrict__ out,
                                                      int *__restrict__ colmm /* null, or [384]: running min / max of the 192 output columns (atomics) */,
                                                      const double *__restrict__ cosd /* [8][8] the LUT's cosine factor, cos((x + 0.5) u pi / div) */, int plain) {
  __shared__ __attribute__((aligned(16))) double s_cpn[2][4][192];  // the tile's planes, widened once where they are made
  __shared__ __attribute__((aligned(16))) float s_lut[4096];    // FDCTLut as the reference holds it (Singles): the in-order sums read it
  __shared__ __attribute__((aligned(16))) double s_row[4][64];  // a wave's row transforms, [u][y]
  __shared__ int s_mm[4 * 384];                                 // at the very end: the waves' column ranges
  int mmn[3] = {INT_MAX, INT_MAX, INT_MAX}, mmx[3] = {INT_MIN, INT_MIN, INT_MIN};  // of this lane's three output columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < 1024; e += 256) reinterpret_cast<float4 *>(s_lut)[e] = reinterpret_cast<const float4 *>(lut)[e];
  const LaneDct first_look(cosd, lane);
  double w[3];
#pragma unroll
  for (int c = 0; c < 3; c++) w[c] = weights[c * 64 + lane];
  const int zz = snake[lane];
  const int64_t niter = (n + 3) / 4;
  int buf = 0;
  // a tile's pixel of this lane: the colour the reference's ConvertToCpnPixels would read
  auto fetch = [&](int64_t t) -> uint32_t {
    const int f = mirror_flags ? mirror_flags[t] : 0;
    const int y = lane >> 3, x = lane & 7;
    const int src = (((f & 2) ? 7 - y : y) << 3) | ((f & 1) ? 7 - x : x);  // ConvertToCpnPixels 3080-3085 / 3093-3098
    if (SRC == 1) return (uint32_t)palettes[(int64_t)pal_idx[t] * pal_size + pal_px[t * 64 + src]];
    if (SRC == 3) {
      const int64_t tile = t / use_lab;
      return (uint32_t)palettes[(t - tile * use_lab) * pal_size + pal_px[tile * 64 + src]];
    }
    if (SRC == 4) {  // row t = the (tile, palette) pair pairs[t] = tile << 32 | palette (all ones: a pad, black)
      const unsigned long long pr = reinterpret_cast<const unsigned long long *>(tiles)[t];
      return pr == ~0ull ? 0u : (uint32_t)palettes[(int64_t)(uint32_t)pr * pal_size + pal_px[(int64_t)(pr >> 32) * 64 + src]];
    }
    if (SRC == 2) {
      const int ww = pal_size - 7;
      const int64_t wy = t / ww, wx = t - wy * ww;
      return tiles[(wy + y) * pal_size + wx + x];  // CopyRGBPixels(ABackBuffer, x, AIndex), 879-887
    }
    return tiles[(pal_idx ? (int64_t)pal_idx[t] : t) * 64 + src];  // (SRC 0 with a row list: row t of the output is tile pal_idx[t])
  };
  // A wave works on its own tile and its own LDS rows: nothing here is shared between waves, so no barrier -- and the NEXT tile's
  // pixel (two or three dependent loads deep) is asked for before this tile's 192 dot products start, not after them
  uint32_t col = 0;
  if (blockIdx.x < niter && blockIdx.x * 4ll + wave < n) col = fetch(blockIdx.x * 4ll + wave);
  __syncthreads();  // s_lut is whole
  const float lnorm = lut_row_norm_up(s_lut, lane, lane);
  for (int64_t it = blockIdx.x; it < niter; it += gridDim.x, buf ^= 1) {
    const int64_t t_out = it * 4 + wave;
    const bool valid = t_out < n;
    float mine[3] = {0.0f, 0.0f, 0.0f};  // this lane's pixel, per plane
    if (valid) {
      float yy, uu, vv;
      if (use_lab && SRC != 3 && SRC != 4)
        rgb_to_lab_det(col & 0xff, (col >> 8) & 0xff, (col >> 16) & 0xff, srgb_lut, yy, uu, vv);
      else
        rgb_to_yuv(col & 0xff, (col >> 8) & 0xff, (col >> 16) & 0xff, yy, uu, vv);
      s_cpn[buf][wave][lane] = (double)yy;
      s_cpn[buf][wave][64 + lane] = (double)uu;
      s_cpn[buf][wave][128 + lane] = (double)vv;
      mine[0] = yy; mine[1] = uu; mine[2] = vv;
    }
    {
      const int64_t tn = (it + gridDim.x) * 4 + wave;
      if (it + gridDim.x < niter && tn < n) col = fetch(tn);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the wave's LDS operations are in order: its reads below see its writes above)
    if (valid) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        // The reference's sum (ref_order_sum) costs 130 vector instructions per coefficient and plane: 64 Single products, Single sums
        // of pairs, 32 conversions, 34 double additions, in DCTInner_asm's order.  What is stored is only Round(z w).  So z is first
        // computed the cheap way -- LaneDct: the LUT is cos x cos x ratio -- together with a bound on how far the reference's z can lie
        // from it:  |z_ref - z_fast| <= sum|p_k| (2^-23 + 2^-24)(1 + 2^-20),  p_k = pixel x LUT entry (every product and every pair
        // sum of the reference rounds to Single once: 2 x 2^-24 relative; the LUT's Singles are within 2^-24 of the doubles they were
        // rounded from, which are this path's cos x cos x ratio to 2^-52; the double-precision steps of both paths stay below 2^-47),
        // and sum|p_k| <= |pixels| |LUT row| (Euclidean norms).  When z_fast w is farther than that (times |w|) from every half-integer, both
        // round to the same integer.  Otherwise -- a few coefficients per thousand -- the coefficient is summed the reference's way, by
        // the whole wave (lane k = product k).
        double t = 0.0;
        bool doubtful = true;
        int o_fast = 0;
        if (!plain) {
          const float sa = lnorm * (__builtin_amdgcn_sqrtf(sum64_dpp(mine[c] * mine[c])) * 1.00001f);  // >= sum |pixel x LUT entry| (Cauchy-Schwarz; lnorm = the LUT row's norm, rounded up; the hardware's root is good to 1 ulp)
          const double z = first_look(&s_cpn[buf][wave][c * 64], s_row[wave], lane);
          t = weighted ? z * w[c] : z;
          doubtful = !first_look_rounds(t, sa * slack_per_sum(weighted, w[c]), o_fast);
        }
        for (unsigned long long m = __builtin_amdgcn_ballot_w64(doubtful); m; m &= m - 1) {
          const int coef = __builtin_ctzll(m);
          const double z = ref_order_sum(mine[c], s_lut[coef * 64 + lane]);
          if (lane == coef) t = weighted ? __dmul_rn(z, w[c]) : z;
        }
        const int16_t o = !doubtful ? (int16_t)o_fast : round_i16(t);
        out[t_out * 192 + c * 64 + zz] = o;
        mmn[c] = min(mmn[c], (int)o);
        mmx[c] = max(mmx[c], (int)o);
      }
    }
  }
  if (colmm) fold_colmm(s_mm, zz, mmn, mmx, colmm);
}

// ---------------------------------------------------------------------------------------------------------------
// A4 + A5 for RGB tiles, plain (non-"special") DCT modes: k_features_i16<0>'s work with a lane per (tile, row) / (tile, u) instead of a lane
// per coefficient -- a wave takes EIGHT tiles.  A lane converts its row's eight pixels, takes them through the 8-point fast DCT (35 double-precision
// operations for the row's eight outputs), the outputs change hands through LDS (transposed), and the lane of (tile, u) takes the eight
// row transforms R[u][y] through the same DCT down the column: 70 operations a lane for 8 x 8 coefficients where a lane per coefficient spends
// sixteen multiply-adds on one.  Weight, the first look's verdict, the in-doubt coefficients in the reference's order by the whole wave,
// exactly as in k_features_i16 and k_window_dcts; a plane's coefficients leave through LDS as 128-byte lines.  (The first look's z may be
// summed in any order: its bound has nine decimal orders of room.)
constexpr int F8_TP = 72;  // pitch (doubles) of a tile's transposed row transforms: eight tiles' lanes then cover the banks evenly
__global__ __launch_bounds__(256) void k_features_tiles8(const uint32_t *__restrict__ tiles, const int32_t *__restrict__ rows, const uint8_t *__restrict__ mirror_flags, int64_t n,
                                                         int weighted, int use_lab, const float *__restrict__ lut, const double *__restrict__ weights,
                                                         const uint8_t *__restrict__ snake, const float *__restrict__ srgb_lut, int16_t *__restrict__ out,
                                                         int *__restrict__ colmm /* null, or [384]: running min / max of the 192 output columns (atomics) */, int plain) {
  __shared__ double s_cw[3][64];
  __shared__ float s_kw[3][64];
  __shared__ int s_zz[64];
  __shared__ __attribute__((aligned(16))) float s_px[4][3][8][64];   // the planes as Singles, for the in-order sums; at the very end: the columns' ranges
  __shared__ __attribute__((aligned(16))) double s_t[4][8 * F8_TP];   // a wave's eight tiles, one plane: row transforms [tile][u][y]
  __shared__ __attribute__((aligned(16))) int16_t s_out[4][8 * 64];   // ... and its coefficients in output order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane >> 3, y = lane & 7, u = y;
  if (tid < 64) fill_coef_factors(tid, lut, weighted, weights, snake, s_cw, s_kw, s_zz);
  __syncthreads();
  int zzr[8];
#pragma unroll
  for (int v = 0; v < 8; v++) zzr[v] = j * 64 + s_zz[v * 8 + u];  // the place of coefficient (u, v) in the wave's run
  int mmn[3] = {INT_MAX, INT_MAX, INT_MAX}, mmx[3] = {INT_MIN, INT_MIN, INT_MIN};  // of output column `lane` of each plane
  int16_t *const so = s_out[wave];
  double *const st = s_t[wave];
  const int64_t ngroups = (n + 7) >> 3;
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < ngroups; g += (int64_t)gridDim.x * 4) {
    const int64_t t_out = g * 8 + j;
    const bool valid = t_out < n;
    float pl[3][8];
    {  // this lane's row of its tile, as ConvertToCpnPixels reads it (mirrors 3080-3085 / 3093-3098)
      const int64_t tile = valid ? (rows ? (int64_t)rows[t_out] : t_out) : (rows ? (int64_t)rows[n - 1] : n - 1);
      const int f = (valid && mirror_flags) ? mirror_flags[t_out] : 0;
      const uint4 *src = reinterpret_cast<const uint4 *>(tiles + tile * 64 + ((f & 2) ? 7 - y : y) * 8);
      const uint4 a = src[0], b = src[1];
      uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      if (f & 1) {
#pragma unroll
        for (int x = 0; x < 4; x++) { const uint32_t tmp = px[x]; px[x] = px[7 - x]; px[7 - x] = tmp; }
      }
#pragma unroll
      for (int x = 0; x < 8; x++) {
        if (use_lab) rgb_to_lab_det(px[x] & 0xff, (px[x] >> 8) & 0xff, (px[x] >> 16) & 0xff, srgb_lut, pl[0][x], pl[1][x], pl[2][x]);
        else rgb_to_yuv(px[x] & 0xff, (px[x] >> 8) & 0xff, (px[x] >> 16) & 0xff, pl[0][x], pl[1][x], pl[2][x]);
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float4 *dst = reinterpret_cast<float4 *>(&s_px[wave][c][j][y * 8]);
        dst[0] = make_float4(pl[c][0], pl[c][1], pl[c][2], pl[c][3]);
        dst[1] = make_float4(pl[c][4], pl[c][5], pl[c][6], pl[c][7]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {  // (unrolled: the planes' registers and ranges are then addressed statically -- no scratch)
      unsigned dmask = 0;  // bit v: coefficient (u, v) of tile j is in doubt
      if (!plain) {
        float sq = 0.0f;
        double p[8], r[8];
#pragma unroll
        for (int x = 0; x < 8; x++) { sq = fmaf(pl[c][x], pl[c][x], sq); p[x] = (double)pl[c][x]; }
        const float root = __builtin_amdgcn_sqrtf(sum8_dpp(sq)) * 1.00001f;  // of the tile's sum of squares; x the LUT row's norm >= sum |pixel x LUT entry| (Cauchy-Schwarz)
        dct8(p, r);
#pragma unroll
        for (int uu = 0; uu < 8; uu++) st[j * F8_TP + uu * 8 + y] = r[uu];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (a wave's LDS operations are in order)
        {
          const double2 *rp = reinterpret_cast<const double2 *>(st + j * F8_TP + u * 8);
          const double2 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
          p[0] = r0.x; p[1] = r0.y; p[2] = r1.x; p[3] = r1.y; p[4] = r2.x; p[5] = r2.y; p[6] = r3.x; p[7] = r3.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next plane's row transforms land after these reads)
        double z[8];
        dct8(p, z);
#pragma unroll
        for (int v = 0; v < 8; v++) {
          const double t = z[v] * s_cw[c][v * 8 + u];  // cDCTUVRatio and the weight in one factor
          int o;
          const bool ok = first_look_rounds(t, s_kw[c][v * 8 + u] * root, o);
          so[zzr[v]] = (int16_t)o;
          dmask |= ok ? 0u : (1u << v);
        }
        if (!valid) dmask = 0;
      } else dmask = valid ? 0xffu : 0u;
      sum_in_doubt(dmask, lane, [&](int sj) { return s_px[wave][c][sj][lane]; }, lut, weighted, weights + c * 64, s_zz, so);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (colmm) {  // output column `lane` of this plane over the run's tiles
#pragma unroll
        for (int jj = 0; jj < 8; jj++)
          if (g * 8 + jj < n) { const int v = so[jj * 64 + lane]; mmn[c] = min(mmn[c], v); mmx[c] = max(mmx[c], v); }
      }
      if (valid) *reinterpret_cast<uint4 *>(out + t_out * 192 + c * 64 + u * 8) = *reinterpret_cast<const uint4 *>(so + j * 64 + u * 8);  // lane = (tile, 16-byte piece)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next plane's coefficients land after these reads)
    }
  }
  if (colmm) fold_colmm(reinterpret_cast<int *>(&s_px[0][0][0][0]), lane, mmn, mmx, colmm);
}

// ---------------------------------------------------------------------------------------------------------------
// The one launch of k_features_i16<SRC>: the tables, TM_FEATURES_PLAIN and the grid are looked up here; a caller names its source (the
// kernel's head says which pointers a SRC reads), the rows, the mode and where the features and, optionally, the columns' ranges go.
struct I16Source { const void *tiles, *pal_px, *pal_idx, *palettes; int pal_size; const void *mirror_flags; };
template <int SRC>
static int launch_features_i16(const I16Source &s, int64_t n, int mode, int use_lab, void *out, void *colmm, hipStream_t stream) {
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  if (n <= 0) return TM_OK;
  hipLaunchKernelGGL(k_features_i16<SRC>, dim3(grid_for(n, 4)), dim3(256), 0, stream, (const uint32_t *)s.tiles, (const uint8_t *)s.pal_px, (const int32_t *)s.pal_idx,
                     (const int32_t *)s.palettes, s.pal_size, (const uint8_t *)s.mirror_flags, n, mode_weighted(mode) ? 1 : 0, use_lab, tab->dct_lut_f32[mode_special(mode)],
                     tab->weights, tab->snake, tab->srgb_lut, (int16_t *)out, (int *)colmm, tab->dct_cos_f64[mode_special(mode)], knobs().features_plain ? 1 : 0);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// RGB tiles (rows: output row i = tile rows[i]): k_features_tiles8 where it applies (the plain DCT's cosines); TM_FEATURES_BY_TILE=1: always
// the tile-at-a-time kernel (tests, A/B)
static int features_rgb(const void *tiles, const void *rows, const void *mirror_flags, int64_t n, int mode, int use_lab, void *out, void *colmm, hipStream_t stream) {
  if (mode_special(mode) || knobs().features_by_tile) return launch_features_i16<0>({tiles, nullptr, rows, nullptr, 0, mirror_flags}, n, mode, use_lab, out, colmm, stream);
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  if (n <= 0) return TM_OK;
  const int64_t groups = (n + 7) / 8;
  hipLaunchKernelGGL(k_features_tiles8, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, 256 * 6))), dim3(256), 0, stream, (const uint32_t *)tiles,
                     (const int32_t *)rows, (const uint8_t *)mirror_flags, n, mode_weighted(mode) ? 1 : 0, use_lab, tab->dct_lut_f32[0], tab->weights, tab->snake, tab->srgb_lut,
                     (int16_t *)out, (int *)colmm, knobs().features_plain ? 1 : 0);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_features_rgb(const void *tiles, int64_t n, const void *mirror_flags, int mode, int use_lab, void *out,
                        hipStream_t stream) {
  TM_CHECK(mode != TM_PVS_WAVELETS, TM_E_UNSUPPORTED, "wavelet features on int16 vectors are unimplemented in the reference too (tilingencoder.pas:3111)");
  TM_CHECK(mode >= 0 && mode <= 4, TM_E_INVAL, "bad TPsyVisMode %d", mode);
  return features_rgb(tiles, nullptr, mirror_flags, n, mode, use_lab, out, nullptr, stream);
}

// the same for a list of rows: output row i = features of tile rows[i] (Reconstruct's queries are the DISTINCT frame tiles)
int launch_features_rgb_rows(const void *tiles, const void *rows, int64_t n, int mode, int use_lab, void *out, hipStream_t stream, void *colmm) {
  TM_CHECK(mode != TM_PVS_WAVELETS && mode >= 0 && mode <= 4, TM_E_INVAL, "bad TPsyVisMode %d", mode);
  return features_rgb(tiles, rows, nullptr, n, mode, use_lab, out, colmm, stream);
}

int launch_features_pal(const void *pal_px, const void *pal_idx, int64_t n, const void *palettes, int pal_size, int mode,
                        void *out, hipStream_t stream) {
  TM_CHECK(mode != TM_PVS_WAVELETS && mode >= 0 && mode <= 4, TM_E_INVAL, "bad TPsyVisMode %d", mode);
  TM_CHECK(pal_size >= 1 && pal_size <= 256, TM_E_INVAL, "bad palette size %d", pal_size);
  return launch_features_i16<1>({nullptr, pal_px, pal_idx, palettes, pal_size, nullptr}, n, mode, 0, out, nullptr, stream);
}

int launch_features_pairs(const void *pal_px, const void *pairs, int64_t n, const void *palettes, int pal_size, void *out, hipStream_t stream) {
  return launch_features_i16<4>({pairs, pal_px, nullptr, palettes, pal_size, nullptr}, n, TM_PVS_WEIGHTED_DCT, 0, out, nullptr, stream);
}

int launch_features_table(const void *pal_px, int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, hipStream_t stream) {
  TM_CHECK(pal_size >= 1 && pal_size <= 256 && npal >= 1, TM_E_INVAL, "bad palette shape %d x %d", npal, pal_size);
  return launch_features_i16<3>({nullptr, pal_px, nullptr, palettes, pal_size, nullptr}, ntiles * npal, TM_PVS_WEIGHTED_DCT, npal, out, nullptr, stream);
}

int launch_features_windows_by_tile(const void *fb, int w, int h, void *out, hipStream_t stream) {
  return launch_features_i16<2>({fb, nullptr, nullptr, nullptr, w, nullptr}, (int64_t)(w - 7) * (h - 7), TM_PVS_WEIGHTED_DCT, 0, out, nullptr, stream);
}

}  // namespace tmx
