// tm_load.hip -- the load stage (A1-A3) for gfx950: tiles, mirror flags and Lab means of the frames (k_load_tiles), the Pearson sums of
// consecutive frames (k_pearson_frames), RGBToLAB on its own (k_rgb_to_lab).
//
// Bit-exactness rules (DESIGN.md "Arithmetic"): every floating-point step is a single IEEE +,-,*,/ issued through
// the __f*_rn / __d*_rn intrinsics (never contracted into FMA), in the order the reference's code performs it
// (RGBToYUV, utils.pas:478-490; RGBToLAB 374-410).  Transcendentals are replaced by host
// built tables (sRGB gamma, cosines) or a +,-,*,/-only Newton cube root, so CPU and GPU agree to the bit.
#include "tm_common.h"
#include "tm_device.h"
#include "tm_internal.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// A1+A2+A3: one wave per tile, one lane per pixel; a wave works through LT_BATCH tiles, then 3 * LT_BATCH of its lanes add up the Lab
// planes -- each sum is 64 Single additions in raster order (1349-1362), a dependent chain that would hold a whole wave per tile.
// LoadFromImage (tilingencoder.pas:1293-1320) -> PrepareInterFrameData (1329-1367) -> mirror heuristics
// (4865-4878) + H/V flip (1393-1411).
#ifndef TM_LT_BATCH
#define TM_LT_BATCH 8  // tiles a wave converts before 3 x that many of its lanes add up the Lab planes (LDS: 780 bytes per tile and wave; measured: 4-6 1.80-1.85 ms, 8 1.78, 12 1.93, 16 2.19, 20 2.65 -- the waves a CU holds matter more than the lanes the sums use)
#endif
constexpr int LT_BATCH = TM_LT_BATCH, LT_TILE = 195, LT_PLANE = 65;  // strides in floats: lane (tile, plane) of the summing phase reads bank 3 * tile + plane
__global__ __launch_bounds__(256) void k_load_tiles(const uint32_t *__restrict__ frames, int nframes, int img_w, int img_h,
                                                    int tm_w, int tm_h, const float *__restrict__ srgb_lut,
                                                    uint32_t *__restrict__ tiles, uint8_t *__restrict__ flags,
                                                    float *__restrict__ lab_means) {
  __shared__ float s_lab[4][LT_BATCH * LT_TILE];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: the tile arithmetic below stays on the scalar unit)
  const int64_t tiles_per_frame = (int64_t)tm_w * tm_h;
  const int64_t total = tiles_per_frame * nframes;
  const int64_t nbatch = (total + 4 * LT_BATCH - 1) / (4 * LT_BATCH);
  float *lab = s_lab[wave];  // a wave only touches its own part: no workgroup barrier
  const int py = lane >> 3, pxl = lane & 7;
  const unsigned lane_off = (unsigned)(py * img_w + pxl);
  for (int64_t it = blockIdx.x; it < nbatch; it += gridDim.x) {
    const int64_t base = (it * 4 + wave) * LT_BATCH;
    // frame, tile row and tile column of the batch's first tile by division, of the others by stepping
    int64_t f = base / tiles_per_frame;
    int sy, sx;
    {
      const int ti = (int)(base - f * tiles_per_frame);
      sy = ti / tm_w;
      sx = ti - sy * tm_w;
    }
    for (int j = 0; j < LT_BATCH; j++, sx++) {
      const int64_t t = base + j;
      if (t >= total) break;
      if (sx == tm_w) { sx = 0; if (++sy == tm_h) { sy = 0; f++; } }
      // the tile's first pixel on the scalar unit, the lane's pixel as a 32-bit offset from it (a 64-bit index per lane was a dozen vector instructions)
      const uint32_t *fp = frames + ((f * img_h + (int64_t)sy * 8) * (int64_t)img_w + (int64_t)sx * 8);
      uint32_t px = 0;
      if (sy * 8 + py < img_h && sx * 8 + pxl < img_w) px = swap_rb(fp[lane_off]);
      float l, a, b;
      rgb_to_lab_det(px & 0xff, (px >> 8) & 0xff, (px >> 16) & 0xff, srgb_lut, l, a, b);
      float *lt = lab + j * LT_TILE + lane;
      lt[0] = l;
      lt[LT_PLANE] = a;
      lt[2 * LT_PLANE] = b;
      // quadrant luma sums (GetTileZoneSum, 4842-4863): integer, order free.  Sums of 4 pixels by quad permutes; lanes 4g..4g+3 then hold
      // group g = (pixel row g / 2, half g & 1).  A row of 16 lanes holds groups 4r..4r+3: row_shr:8 leaves (4r) + (4r+2) in its lanes 8..11
      // and (4r+1) + (4r+3) in lanes 12..15 -- the left and right halves of pixel rows 2r and 2r+1 --, and the scalar unit adds two rows each
      int luma = (int)(px & 0xff) * 299 + (int)((px >> 8) & 0xff) * 587 + (int)((px >> 16) & 0xff) * 114;
      luma += __builtin_amdgcn_update_dpp(0, luma, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
      luma += __builtin_amdgcn_update_dpp(0, luma, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
      luma += __builtin_amdgcn_update_dpp(0, luma, 0x118, 0xf, 0xf, true);   // row_shr:8 (lanes 0..7 of a row add nothing)
      const int q00 = __builtin_amdgcn_readlane(luma, 8) + __builtin_amdgcn_readlane(luma, 24);    // [bottom][right]
      const int q01 = __builtin_amdgcn_readlane(luma, 12) + __builtin_amdgcn_readlane(luma, 28);
      const int q10 = __builtin_amdgcn_readlane(luma, 40) + __builtin_amdgcn_readlane(luma, 56);
      const int q11 = __builtin_amdgcn_readlane(luma, 44) + __builtin_amdgcn_readlane(luma, 60);
      const bool hm = q00 + q10 < q01 + q11;
      const bool vm = q00 + q01 < q10 + q11;
      const int src = ((vm ? 7 - py : py) << 3) | (hm ? 7 - pxl : pxl);
      const uint32_t canon = __shfl(px, src);
      (tiles + t * 64)[lane] = canon;
      if (lane == 0) flags[t] = (uint8_t)((hm ? 1 : 0) | (vm ? 2 : 0));
    }
    // Result[di+c] += lab, 64 Singles in raster order, then *= 1/64 (1349-1362): one lane per (tile, plane)
    if (lane < 3 * LT_BATCH) {
      const int j = lane / 3, c = lane - j * 3;
      if (base + j < total) {
        const float *p = lab + j * LT_TILE + c * LT_PLANE;
        float s = 0.0f;
        for (int k = 0; k < 64; k++) s = __fadd_rn(s, p[k]);
        lab_means[(base + j) * 3 + c] = __fmul_rn(s, 1.0f / 64);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// PearsonCorrelation (tilingencoder.pas:2201-2228) of consecutive frames' Lab tile means: one thread per frame, the
// reference's exact sequence (Math.mean sums in double; everything else sequential Single), so the sums are bit
// identical to a CPU restatement and 300 frames run side by side.  Output: num, sum dx^2, sum dy^2 per frame.
constexpr int PC = 2048;  // values per staged chunk
__global__ __launch_bounds__(64) void k_pearson_frames(const float *__restrict__ lab, int nframes, int per, float *__restrict__ correl) {
  // one wave per frame.  Only the ADDITIONS of the reference's sums are a chain; everything that feeds them is element-wise, so all
  // 64 lanes prepare a chunk in LDS (the doubles of the mean's terms, then the three products, each rounded exactly as the sequential
  // code rounds it) and lanes 0..2 only add, reading 16 bytes at a time
  __shared__ __attribute__((aligned(16))) unsigned char s_raw[2 * PC * 8];
  __shared__ double s_sum[2];
  double (*s_d)[PC] = reinterpret_cast<double (*)[PC]>(s_raw);  // [2][PC], first pass
  float (*s_p)[PC] = reinterpret_cast<float (*)[PC]>(s_raw);    // [3][PC], second pass
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f == 0) { if (lane < 3) correl[lane] = 0.0f; return; }
  const float *x = lab + (int64_t)(f - 1) * per, *y = lab + (int64_t)f * per;
  double acc = 0.0;
  for (int c0 = 0; c0 < per; c0 += PC) {
    const int n = min(PC, per - c0);
    __syncthreads();
    {  // all of a chunk's loads in flight at once: a lone wave has nothing else to cover their latency with
      float xv[PC / 64], yv[PC / 64];
#pragma unroll
      for (int u = 0; u < PC / 64; u++) { const int i = u * 64 + lane; xv[u] = i < n ? x[c0 + i] : 0.0f; yv[u] = i < n ? y[c0 + i] : 0.0f; }
#pragma unroll
      for (int u = 0; u < PC / 64; u++) { const int i = u * 64 + lane; if (i < n) { s_d[0][i] = (double)xv[u]; s_d[1][i] = (double)yv[u]; } }
    }
    __syncthreads();
    if (lane < 2) {
      const double *src = s_d[lane];
      int i = 0;
#pragma unroll 1
      for (; i + 32 <= n; i += 32) {  // sixteen reads issued before the first addition: their latency is paid once per 32 terms
        double2 v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = *reinterpret_cast<const double2 *>(src + i + 2 * u);
#pragma unroll
        for (int u = 0; u < 16; u++) { acc = __dadd_rn(acc, v[u].x); acc = __dadd_rn(acc, v[u].y); }
      }
      for (; i < n; i++) acc = __dadd_rn(acc, src[i]);
    }
  }
  if (lane < 2) s_sum[lane] = acc;
  __syncthreads();
  const float mx = (float)__ddiv_rn(s_sum[0], (double)per), my = (float)__ddiv_rn(s_sum[1], (double)per);
  float chain = 0.0f;  // lane 0: num = sum dx*dy, lane 1: denx = sum dx*dx, lane 2: deny = sum dy*dy
  for (int c0 = 0; c0 < per; c0 += PC) {
    const int n = min(PC, per - c0);
    __syncthreads();
    {
      float xv[PC / 64], yv[PC / 64];
#pragma unroll
      for (int u = 0; u < PC / 64; u++) { const int i = u * 64 + lane; xv[u] = i < n ? x[c0 + i] : 0.0f; yv[u] = i < n ? y[c0 + i] : 0.0f; }
#pragma unroll
      for (int u = 0; u < PC / 64; u++) {
        const int i = u * 64 + lane;
        if (i < n) {
          const float dx = __fsub_rn(xv[u], mx), dy = __fsub_rn(yv[u], my);
          s_p[0][i] = __fmul_rn(dx, dy);
          s_p[1][i] = __fmul_rn(dx, dx);
          s_p[2][i] = __fmul_rn(dy, dy);
        }
      }
    }
    __syncthreads();
    if (lane < 3) {
      const float *src = s_p[lane];
      int i = 0;
#pragma unroll 1
      for (; i + 64 <= n; i += 64) {
        float4 v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = *reinterpret_cast<const float4 *>(src + i + 4 * u);
#pragma unroll
        for (int u = 0; u < 16; u++) {
          chain = __fadd_rn(chain, v[u].x); chain = __fadd_rn(chain, v[u].y); chain = __fadd_rn(chain, v[u].z); chain = __fadd_rn(chain, v[u].w);
        }
      }
      for (; i < n; i++) chain = __fadd_rn(chain, src[i]);
    }
  }
  // the three raw sums go back to the host, which finishes with IEEE sqrt/divide (device __fsqrt_rn is a bare
  // v_sqrt_f32: 1 ulp, not correctly rounded)
  if (lane < 3) correl[f * 3 + lane] = chain;
}

int launch_pearson(const void *lab, int nframes, int per, void *correl, hipStream_t stream) {
  TM_TRY(require_device());
  if (nframes <= 0) return TM_OK;
  hipLaunchKernelGGL(k_pearson_frames, dim3(nframes), dim3(64), 0, stream, (const float *)lab, nframes, per, (float *)correl);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// RGBToLAB (utils.pas:374-410) of n colours 0x00RRGGBB -> [n][3] Singles: the colour math of the load and feature kernels on its own
__global__ void k_rgb_to_lab(const uint32_t *__restrict__ rgb, int64_t n, const float *__restrict__ srgb_lut, float *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t c = rgb[i];
    float l, a, b;
    rgb_to_lab_det((c >> 16) & 0xff, (c >> 8) & 0xff, c & 0xff, srgb_lut, l, a, b);
    out[i * 3] = l; out[i * 3 + 1] = a; out[i * 3 + 2] = b;
  }
}
int launch_rgb_to_lab(const void *rgb, int64_t n, void *out, hipStream_t stream) {
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  TM_CHECK(n >= 0 && (n == 0 || (rgb && out)), TM_E_INVAL, "tm_stage_rgb_to_lab: bad arguments");
  if (n == 0) return TM_OK;
  hipLaunchKernelGGL(k_rgb_to_lab, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 256 * 16)), dim3(256), 0, stream, (const uint32_t *)rgb, n, tab->srgb_lut, (float *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_load(const void *frames, int nframes, int img_w, int img_h, int tm_w, int tm_h, void *tiles, void *flags,
                void *lab_means, hipStream_t stream) {
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  TM_CHECK(nframes >= 0 && img_w > 0 && img_h > 0 && tm_w > 0 && tm_h > 0, TM_E_INVAL, "tm_stage_load: bad dimensions");
  const int64_t total = (int64_t)nframes * tm_w * tm_h;
  if (total == 0) return TM_OK;
  hipLaunchKernelGGL(k_load_tiles, dim3(grid_for(total, 4 * LT_BATCH)), dim3(256), 0, stream, (const uint32_t *)frames, nframes, img_w,
                     img_h, tm_w, tm_h, tab->srgb_lut, (uint32_t *)tiles, (uint8_t *)flags, (float *)lab_means);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx
