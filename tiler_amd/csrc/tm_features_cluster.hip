// tm_features_cluster.hip -- the clustering's int32[192] features of tiles (A6) for gfx950: the DCT modes (k_features_cluster_i32) and
// pvsWavelets (k_features_cluster_wavelet_i32).  Every step of the reference-order paths is a single IEEE operation issued through the
// __d*_rn intrinsics, in the order the reference's code performs it (DESIGN.md "Arithmetic").
#include "tm_common.h"
#include "tm_dct.h"
#include "tm_internal.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// A6 as DoPalettization uses it (tilingencoder.pas:4126, 4160): UseLAB planes, double LUT, sequential double sum
// (DCTInner<PDouble>, utils.pas:782-872), weight, then the build's Round() to int32 (DESIGN.md "k-means").
__global__ __launch_bounds__(256) void k_features_cluster_i32(const uint32_t *__restrict__ tiles, int64_t n, int weighted,
                                                              const double *__restrict__ lut, const double *__restrict__ weights,
                                                              const uint8_t *__restrict__ snake, const float *__restrict__ srgb_lut,
                                                              int32_t *__restrict__ out, const double *__restrict__ cosd /* [8][8] the LUT's cosine factor */, int plain) {
  // the planes as DOUBLES, widened once by the lane that made them
  __shared__ __attribute__((aligned(16))) double s_cpn[2][4][192];
  __shared__ __attribute__((aligned(16))) double s_row[4][64];  // a wave's row transforms, [u][y]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // The reference sums a coefficient's 64 double products one after the other (DCTInner<PDouble>, utils.pas:782-872) and stores Round(z w).
  // As in k_features_i16: z first by the LUT's two cosine factors (LaneDct), which differs from the sequential sum by less than
  // 128 x 2^-53 x sum|pixel x LUT| < 4e-10 here (|pixel| <= 128, 64 of them, |w| < 2.7); a coefficient whose z w lies within 1e-6 of a
  // half-integer -- two in a million -- is summed the reference's way.
  const LaneDct first_look(cosd, lane);
  double w[3];
#pragma unroll
  for (int c = 0; c < 3; c++) w[c] = weights[c * 64 + lane];
  const int zz = snake[lane];
  const int64_t niter = (n + 3) / 4;
  int buf = 0;
  for (int64_t it = blockIdx.x; it < niter; it += gridDim.x, buf ^= 1) {
    const int64_t t = it * 4 + wave;
    const bool valid = t < n;
    if (valid) {
      const uint32_t col = tiles[t * 64 + lane];
      float yy, uu, vv;
      rgb_to_lab_det(col & 0xff, (col >> 8) & 0xff, (col >> 16) & 0xff, srgb_lut, yy, uu, vv);
      s_cpn[buf][wave][lane] = (double)yy;
      s_cpn[buf][wave][64 + lane] = (double)uu;
      s_cpn[buf][wave][128 + lane] = (double)vv;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (a wave reads only what it wrote: its LDS operations are in order)
    if (valid) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *cp = &s_cpn[buf][wave][c * 64];
        auto in_order = [&]() -> double {  // the reference's sum
          double r = 0.0;
          for (int k = 0; k < 64; k += 2) {
            const double2 cv = *reinterpret_cast<const double2 *>(cp + k);
            const double2 lv = *reinterpret_cast<const double2 *>(lut + lane * 64 + k);
            r = __dadd_rn(r, __dmul_rn(cv.x, lv.x));
            r = __dadd_rn(r, __dmul_rn(cv.y, lv.y));
          }
          return weighted ? __dmul_rn(r, w[c]) : r;
        };
        double tv = 0.0;
        bool doubtful = true;
        if (!plain) {
          const double z = first_look(cp, s_row[wave], lane);
          tv = weighted ? z * w[c] : z;
          doubtful = !(fabs(tv - floor(tv) - 0.5) > 1e-6) || !(fabs(tv) < 1.0e9);
        }
        if (__builtin_amdgcn_ballot_w64(doubtful)) {  // (uniform)
          const double ex = in_order();
          if (doubtful) tv = ex;
        }
        out[t * 192 + c * 64 + zz] = (int32_t)__double2ll_rn(tv);
      }
    }
  }
}

// The same with Mode = pvsWavelets: WaveletGS<Double>(plane, out, 8, 8, 2) per channel (tilingencoder.pas:2727-2764, 3150-3157),
// i.e. normalised Haar levels on the 8x8, then the top-left 4x4, then the top-left 2x2.  A level maps rows into tempX (low half
// (a[2x] + a[2x+1]) f, high half (a[2x] - a[2x+1]) f), then the columns of tempX into tempY the same way, and copies the level's
// square back; entries outside it keep their value.  One wave per tile, one lane per coefficient (v, u), the pairs fetched by
// cross-lane reads.  Each step is one rounded add / subtract and one rounded multiply, as in the reference (no contraction).
// f = 1.0 / sqrt(2.0) in double steps = 0.7071067811865475, one ulp below the correctly rounded 1/sqrt(2).
__global__ __launch_bounds__(256) void k_features_cluster_wavelet_i32(const uint32_t *__restrict__ tiles, int64_t n, const uint8_t *__restrict__ snake,
                                                                      const float *__restrict__ srgb_lut, int32_t *__restrict__ out) {
  constexpr double f = 0.7071067811865475;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = lane & 7, v = lane >> 3;
  const int zz = snake[lane];
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < n; t += (int64_t)gridDim.x * 4) {  // (uniform in the wave)
    const uint32_t col = tiles[t * 64 + lane];
    float pl[3];
    rgb_to_lab_det(col & 0xff, (col >> 8) & 0xff, (col >> 16) & 0xff, srgb_lut, pl[0], pl[1], pl[2]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double a = (double)pl[c];
#pragma unroll
      for (int d = 8; d >= 2; d >>= 1) {
        const int h = d >> 1;
        const int xs = u < h ? u : u - h, ys = v < h ? v : v - h;  // (source indices of lanes outside the level stay inside the tile)
        const double r0 = __shfl(a, (v * 8 + 2 * xs) & 63), r1 = __shfl(a, (v * 8 + 2 * xs + 1) & 63);
        const double tx = u < h ? __dmul_rn(__dadd_rn(r0, r1), f) : __dmul_rn(__dsub_rn(r0, r1), f);  // tempX[v][u]
        const double c0 = __shfl(tx, (2 * ys * 8 + u) & 63), c1 = __shfl(tx, ((2 * ys + 1) * 8 + u) & 63);
        const double ty = v < h ? __dmul_rn(__dadd_rn(c0, c1), f) : __dmul_rn(__dsub_rn(c0, c1), f);  // tempY[v][u]
        if (u < d && v < d) a = ty;
      }
      out[t * 192 + c * 64 + zz] = (int32_t)__double2ll_rn(a);  // Round() (banker's), |a| <= 8 x the plane's largest magnitude
    }
  }
}

int launch_features_cluster(const void *tiles, int64_t n, int mode, void *out, hipStream_t stream) {
  const DeviceTables *tab;
  TM_TRY(get_tables(&tab));
  TM_CHECK(mode >= 0 && mode <= 4, TM_E_INVAL, "bad TPsyVisMode %d", mode);
  if (n <= 0) return TM_OK;
  if (mode == TM_PVS_WAVELETS) {  // the double path has the Haar branch (3150-3157); only the int16 one asserts
    hipLaunchKernelGGL(k_features_cluster_wavelet_i32, dim3(grid_for(n, 4)), dim3(256), 0, stream, (const uint32_t *)tiles, n, tab->snake, tab->srgb_lut,
                       (int32_t *)out);
    TM_HIP(hipGetLastError());
    return TM_OK;
  }
  hipLaunchKernelGGL(k_features_cluster_i32, dim3(grid_for(n, 4)), dim3(256), 0, stream, (const uint32_t *)tiles, n,
                     mode_weighted(mode) ? 1 : 0, tab->dct_lut_f64[mode_special(mode)], tab->weights, tab->snake, tab->srgb_lut,
                     (int32_t *)out, tab->dct_cos_f64[mode_special(mode)], knobs().features_plain ? 1 : 0);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx
