// tm_dct.h -- what the DCT feature kernels share (tm_features.hip, tm_features_cluster.hip, tm_window_dcts.hip; no other file includes it).
// All of them take a separable first look at a coefficient and sum it in the reference's order only when the rounding is in doubt
// (DESIGN.md 14.2); every decision of that scheme is stated here once.  Bit-exactness rules (DESIGN.md "Arithmetic"): every step of the
// in-doubt path is a single IEEE +,-,*,/ issued through the __f*_rn / __d*_rn intrinsics (never contracted into FMA), in the order the
// reference's code performs it (DCTInner_asm, utils.pas:874-1035).  The first look may be summed in any order; the in-doubt path may not.
#pragma once
#include "tm_common.h"
#include "tm_device.h"

namespace tmx {

// tm_features.hip: k_features_i16<2> over every 8 x 8 window of a frame buffer, a window at a time (launch_window_dcts under
// TM_WINDOW_DCTS_BY_TILE: the tests' reference for k_window_dcts; the template is instantiated in that file only)
int launch_features_windows_by_tile(const void *fb, int w, int h, void *out, hipStream_t stream);

// The first look's verdict on one coefficient, in Single arithmetic (double-precision instructions issue at a quarter of the Singles' rate
// here, and the verdict was a third of a coefficient's): t = z w from the separable transform (double), sa >= sum |pixel x LUT entry|, wabs = |w|.
// The reference's z_ref w lies within slack = sa (2^-23 + 2^-24)(1 + 2^-17)(1 + 2^-20) |w| + 1e-9 (|t| + 1) of t (k_features_i16 has the
// derivation), and tf = Single(t) within |t| 2^-24 of t: when tf is farther than the two together from every half-integer, Round(z_ref w) =
// rint(tf).  Returns false (in doubt: the caller sums the coefficient in the reference's order) otherwise, and for values no int16 path needs.
// (sw = sa x 1.82e-7 |w|: the caller folds what is constant per coefficient.  slack < 0.25 also bounds |t| by 4 x 10^6: rintf is exact there.)
__device__ __forceinline__ bool first_look_rounds(double t, float sw, int &o) {
  const float tf = (float)t;
  const float slack = fmaf(fabsf(tf), 6.21e-8f, sw + 1.1e-9f);
  const float fr = __builtin_amdgcn_fractf(tf);  // tf - floor(tf), exact
  o = (int)rintf(tf);
  return fabsf(fr - 0.5f) > slack && slack < 0.25f;
}

// what of sw is the coefficient's own, per unit of sa: 1.82e-7 > (2^-23 + 2^-24) (1 + 2^-17)(1 + 2^-20), times |w| as a Single, rounded up
__device__ __forceinline__ float slack_per_sum(bool weighted, double w) { return 1.82e-7f * (weighted ? fabsf((float)w) * 1.000001f : 1.0f); }

// cDCTUVRatio (utils.pas:100-109) of coefficient cf = v * 8 + u: 0.5, Single(sqrt(0.5)), 1
__device__ __forceinline__ double dct_uv_ratio(int cf) { return (cf == 0) ? 0.5 : (((cf & 7) == 0 || (cf >> 3) == 0) ? 0.707106769084930419921875 : 1.0); }

// the Euclidean norm of row `row` of the Single LUT, rounded up (4 for the plain DCT's rows); rot rotates the order of the reads (a wave
// whose lanes read their own rows from LDS passes its lane: no bank conflict)
__device__ __forceinline__ float lut_row_norm_up(const float *lut, int row, int rot) {
  double q2 = 0.0;
  for (int k = 0; k < 64; k++) { const double v = (double)lut[row * 64 + ((k + rot) & 63)]; q2 = fma(v, v, q2); }
  return (float)(sqrt(q2) * (1.0 + 1e-6));
}

// Per coefficient cf = v * 8 + u, for the kernels whose lanes hold eight coefficients each: cDCTUVRatio x weight, what of the slack is the
// coefficient's own (1.82e-7 x |weight| x the LUT row's norm), the zig-zag place.  The first 64 threads call it, a barrier follows.
// weighted == false: every weight is 1, `weights` is not read.
__device__ __forceinline__ void fill_coef_factors(int cf, const float *lut, bool weighted, const double *weights, const uint8_t *snake, double (&s_cw)[3][64],
                                                  float (&s_kw)[3][64], int (&s_zz)[64]) {
  const float ln = lut_row_norm_up(lut, cf, 0);
  for (int c = 0; c < 3; c++) {
    const double wv = weighted ? weights[c * 64 + cf] : 1.0;
    s_cw[c][cf] = dct_uv_ratio(cf) * wv;
    s_kw[c][cf] = slack_per_sum(true, wv) * ln * 1.000001f;
  }
  s_zz[cf] = snake[cf];
}

// v + v of the lane a row operation names (ctrl: the DPP control word), for Singles and 32-bit integers
template <int CTRL, class T>
__device__ __forceinline__ T dpp_add(T v) { return v + __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)); }
// the sum over each group of eight lanes, in all eight (row moves: lane ^ 1, lane ^ 2, the mirror image inside eight)
template <class T>
__device__ __forceinline__ T sum8_dpp(T v) { return dpp_add<0x141>(dpp_add<0x4E>(dpp_add<0xB1>(v))); }
// the sum over the wave, uniform (row operations and four lane reads, no LDS; 64 non-negative Singles: within 2^-17 of exact)
__device__ __forceinline__ float sum64_dpp(float v) {
  const int s = __builtin_bit_cast(int, dpp_add<0x140>(sum8_dpp(v)));  // the mirror image inside sixteen: every lane has its row's sum
  return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 16))) +
         (__builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(s, 48)));
}

// the 8-point DCT-II without its scale factors, r[u] = sum p[x] cos((x + 0.5) u pi / 8), by the even / odd split: 35 double-precision
// operations for the eight outputs (first look only: contracted multiply-adds, its own order of summation)
__device__ __forceinline__ void dct8(const double (&p)[8], double (&r)[8]) {
  constexpr double C1 = 0.98078528040323044913, C2 = 0.92387953251128675613, C3 = 0.83146961230254523708, C4 = 0.70710678118654752440,
                   C5 = 0.55557023301960222474, C6 = 0.38268343236508977173, C7 = 0.19509032201612826785;  // cos(k pi / 16)
  const double s0 = p[0] + p[7], s1 = p[1] + p[6], s2 = p[2] + p[5], s3 = p[3] + p[4], d0 = p[0] - p[7], d1 = p[1] - p[6], d2 = p[2] - p[5], d3 = p[3] - p[4];
  const double e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
  r[0] = e0 + e1;
  r[4] = C4 * (e0 - e1);
  r[2] = fma(C2, e2, C6 * e3);
  r[6] = fma(C6, e2, -(C2 * e3));
  r[1] = fma(C1, d0, fma(C3, d1, fma(C5, d2, C7 * d3)));
  r[3] = fma(C3, d0, fma(-C7, d1, fma(-C1, d2, -(C5 * d3))));
  r[5] = fma(C5, d0, fma(-C1, d1, fma(C7, d2, C3 * d3)));
  r[7] = fma(C7, d0, fma(-C5, d1, fma(C3, d2, -(C1 * d3))));
}

// The first look with a lane per coefficient (k_features_i16, k_features_cluster_i32): lane = v * 8 + u is coefficient (u, v); in the row
// pass the same lane stands for (u, row y = lane >> 3).  The LUT is cos x cos x ratio: a row transform shared by the eight coefficients of a
// column of the LUT, then a column transform, 16 fused multiply-adds in double.
struct LaneDct {
  double au[8], av[8], ruv;
  // cosd: [8][8] the LUT's cosine factor, cos((x + 0.5) u pi / div)
  __device__ __forceinline__ LaneDct(const double *cosd, int lane) : ruv(dct_uv_ratio(lane)) {
#pragma unroll
    for (int x = 0; x < 8; x++) { au[x] = cosd[(lane & 7) * 8 + x]; av[x] = cosd[(lane >> 3) * 8 + x]; }
  }
  // z of this lane's coefficient of the plane cp (64 doubles in LDS); s_row: the wave's own 64 doubles, its row transforms [u][y]
  __device__ __forceinline__ double operator()(const double *cp, double *s_row, int lane) const {
    const double2 *fp = reinterpret_cast<const double2 *>(cp + (lane >> 3) * 8);
    const double2 f0 = fp[0], f1 = fp[1], f2 = fp[2], f3 = fp[3];
    double r = au[0] * f0.x;
    r = fma(au[1], f0.y, r); r = fma(au[2], f1.x, r); r = fma(au[3], f1.y, r);
    r = fma(au[4], f2.x, r); r = fma(au[5], f2.y, r); r = fma(au[6], f3.x, r); r = fma(au[7], f3.y, r);
    s_row[(lane & 7) * 8 + (lane >> 3)] = r;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the wave's LDS operations are in order: its reads below see its writes above)
    const double2 *rp = reinterpret_cast<const double2 *>(&s_row[(lane & 7) * 8]);
    const double2 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next plane's row transforms land after these reads)
    double z = av[0] * r0.x;
    z = fma(av[1], r0.y, z); z = fma(av[2], r1.x, z); z = fma(av[3], r1.y, z);
    z = fma(av[4], r2.x, z); z = fma(av[5], r2.y, z); z = fma(av[6], r3.x, z); z = fma(av[7], r3.y, z);
    return z * ruv;
  }
};

// z of one coefficient in DCTInner_asm's order (utils.pas:892-921), by the whole wave and uniform over it: lane k holds pixel k (`mine`) and
// LUT entry k of the coefficient's row; the order's pairings are lane exchanges -- xor 4 in Single, xor 8 and xor 2 in double, then the four
// 16-element steps in sequence.  This is the project's bit-exactness contract: 64 Single products, Single sums of pairs, 32 conversions,
// 34 double additions.
__device__ __forceinline__ double ref_order_sum(float mine, float lut_entry) {
  const float e = __fmul_rn(mine, lut_entry);
  const float s4 = __fadd_rn(e, __shfl_xor(e, 4));                 // (p0+p4, p1+p5, p2+p6, p3+p7 | p8+p12, ...): Single
  double d = (double)s4;
  d = __dadd_rn(d, __shfl_xor(d, 8));                              // (double)s + (double)t
  d = __dadd_rn(d, __shfl_xor(d, 2));                              // ... + the second pair: a0 in lane 16 j, a1 in lane 16 j + 1
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) { acc0 = __dadd_rn(acc0, __shfl(d, 16 * j)); acc1 = __dadd_rn(acc1, __shfl(d, 16 * j + 1)); }
  return __dadd_rn(acc0, acc1);
}

// Round(): half to even (3126), then the store into a SmallInt (the low 16 bits)
__device__ __forceinline__ int16_t round_i16(double t) { return fabs(t) < 2.0e9 ? (int16_t)__double2int_rn(t) : (int16_t)__double2ll_rn(t); }

// The coefficients in doubt of a wave's run of eight tiles or windows (k_features_tiles8, k_window_dcts), one after the other by the whole
// wave.  Lane (item j, u) says in dmask which of its coefficients (u, v) are in doubt (bit v); pixel(sj) is this lane's pixel -- lane = y * 8 + x
// -- of item sj in the plane at hand; w: that plane's 64 weights, not read when weighted == false; so: the run's coefficients [item][zig-zag place].
// (Unweighted is a flag and not a null `w`: a pointer the kernel chose itself no longer counts as its read-only argument, and the weight then
// comes by a vector load where the scalar unit fetched it -- DESIGN.md section 25 has the measurement.)
template <class Pixel>
__device__ __forceinline__ void sum_in_doubt(unsigned dmask, int lane, Pixel pixel, const float *lut, bool weighted, const double *w, const int (&s_zz)[64], int16_t *so) {
  for (unsigned long long m = __builtin_amdgcn_ballot_w64(dmask != 0); m; m &= m - 1) {
    const int src = __builtin_ctzll(m);
    const int sj = src >> 3, su = src & 7;
    const float mine = pixel(sj);
    for (unsigned vm = (unsigned)__builtin_amdgcn_readlane((int)dmask, src); vm; vm &= vm - 1) {
      const int coef = __builtin_ctz(vm) * 8 + su;
      const double z = ref_order_sum(mine, lut[coef * 64 + lane]);
      const double t = weighted ? __dmul_rn(z, w[coef]) : z;
      if (lane == src) so[sj * 64 + s_zz[coef]] = round_i16(t);
    }
  }
}

// The search's digit plan wants the output columns' ranges: kept by the feature kernel, a pass over all rows saved there.  A lane holds the
// running min / max of column `col` of each plane; the four waves of a workgroup hold the same columns: their ranges meet in LDS (s_mm: 4 x 384
// ints), one atomic pair per column and workgroup into colmm ([384]: min, then max, of the 192 output columns).
__device__ __forceinline__ void fold_colmm(int *s_mm, int col, const int (&mmn)[3], const int (&mmx)[3], int *colmm) {
  const int wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; c++) { s_mm[wave * 384 + c * 64 + col] = mmn[c]; s_mm[wave * 384 + 192 + c * 64 + col] = mmx[c]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 192; i += 256) {
    const int a = min(min(s_mm[i], s_mm[384 + i]), min(s_mm[768 + i], s_mm[1152 + i]));
    const int b = max(max(s_mm[192 + i], s_mm[384 + 192 + i]), max(s_mm[768 + 192 + i], s_mm[1152 + 192 + i]));
    if (a != INT_MAX) { atomicMin(&colmm[i], a); atomicMax(&colmm[192 + i], b); }
  }
}

}  // namespace tmx
