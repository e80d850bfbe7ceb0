// tm_kmeans_tile.hip -- what the build's k-means (tm_kmeans.hip) has for D = 192 alone, the tile -> palette clustering of DoPalettization:
// the register-tiled assignment step, the iterations that skip what cannot change, and all of those in one resident launch.
#include "tm_kmeans.h"

namespace tmx {


// Assignment step for D = 192, register-tiled: every thread scores PPT points against 16 centroids at a time, so each
// centroid value fetched from LDS (a wave-wide broadcast) feeds PPT x 3 double-precision operations instead of 3 -- the
// untiled form is bound by LDS return bandwidth, not by the FP64 pipe.  The arithmetic per (point, centroid) is unchanged:
// sum over dimensions in order of (p - c)^2, one IEEE subtraction and one fused multiply-add each.  One workgroup per CU-sized slice of the points
// (rows_per_block <= 256 * PPT, chosen by the host so that the slices fill the chip evenly); the next 8-dimension chunk is
// fetched into registers while the current one is being scored.
// The exact integer sums are carried from iteration to iteration: a point that changes cluster adds its row to the new
// cluster and subtracts it from the old one (u64 arithmetic: exact and order-free), all threads of the workgroup
// cooperating on one moved row at a time (coalesced read, one dimension per thread), accumulated in LDS and flushed once.
// LOOK: the first look of tm_kmeans.h -- the same passes with Single accumulators in pairs (packed subtractions and fused multiply-adds:
// a quarter of the chain's issue time), the centroids staged as Singles, their norms summed on the way; the points the look cannot
// decide are listed in LDS and go through the chain itself, a lane per (point, centroid) pair, before anything is written.
constexpr int A_DCH = 8;   // dimensions staged per pass
constexpr int A_MU = 8;    // moved rows a wave has in flight
typedef float a_f2 __attribute__((ext_vector_type(2)));
template <int PPT, bool LOOK>
__global__ __launch_bounds__(256) void k_assign192(const int32_t *__restrict__ pts, const int32_t *__restrict__ pts_chunked, int64_t n_total,
                                                   const uint32_t *__restrict__ w, Seg *__restrict__ segs,
                                                   int k, const double *__restrict__ cent, int32_t *__restrict__ assign,
                                                   u64 *__restrict__ sums, u64 *__restrict__ cnts, int rows_per_block, int lds_delta,
                                                   const int *__restrict__ quiet, double *__restrict__ ub, double *__restrict__ lb,
                                                   u64 *__restrict__ look_stats) {
  if (*quiet >= 0) return;  // converged earlier in this batch of launches
  constexpr int D = 192, ROWS = 256 * PPT, PITCH = A_DCH + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  double(*s_cent)[KCH] = reinterpret_cast<double(*)[KCH]>(s_raw);                       // [A_DCH][KCH]
  float(*s_centf)[KCH] = reinterpret_cast<float(*)[KCH]>(s_raw);                        // LOOK: the same as Singles, in its first half
  int32_t *s_pts = reinterpret_cast<int32_t *>(s_raw + A_DCH * KCH * 8);               // [ROWS][PITCH]
  int32_t *s_moved = s_pts + ROWS * PITCH;                                             // [ROWS][3]: row, old, new
  u64 *s_delta = reinterpret_cast<u64 *>(s_moved + ROWS * 3 + (ROWS & 1));             // [kk][D+1] when lds_delta
  // LOOK, once the passes are over, in s_pts' place (24 of its 36 bytes per row): what the chain found for a row in doubt, and their list
  double *s_xd = reinterpret_cast<double *>(s_pts);                                     // [ROWS][2]: smallest, second smallest
  int32_t *s_xc = s_pts + ROWS * 4;                                                     // [ROWS]: whose the smallest is
  int32_t *s_doubt = s_xc + ROWS;                                                       // [ROWS]
  __shared__ int s_nmoved, s_ndoubt;
  __shared__ double s_nrm[A_DCH * KCH], s_E[KCH];  // LOOK: the centroids' norms in partial sums, then E(c)
  const int seg = blockIdx.y;
  const Seg sg = segs[seg];
  const int kk = sg.kk, tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int nrows = (int)max((int64_t)0, min((int64_t)rows_per_block, sg.count - row0));
  if (nrows <= 0) return;
  if (tid == 0) { s_nmoved = 0; s_ndoubt = 0; }
  if (lds_delta)
    for (int e = tid; e < kk * (D + 1); e += 256) s_delta[e] = 0;
  double bd[PPT], bd2[PPT];  // smallest and second smallest distance (the second only feeds the bounds of the later iterations)
  int bc[PPT];
  double ubv[PPT], lbv[PPT];  // the bounds the later iterations start from
#pragma unroll
  for (int m = 0; m < PPT; m++) { bd[m] = 0.0; bd2[m] = 1.0e300; bc[m] = -1; ubv[m] = 0.0; lbv[m] = 0.0; }
  const int4 zero4 = make_int4(0, 0, 0, 0);
  if constexpr (LOOK) {
    float bs[PPT], mx[PPT];            // the smallest Single sum; the row's largest magnitude as a Single
    double bhi[PPT], blo[PPT], olo[PPT];  // hi and lo of the Single argmin; the smallest lo among the others
#pragma unroll
    for (int m = 0; m < PPT; m++) { bs[m] = 0.0f; mx[m] = 0.0f; bhi[m] = 0.0; blo[m] = 0.0; olo[m] = 1.0e150; }
#pragma unroll 1
    for (int c0 = 0; c0 < kk; c0 += KCH) {
      a_f2 s[PPT][KCH / 2];
#pragma unroll
      for (int m = 0; m < PPT; m++)
#pragma unroll
        for (int c = 0; c < KCH / 2; c++) s[m][c] = a_f2{0.0f, 0.0f};
      int4 pre[2 * PPT];
      double pre_c = 0.0, nrm = 0.0;
      // as below, but a slot beyond the slice reads the slice's last row (nothing of such a slot is used) instead of choosing between the load
      // and a zero: that choice makes the loads flat ones (one of the two addresses is private memory), and a flat load counts as an LDS
      // operation as well, so the scoring's first wait for its LDS reads waits for the whole prefetch
      auto fetch = [&](int j0) {
#pragma unroll
        for (int m = 0; m < 2 * PPT; m++) {
          const int r = min((tid >> 1) + 128 * m, nrows - 1);
          pre[m] = *reinterpret_cast<const int4 *>(pts_chunked + ((int64_t)(j0 / A_DCH) * n_total + sg.begin + row0 + r) * A_DCH + (tid & 1) * 4);
        }
        if (tid < A_DCH * KCH) {
          const int j = tid / KCH, c = tid - j * KCH;
          pre_c = c0 + c < kk ? cent[((int64_t)seg * k + c0 + c) * D + j0 + j] : 0.0;
        }
      };
      auto stage = [&]() {
#pragma unroll
        for (int m = 0; m < 2 * PPT; m++) {
          int32_t *dst = s_pts + ((tid >> 1) + 128 * m) * PITCH + (tid & 1) * 4;
          dst[0] = pre[m].x; dst[1] = pre[m].y; dst[2] = pre[m].z; dst[3] = pre[m].w;
        }
        if (tid < A_DCH * KCH) { s_centf[tid / KCH][tid % KCH] = (float)pre_c; nrm = __fma_rn(pre_c, pre_c, nrm); }
      };
      fetch(0);
      __syncthreads();  // previous pass (or the zeroing above) done with the buffers
      stage();
      __syncthreads();
#pragma unroll 1
      for (int j0 = 0; j0 < D; j0 += A_DCH) {
        if (j0 + A_DCH < D) fetch(j0 + A_DCH);
#pragma unroll 2
        for (int j = 0; j < A_DCH; j++) {
          a_f2 pj[PPT];
#pragma unroll
          for (int m = 0; m < PPT; m++) {
            const float v = (float)s_pts[(tid + 256 * m) * PITCH + j];
            mx[m] = __builtin_fmaxf(mx[m], __builtin_fabsf(v));
            pj[m] = a_f2{v, v};
          }
#pragma unroll
          for (int c = 0; c < KCH; c += 4) {
            const float4 cv = *reinterpret_cast<const float4 *>(&s_centf[j][c]);
            const a_f2 c01{cv.x, cv.y}, c23{cv.z, cv.w};
#pragma unroll
            for (int m = 0; m < PPT; m++) {
              const a_f2 t0 = pj[m] - c01, t1 = pj[m] - c23;
              s[m][c / 2] = __builtin_elementwise_fma(t0, t0, s[m][c / 2]);
              s[m][c / 2 + 1] = __builtin_elementwise_fma(t1, t1, s[m][c / 2 + 1]);
            }
          }
        }
        __syncthreads();
        if (j0 + A_DCH < D) stage();
        __syncthreads();
      }
      // E(c) of this pass's centroids: eight partial sums of squares each (any order: rounded up by FL_ETA, nine orders above their rounding)
      if (tid < A_DCH * KCH) s_nrm[tid] = nrm;
      __syncthreads();
      if (tid < KCH) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < A_DCH; j++) q += s_nrm[j * KCH + tid];
        s_E[tid] = sqrt(q) * (FL_CENT * (1.0 + FL_ETA)) + 1.0e-30;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < KCH; c++) {
        if (c0 + c >= kk) break;  // (uniform)
        const double e = s_E[c];
#pragma unroll
        for (int m = 0; m < PPT; m++) {
          const float sv = s[m][c >> 1][c & 1];
          const double rt = (double)sqrtf(sv);
          const double hi = __fma_rn(rt, 1.0 + FL_GAMMA, e), lo = __fma_rn(rt, 1.0 - FL_GAMMA, -e);
          if (bc[m] < 0 || sv < bs[m]) {
            if (bc[m] >= 0) olo[m] = fmin(olo[m], blo[m]);
            bs[m] = sv; bc[m] = c0 + c; bhi[m] = hi; blo[m] = lo;
          } else olo[m] = fmin(olo[m], lo);
        }
      }
    }
    // decided, or in doubt -> the list
    bool doubt[PPT];
#pragma unroll
    for (int m = 0; m < PPT; m++) {
      const int r = tid + 256 * m;
      const bool decided = olo[m] * (1.0 - FL_ETA) > bhi[m] * (1.0 + FL_ETA) && mx[m] < FL_INT_EXACT;
      doubt[m] = r < nrows && !decided;
      ubv[m] = bhi[m] * (1.0 + FL_ETA);
      lbv[m] = olo[m] - fabs(olo[m]) * FL_ETA;
      if (doubt[m]) s_doubt[atomicAdd(&s_ndoubt, 1)] = r;  // (s_pts has been read for the last time: the barriers behind the last pass)
    }
    __syncthreads();
    const int ndoubt = s_ndoubt;
    if (ndoubt) {  // (uniform in the workgroup) the chain: 16 points per step, a lane per (point, centroid) pair, every accumulator its 192 terms in order
      const int cl = tid & 15;
#pragma unroll 1
      for (int t0 = 0; t0 < ndoubt; t0 += 16) {
        const int t = t0 + (tid >> 4);
        const bool act = t < ndoubt;
        const int r = s_doubt[act ? t : 0];
        const int32_t *rp = pts + (sg.begin + row0 + r) * D;
        double xd = 1.0e300, xd2 = 1.0e300;
        int xc = 0x7fffffff;
#pragma unroll 1
        for (int c0 = 0; c0 < kk; c0 += KCH) {
          const int ci = c0 + cl;
          const double *cp = cent + ((int64_t)seg * k + min(ci, kk - 1)) * D;
          double sacc = 0.0;
#pragma unroll 8
          for (int j = 0; j < D; j++) { const double d0 = __dsub_rn((double)rp[j], cp[j]); sacc = __fma_rn(d0, d0, sacc); }
          if (ci < kk) {  // this lane's centroids come in ascending order: strict `<` keeps the lowest index among equals
            if (sacc < xd) { xd2 = xd; xd = sacc; xc = ci; }
            else if (sacc < xd2) xd2 = sacc;
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {  // the 16 lanes of a point: the best by (distance, index); the second best distance = the smallest of the rest
          const double od = __shfl_xor(xd, o), od2 = __shfl_xor(xd2, o);
          const int oc = __shfl_xor(xc, o);
          const bool take = od < xd || (od == xd && oc < xc);
          const double loser = take ? xd : od;
          xd2 = fmin(fmin(xd2, od2), loser);
          if (take) { xd = od; xc = oc; }
        }
        if (act && cl == 0) { s_xd[r * 2] = xd; s_xd[r * 2 + 1] = xd2; s_xc[r] = xc; }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < PPT; m++)
        if (doubt[m]) {
          const int r = tid + 256 * m;
          bc[m] = s_xc[r];
          ubv[m] = sqrt(s_xd[r * 2]) * (1.0 + 1e-12);
          lbv[m] = sqrt(s_xd[r * 2 + 1]) * (1.0 - 1e-12);
        }
    }
    if (look_stats && tid == 0) {  // one add per workgroup
      atomicAdd(&look_stats[0], (u64)nrows);
      if (ndoubt) atomicAdd(&look_stats[1], (u64)ndoubt);
    }
  } else {
#pragma unroll 1
  for (int c0 = 0; c0 < kk; c0 += KCH) {
    double s[PPT][KCH];
#pragma unroll
    for (int m = 0; m < PPT; m++)
#pragma unroll
      for (int c = 0; c < KCH; c++) s[m][c] = 0.0;
    int4 pre[2 * PPT];
    double pre_c = 0.0;
    auto fetch = [&](int j0) {  // global -> registers: 2 threads x 16 B per row, 128 rows per slot; one centroid value per thread < 128
#pragma unroll
      for (int m = 0; m < 2 * PPT; m++) {
        const int r = (tid >> 1) + 128 * m;
        // chunk-major copy [j0 / 8][point][8]: the workgroup's rows of one chunk are one contiguous block (row-major pts would
        // give 32 useful bytes per 128-byte line and re-fetch every line four times over the 24 chunks)
        pre[m] = r < nrows ? *reinterpret_cast<const int4 *>(pts_chunked + ((int64_t)(j0 / A_DCH) * n_total + sg.begin + row0 + r) * A_DCH + (tid & 1) * 4) : zero4;
      }
      if (tid < A_DCH * KCH) {
        const int j = tid / KCH, c = tid - j * KCH;
        pre_c = c0 + c < kk ? cent[((int64_t)seg * k + c0 + c) * D + j0 + j] : 0.0;
      }
    };
    auto stage = [&]() {  // registers -> LDS
#pragma unroll
      for (int m = 0; m < 2 * PPT; m++) {
        int32_t *dst = s_pts + ((tid >> 1) + 128 * m) * PITCH + (tid & 1) * 4;
        dst[0] = pre[m].x; dst[1] = pre[m].y; dst[2] = pre[m].z; dst[3] = pre[m].w;
      }
      if (tid < A_DCH * KCH) s_cent[tid / KCH][tid % KCH] = pre_c;
    };
    fetch(0);
    __syncthreads();  // previous pass (or the zeroing above) done with the buffers
    stage();
    __syncthreads();
#pragma unroll 1
    for (int j0 = 0; j0 < D; j0 += A_DCH) {
      if (j0 + A_DCH < D) fetch(j0 + A_DCH);
#pragma unroll 2
      for (int j = 0; j < A_DCH; j++) {
        double pj[PPT];
#pragma unroll
        for (int m = 0; m < PPT; m++) pj[m] = (double)s_pts[(tid + 256 * m) * PITCH + j];
#pragma unroll
        for (int c = 0; c < KCH; c += 2) {
          const double2 cv = *reinterpret_cast<const double2 *>(&s_cent[j][c]);
#pragma unroll
          for (int m = 0; m < PPT; m++) {
            const double t0 = __dsub_rn(pj[m], cv.x), t1 = __dsub_rn(pj[m], cv.y);
            s[m][c] = __fma_rn(t0, t0, s[m][c]);
            s[m][c + 1] = __fma_rn(t1, t1, s[m][c + 1]);
          }
        }
      }
      __syncthreads();
      if (j0 + A_DCH < D) stage();
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < PPT; m++)
#pragma unroll
      for (int c = 0; c < KCH; c++)
        if (c0 + c < kk) {
          if (bc[m] < 0 || s[m][c] < bd[m]) { if (bc[m] >= 0) bd2[m] = bd[m]; bd[m] = s[m][c]; bc[m] = c0 + c; }
          else if (s[m][c] < bd2[m]) bd2[m] = s[m][c];
        }
  }
#pragma unroll
  for (int m = 0; m < PPT; m++) { ubv[m] = sqrt(bd[m]) * (1.0 + 1e-12); lbv[m] = sqrt(bd2[m]) * (1.0 - 1e-12); }
  }
  if (ub) {  // Euclidean bounds for the skipping iterations, rounded the safe way: ub >= the distance to the own centroid, lb <= to any other
#pragma unroll
    for (int m = 0; m < PPT; m++) {
      const int r = tid + 256 * m;
      if (r >= nrows) continue;
      const int64_t gi = sg.begin + row0 + r;
      ub[gi] = ubv[m];
      lb[gi] = lbv[m];
    }
  }
  // moved points -> list
#pragma unroll
  for (int m = 0; m < PPT; m++) {
    const int r = tid + 256 * m;
    if (r >= nrows) continue;
    const int64_t gi = sg.begin + row0 + r;
    const int old = assign[gi];
    if (old == bc[m]) continue;
    assign[gi] = bc[m];
    const int slot = atomicAdd(&s_nmoved, 1);
    s_moved[slot * 3] = r; s_moved[slot * 3 + 1] = old; s_moved[slot * 3 + 2] = bc[m];
  }
  __syncthreads();
  const int nmoved = s_nmoved;
  if (nmoved == 0) return;
  if (tid == 0) atomicAdd(&segs[seg].changed, nmoved);
  // a wave per moved row: lane -> dimensions lane, +64, +128; 192 = the weight.  A wave asks for A_MU rows before it adds the first (32 rows
  // of the workgroup in flight): the first iteration moves every row of the slice, and with eight rows in flight its 768 rows were 96
  // round trips to memory one behind the other
#pragma unroll 1
  for (int e0 = tid >> 6; e0 < nmoved; e0 += 4 * A_MU) {
    int pv[A_MU][3], oldv[A_MU], nwv[A_MU];
    long long wv[A_MU];
#pragma unroll
    for (int u = 0; u < A_MU; u++) {
      const int e = e0 + 4 * u;
      const bool ok = e < nmoved;
      const int ee = ok ? e : e0;
      const int64_t gi = sg.begin + row0 + s_moved[ee * 3];
      oldv[u] = s_moved[ee * 3 + 1];
      nwv[u] = ok ? s_moved[ee * 3 + 2] : -1;
      wv[u] = w ? (long long)w[gi] : 1;
#pragma unroll
      for (int q = 0; q < 3; q++) pv[u][q] = pts[gi * D + (tid & 63) + 64 * q];
    }
#pragma unroll
    for (int u = 0; u < A_MU; u++) {
      const int old = oldv[u], nw = nwv[u];
      if (nw < 0) continue;  // (uniform in the wave)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int j = (tid & 63) + 64 * q;
        if (j > D) break;
        const u64 v = q < 3 ? (u64)(wv[u] * pv[u][q < 3 ? q : 0]) : (u64)wv[u];
        if (lds_delta) {
          atomicAdd(&s_delta[nw * (D + 1) + j], v);
          if (old >= 0) atomicAdd(&s_delta[old * (D + 1) + j], (u64)0 - v);
        } else {
          u64 *base = j < D ? sums + (int64_t)seg * k * D : cnts + (int64_t)seg * k;
          const int64_t stride = j < D ? D : 1, off = j < D ? j : 0;
          atomicAdd(&base[nw * stride + off], v);
          if (old >= 0) atomicAdd(&base[old * stride + off], (u64)0 - v);
        }
      }
    }
  }
  if (lds_delta) {
    __syncthreads();
    for (int e = tid; e < kk * (D + 1); e += 256) {
      const u64 v = s_delta[e];
      if (v == 0) continue;
      const int c = e / (D + 1), j = e - c * (D + 1);
      if (j == D) atomicAdd(&cnts[(int64_t)seg * k + c], v);
      else atomicAdd(&sums[((int64_t)seg * k + c) * D + j], v);
    }
  }
}

__global__ void k_chunk_major(const int32_t *__restrict__ pts, int64_t n, int32_t *__restrict__ out) {  // [n][192] -> [24][n][8]
  const int64_t total = n * 48;  // int4 elements
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / 48;
    const int v = (int)(e - i * 48), ch = v >> 1, half = v & 1;
    reinterpret_cast<int4 *>(out)[((int64_t)ch * n + i) * 2 + half] = reinterpret_cast<const int4 *>(pts)[e];
  }
}

void launch_chunk_major(const int32_t *pts, int64_t n, int32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_chunk_major, dim3((unsigned)std::min<int64_t>((n * 48 + 255) / 256, 8192)), dim3(256), 0, stream, pts, n, out);
}

Assign192Shape assign192_shape(int64_t maxcount, int nseg, int k, int cus) {
  constexpr int occ = 2;  // workgroups per CU the slices are sized for
  const int64_t slots = std::max<int64_t>(1, (int64_t)cus * occ / std::max(1, std::min(nseg, cus * occ)));  // workgroups per segment in one round
  const int64_t per_slot = (maxcount + slots - 1) / slots;
  const int64_t rounds = (per_slot + 256 * 5 - 1) / (256 * 5);
  Assign192Shape sh;
  sh.rows = (int)std::max<int64_t>(1, (per_slot + rounds - 1) / rounds);
  sh.ppt = (sh.rows + 255) / 256;
  sh.nblk = (int)((maxcount + sh.rows - 1) / sh.rows);
  const size_t fixed = (size_t)A_DCH * KCH * 8 + (size_t)256 * sh.ppt * (A_DCH + 1) * 4 + (size_t)(256 * sh.ppt * 3 + 1) * 4;
  sh.lds_delta = fixed + (size_t)k * 193 * 8 <= 150 * 1024 ? 1 : 0;
  sh.lds = fixed + (sh.lds_delta ? (size_t)k * 193 * 8 : 0) + 16;
  return sh;
}

template <int PPT, bool LOOK>
static void launch_assign192_t(const Assign192Shape &sh, int nseg, hipStream_t stream, const int32_t *pts, const int32_t *ptsc, int64_t ntot, const uint32_t *w, Seg *ds,
                               int k, const double *cent, int32_t *assign, u64 *sums, u64 *cnts, const int *quiet, double *ub, double *lb, u64 *look_stats) {
  static bool attr_set = false;
  if (!attr_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_assign192<PPT, LOOK>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048); attr_set = true; }
  hipLaunchKernelGGL((k_assign192<PPT, LOOK>), dim3(sh.nblk, nseg), dim3(256), sh.lds, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, sh.rows, sh.lds_delta, quiet, ub, lb,
                     look_stats);
}
template <bool LOOK>
static void launch_assign192_l(const Assign192Shape &sh, int nseg, hipStream_t stream, const int32_t *pts, const int32_t *ptsc, int64_t ntot, const uint32_t *w, Seg *ds,
                               int k, const double *cent, int32_t *assign, u64 *sums, u64 *cnts, const int *quiet, double *ub, double *lb, u64 *look_stats) {
  switch (sh.ppt) {
    case 1: launch_assign192_t<1, LOOK>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats); break;
    case 2: launch_assign192_t<2, LOOK>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats); break;
    case 3: launch_assign192_t<3, LOOK>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats); break;
    case 4: launch_assign192_t<4, LOOK>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats); break;
    default: launch_assign192_t<5, LOOK>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats); break;
  }
}
void launch_assign192(const Assign192Shape &sh, int nseg, hipStream_t stream, const int32_t *pts, const int32_t *ptsc, int64_t ntot, const uint32_t *w, Seg *ds,
                      int k, const double *cent, int32_t *assign, u64 *sums, u64 *cnts, const int *quiet, double *ub, double *lb, u64 *look_stats) {
  if (knobs().km_first_look) launch_assign192_l<true>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, look_stats);
  else launch_assign192_l<false>(sh, nseg, stream, pts, ptsc, ntot, w, ds, k, cent, assign, sums, cnts, quiet, ub, lb, nullptr);
}

// ---- D = 192: iterations that skip what cannot change (Hamerly's bounds, made exact) ------------------------------------------
// After a few full iterations most tiles sit firmly in their cluster and the centroids barely move, yet the assignment step costs
// the same 16 x 192 double-precision distance terms per tile every time.  Per point two Euclidean bounds are kept: ub >= its distance
// to its own centroid, lb <= its distance to every other one; a centroid update moves them by the centroids' displacements.  While
//      ub < max(lb, half the distance from the own centroid to the nearest other one)
// holds WITH a relative margin of 1e-9 on both sides, the own centroid is strictly the nearest by a margin six orders of magnitude above
// the rounding of the distance arithmetic (192 fused multiply-adds: relative error below 1e-13) and of the bound bookkeeping (every
// step rounds the safe way, with margins of 1e-12), so the assignment the full computation would make -- computed distances, ties to
// the lowest index -- is the one the point already has: it is skipped.  Otherwise the distance to the own centroid is computed
// (tightening ub), and if the test still fails the point is listed and goes through k_assign192 itself, which reads its rows through the list.
// The result is therefore bit for bit that of the plain iterations (and of the oracle); only the work differs.
constexpr double H_ETA = 1e-9;   // margin of the skip test
constexpr int H_SLICE = 1024;    // points per workgroup of k_h_bounds
__global__ __launch_bounds__(256) void k_h_bounds(const int32_t *__restrict__ pts, int64_t n, const Seg *__restrict__ segs,
                                                  const double *__restrict__ cent /* [k][192] */, const int32_t *__restrict__ assign, double *__restrict__ ub, double *__restrict__ lb,
                                                  const double *__restrict__ cmove /* [k] displacement of each centroid, then the largest, the second largest, whose */,
                                                  const double *__restrict__ shalf /* [k] half the distance to the nearest other centroid */, int k,
                                                  int32_t *__restrict__ need, unsigned *__restrict__ need_cnt, const int *__restrict__ quiet) {
  __shared__ int s_list[H_SLICE], s_need[H_SLICE];
  __shared__ int s_nlist, s_nneed;
  __shared__ unsigned s_base;
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * H_SLICE;
  // (the slice's assignments and bounds are asked for together with the flag and the displacements: one round trip, not two)
  constexpr int RB = H_SLICE / 256;
  int b_a[RB];
  double b_u[RB], b_l[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) {
    const int64_t i = i0 + r * 256 + tid;
    const int64_t ii = i < n ? i : i0;  // (the slice's first point exists)
    b_a[r] = assign[ii]; b_u[r] = ub[ii]; b_l[r] = lb[ii];
  }
  const double dmax = cmove[k], dmax2 = cmove[k + 1];
  const int amax = (int)cmove[k + 2];
  if (*quiet >= 0) return;
  if (tid == 0) { s_nlist = 0; s_nneed = 0; }
  __syncthreads();
  // pass 1, every point of the slice: move the bounds with the centroids; the points whose loosened bounds no longer prove them -> LDS list.
  // The four points of a thread go through it side by side -- their loads first, then the table look-ups that depend on them, then the
  // arithmetic, one list append per wave: with a loop that could leave early and an LDS atomic per listed point the compiler kept the
  // points apart, and every point paid its two dependent round trips to memory on its own (this launch is ~20 % of an iteration)
  {
    constexpr int R = H_SLICE / 256;
    int a[R];
    double u[R], l[R], mv[R], sh[R];
    bool valid[R], listed[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      valid[r] = i0 + r * 256 + tid < n;
      a[r] = b_a[r]; u[r] = b_u[r]; l[r] = b_l[r];
    }
#pragma unroll
    for (int r = 0; r < R; r++) { mv[r] = cmove[a[r]]; sh[r] = shalf[a[r]]; }
    int cnt = 0;
    unsigned long long bal[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int64_t i = i0 + r * 256 + tid;
      const double un = (u[r] + mv[r]) * (1.0 + 1e-15);
      double ln = l[r] - (a[r] == amax ? dmax2 : dmax);  // lb bounds the OTHER centroids: the own one's displacement does not loosen it
      ln -= fabs(ln) * 1e-15;
      if (valid[r]) { ub[i] = un; lb[i] = ln; }
      listed[r] = valid[r] && !(un * (1.0 + H_ETA) < fmax(sh[r], ln) * (1.0 - H_ETA));
      bal[r] = __builtin_amdgcn_ballot_w64(listed[r]);
      cnt += __popcll(bal[r]);
    }
    if (cnt) {  // (uniform in the wave)
      const int lane = tid & 63;
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_nlist, cnt);
      base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (listed[r]) s_list[base + __popcll(bal[r] & ((1ull << lane) - 1ull))] = r * 256 + tid;
        base += __popcll(bal[r]);
      }
    }
  }
  __syncthreads();
  // pass 2, the listed ones: the distance to the own centroid tightens ub; 16 lanes per point (12 dimensions each, the row and the centroid's
  // row read as they lie in memory -- a slice without listed points, most of them late in a clustering, reads no centroid at all).  The
  // partial sums add in another order than the scoring's chain does: both stay within 2.2e-14 (relative) of the exact sum, far inside the
  // factor 1 + 1e-12 that makes the root an upper bound of the distance AS SCORED.  Still unproven -> the global list
  const int nlist = s_nlist;
  if (nlist == 0) return;
  const int l16 = tid & 15;
  for (int t0 = 0; t0 < nlist; t0 += 16) {
    const int t = t0 + (tid >> 4);
    const bool act = t < nlist;
    const int64_t i = i0 + s_list[act ? t : 0];
    const int a = assign[i];
    const int4 *p = reinterpret_cast<const int4 *>(pts + i * 192 + l16 * 12);
    const double2 *c = reinterpret_cast<const double2 *>(cent + (int64_t)a * 192 + l16 * 12);
    const int4 v0 = p[0], v1 = p[1], v2 = p[2];
    const double2 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5];
    const int pv[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    const double cv[12] = {c0.x, c0.y, c1.x, c1.y, c2.x, c2.y, c3.x, c3.y, c4.x, c4.y, c5.x, c5.y};
    double sd = 0.0;
#pragma unroll
    for (int j = 0; j < 12; j++) { const double d0 = __dsub_rn((double)pv[j], cv[j]); sd = __fma_rn(d0, d0, sd); }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    if (act && l16 == 0) {
      const double u = sqrt(sd) * (1.0 + 1e-12);
      ub[i] = u;
      if (!(u * (1.0 + H_ETA) < fmax(shalf[a], lb[i]) * (1.0 - H_ETA))) s_need[atomicAdd(&s_nneed, 1)] = s_list[t];
    }
  }
  // the workgroup's share of the global list with ONE atomic on its counter (a counter every listed point of the launch adds to
  // serialises them: ~6 ns each, and the early iterations list tens of thousands)
  __syncthreads();
  const int nneed = s_nneed;
  if (nneed == 0) return;
  if (tid == 0) s_base = atomicAdd(need_cnt, (unsigned)nneed);
  __syncthreads();
  for (int t = tid; t < nneed; t += 256) need[s_base + t] = (int32_t)(i0 + s_need[t]);
}

// The listed points through the full computation: k_assign192's arithmetic (sum over dimensions in order of (p - c)^2, one IEEE subtraction
// and one fused multiply-add each, ties -> lowest centroid) and its carried sums, shaped for FEW points: one point per lane read straight
// from the chunk-major copy (32 bytes per chunk, the next chunk in flight), the centroids broadcast from LDS (staged from the transposed
// copy k_h_update leaves; reading them as scalar operands through the scalar cache instead measured 20 % slower: 24 KB of centroids do
// not stay in it).  (A thread-per-point form of it was the first list kernel; the four-lane form below replaced it.)
// The same, a point spread over 4 lanes (each lane scores 4 of the 16 centroids of a pass): the thread-per-point shape leaves a lone wave per
// SIMD with 6 144 dependent-ish double-precision operations and its workgroup's four waves queueing for 24 KB of LDS reads per point; here
// the chain is a quarter as long and the list covers four times as many compute units.  Every accumulator still sums its 192 terms in
// order, so the distances are the same doubles; the lanes' (best, second best) merge by (distance, centroid index), which is what the
// in-order scan with its strict `<` computes.
template <int N>
__device__ __forceinline__ void pin_accumulators(double (&s)[N]) {  // an empty statement the optimiser must have the values ready for
#pragma unroll
  for (int c = 0; c < N; c++) asm volatile("" : "+v"(s[c]));
}

template <int Q>
__device__ __forceinline__ int quad_bcast(int v) {  // lane Q of every group of four lanes, to its whole group
  return __builtin_amdgcn_update_dpp(0, v, Q | (Q << 2) | (Q << 4) | (Q << 6), 0xf, 0xf, true);
}

__device__ __forceinline__ void assign192_list4_body(const int32_t *__restrict__ pts, const int32_t *__restrict__ pts_chunked, int64_t n_total,
                                                         const uint32_t *__restrict__ w, Seg *__restrict__ segs, int k, const double *__restrict__ cent_t /* [192][kt] */,
                                                         int kt, int32_t *__restrict__ assign, u64 *__restrict__ sums, u64 *__restrict__ cnts,
                                                         double *__restrict__ ub, double *__restrict__ lb, const int32_t *__restrict__ need,
                                                         const unsigned cnt /* the list's length; no list: every point */) {
  constexpr int D = 192, NP = 64, CPL = KCH / 4;  // points per pass of a workgroup, centroids per lane and pass
  if (blockIdx.x * (unsigned)NP >= cnt) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ int s_nmoved;
  const int kk = segs[0].kk, tid = threadIdx.x, slot = tid >> 2, sub = tid & 3;
  double *s_c = reinterpret_cast<double *>(s_raw);                    // [D][KCH]
  u64 *s_delta = reinterpret_cast<u64 *>(s_raw + D * KCH * 8);       // [kk][D + 1]
  int32_t *s_moved = reinterpret_cast<int32_t *>(s_delta + kk * (D + 1));  // [NP][3]: slot, old, new
  // a fixed grid walks the list (a workgroup per 64 listed points was 5 000 workgroups launched to find that 4 950 have nothing to do,
  // each staging the centroids first); with at most KCH centroids they are staged once per workgroup
  const bool single = kk <= KCH;
  // The four lanes of a point each fetch a quarter of its row (48 dimensions, 12 loads of 16 bytes, all of them in flight together: ONE
  // round trip to memory per point -- the chunk-major copy the plain iterations stream cost a listed point twelve round trips, two chunks
  // at a time, and a short list is all latency) and hand the values round inside their group of four with DPP broadcasts, in the order
  // of the dimensions.  The first pass's rows are asked for before anything else.
  auto fetch = [&](unsigned row0, int4 (&x)[12], int64_t &gi, bool &active) {
    active = row0 + slot < cnt;
    gi = need ? need[active ? row0 + slot : row0] : (int64_t)(active ? row0 + slot : row0);
    const int4 *src = reinterpret_cast<const int4 *>(pts + gi * D + sub * 48);
#pragma unroll
    for (int u = 0; u < 12; u++) x[u] = src[u];
  };
  int4 x[12];
  int64_t gi;
  bool active;
  fetch(blockIdx.x * (unsigned)NP, x, gi, active);
  for (int e = tid; e < kk * (D + 1); e += 256) s_delta[e] = 0;
  if (tid == 0) s_nmoved = 0;
  if (single)
    for (int e = tid; e < D * KCH; e += 256) s_c[e] = cent_t[(int64_t)(e / KCH) * kt + (e % KCH)];
  __syncthreads();
  int total_moved = 0;
#pragma unroll 1
  for (unsigned row0 = blockIdx.x * (unsigned)NP; row0 < cnt; row0 += gridDim.x * (unsigned)NP) {
    double bd = 1.0e300, bd2 = 1.0e300;
    int bc = 0x7fffffff;
#pragma unroll 1
    for (int c0 = 0; c0 < kk; c0 += KCH) {
      if (!single) {
        __syncthreads();
        for (int e = tid; e < D * KCH; e += 256) s_c[e] = cent_t[(int64_t)(e / KCH) * kt + c0 + (e % KCH)];
        __syncthreads();
      }
      double s[CPL];
#pragma unroll
      for (int c = 0; c < CPL; c++) s[c] = 0.0;
      auto term = [&](int v, int j) {  // dimension j of the point against this lane's CPL centroids
        const double pj = (double)v;
        const double *cj = s_c + j * KCH + sub * CPL;
#pragma unroll
        for (int c = 0; c < CPL; c += 2) {
          const double2 cv = *reinterpret_cast<const double2 *>(cj + c);
          const double t0 = __dsub_rn(pj, cv.x), t1 = __dsub_rn(pj, cv.y);
          s[c] = __fma_rn(t0, t0, s[c]);
          s[c + 1] = __fma_rn(t1, t1, s[c + 1]);
        }
      };
      auto quarter = [&](auto qtag) {  // the 48 dimensions lane Q of the group holds
        constexpr int Q = decltype(qtag)::value;
#pragma unroll
        for (int u = 0; u < 12; u++) {
          term(quad_bcast<Q>(x[u].x), Q * 48 + u * 4);
          term(quad_bcast<Q>(x[u].y), Q * 48 + u * 4 + 1);
          term(quad_bcast<Q>(x[u].z), Q * 48 + u * 4 + 2);
          term(quad_bcast<Q>(x[u].w), Q * 48 + u * 4 + 3);
          // the accumulators pinned here: without it the optimiser sinks the whole unrolled chain of multiply-adds below its 384 centroid
          // reads, which then all have to stay live (1 500 spilled registers, the kernel eight times slower)
          pin_accumulators(s);
        }
      };
      quarter(std::integral_constant<int, 0>{});
      quarter(std::integral_constant<int, 1>{});
      quarter(std::integral_constant<int, 2>{});
      quarter(std::integral_constant<int, 3>{});
#pragma unroll
      for (int c = 0; c < CPL; c++) {
        const int ci = c0 + sub * CPL + c;
        if (ci < kk) {  // this lane's centroids come in ascending order: strict `<` keeps the lowest index among equals
          if (s[c] < bd) { bd2 = bd; bd = s[c]; bc = ci; }
          else if (s[c] < bd2) bd2 = s[c];
        }
      }
    }
    const int64_t gi_cur = gi;
    const bool active_cur = active;
    {  // the next pass's rows, while this one's results are merged and written
      const unsigned nrow0 = row0 + gridDim.x * (unsigned)NP;
      if (nrow0 < cnt) fetch(nrow0, x, gi, active);
    }
    // the four lanes of a point: the best by (distance, index); the second best distance = the smallest of the rest
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
      const double od = __shfl_xor(bd, o), od2 = __shfl_xor(bd2, o);
      const int oc = __shfl_xor(bc, o);
      const bool take = od < bd || (od == bd && oc < bc);
      const double loser = take ? bd : od;
      bd2 = fmin(fmin(bd2, od2), loser);
      if (take) { bd = od; bc = oc; }
    }
    if (active_cur && sub == 0) {
      ub[gi_cur] = sqrt(bd) * (1.0 + 1e-12);
      lb[gi_cur] = sqrt(bd2) * (1.0 - 1e-12);
      const int old = assign[gi_cur];
      if (old != bc) {
        assign[gi_cur] = bc;
        const int m = atomicAdd(&s_nmoved, 1);
        s_moved[m * 3] = slot; s_moved[m * 3 + 1] = old; s_moved[m * 3 + 2] = bc;
      }
    }
    __syncthreads();
    const int nmoved = s_nmoved;
    total_moved += nmoved;
#pragma unroll 2
    for (int e = tid >> 6; e < nmoved; e += 4) {  // a wave per moved row between the carried sums (coalesced read, three dimensions per lane)
      const int old = s_moved[e * 3 + 1], nw = s_moved[e * 3 + 2];
      const int64_t mi = need ? need[row0 + s_moved[e * 3]] : (int64_t)(row0 + s_moved[e * 3]);
      const long long wi = w ? (long long)w[mi] : 1;
#pragma unroll
      for (int j = tid & 63; j <= D; j += 64) {
        const u64 v = j < D ? (u64)(wi * pts[mi * D + j]) : (u64)wi;
        atomicAdd(&s_delta[nw * (D + 1) + j], v);
        if (old >= 0) atomicAdd(&s_delta[old * (D + 1) + j], (u64)0 - v);
      }
    }
    __syncthreads();  // the moved list has been read
    if (tid == 0) s_nmoved = 0;
    __syncthreads();
  }
  if (total_moved == 0) return;
  if (tid == 0) atomicAdd(&segs[0].changed, total_moved);
  for (int e = tid; e < kk * (D + 1); e += 256) {
    const u64 v = s_delta[e];
    if (v == 0) continue;
    const int c = e / (D + 1), j = e - c * (D + 1);
    if (j == D) atomicAdd(&cnts[c], v);
    else atomicAdd(&sums[(int64_t)c * D + j], v);
  }
}

// The same for at most KCH centroids, a lane per (point, centroid) pair: 16 points per pass of a workgroup, their rows staged through
// LDS (the 16 lanes of a point read one address), one chain of 192 terms per lane instead of four of them.  Late in a clustering the list
// holds a few thousand points: with 64 points per workgroup that was 16-80 busy workgroups each working through four-chain passes; here
// it is four times as many workgroups with passes a third as long.  Every accumulator still sums its 192 terms in order; the 16 lanes'
// (best, second best) merge by (distance, centroid index), which is what the in-order scan with its strict `<` computes.
constexpr int L16_P = 16;
__device__ __forceinline__ void assign192_list16_body(const int32_t *__restrict__ pts, int64_t n_total, const uint32_t *__restrict__ w, Seg *__restrict__ segs,
                                                          const double *__restrict__ cent_t /* [192][kt] */, int kt, int32_t *__restrict__ assign, u64 *__restrict__ sums,
                                                          u64 *__restrict__ cnts, double *__restrict__ ub, double *__restrict__ lb,
                                                          const int32_t *__restrict__ need, const unsigned cnt) {
  constexpr int D = 192;
  if (blockIdx.x * (unsigned)L16_P >= cnt) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  double *const s_c = reinterpret_cast<double *>(s_raw);                 // [D][KCH] (zero beyond kk: cent_t is)
  u64 *const s_delta = reinterpret_cast<u64 *>(s_raw + D * KCH * 8);    // [kk][D + 1]
  __shared__ __attribute__((aligned(16))) int s_rows[L16_P * D];
  __shared__ int s_moved[L16_P * 3], s_gi[L16_P], s_nmoved;
  const int kk = segs[0].kk, tid = threadIdx.x, pslot = tid >> 4, cl = tid & 15, wave = tid >> 6, lane = tid & 63;
  auto stage = [&](unsigned row0, int4 (&x)[3]) {  // the pass's rows: 16 x 768 bytes, three 16-byte pieces per thread
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const int piece = u * 256 + tid, pr = piece / 48, off = piece - pr * 48;
      const int64_t gi = need[min(row0 + (unsigned)pr, cnt - 1)];
      x[u] = reinterpret_cast<const int4 *>(pts + gi * D)[off];
    }
  };
  int4 x[3];
  stage(blockIdx.x * (unsigned)L16_P, x);
  for (int e = tid; e < kk * (D + 1); e += 256) s_delta[e] = 0;
  if (tid == 0) s_nmoved = 0;
  for (int e = tid; e < D * KCH; e += 256) s_c[e] = cent_t[(int64_t)(e / KCH) * kt + (e % KCH)];
  int total_moved = 0;
#pragma unroll 1
  for (unsigned row0 = blockIdx.x * (unsigned)L16_P; row0 < cnt; row0 += gridDim.x * (unsigned)L16_P) {
    __syncthreads();  // the rows of the pass before are no longer read (first pass: s_c, s_delta are whole)
#pragma unroll
    for (int u = 0; u < 3; u++) reinterpret_cast<int4 *>(s_rows)[u * 256 + tid] = x[u];
    if (tid < L16_P) s_gi[tid] = need[min(row0 + (unsigned)tid, cnt - 1)];
    __syncthreads();
    {
      const unsigned nrow0 = row0 + gridDim.x * (unsigned)L16_P;
      if (nrow0 < cnt) stage(nrow0, x);  // the next pass's rows, while this one is scored
    }
    const bool active = row0 + pslot < cnt;
    const int64_t gi = s_gi[pslot];
    double sacc = 0.0;
    {
      const int *rp = s_rows + pslot * D;
      const double *cp = s_c + cl;
#pragma unroll 16
      for (int j = 0; j < D; j++) {
        const double t0 = __dsub_rn((double)rp[j], cp[j * KCH]);
        sacc = __fma_rn(t0, t0, sacc);
      }
    }
    double bd = cl < kk ? sacc : 1.0e300, bd2 = 1.0e300;
    int bc = cl < kk ? cl : 0x7fffffff;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {  // the 16 lanes of a point: the best by (distance, index); the second best distance = the smallest of the rest
      const double od = __shfl_xor(bd, o), od2 = __shfl_xor(bd2, o);
      const int oc = __shfl_xor(bc, o);
      const bool take = od < bd || (od == bd && oc < bc);
      const double loser = take ? bd : od;
      bd2 = fmin(fmin(bd2, od2), loser);
      if (take) { bd = od; bc = oc; }
    }
    if (active && cl == 0) {
      ub[gi] = sqrt(bd) * (1.0 + 1e-12);
      lb[gi] = sqrt(bd2) * (1.0 - 1e-12);
      const int old = assign[gi];
      if (old != bc) {
        assign[gi] = bc;
        const int m = atomicAdd(&s_nmoved, 1);
        s_moved[m * 3] = pslot; s_moved[m * 3 + 1] = old; s_moved[m * 3 + 2] = bc;
      }
    }
    __syncthreads();
    const int nmoved = s_nmoved;
    total_moved += nmoved;
    for (int e = wave; e < nmoved; e += 4) {  // a wave per moved row between the carried sums (its row is still in LDS)
      const int old = s_moved[e * 3 + 1], nw = s_moved[e * 3 + 2], ps = s_moved[e * 3];
      const int64_t mi = s_gi[ps];
      const long long wi = w ? (long long)w[mi] : 1;
#pragma unroll
      for (int j = lane; j <= D; j += 64) {
        const u64 v = j < D ? (u64)(wi * s_rows[ps * D + j]) : (u64)wi;
        atomicAdd(&s_delta[nw * (D + 1) + j], v);
        if (old >= 0) atomicAdd(&s_delta[old * (D + 1) + j], (u64)0 - v);
      }
    }
    __syncthreads();  // the moved list has been read
    if (tid == 0) s_nmoved = 0;
  }
  if (total_moved == 0) return;
  if (tid == 0) atomicAdd(&segs[0].changed, total_moved);
  for (int e = tid; e < kk * (D + 1); e += 256) {
    const u64 v = s_delta[e];
    if (v == 0) continue;
    const int c = e / (D + 1), j = e - c * (D + 1);
    if (j == D) atomicAdd(&cnts[c], v);
    else atomicAdd(&sums[(int64_t)c * D + j], v);
  }
}

// The list kernel: the four-lanes-per-point passes for long lists (the early iterations: tens of thousands of unproven points, where 64
// points per pass keep the chip's double-precision pipes full), the lane-per-pair passes for short ones (measured on the two bench
// clips: 31.9 against 21.7 microseconds per launch over the frozen clip's 87 iterations, 17.3 against 19.7 over the literal clip's 295).
#ifndef TM_LIST16_BELOW
#define TM_LIST16_BELOW 8192
#endif
constexpr unsigned LIST16_BELOW = TM_LIST16_BELOW;
__global__ __launch_bounds__(256) void k_assign192_list4(const int32_t *__restrict__ pts, const int32_t *__restrict__ pts_chunked, int64_t n_total,
                                                         const uint32_t *__restrict__ w, Seg *__restrict__ segs, int k, const double *__restrict__ cent_t /* [192][kt] */,
                                                         int kt, int32_t *__restrict__ assign, u64 *__restrict__ sums, u64 *__restrict__ cnts, const int *__restrict__ quiet,
                                                         double *__restrict__ ub, double *__restrict__ lb, const int32_t *__restrict__ need,
                                                         const unsigned *__restrict__ need_cnt) {
  const int q0 = *quiet;                                   // (the two control words in one round trip)
  const unsigned cnt0 = need ? *need_cnt : (unsigned)n_total;
  if (q0 >= 0) return;
  if (need && k <= KCH && cnt0 < LIST16_BELOW) assign192_list16_body(pts, n_total, w, segs, cent_t, kt, assign, sums, cnts, ub, lb, need, cnt0);
  else assign192_list4_body(pts, pts_chunked, n_total, w, segs, k, cent_t, kt, assign, sums, cnts, ub, lb, need, cnt0);
}

// the seeds' centroids into the transposed copy the list kernels read (k_h_update keeps it current afterwards)
__global__ void k_cent_transpose(const Seg *__restrict__ segs, const double *__restrict__ cent, double *__restrict__ cent_t, int kt) {
  const int kk = segs[0].kk;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < kk * 192; e += gridDim.x * blockDim.x) { const int c = e / 192, j = e - c * 192; cent_t[(int64_t)j * kt + c] = cent[e]; }
}

// k_update_all for one segment, plus what the bounds need: how far every centroid moved (rounded up) and half its distance to the
// nearest other centroid (rounded down)
__global__ __launch_bounds__(1024) void k_h_update(Seg *__restrict__ segs, int k, u64 *__restrict__ sums, u64 *__restrict__ cnts, double *__restrict__ cent,
                                                   double *__restrict__ cent_t /* [192][kt], zero beyond kk */, int kt, double *__restrict__ cmove,
                                                   double *__restrict__ shalf, unsigned *__restrict__ need_cnt, int it, int *__restrict__ quiet_iter,
                                                   int *host_quiet = nullptr /* page-locked host word that gets the flag too */) {
  extern __shared__ double s_new[];  // [kk][193] (odd pitch: the pair loop reads two rows at once)
  __shared__ unsigned long long s_min[H_MAXK];
  __shared__ double s_move[H_MAXK];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // (the first centroid of every wave is asked for together with the two words that say how many there are and whether anything moved:
  // one round trip to memory instead of two at the head of a launch that is all latency)
  u64 cn0 = 0, sm0[3] = {0, 0, 0};
  double old0[3] = {0.0, 0.0, 0.0};
  if (wave < k) {
    cn0 = cnts[wave];
#pragma unroll
    for (int u = 0; u < 3; u++) { old0[u] = cent[wave * 192 + lane + 64 * u]; sm0[u] = sums[wave * 192 + lane + 64 * u]; }
  }
  const int kk = segs[0].kk;
  const bool changed = segs[0].changed != 0;
  if (*quiet_iter >= 0) return;
  auto wave_sum = [&](double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; };
  if (tid < H_MAXK) s_min[tid] = 0x7ff0000000000000ull;  // +inf
  if (tid == 0) *need_cnt = 0;
  // a wave per centroid, 3 dimensions per lane: new position, displacement (the sums only feed the bounds, margins of 1e-9: their order is free)
  for (int c = wave; c < kk; c += 16) {
    const u64 cn = c == wave ? cn0 : cnts[c];
    double sd = 0.0;
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const int j = lane + 64 * u;
      const double old = c == wave ? old0[u] : cent[c * 192 + j];
      double nw = old;
      if (changed && cn > 0) { nw = __ddiv_rn((double)(long long)(c == wave ? sm0[u] : sums[c * 192 + j]), (double)(long long)cn); cent[c * 192 + j] = nw; }
      s_new[c * 193 + j] = nw;
      cent_t[(int64_t)j * kt + c] = nw;
      const double t = nw - old;
      sd += t * t;
    }
    sd = wave_sum(sd);
    if (lane == 0) { const double mv = sqrt(sd) * (1.0 + 1e-9); cmove[c] = mv; s_move[c] = mv; }
  }
  __syncthreads();
  for (int pr = tid >> 4; pr < kk * kk; pr += 64) {  // pairwise distances, 16 lanes per pair: the smallest per centroid (non-negative doubles order like their bit patterns)
    const int a = pr / kk, b = pr - a * kk;
    if (a >= b) continue;  // (uniform in a group of 16 lanes, and the exchanges below stay inside one)
    double sd = 0.0;
#pragma unroll
    for (int u = 0; u < 12; u++) { const int j = (tid & 15) + 16 * u; const double t = s_new[a * 193 + j] - s_new[b * 193 + j]; sd += t * t; }
    for (int o = 8; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    if ((tid & 15) == 0) {
      atomicMin(&s_min[a], (unsigned long long)__double_as_longlong(sd));
      atomicMin(&s_min[b], (unsigned long long)__double_as_longlong(sd));
    }
  }
  __syncthreads();
  if (tid < kk) shalf[tid] = kk > 1 ? 0.5 * sqrt(__longlong_as_double((long long)s_min[tid])) * (1.0 - 1e-9) : 1.0e300;
  if (wave == 0) {  // the largest displacement, the largest among the others, and whose the largest is (the first of several): over the lanes of a wave
    static_assert(H_MAXK <= 64, "one lane per centroid");
    const double v = lane < kk ? s_move[lane] : 0.0;
    double mx = v;
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    const int amx = __builtin_ctzll(__builtin_amdgcn_ballot_w64(v == mx && (lane < kk || mx == 0.0)));
    double mx2 = lane == amx ? 0.0 : v;
    for (int o = 32; o > 0; o >>= 1) mx2 = fmax(mx2, __shfl_xor(mx2, o));
    if (lane == 0) {
      cmove[k] = mx; cmove[k + 1] = mx2; cmove[k + 2] = (double)amx;
      if (!changed && *quiet_iter < 0) {
        *quiet_iter = it;
        if (host_quiet) __hip_atomic_store(host_quiet, it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      segs[0].changed = 0;
    }
  }
}

// ---- D = 192, at most KCH centroids: ALL skipping iterations in ONE resident launch (round 5) -----------------------------------------
// The three launches of a skipping iteration (k_h_bounds, k_assign192_list4, k_h_update) are each a chain of dependent round trips to
// memory -- 11 + 14.5 + 8.3 microseconds for a few thousand unproven points out of 320 705, 295 times on the literal bench clip.  Here one
// workgroup of 1024 threads per CU stays resident for the whole clustering:
//   * a workgroup OWNS up to 2 x 1024 points (interleaved over the grid, so that unproven points spread evenly); their assignment and
//     their two bounds live in LDS (bounds as Singles rounded the safe way: a bound only has to be a bound), so the pass over all points
//     that moves the bounds with the centroids touches no memory at all;
//   * every workgroup keeps its own copy of the centroids and of the carried integer sums, and applies every iteration's update itself
//     (16 x 192 quotients, displacements, pairwise half-distances: identical arithmetic in every workgroup, so no exchange);
//   * what crosses workgroups per iteration is ONE thing: the integer deltas of the sums caused by the points that moved (u64 atomic adds
//     into one of three rotating buffers, exact and order-free) plus their count, behind ONE barrier of the grid.  Every cross-workgroup
//     datum is an agent-scope atomic on both sides (adds, relaxed 8-byte loads, relaxed stores to clear), every storing wave drains its
//     vmcnt before its workgroup arrives, every load of the data comes after a workgroup barrier behind the poll: the hand-off form of
//     MI355X_MICROARCH.md "Valid forms" that needs no L2 write-back and no L1 invalidate -- the two fences were 23 of the 103 microseconds
//     of round 2's resident attempt, its thread-per-point passes most of the rest;
//   * unproven points: the distance to the own centroid first (16 lanes per point, k_h_bounds' arithmetic), then the full scoring with a
//     lane per (point, centroid) pair, 64 points per pass, rows in LDS -- k_assign192_list4's lane-per-pair arithmetic: every accumulator
//     sums its 192 terms in order, ties to the lowest centroid.
// The skip rule is sound (every bound rounded the safe way, the margins of k_h_bounds), so the assignments, hence the sums, centroids and
// iteration count, are bit for bit those of the plain iterations, of the three-launch path (TM_KM_LAUNCHES=1) and of the oracle.
#ifndef TM_KMR_STAMPS
#define TM_KMR_STAMPS 0
#endif
constexpr int HR_NT = 1024, HR_P = 64, HR_PITCH = KCH + 1, HR_MAXR = 2, HR_E = KCH * 193;
constexpr int HR_NSTAMP = 12;
struct HrState {                    // zeroed before the launch
  u64 delta[3][HR_E];              // the sums' deltas of one iteration ([c][193], the count last); three in rotation
  unsigned changed[3];             // points that moved in that iteration
  unsigned timeout;                // a barrier gave up (a workgroup was not resident)
  BarrierLine bar[8], top[8];      // grid_barrier's
  u64 stamps[HR_NSTAMP + 4];       // diagnostic build: s_memtime spans of workgroup 0's phases; listed / rechecked-and-failed points of all workgroups
#if TM_KMR_STAMPS
  unsigned log[300][10];           // per iteration: workgroup 0's spans of phases 1-7, its listed and scored points, the points scored by all
#endif
};
#if TM_KMR_STAMPS
#define HR_STAMP(i) do { if (g == 0 && tid == 0) { const u64 t_ = __builtin_amdgcn_s_memtime(); s_stamp[i] += t_ - st_last; st_last = t_; } } while (0)
#else
#define HR_STAMP(i) do { } while (0)
#endif

// exchanges inside a row of 16 lanes without the LDS crossbar a __shfl_xor goes through (a data-parallel-primitive move is one vector
// instruction): lane ^ 1, lane ^ 2 (quad permutations), then the mirror image inside 8 and inside 16 lanes -- after the four steps every lane
// of a row has combined all sixteen
template <int CTRL>
__device__ __forceinline__ int hr_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ double hr_dpp(double v) { return __hiloint2double(hr_dpp<CTRL>(__double2hiint(v)), hr_dpp<CTRL>(__double2loint(v))); }
constexpr int HR_X1 = 0xB1, HR_X2 = 0x4E, HR_M8 = 0x141, HR_M16 = 0x140;  // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ double hr_sum16(double v) {
  v += hr_dpp<HR_X1>(v); v += hr_dpp<HR_X2>(v); v += hr_dpp<HR_M8>(v); v += hr_dpp<HR_M16>(v);
  return v;
}

__device__ __forceinline__ float hr_up(double x) { return (float)(x * (1.0 + 1.2e-7)); }                       // a Single >= x (x >= 0, far below FLT_MAX)
__device__ __forceinline__ float hr_down(double x) { x = fmin(x, 1.0e37); return (float)(x - fabs(x) * 1.2e-7); }  // a Single <= x

__device__ __forceinline__ bool hr_barrier(HrState *st, unsigned &epoch, unsigned nblk, int *s_ok) {  // (~2 s: an iteration is microseconds)
  return grid_barrier<(1u << 21)>(st, epoch, nblk, blockIdx.x, s_ok);
}

template <int ROUNDS /* 1024-point rounds a workgroup owns: a constant, so that the LDS arrays' places are */>
__global__ __launch_bounds__(HR_NT) void k_h_resident(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, int64_t n, Seg *__restrict__ segs, int k,
                                                      double *__restrict__ cent /* [k][192], in and out */, const u64 *__restrict__ sums, const u64 *__restrict__ cnts,
                                                      const double *__restrict__ cmove, const double *__restrict__ shalf, int32_t *__restrict__ assign,
                                                      const double *__restrict__ ub, const double *__restrict__ lb, HrState *__restrict__ st, int it0, int max_iter,
                                                      int *__restrict__ quiet_iter) {
  constexpr int D = 192, rounds = ROUNDS;
  static_assert(ROUNDS >= 1 && ROUNDS <= HR_MAXR, "rounds");
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  double *const s_c = reinterpret_cast<double *>(s_raw);                                      // [D][HR_PITCH]: centroid c, dimension j at j * HR_PITCH + c
  u64 *const s_sum = reinterpret_cast<u64 *>(s_raw + D * HR_PITCH * 8);                      // [KCH][193] carried sums, the count last
  u64 *const s_delta = s_sum + HR_E;                                                          // [KCH][193] this workgroup's deltas of the iteration
  int *const s_rows = reinterpret_cast<int *>(s_delta + HR_E);                                // [HR_P][D] rows of the points being scored
  float *const s_ub = reinterpret_cast<float *>(s_rows + HR_P * D);                           // [rounds * 1024]
  float *const s_lb = s_ub + rounds * HR_NT;
  uint16_t *const s_list = reinterpret_cast<uint16_t *>(s_lb + rounds * HR_NT);              // slots whose loosened bounds prove nothing
  uint16_t *const s_need = s_list + rounds * HR_NT;                                           // slots to score
  unsigned *const s_w = reinterpret_cast<unsigned *>(s_need + rounds * HR_NT);                // the points' weights (a moved point's comes from here, not from memory behind the chain)
  uint8_t *const s_a = reinterpret_cast<uint8_t *>(s_w + rounds * HR_NT);                     // assignment (0xff: no point in the slot)
  __shared__ double s_move[KCH + 2], s_half[KCH];
  __shared__ unsigned long long s_min[KCH];
  __shared__ int s_amax, s_nlist, s_nneed, s_nmoved, s_ok;
  __shared__ int s_moved[HR_P * 3];
  __shared__ unsigned s_wt[HR_P];
  __shared__ uint16_t s_pair[KCH * (KCH - 1) / 2];  // the centroid pairs a < b, a | b << 8
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = tid >> 4, l16 = tid & 15;
  const int g = blockIdx.x;
  const unsigned G = gridDim.x;
  if (*quiet_iter >= 0) return;  // converged in the plain iterations (every workgroup reads the same word)
  const int kk = segs[0].kk;
  auto gidx = [&](int slot) { return (int64_t)slot * G + g; };  // point i belongs to workgroup i % G: every workgroup the same share of every stretch of the tiles
#if TM_KMR_STAMPS
  __shared__ u64 s_stamp[HR_NSTAMP];  // (accumulated in LDS, written out at the end: a global read-modify-write per stamp costs more than most phases)
  __shared__ u64 s_prev[8];
  if (tid < HR_NSTAMP) s_stamp[tid] = 0;
  if (tid < 8) s_prev[tid] = 0;
  __syncthreads();
  u64 st_last = __builtin_amdgcn_s_memtime();
#endif
  // ---- state in: the centroids, the carried sums, the bounds the last plain iteration left, what the last update says about the centroids
  for (int e = tid; e < D * HR_PITCH; e += HR_NT) { const int j = e / HR_PITCH, c = e - j * HR_PITCH; s_c[e] = c < kk ? cent[c * D + j] : 0.0; }
  for (int e = tid; e < HR_E; e += HR_NT) {
    const int c = e / 193, j = e - c * 193;
    s_sum[e] = c < kk ? (j < D ? sums[c * D + j] : cnts[c]) : 0;
    s_delta[e] = 0;
  }
  for (int r = 0; r < rounds; r++) {
    const int slot = r * HR_NT + tid;
    const int64_t i = gidx(slot);
    const bool valid = i < n;
    s_a[slot] = valid ? (uint8_t)assign[i] : (uint8_t)0xff;
    s_ub[slot] = valid ? hr_up(ub[i]) : 0.0f;
    s_lb[slot] = valid ? hr_down(lb[i]) : 0.0f;
    s_w[slot] = valid && w ? w[i] : 1u;
  }
  if (tid < KCH) { s_move[tid] = tid < kk ? cmove[tid] : 0.0; s_half[tid] = tid < kk ? shalf[tid] : 0.0; }
  if (tid < kk * kk) {
    const int a = tid / kk, b2 = tid - a * kk;
    if (a < b2) s_pair[a * kk - a * (a + 1) / 2 + (b2 - a - 1)] = (uint16_t)(a | (b2 << 8));
  }
  if (tid == 0) { s_move[KCH] = cmove[k]; s_move[KCH + 1] = cmove[k + 1]; s_amax = (int)cmove[k + 2]; s_nlist = 0; s_nneed = 0; s_nmoved = 0; }
  unsigned epoch = 0;
  int it = it0, quiet_at = -1;
  __syncthreads();
  HR_STAMP(0);
  for (; it < max_iter; it++) {
    const int b = it % 3;
    // ---- pass over all owned points: the bounds move with the centroids; what they no longer prove goes on the list
    {
      const double dmax = s_move[KCH], dmax2 = s_move[KCH + 1];
      const int amax = s_amax;
      int cnt = 0;
      unsigned long long bal[HR_MAXR];
      bool listed[HR_MAXR];
#pragma unroll
      for (int r = 0; r < HR_MAXR; r++) {
        listed[r] = false;
        if (r < rounds) {
          const int slot = r * HR_NT + tid;
          const int a = s_a[slot];
          const bool valid = a != 0xff;
          const int ac = valid ? a : 0;
          const double un = (double)s_ub[slot] + s_move[ac];
          const double ln = (double)s_lb[slot] - (a == amax ? dmax2 : dmax);  // lb bounds the OTHER centroids: the own one's displacement does not loosen it
          const float unf = hr_up(un), lnf = hr_down(ln);
          if (valid) { s_ub[slot] = unf; s_lb[slot] = lnf; }
          listed[r] = valid && !((double)unf * (1.0 + H_ETA) < fmax(s_half[ac], (double)lnf) * (1.0 - H_ETA));
        }
        bal[r] = __builtin_amdgcn_ballot_w64(listed[r]);
        cnt += __popcll(bal[r]);
      }
      if (cnt) {  // (uniform in the wave)
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_nlist, cnt);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int r = 0; r < HR_MAXR; r++) {
          if (listed[r]) s_list[base + __popcll(bal[r] & ((1ull << lane) - 1ull))] = (uint16_t)(r * HR_NT + tid);
          base += __popcll(bal[r]);
        }
      }
    }
    __syncthreads();
    HR_STAMP(1);
    // ---- the listed points: the distance to the own centroid tightens ub (16 lanes per point, 12 dimensions each: k_h_bounds' arithmetic -- the
    // partial sums add in another order than the scoring's chain; both stay within 2.2e-14 of the exact sum, far inside the factor 1 + 1e-12).
    // Still unproven -> the need list; the first HR_P of them leave their rows in LDS for the scoring.
    const int nlist = s_nlist;
    {
      auto rfetch = [&](int t0, int4 (&x)[3], int &slot) {
        const int t = t0 + grp;
        slot = s_list[t < nlist ? t : 0];
        const int4 *p = reinterpret_cast<const int4 *>(pts + gidx(slot) * D + l16 * 12);
        x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
      };
      int4 x[3] = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0)};
      int slot = 0;
      if (nlist > 0) rfetch(0, x, slot);
#pragma unroll 1
      for (int t0 = 0; t0 < nlist; t0 += HR_P) {
        const bool act = t0 + grp < nlist;
        const int4 v0 = x[0], v1 = x[1], v2 = x[2];
        const int cslot = slot;
        if (t0 + HR_P < nlist) rfetch(t0 + HR_P, x, slot);  // the next pass's rows, while this one's are summed
        const int a = s_a[cslot];
        const int pv[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        double sd = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) { const double d0 = __dsub_rn((double)pv[j], s_c[(l16 * 12 + j) * HR_PITCH + a]); sd = __fma_rn(d0, d0, sd); }
        sd = hr_sum16(sd);
        int np = -1;
        if (act && l16 == 0) {
          const float uf = hr_up(sqrt(sd) * (1.0 + 1e-12));
          s_ub[cslot] = uf;
          if (!((double)uf * (1.0 + H_ETA) < fmax(s_half[a], (double)s_lb[cslot]) * (1.0 - H_ETA))) { np = atomicAdd(&s_nneed, 1); s_need[np] = (uint16_t)cslot; }
        }
        np = __shfl(np, lane & 48);
        if (np >= 0 && np < HR_P) {
          int4 *dst = reinterpret_cast<int4 *>(s_rows + np * D + l16 * 12);
          dst[0] = v0; dst[1] = v1; dst[2] = v2;
        }
      }
    }
    __syncthreads();
    HR_STAMP(2);
    // ---- full scoring of the need list, HR_P points per pass, a lane per (point, centroid) pair
    const int nneed = s_nneed;
    int total_moved = 0;
#if TM_KMR_STAMPS
    if (tid == 0 && (nlist | nneed)) { atomicAdd(&st->stamps[HR_NSTAMP], (u64)nlist); atomicAdd(&st->stamps[HR_NSTAMP + 1], (u64)nneed); }
#endif
#pragma unroll 1
    for (int base = 0; base < nneed; base += HR_P) {
      if (base > 0) {  // (the first pass's rows came from the recheck)
#pragma unroll
        for (int u = 0; u < 3; u++) {
          const int piece = u * HR_NT + tid, pr = piece / 48, off = piece - pr * 48;
          const int sl = s_need[min(base + pr, nneed - 1)];
          reinterpret_cast<int4 *>(s_rows)[piece] = reinterpret_cast<const int4 *>(pts + gidx(sl) * D)[off];
        }
        __syncthreads();
      }
      const bool active = base + grp < nneed;
      const int slot = s_need[active ? base + grp : base];
      double bd = 1.0e300, bd2 = 1.0e300;
      int bc = 0x7fffffff;
      if (base + (wave << 2) < nneed) {  // (uniform in the wave: the waves without a point skip the chain)
        // 192 terms in order, four dimensions per step: the NEXT step's LDS reads (a 16-byte read of the row, four centroid values) are
        // issued before this step's arithmetic -- the scheduling barriers keep them there: left alone the compiler reads each operand right
        // before its use and waits out an LDS round trip every second term (24 000 cycles per pass with a lone wave per SIMD; the stamps)
        double sacc = 0.0;
        const int4 *rp = reinterpret_cast<const int4 *>(s_rows + grp * D);
        const double *cp = s_c + l16;
        auto ld = [&](int jb, int4 &r, double (&c)[4]) {
          r = rp[jb];
#pragma unroll
          for (int u = 0; u < 4; u++) c[u] = cp[(jb * 4 + u) * HR_PITCH];
        };
        auto acc = [&](const int4 &r, const double (&c)[4]) {
          const int v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
          for (int u = 0; u < 4; u++) { const double t = __dsub_rn((double)v[u], c[u]); sacc = __fma_rn(t, t, sacc); }
        };
        int4 ra, rb;
        double ca[4], cb[4];
        ld(0, ra, ca);
#pragma unroll
        for (int jb = 0; jb < D / 4; jb += 2) {
          ld(jb + 1, rb, cb);
          __builtin_amdgcn_sched_barrier(0);
          acc(ra, ca);
          __builtin_amdgcn_sched_barrier(0);
          if (jb + 2 < D / 4) ld(jb + 2, ra, ca);
          __builtin_amdgcn_sched_barrier(0);
          acc(rb, cb);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (l16 < kk) { bd = sacc; bc = l16; }
        // the 16 lanes of a point: the best by (distance, index); the second best distance = the smallest of the rest (whatever the pairing)
        auto merge = [&](auto ctrl) {
          constexpr int C = decltype(ctrl)::value;
          const double od = hr_dpp<C>(bd), od2 = hr_dpp<C>(bd2);
          const int oc = hr_dpp<C>(bc);
          const bool take = od < bd || (od == bd && oc < bc);
          const double loser = take ? bd : od;
          bd2 = fmin(fmin(bd2, od2), loser);
          if (take) { bd = od; bc = oc; }
        };
        merge(std::integral_constant<int, HR_X1>{}); merge(std::integral_constant<int, HR_X2>{});
        merge(std::integral_constant<int, HR_M8>{}); merge(std::integral_constant<int, HR_M16>{});
        if (active && l16 == 0) {
          s_ub[slot] = hr_up(sqrt(bd) * (1.0 + 1e-12));
          s_lb[slot] = hr_down(sqrt(bd2) * (1.0 - 1e-12));
          const int old = s_a[slot];
          if (old != bc) {
            s_a[slot] = (uint8_t)bc;
            const int m = atomicAdd(&s_nmoved, 1);
            s_moved[m * 3] = grp; s_moved[m * 3 + 1] = old; s_moved[m * 3 + 2] = bc;
            s_wt[grp] = s_w[slot];
          }
        }
      }
      __syncthreads();
      const int nmoved = s_nmoved;
      total_moved += nmoved;
      for (int e = wave; e < nmoved; e += HR_NT / 64) {  // a wave per moved row between the carried sums (its row is in LDS)
        const int ps = s_moved[e * 3], old = s_moved[e * 3 + 1], nw = s_moved[e * 3 + 2];
        const long long wi = (long long)s_wt[ps];
#pragma unroll
        for (int j = lane; j <= D; j += 64) {
          const u64 v = j < D ? (u64)(wi * s_rows[ps * D + j]) : (u64)wi;
          atomicAdd(&s_delta[nw * 193 + j], v);
          atomicAdd(&s_delta[old * 193 + j], (u64)0 - v);
        }
      }
      __syncthreads();  // the moved list and the rows have been read
      if (tid == 0) s_nmoved = 0;
    }
    HR_STAMP(3);
    // ---- this workgroup's deltas -> the iteration's buffer
    if (total_moved) {
      for (int e = tid; e < HR_E; e += HR_NT) {
        const u64 v = s_delta[e];
        if (v == 0) continue;
        s_delta[e] = 0;
        __hip_atomic_fetch_add(&st->delta[b][e], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (tid == 0) __hip_atomic_fetch_add(&st->changed[b], (unsigned)total_moved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    HR_STAMP(4);
    if (!hr_barrier(st, epoch, G, &s_ok)) return;
    HR_STAMP(5);
    if (tid == 0) { s_nlist = 0; s_nneed = 0; }  // (every thread has read them: the barrier; the next pass over the points comes behind further ones)
    // ---- every workgroup: the iteration's deltas into its own sums; new centroids; what the bounds need
    const unsigned tot = __hip_atomic_load(&st->changed[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {
      u64 dv[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int e = u * HR_NT + tid; dv[u] = e < HR_E ? __hip_atomic_load(&st->delta[b][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0; }
      // the buffer of the iteration after next: read for the last time before the barrier just passed, added to again only behind the next one
      const int b2 = (it + 2) % 3;
      const int per = (HR_E + (int)G - 1) / (int)G;
      // (with fewer than four workgroups a share is longer than the workgroup: up to HR_E = 3 088 entries with one, 1 544 with two, 1 030 with three)
      for (int e = g * per + tid; e < min(HR_E, (g + 1) * per); e += HR_NT) __hip_atomic_store(&st->delta[b2][e], (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g == 0 && tid == 0) __hip_atomic_store(&st->changed[b2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int u = 0; u < 4; u++) { const int e = u * HR_NT + tid; if (e < HR_E && dv[u]) s_sum[e] += dv[u]; }
    }
    if (tot == 0) { quiet_at = it; break; }
    if (tid < KCH) s_min[tid] = 0x7ff0000000000000ull;  // +inf
    __syncthreads();
    HR_STAMP(6);
    // a wave per centroid, 3 dimensions per lane: new position = exact integer sum / weight (one IEEE division; an empty cluster keeps its
    // centroid), displacement (rounded up; the sums here only feed the bounds, margins of 1e-9: their order is free)
    if (wave < kk) {
      const int c = wave;
      const u64 cn = s_sum[c * 193 + D];
      double sd = 0.0;
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int j = lane + 64 * u;
        const double old = s_c[j * HR_PITCH + c];
        double nw = old;
        if (cn > 0) { nw = __ddiv_rn((double)(long long)s_sum[c * 193 + j], (double)(long long)cn); s_c[j * HR_PITCH + c] = nw; }
        const double t = nw - old;
        sd += t * t;
      }
      sd = hr_sum16(sd);
      sd += __shfl_xor(sd, 16);
      sd += __shfl_xor(sd, 32);
      if (lane == 0) s_move[c] = sqrt(sd) * (1.0 + 1e-9);
    }
    __syncthreads();
    for (int pr = grp; pr < kk * (kk - 1) / 2; pr += HR_NT / 16) {  // pairwise distances, 16 lanes per pair: the smallest per centroid (non-negative doubles order like their bit patterns)
      const int ca = s_pair[pr] & 0xff, cb = s_pair[pr] >> 8;
      double sd = 0.0;
#pragma unroll
      for (int u = 0; u < 12; u++) { const int j = l16 + 16 * u; const double t = s_c[j * HR_PITCH + ca] - s_c[j * HR_PITCH + cb]; sd += t * t; }
      sd = hr_sum16(sd);
      if (l16 == 0) {
        atomicMin(&s_min[ca], (unsigned long long)__double_as_longlong(sd));
        atomicMin(&s_min[cb], (unsigned long long)__double_as_longlong(sd));
      }
    }
    if (tid == HR_NT - 1) {  // the largest displacement, the largest among the others, and whose the largest is (the first of several): sixteen values, one lane
      double mv[KCH];
#pragma unroll
      for (int c = 0; c < KCH; c++) mv[c] = s_move[c];
      double mx = 0.0, mx2 = 0.0;
      int amx = 0;
#pragma unroll
      for (int c = 0; c < KCH; c++) {
        const double v = c < kk ? mv[c] : 0.0;
        if (v > mx) { mx2 = mx; mx = v; amx = c; } else mx2 = fmax(mx2, v);
      }
      s_move[KCH] = mx; s_move[KCH + 1] = mx2; s_amax = amx;
    }
    __syncthreads();
    if (tid < kk) s_half[tid] = kk > 1 ? 0.5 * sqrt(__longlong_as_double((long long)s_min[tid])) * (1.0 - 1e-9) : 1.0e300;
    __syncthreads();
    HR_STAMP(7);
#if TM_KMR_STAMPS
    if (g == 0 && tid < 7 && it < 300) { st->log[it][tid] = (unsigned)(s_stamp[tid + 1] - s_prev[tid]); s_prev[tid] = s_stamp[tid + 1]; }
    if (g == 0 && tid == 0 && it < 300) { st->log[it][7] = (unsigned)nlist; st->log[it][8] = (unsigned)nneed; st->log[it][9] = tot; }
#endif
  }
  // ---- state out
  __syncthreads();
#if TM_KMR_STAMPS
  if (g == 0 && tid < HR_NSTAMP) st->stamps[tid] = s_stamp[tid];
#endif
  for (int r = 0; r < rounds; r++) {
    const int slot = r * HR_NT + tid;
    const int64_t i = gidx(slot);
    if (i < n) assign[i] = (int32_t)s_a[slot];
  }
  if (g == 0) {
    for (int e = tid; e < kk * D; e += HR_NT) { const int c = e / D, j = e - c * D; cent[e] = s_c[j * HR_PITCH + c]; }
    if (tid == 0) { segs[0].changed = 0; if (quiet_at >= 0) *quiet_iter = quiet_at; }
  }
}

// ---- host side of the skipping iterations --------------------------------------------------------------------------------------------
int tile_skip_setup(TileRun &t) {
  const int k = t.k;
  const size_t n1 = (size_t)std::max<int64_t>(t.n, 1);
  t.kt = (k + KCH - 1) / KCH * KCH;
  t.l_lds = (size_t)192 * KCH * 8 + (size_t)k * 193 * 8 + (size_t)256 * 3 * 4 + 16;
  // a dynamic-LDS request above the CU's 160 KB comes back from the launch as a bare "invalid argument" (round 2's scratch records hold one,
  // from a k = 64 build of these kernels that kept more in LDS): refuse it here, by name
  TM_CHECK(t.l_lds <= 160 * 1024 && (size_t)k * 193 * 8 <= 160 * 1024, TM_E_INVAL, "k-means: %d centroids need %zu bytes of LDS in the list kernel (the CU has 163840)", k, t.l_lds);
  TM_TRY(t.ub.alloc(n1 * 8)); TM_TRY(t.lb.alloc(n1 * 8)); TM_TRY(t.cent_t.alloc((size_t)t.kt * 192 * 8));
  TM_TRY(t.move.alloc((size_t)(k + 3) * 8)); TM_TRY(t.half.alloc((size_t)k * 8)); TM_TRY(t.need.alloc(n1 * 4)); TM_TRY(t.cnt.alloc(8));
  TM_HIP(hipMemsetAsync(t.cnt.p, 0, 8, t.stream));
  TM_HIP(hipMemsetAsync(t.cent_t.p, 0, (size_t)t.kt * 192 * 8, t.stream));
  hipLaunchKernelGGL(k_cent_transpose, dim3(12), dim3(256), 0, t.stream, t.ds, t.cent, t.cent_t.as<double>(), t.kt);
  if ((size_t)k * 193 * 8 > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_h_update), hipFuncAttributeMaxDynamicSharedMemorySize, k * 193 * 8);
  if (t.l_lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_assign192_list4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.l_lds);
  return TM_OK;
}

void tile_skip_iteration(TileRun &t, int iter, int *pin_dev) {
  if (iter < H_WARM) {
    const bool last_plain = iter == H_WARM - 1;  // it leaves the bounds the skipping iterations start from
    launch_assign192(t.a192, 1, t.stream, t.pts, t.ptsc, t.n, t.w, t.ds, t.k, t.cent, t.assign, t.sums, t.cnts, t.quiet, last_plain ? t.ub.as<double>() : nullptr,
                     last_plain ? t.lb.as<double>() : nullptr, t.look);
  } else {
    hipLaunchKernelGGL(k_h_bounds, dim3((int)((t.n + H_SLICE - 1) / H_SLICE)), dim3(256), 0, t.stream, t.pts, t.n, t.ds, (const double *)t.cent, t.assign, t.ub.as<double>(),
                       t.lb.as<double>(), t.move.as<double>(), t.half.as<double>(), t.k, t.need.as<int32_t>(), t.cnt.as<unsigned>(), t.quiet);
    hipLaunchKernelGGL(k_assign192_list4, dim3((unsigned)std::min<int64_t>((t.n + 63) / 64, t.k <= KCH ? 1024 : 768)), dim3(256), t.l_lds, t.stream, t.pts, t.ptsc, t.n, t.w, t.ds,
                       t.k, t.cent_t.as<double>(), t.kt, t.assign, t.sums, t.cnts, t.quiet, t.ub.as<double>(), t.lb.as<double>(), t.need.as<int32_t>(), t.cnt.as<unsigned>());
  }
  hipLaunchKernelGGL(k_h_update, dim3(1), dim3(1024), (size_t)t.k * 193 * 8, t.stream, t.ds, t.k, t.sums, t.cnts, t.cent, t.cent_t.as<double>(), t.kt, t.move.as<double>(),
                     t.half.as<double>(), t.cnt.as<unsigned>(), iter, t.quiet, pin_dev);
}

// ---- host side of the resident launch ----------------------------------------------------------------------------------------------
// At most KCH centroids and points that fit the chip's LDS HR_MAXR rounds deep, a workgroup per CU.
ResidentPlan resident_plan(int64_t n, int k, int cus) {
  ResidentPlan no{0, 0, 0}, p;
  if (n <= 0 || k > KCH) return no;
  p.grid = (int)std::min<int64_t>(cus, (n + HR_NT - 1) / HR_NT);
  p.rounds = (int)(((n + p.grid - 1) / p.grid + HR_NT - 1) / HR_NT);  // a workgroup owns the points i with i % grid == its index: slots of 1024
  p.lds = (size_t)192 * HR_PITCH * 8 + (size_t)HR_E * 16 + (size_t)HR_P * 192 * 4 + (size_t)p.rounds * HR_NT * (4 + 4 + 2 + 2 + 4 + 1) + 16;
  return p.rounds <= HR_MAXR && p.lds <= 160 * 1024 - 2048 ? p : no;
}

// Should a workgroup not become resident (another process holding CUs with a resident launch of its own) the barrier gives up: gave_up.
int tile_resident(TileRun &t, const ResidentPlan &plan, Resident *verdict, int *iters) {
  DevBuf hstate;
  TM_TRY(hstate.alloc(sizeof(HrState)));
  TM_HIP(hipMemsetAsync(hstate.p, 0, sizeof(HrState), t.stream));
  std::unique_lock<std::mutex> resident_lock(resident_launch_lock());
  auto kres = plan.rounds == 1 ? &k_h_resident<1> : &k_h_resident<2>;
  static_assert(HR_MAXR == 2, "one instantiation per number of rounds");
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kres), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
  for (int i = 0; i < H_WARM; i++) tile_skip_iteration(t, i, nullptr);
  hipLaunchKernelGGL(kres, dim3(plan.grid), dim3(HR_NT), plan.lds, t.stream, t.pts, t.w, t.n, t.ds, t.k, t.cent, t.sums, t.cnts, t.move.as<double>(), t.half.as<double>(), t.assign,
                     t.ub.as<double>(), t.lb.as<double>(), hstate.as<HrState>(), H_WARM, t.max_iter, t.quiet);
  TM_HIP(hipGetLastError());
  int q = -1;
  HrState *hs_dev = hstate.as<HrState>();
  unsigned timed_out = 0;
#if TM_KMR_STAMPS
  std::vector<u64> stamps(HR_NSTAMP + 4);
  std::vector<unsigned> hlog(300 * 10);
#endif
  {
    HostRead hr_(t.stream);
    TM_TRY(hr_.get(&q, t.quiet, 4));
    TM_TRY(hr_.get(&timed_out, &hs_dev->timeout, 4));
#if TM_KMR_STAMPS
    TM_TRY(hr_.get(stamps.data(), hs_dev->stamps, stamps.size() * 8));
    TM_TRY(hr_.get(hlog.data(), hs_dev->log, hlog.size() * 4));
#endif
    TM_TRY(hr_.wait());
  }
  resident_lock.unlock();
  if (knobs().km_resident_fail) timed_out = 1;  // (tests: the path a barrier that gave up takes)
  *verdict = timed_out ? Resident::gave_up : Resident::done;
  if (timed_out) return TM_OK;
  const int it = q >= 0 ? q : t.max_iter;
  *iters = it;
#if TM_KMR_STAMPS
  const double ni = std::max(1, it - H_WARM + (q >= 0 ? 1 : 0));
  static const char *names[8] = {"state in", "bounds pass", "own-centroid recheck", "scoring", "flush", "barrier", "deltas in", "update"};
  fprintf(stderr, "[tm_kmr stamps] %d workgroups x %d rounds, %d resident iterations; workgroup 0, s_memtime ticks per iteration:", plan.grid, plan.rounds, (int)ni);
  for (int i2 = 1; i2 < 8; i2++) fprintf(stderr, " %s %.0f,", names[i2], (double)stamps[i2] / ni);
  fprintf(stderr, " state in %.0f (once); per iteration %.1f points listed, %.1f scored (all workgroups)\n", (double)stamps[0], (double)stamps[HR_NSTAMP] / ni,
          (double)stamps[HR_NSTAMP + 1] / ni);
  for (int i2 = H_WARM; i2 < std::min(it, 300); i2 += (i2 < 16 ? 1 : i2 < 64 ? 8 : 32))
    fprintf(stderr, "[tm_kmr log] iteration %3d: bounds %5u recheck %5u scoring %6u flush %5u barrier %6u deltas %5u update %5u | wg0 listed %4u scored %4u | moved (all) %u\n", i2, hlog[i2 * 10],
            hlog[i2 * 10 + 1], hlog[i2 * 10 + 2], hlog[i2 * 10 + 3], hlog[i2 * 10 + 4], hlog[i2 * 10 + 5], hlog[i2 * 10 + 6], hlog[i2 * 10 + 7], hlog[i2 * 10 + 8], hlog[i2 * 10 + 9]);
#endif
  return TM_OK;
}

}  // namespace tmx
