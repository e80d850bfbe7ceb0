// tm_kmeans_assign192.hip -- the assignment step of the build's k-means (tm_kmeans.hip) for D = 192, the tile -> palette clustering of
// DoPalettization: register-tiled, with the first look of tm_kmeans.h.  The plain iterations of every path run it.
#include "tm_kmeans_tile.h"

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
// k_assign192's dynamic LDS, in bytes, for 256 * ppt rows a workgroup and `kdelta` centroids whose sums' deltas are gathered in LDS (none: they go
// to memory one by one): the kernel carves it, the host sizes it
struct Assign192Lds {
  int rows, kdelta;
  constexpr Assign192Lds(int ppt, int kdelta_) : rows(256 * ppt), kdelta(kdelta_) {}
  constexpr int cent() const { return 0; }                            // double [A_DCH][KCH]; LOOK: the same as Singles, in its first half
  constexpr int pts() const { return A_DCH * KCH * 8; }               // int32 [rows][A_DCH + 1]
  constexpr int moved() const { return pts() + rows * (A_DCH + 1) * 4; }  // int32 [rows][3]: row, old, new
  constexpr int delta() const { return moved() + rows * 3 * 4; }      // u64 [kdelta][T_ROW]
  // LOOK, once the passes are over, in pts' place (24 of its 36 bytes per row): what the chain found for a row in doubt, and their list
  constexpr int xd() const { return pts(); }                          // double [rows][2]: smallest, second smallest
  constexpr int xc() const { return xd() + rows * 16; }               // int32 [rows]: whose the smallest is
  constexpr int doubt() const { return xc() + rows * 4; }             // int32 [rows]
  constexpr size_t used() const { return (size_t)delta() + (size_t)kdelta * T_ROW * 8 + 4; }  // (4: the pad word an odd row count would need)
  constexpr size_t bytes() const { return used() + 16; }
};
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
  constexpr Assign192Lds L(PPT, 0);  // (the offsets do not depend on how many centroids' deltas follow them)
  static_assert(L.rows == ROWS && L.doubt() + ROWS * 4 <= L.moved(), "the first look's results fit in the staged rows' place");
  double(*s_cent)[KCH] = reinterpret_cast<double(*)[KCH]>(s_raw + L.cent());
  float(*s_centf)[KCH] = reinterpret_cast<float(*)[KCH]>(s_raw + L.cent());
  int32_t *s_pts = reinterpret_cast<int32_t *>(s_raw + L.pts());
  int32_t *s_moved = reinterpret_cast<int32_t *>(s_raw + L.moved());
  u64 *s_delta = reinterpret_cast<u64 *>(s_raw + L.delta());                            // [kk][D+1] when lds_delta
  double *s_xd = reinterpret_cast<double *>(s_raw + L.xd());
  int32_t *s_xc = reinterpret_cast<int32_t *>(s_raw + L.xc());
  int32_t *s_doubt = reinterpret_cast<int32_t *>(s_raw + L.doubt());
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
      // E(c) of this pass's centroids: eight partial sums of squares each (any order: rounded up by KM_ETA, nine orders above their rounding)
      if (tid < A_DCH * KCH) s_nrm[tid] = nrm;
      __syncthreads();
      if (tid < KCH) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < A_DCH; j++) q += s_nrm[j * KCH + tid];
        s_E[tid] = sqrt(q) * (FL_CENT * (1.0 + KM_ETA)) + 1.0e-30;
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
      const bool decided = olo[m] * (1.0 - KM_ETA) > bhi[m] * (1.0 + KM_ETA) && mx[m] < FL_INT_EXACT;
      doubt[m] = r < nrows && !decided;
      ubv[m] = bhi[m] * (1.0 + KM_ETA);
      lbv[m] = olo[m] - fabs(olo[m]) * KM_ETA;
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
          ubv[m] = h_ub_of_sum(s_xd[r * 2]);
          lbv[m] = h_lb_of_sum(s_xd[r * 2 + 1]);
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
  for (int m = 0; m < PPT; m++) { ubv[m] = h_ub_of_sum(bd[m]); lbv[m] = h_lb_of_sum(bd2[m]); }
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
  sh.lds_delta = Assign192Lds(sh.ppt, k).used() <= 150 * 1024 ? 1 : 0;
  sh.lds = Assign192Lds(sh.ppt, sh.lds_delta ? k : 0).bytes();
  return sh;
}

template <int PPT, bool LOOK>
static void launch_assign192_t(const Assign192Shape &sh, int nseg, hipStream_t stream, const Assign192Args &a) {
  static bool attr_set = false;
  if (!attr_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_assign192<PPT, LOOK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DYN_LDS_CEILING); attr_set = true; }
  hipLaunchKernelGGL((k_assign192<PPT, LOOK>), dim3(sh.nblk, nseg), dim3(256), sh.lds, stream, a.pts, a.ptsc, a.ntot, a.w, a.ds, a.k, a.cent, a.assign, a.sums, a.cnts, sh.rows, sh.lds_delta,
                     a.quiet, a.ub, a.lb, LOOK ? a.look_stats : nullptr);
}
void launch_assign192(const Assign192Shape &sh, int nseg, hipStream_t stream, const Assign192Args &a) {
  using Launcher = void (*)(const Assign192Shape &, int, hipStream_t, const Assign192Args &);
  static const Launcher by_look_and_ppt[2][5] = {
      {launch_assign192_t<1, false>, launch_assign192_t<2, false>, launch_assign192_t<3, false>, launch_assign192_t<4, false>, launch_assign192_t<5, false>},
      {launch_assign192_t<1, true>, launch_assign192_t<2, true>, launch_assign192_t<3, true>, launch_assign192_t<4, true>, launch_assign192_t<5, true>}};
  by_look_and_ppt[knobs().km_first_look ? 1 : 0][std::min(std::max(sh.ppt, 1), 5) - 1](sh, nseg, stream, a);
}

}  // namespace tmx
