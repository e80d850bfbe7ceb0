// tm_kmeans_skip.hip -- the D = 192 iterations that skip what cannot change (the rule and its bound forms: tm_kmeans_tile.h), three launches
// each: k_h_bounds, the list kernel k_assign192_list4, k_h_update.
#include "tm_kmeans_tile.h"

namespace tmx {

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
      const double un = h_round_up(h_ub_moved(u[r], mv[r]));
      const double ln = h_round_down(h_lb_moved(l[r], a[r] == amax, dmax, dmax2));
      if (valid[r]) { ub[i] = un; lb[i] = ln; }
      listed[r] = valid[r] && !H_PROVEN(un, sh[r], ln);
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
  // factor 1 + H_ROOT that makes the root an upper bound of the distance AS SCORED.  Still unproven -> the global list
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
      const double u = h_ub_of_sum(sd);
      ub[i] = u;
      if (!H_PROVEN(u, shalf[a], lb[i])) s_need[atomicAdd(&s_nneed, 1)] = s_list[t];
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
// the list kernel's dynamic LDS for `centroids` of them: the kernel carves it by the live ones, the host sizes it by k
struct ListLds {
  int centroids;
  __host__ __device__ explicit ListLds(int centroids_) : centroids(centroids_) {}
  static constexpr int cent() { return 0; }                                   // byte offset: double [192][KCH], a pass's centroids, transposed
  static constexpr int delta() { return 192 * KCH * 8; }                      // byte offset: u64 [centroids][T_ROW]
  __host__ __device__ int delta_len() const { return centroids * T_ROW; }     // its u64s; behind them int32 [64][3]: slot, old, new (the four-lane body's)
  __host__ __device__ size_t bytes() const { return (size_t)delta() + (size_t)delta_len() * 8 + 256 * 3 * 4 + 16; }
};

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
  const ListLds L(kk);
  double *s_c = reinterpret_cast<double *>(s_raw + L.cent());
  u64 *s_delta = reinterpret_cast<u64 *>(s_raw + L.delta());
  int32_t *s_moved = reinterpret_cast<int32_t *>(s_delta + L.delta_len());
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
      ub[gi_cur] = h_ub_of_sum(bd);
      lb[gi_cur] = h_lb_of_sum(bd2);
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
  double *const s_c = reinterpret_cast<double *>(s_raw + ListLds::cent());    // (zero beyond kk: cent_t is)
  u64 *const s_delta = reinterpret_cast<u64 *>(s_raw + ListLds::delta());
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
      ub[gi] = h_ub_of_sum(bd);
      lb[gi] = h_lb_of_sum(bd2);
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
struct UpdateLds {  // k_h_update's dynamic LDS: the new centroids as rows of T_ROW doubles
  int k;
  size_t bytes() const { return (size_t)k * T_ROW * 8; }
};
__global__ __launch_bounds__(1024) void k_h_update(Seg *__restrict__ segs, int k, u64 *__restrict__ sums, u64 *__restrict__ cnts, double *__restrict__ cent,
                                                   double *__restrict__ cent_t /* [192][kt], zero beyond kk */, int kt, double *__restrict__ cmove,
                                                   double *__restrict__ shalf, unsigned *__restrict__ need_cnt, int it, int *__restrict__ quiet_iter,
                                                   int *host_quiet = nullptr /* page-locked host word that gets the flag too */) {
  extern __shared__ double s_new[];  // UpdateLds: [kk][T_ROW] (odd pitch: the pair loop reads two rows at once)
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
  // a wave per centroid, 3 dimensions per lane: new position, displacement (the sums only feed the bounds: h_displacement)
  for (int c = wave; c < kk; c += 16) {
    const u64 cn = c == wave ? cn0 : cnts[c];
    double sd = 0.0;
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const int j = lane + 64 * u;
      const double old = c == wave ? old0[u] : cent[c * 192 + j];
      double nw = old;
      if (changed && cn > 0) { nw = __ddiv_rn((double)(long long)(c == wave ? sm0[u] : sums[c * 192 + j]), (double)(long long)cn); cent[c * 192 + j] = nw; }
      s_new[c * T_ROW + j] = nw;
      cent_t[(int64_t)j * kt + c] = nw;
      const double t = nw - old;
      sd += t * t;
    }
    sd = wave_sum(sd);
    if (lane == 0) { const double mv = h_displacement(sd); cmove[c] = mv; s_move[c] = mv; }
  }
  __syncthreads();
  for (int pr = tid >> 4; pr < kk * kk; pr += 64) {  // pairwise distances, 16 lanes per pair: the smallest per centroid (non-negative doubles order like their bit patterns)
    const int a = pr / kk, b = pr - a * kk;
    if (a >= b) continue;  // (uniform in a group of 16 lanes, and the exchanges below stay inside one)
    double sd = 0.0;
#pragma unroll
    for (int u = 0; u < 12; u++) { const int j = (tid & 15) + 16 * u; const double t = s_new[a * T_ROW + j] - s_new[b * T_ROW + j]; sd += t * t; }
    for (int o = 8; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    if ((tid & 15) == 0) {
      atomicMin(&s_min[a], (unsigned long long)__double_as_longlong(sd));
      atomicMin(&s_min[b], (unsigned long long)__double_as_longlong(sd));
    }
  }
  __syncthreads();
  if (tid < kk) shalf[tid] = kk > 1 ? h_half_distance(s_min[tid]) : H_ALONE;
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

// ---- host side of the skipping iterations --------------------------------------------------------------------------------------------
int tile_skip_setup(TileRun &t) {
  const int k = t.k;
  const size_t n1 = (size_t)std::max<int64_t>(t.n, 1);
  t.kt = (k + KCH - 1) / KCH * KCH;
  const size_t l_lds = ListLds(k).bytes(), u_lds = UpdateLds{k}.bytes();
  // a dynamic-LDS request above the CU's 160 KB comes back from the launch as a bare "invalid argument" (round 2's scratch records hold one,
  // from a k = 64 build of these kernels that kept more in LDS): refuse it here, by name
  TM_CHECK(l_lds <= (size_t)CU_LDS_BYTES && u_lds <= (size_t)CU_LDS_BYTES, TM_E_INVAL, "k-means: %d centroids need %zu bytes of LDS in the list kernel (the CU has 163840)", k, l_lds);
  TM_TRY(t.ub.alloc(n1 * 8)); TM_TRY(t.lb.alloc(n1 * 8)); TM_TRY(t.cent_t.alloc((size_t)t.kt * 192 * 8));
  TM_TRY(t.move.alloc((size_t)(k + 3) * 8)); TM_TRY(t.half.alloc((size_t)k * 8)); TM_TRY(t.need.alloc(n1 * 4)); TM_TRY(t.cnt.alloc(8));
  TM_HIP(hipMemsetAsync(t.cnt.p, 0, 8, t.stream));
  TM_HIP(hipMemsetAsync(t.cent_t.p, 0, (size_t)t.kt * 192 * 8, t.stream));
  hipLaunchKernelGGL(k_cent_transpose, dim3(12), dim3(256), 0, t.stream, t.ds, t.cent, t.cent_t.as<double>(), t.kt);
  if (u_lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_h_update), hipFuncAttributeMaxDynamicSharedMemorySize, (int)u_lds);
  if (l_lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_assign192_list4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l_lds);
  return TM_OK;
}

void tile_skip_iteration(TileRun &t, int iter, int *pin_dev) {
  if (iter < H_WARM) {
    const bool last_plain = iter == H_WARM - 1;  // it leaves the bounds the skipping iterations start from
    launch_assign192(t.a192, 1, t.stream, t.assign192_args(last_plain ? t.ub.as<double>() : nullptr, last_plain ? t.lb.as<double>() : nullptr));
  } else {
    hipLaunchKernelGGL(k_h_bounds, dim3((int)((t.n + H_SLICE - 1) / H_SLICE)), dim3(256), 0, t.stream, t.pts, t.n, t.ds, (const double *)t.cent, t.assign, t.ub.as<double>(),
                       t.lb.as<double>(), t.move.as<double>(), t.half.as<double>(), t.k, t.need.as<int32_t>(), t.cnt.as<unsigned>(), t.quiet);
    hipLaunchKernelGGL(k_assign192_list4, dim3((unsigned)std::min<int64_t>((t.n + 63) / 64, t.k <= KCH ? 1024 : 768)), dim3(256), ListLds(t.k).bytes(), t.stream, t.pts, t.ptsc, t.n, t.w, t.ds,
                       t.k, t.cent_t.as<double>(), t.kt, t.assign, t.sums, t.cnts, t.quiet, t.ub.as<double>(), t.lb.as<double>(), t.need.as<int32_t>(), t.cnt.as<unsigned>());
  }
  hipLaunchKernelGGL(k_h_update, dim3(1), dim3(1024), UpdateLds{t.k}.bytes(), t.stream, t.ds, t.k, t.sums, t.cnts, t.cent, t.cent_t.as<double>(), t.kt, t.move.as<double>(),
                     t.half.as<double>(), t.cnt.as<unsigned>(), iter, t.quiet, pin_dev);
}

}  // namespace tmx
