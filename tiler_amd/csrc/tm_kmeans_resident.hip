// tm_kmeans_resident.hip -- D = 192, at most KCH centroids: all skipping iterations of a clustering in one resident launch.
#include "tm_kmeans_tile.h"

namespace tmx {

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
constexpr int HR_NT = 1024, HR_P = 64, HR_PITCH = KCH + 1, HR_MAXR = 2, HR_E = KCH * T_ROW;
constexpr int HR_NSTAMP = 12;
struct HrState {                    // zeroed before the launch
  u64 delta[3][HR_E];              // the sums' deltas of one iteration ([c][T_ROW], the count last); three in rotation
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

// k_h_resident's dynamic LDS, in bytes, for a workgroup that owns `rounds` rounds of HR_NT points: the kernel carves it, the host sizes it
struct ResidentLds {
  int slots;
  constexpr explicit ResidentLds(int rounds) : slots(rounds * HR_NT) {}
  constexpr int cent() const { return 0; }                              // double [192][HR_PITCH]: centroid c, dimension j at j * HR_PITCH + c
  constexpr int sum() const { return 192 * HR_PITCH * 8; }              // u64 [KCH][T_ROW] carried sums, the count last
  constexpr int delta() const { return sum() + HR_E * 8; }              // u64 [KCH][T_ROW] this workgroup's deltas of the iteration
  constexpr int rows() const { return delta() + HR_E * 8; }             // int [HR_P][192] rows of the points being scored
  constexpr int ub() const { return rows() + HR_P * 192 * 4; }          // float [slots]
  constexpr int lb() const { return ub() + slots * 4; }                 // float [slots]
  constexpr int list() const { return lb() + slots * 4; }               // uint16_t [slots]: slots whose loosened bounds prove nothing
  constexpr int need() const { return list() + slots * 2; }             // uint16_t [slots]: slots to score
  constexpr int w() const { return need() + slots * 2; }                // unsigned [slots]: the points' weights (a moved point's comes from here, not from memory behind the chain)
  constexpr int a() const { return w() + slots * 4; }                   // uint8_t [slots]: assignment (0xff: no point in the slot)
  constexpr size_t bytes() const { return (size_t)a() + slots + 16; }
};

template <int ROUNDS /* 1024-point rounds a workgroup owns: a constant, so that the LDS arrays' places are */>
__global__ __launch_bounds__(HR_NT) void k_h_resident(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, int64_t n, Seg *__restrict__ segs, int k,
                                                      double *__restrict__ cent /* [k][192], in and out */, const u64 *__restrict__ sums, const u64 *__restrict__ cnts,
                                                      const double *__restrict__ cmove, const double *__restrict__ shalf, int32_t *__restrict__ assign,
                                                      const double *__restrict__ ub, const double *__restrict__ lb, HrState *__restrict__ st, int it0, int max_iter,
                                                      int *__restrict__ quiet_iter) {
  constexpr int D = 192, rounds = ROUNDS;
  static_assert(ROUNDS >= 1 && ROUNDS <= HR_MAXR, "rounds");
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  constexpr ResidentLds L(ROUNDS);
  double *const s_c = reinterpret_cast<double *>(s_raw + L.cent());
  u64 *const s_sum = reinterpret_cast<u64 *>(s_raw + L.sum());
  u64 *const s_delta = reinterpret_cast<u64 *>(s_raw + L.delta());
  int *const s_rows = reinterpret_cast<int *>(s_raw + L.rows());
  float *const s_ub = reinterpret_cast<float *>(s_raw + L.ub());
  float *const s_lb = reinterpret_cast<float *>(s_raw + L.lb());
  uint16_t *const s_list = reinterpret_cast<uint16_t *>(s_raw + L.list());
  uint16_t *const s_need = reinterpret_cast<uint16_t *>(s_raw + L.need());
  unsigned *const s_w = reinterpret_cast<unsigned *>(s_raw + L.w());
  uint8_t *const s_a = reinterpret_cast<uint8_t *>(s_raw + L.a());
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
    const int c = e / T_ROW, j = e - c * T_ROW;
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
          const float unf = hr_up(h_ub_moved((double)s_ub[slot], s_move[ac])), lnf = hr_down(h_lb_moved((double)s_lb[slot], a == amax, dmax, dmax2));
          if (valid) { s_ub[slot] = unf; s_lb[slot] = lnf; }
          listed[r] = valid && !H_PROVEN((double)unf, s_half[ac], (double)lnf);
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
    // partial sums add in another order than the scoring's chain; both stay within 2.2e-14 of the exact sum, far inside the factor 1 + H_ROOT).
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
          const float uf = hr_up(h_ub_of_sum(sd));
          s_ub[cslot] = uf;
          if (!H_PROVEN((double)uf, s_half[a], (double)s_lb[cslot])) { np = atomicAdd(&s_nneed, 1); s_need[np] = (uint16_t)cslot; }
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
          s_ub[slot] = hr_up(h_ub_of_sum(bd));
          s_lb[slot] = hr_down(h_lb_of_sum(bd2));
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
          atomicAdd(&s_delta[nw * T_ROW + j], v);
          atomicAdd(&s_delta[old * T_ROW + j], (u64)0 - v);
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
    // centroid), displacement (h_displacement: the sums here only feed the bounds)
    if (wave < kk) {
      const int c = wave;
      const u64 cn = s_sum[c * T_ROW + D];
      double sd = 0.0;
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int j = lane + 64 * u;
        const double old = s_c[j * HR_PITCH + c];
        double nw = old;
        if (cn > 0) { nw = __ddiv_rn((double)(long long)s_sum[c * T_ROW + j], (double)(long long)cn); s_c[j * HR_PITCH + c] = nw; }
        const double t = nw - old;
        sd += t * t;
      }
      sd = hr_sum16(sd);
      sd += __shfl_xor(sd, 16);
      sd += __shfl_xor(sd, 32);
      if (lane == 0) s_move[c] = h_displacement(sd);
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
    if (tid < kk) s_half[tid] = kk > 1 ? h_half_distance(s_min[tid]) : H_ALONE;
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

// ---- host side of the resident launch ----------------------------------------------------------------------------------------------
// At most KCH centroids and points that fit the chip's LDS HR_MAXR rounds deep, a workgroup per CU.
ResidentPlan resident_plan(int64_t n, int k, int cus) {
  ResidentPlan no{0, 0, 0}, p;
  if (n <= 0 || k > KCH) return no;
  p.grid = (int)std::min<int64_t>(cus, (n + HR_NT - 1) / HR_NT);
  p.rounds = (int)(((n + p.grid - 1) / p.grid + HR_NT - 1) / HR_NT);  // a workgroup owns the points i with i % grid == its index: slots of 1024
  p.lds = ResidentLds(p.rounds).bytes();
  return p.rounds <= HR_MAXR && p.lds <= DYN_LDS_CEILING ? p : no;
}

// Should a workgroup not become resident (another process holding CUs with a resident launch of its own) the barrier gives up: gave_up.
int tile_resident(TileRun &t, const ResidentPlan &plan, Resident *verdict, int *iters, Seg *host_seg, u64 *host_look) {
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
    if (host_seg) TM_TRY(hr_.get(host_seg, t.ds, sizeof(Seg)));  // (what the caller would read straight behind this: one round trip for both)
    if (host_look && t.look) TM_TRY(hr_.get(host_look, t.look, 16));
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
