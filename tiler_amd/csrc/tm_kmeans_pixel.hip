// tm_kmeans_pixel.hip -- the build's k-means (tm_kmeans.hip) for D = 3, the colour quantisation of QuantizeUsingYakmo.
#include "tm_kmeans.h"

namespace tmx {

// ---- D = 3, one launch for the whole clustering -----------------------------------------------------------------
// The pixel k-means of QuantizeUsingYakmo (tilingencoder.pas:4434-4532) runs ~180 Lloyd iterations over a few hundred thousand
// distinct colours per palette: a few microseconds of arithmetic per iteration, so as separate launches (two per iteration, two per
// farthest-first pick) it was bound by launch latency alone.  Here every workgroup keeps its 4096 points in REGISTERS for the whole
// clustering (packed colour, weight, assignment), the workgroups of one segment (= one palette) meet at a barrier of their own once
// per iteration (a counter in global memory: agent-scope release / acquire around a relaxed poll), and the segments run their own
// number of iterations side by side.  Everything that crosses workgroups is an integer atomic -- the carried sums and counts
// (exact, order-free), the farthest-first pick (64-bit max of distance << 32 | ~index: largest distance, then lowest index), the
// changed-points counter -- so the result is the one the multi-launch path and the oracle give, bit for bit.
#ifndef TM_KM3_STAMPS
#define TM_KM3_STAMPS 0
#endif
#if TM_KM3_STAMPS
#define P3_STAMP(i) do { if (bx == 0 && tid == 0) { const u64 t_ = __builtin_amdgcn_s_memtime(); st->stamps[i] += t_ - st_last; st_last = t_; } } while (0)
#else
#define P3_STAMP(i) do { } while (0)
#endif
#ifndef TM_KM3_NT
#define TM_KM3_NT 256
#endif
#ifndef TM_KM3_PPT
#define TM_KM3_PPT 16
#endif
#ifndef TM_KM3_PU
#define TM_KM3_PU 4  // points of a thread whose bounds are tested together (the dependent LDS round trips of a batch overlap)
#endif
constexpr int P3_PPT = TM_KM3_PPT, P3_NT = TM_KM3_NT, P3_ROWS = P3_PPT * P3_NT, P3_MAXK = 64, P3_NCOPY = 4;
// workgroups a CU is asked to hold (LDS: ten bytes a point + 12 KB).  Measured (round 3): 1024 x 12 and 512 x 20 / 24 points per workgroup, one
// per CU and a third as many participants at a palette's barrier, take 13.8-13.9 / 14.3 / 14.9 ms for PreparePalettes against 13.7 with 256 x 16
constexpr int P3_WGS = (P3_ROWS * 10 + 12288) * 3 <= CU_LDS_BYTES && P3_NT * 3 <= 1024 ? 3 : 1;
static_assert(TM_KM3_NT != 256 || TM_KM3_PPT != 16 || P3_WGS == 3, "the shipped shape holds three workgroups per CU");
static_assert(P3_PPT % 4 == 0 && P3_ROWS <= 65535 && P3_NT >= 192, "pixel k-means shape");
constexpr int P3_UNIT = 128;  // the per-point distance bounds are 16-bit fixed point, 1/128 of a colour step (distances stay below 442)

struct Seg3 {
  int64_t begin, count;
  int blk_first, blk_count;
  int kk, iters;        // out
  int nseg;             // element 0 only
  int pad;
};
struct Seg3State {      // zeroed before the launch
  u64 sums[P3_MAXK][3];
  u64 cnts[P3_MAXK];
  u64 pick[P3_MAXK];
  unsigned changed[3], timeout, pad[4];
  BarrierLine bar[8], top[8];  // grid_barrier's, for the segment's workgroups
#if TM_KM3_STAMPS
  u64 stamps[8];  // diagnostic build: s_memtime spans of workgroup 0's phases, summed over the iterations
#endif
};

__device__ __forceinline__ bool p3_barrier(Seg3State *st, unsigned &epoch, unsigned nblk, unsigned bx) {
  __shared__ int s_ok;
  return grid_barrier<(1u << 24)>(st, epoch, nblk, bx, &s_ok);
}

__global__ __launch_bounds__(P3_NT, P3_WGS) void k_kmeans3_persistent(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, Seg3 *__restrict__ segs,
                                                             Seg3State *__restrict__ state, int k, int max_iter, int32_t *__restrict__ assign,
                                                             double *__restrict__ cent) {
  // the workgroup's points stay on chip for the whole clustering: packed colour and assignment in LDS (slot m * NT + tid: no bank
  // conflicts), so the loops over a thread's points stay rolled and the register file holds only the P3_G points in flight
  __shared__ double s_cent[P3_MAXK][3];
  __shared__ double s_dsq[P3_MAXK][3];  // squared displacement of each centroid coordinate in the last update
  __shared__ int s_half[P3_MAXK];      // half the distance to the nearest other centroid, rounded down (P3_UNIT)
  __shared__ int2 s_mh[P3_MAXK];       // (s_move, s_half) of a centroid side by side: the pass over all points fetches both with one read
  __shared__ int s_move[P3_MAXK + 3];  // displacement of each centroid in the last update, rounded up; then the largest, the second largest, whose
  __shared__ uint32_t s_col[P3_ROWS];   // colour | assignment << 24 (0xff: none yet, 0xfe: slot past the end of the segment)
  // farthest-first distances, then the points' bounds: ub >= the distance to the own centroid, lb <= the distance to every other one
  __shared__ union { int md[P3_ROWS]; uint32_t bnd[P3_ROWS]; } s_u;  // bnd: ub | lb << 16
  __shared__ u64 s_acc[P3_NCOPY][P3_MAXK][4];                      // the sums' deltas of one iteration
  __shared__ uint16_t s_list[P3_NT / 64][P3_ROWS / (P3_NT / 64)];  // every wave's list of the points it has to score
  __shared__ u64 s_red[P3_NT / 64];
  __shared__ int s_chg;
  const int tid = threadIdx.x;
  int seg;
  {
    int lo = 0, hi = segs[0].nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].blk_first <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    seg = lo;
  }
  const Seg3 sg = segs[seg];
  const int bx = (int)blockIdx.x - sg.blk_first;
  const unsigned nbx = (unsigned)sg.blk_count;
  Seg3State *st = state + seg;
  unsigned epoch = 0;
  const int64_t base = (int64_t)bx * P3_ROWS;
  for (int r = tid; r < P3_ROWS; r += P3_NT) {
    uint32_t cc = 0xfe000000u;
    if (base + r < sg.count) {
      const int32_t *p = pts + (sg.begin + base + r) * 3;
      cc = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | 0xff000000u;
    }
    s_col[r] = cc;
    s_u.md[r] = INT_MAX;
  }
  // ---- farthest-first from the segment's first point
  int kk = 1;
  int cr, cg, cb;
  {
    const int32_t *p0 = pts + sg.begin * 3;
    cr = p0[0]; cg = p0[1]; cb = p0[2];
  }
  if (tid < 3) s_cent[0][tid] = (double)(tid == 0 ? cr : tid == 1 ? cg : cb);
  for (int c = 1; c < k; c++) {
    u64 best = 0;
    for (int r = tid; r < P3_ROWS; r += P3_NT) {  // (each thread only ever touches its own slots: no barrier needed for s_col / md)
      const uint32_t cc = s_col[r];
      if ((cc >> 24) == 0xfeu) continue;
      const int dr = (int)(cc & 0xff) - cr, dg = (int)((cc >> 8) & 0xff) - cg, db = (int)((cc >> 16) & 0xff) - cb;
      const int m = min(s_u.md[r], dr * dr + dg * dg + db * db);
      s_u.md[r] = m;
      const u64 key = ((u64)(uint32_t)m << 32) | (u64)(0xffffffffu - (uint32_t)(base + r));
      best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(best, o); best = other > best ? other : best; }
    if ((tid & 63) == 0) s_red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      for (int wv = 1; wv < P3_NT / 64; wv++) best = s_red[wv] > best ? s_red[wv] : best;
      if (best >> 32) atomicMax(&st->pick[c], best);
    }
    if (!p3_barrier(st, epoch, nbx, (unsigned)bx)) return;
    const u64 win = __hip_atomic_load(&st->pick[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((win >> 32) == 0) break;  // no distinct point left
    const int32_t *pc = pts + (sg.begin + (int64_t)(0xffffffffu - (uint32_t)win)) * 3;
    cr = pc[0]; cg = pc[1]; cb = pc[2];
    if (tid < 3) s_cent[kk][tid] = (double)(tid == 0 ? cr : tid == 1 ? cg : cb);
    kk++;
  }
  // ---- Lloyd
  // Per point two bounds are kept (Hamerly): ub >= its distance to its own centroid, lb <= its distance to every other one; a centroid
  // update loosens them by the centroids' displacements.  While ub <= max(lb, half the distance from the own centroid to the nearest
  // other one) the own centroid is strictly the nearest -- every bound is rounded the safe way to 1/128 and carries a margin of a
  // whole unit, six orders of magnitude above the rounding of the distance arithmetic, so the order of the COMPUTED distances is the
  // same and strict -- and the point keeps its assignment without being scored.  A point that fails first gets its ub tightened
  // (distance to its own centroid, in the arithmetic of the scoring); if it still fails it goes on its wave's list and is scored
  // against every centroid as before.  Each wave compacts and scores its own 1024 points: no barrier between the two.
  int it = 0;
#if TM_KM3_STAMPS
  u64 st_last = __builtin_amdgcn_s_memtime();
#endif
  const int wave = tid >> 6, lane = tid & 63;
  if (tid < P3_MAXK) { s_move[tid] = 0; s_half[tid] = 0; s_mh[tid] = make_int2(0, 0); }
  if (tid < 3) s_move[P3_MAXK + tid] = 0;
  for (;;) {
    __syncthreads();  // s_cent, s_move, s_half of this iteration are in place; the farthest-first pass is done with the union; the previous flush with s_acc
    for (int e = tid; e < P3_NCOPY * P3_MAXK * 4; e += P3_NT) (&s_acc[0][0][0])[e] = 0;
    if (tid == 0) s_chg = 0;
    __syncthreads();
    P3_STAMP(0);  // zeroing
    const int mv1 = s_move[P3_MAXK], mv2 = s_move[P3_MAXK + 1], amax = s_move[P3_MAXK + 2];
    int nlist = 0;  // uniform in the wave
    uint16_t *const mylist = s_list[wave];
    // Pass A, every point: the bounds loosened by the centroids' displacements; the points whose bounds no longer prove their assignment (and
    // the ones not assigned yet) go on the wave's list.  Pass B, the listed points only, 64 at a time: the real distance to the own centroid
    // as the new ub; what still fails stays on the list (compacted in place, order kept) and is scored.  One in seven points is listed, one
    // in fifteen scored: with the recheck inside pass A every wave ran its double-precision arithmetic for all of its points, because some
    // lane of every batch needed it.
    int ntight = 0;
    constexpr int PU = TM_KM3_PU;  // points of a thread in flight: their LDS round trips overlap
#pragma unroll 1
    for (int m0 = 0; m0 < P3_PPT; m0 += PU) {
      uint32_t cc[PU], bn[PU];
#pragma unroll
      for (int i = 0; i < PU; i++) {
        const int r = (m0 + i) * P3_NT + tid;
        cc[i] = s_col[r];
        bn[i] = s_u.bnd[r];
      }
      // (no branch around a point's table look-up: the compiler then waits for every look-up on its own, one LDS round trip after the
      // other; fetched for all the points of the batch at once -- entry 62 / 63 for the slots without a centroid, never used -- they overlap)
      int2 mh[PU];
#pragma unroll
      for (int i = 0; i < PU; i++) mh[i] = s_mh[(cc[i] >> 24) & (P3_MAXK - 1)];
#pragma unroll
      for (int i = 0; i < PU; i++) {
        const int r = (m0 + i) * P3_NT + tid;
        const int a = (int)(cc[i] >> 24);
        const bool has = a < 0xfe;
        const int u = min(65535, (int)(bn[i] & 0xffffu) + mh[i].x);
        const int l = max(0, (int)(bn[i] >> 16) - (a == amax ? mv2 : mv1));  // lb bounds the OTHER centroids: the own one's displacement does not loosen it
        s_u.bnd[r] = has ? ((uint32_t)u | ((uint32_t)l << 16)) : bn[i];
        const bool listed = has ? u > max(l, mh[i].y) : a == 0xff;  // (not assigned yet: scored)
        const unsigned long long tb = __builtin_amdgcn_ballot_w64(listed);
        if (listed) mylist[ntight + __popcll(tb & ((1ull << lane) - 1ull))] = (uint16_t)r;
        ntight += __popcll(tb);
#if TM_KM3_STAMPS
        if (bx == 0 && lane == 0) atomicAdd(&st->stamps[7], (u64)__popcll(tb) << 32);
#endif
      }
    }
#pragma unroll 1
    for (int e0 = 0; e0 < ntight; e0 += 64) {
      const bool valid = e0 + lane < ntight;
      const int r = valid ? (int)mylist[e0 + lane] : tid;
      const uint32_t cc = s_col[r], bn = s_u.bnd[r];
      const int a = (int)(cc >> 24);
      bool full = valid;
      if (valid && a < 0xfe) {
        // the distance to the own centroid, in the scoring's arithmetic, as the new ub (single-precision root, as in the scoring)
        const double t0 = __dsub_rn((double)(int)(cc & 0xff), s_cent[a][0]), t1 = __dsub_rn((double)(int)((cc >> 8) & 0xff), s_cent[a][1]),
                     t2 = __dsub_rn((double)(int)((cc >> 16) & 0xff), s_cent[a][2]);
        const double sd = __fma_rn(t2, t2, __fma_rn(t1, t1, __fma_rn(t0, t0, 0.0)));
        const int u = min(65535, (int)(__fsqrt_rn((float)sd) * (float)P3_UNIT) + 2), l = (int)(bn >> 16);
        s_u.bnd[r] = (uint32_t)u | ((uint32_t)l << 16);
        full = u > max(l, s_half[a]);
      }
      const unsigned long long fb = __builtin_amdgcn_ballot_w64(full);
      if (full) mylist[nlist + __popcll(fb & ((1ull << lane) - 1ull))] = (uint16_t)r;  // (nlist <= e0: never over an entry still to be read)
      nlist += __popcll(fb);
#if TM_KM3_STAMPS
      if (bx == 0 && lane == 0) atomicAdd(&st->stamps[7], (u64)__popcll(fb));
#endif
    }
    P3_STAMP(1);  // bounds of the 16 passes
    int changed = 0;
    // G listed points per lane at a time against one centroid after the other: a centroid read from LDS (a broadcast) serves G points.
    // Per (point, centroid): sum over dimensions in order of (p - c)^2, one IEEE subtraction and one fused multiply-add each;
    // ties -> lowest centroid.
    auto score = [&](auto gtag, const int e0) {
      constexpr int G = decltype(gtag)::value;
      double px[G][3], bd[G], bd2[G];
      int bc[G], rr[G];
      uint32_t cc[G], wv[G];
#pragma unroll
      for (int m = 0; m < G; m++) {
        const int e = e0 + m * 64 + lane;
        rr[m] = e < nlist ? (int)mylist[e] : -1;
        // the weight is only needed if the point moves, but it comes from memory: asked for now, it arrives under the distance arithmetic
        // instead of behind it (a round trip to L2 or HBM at the end of every scoring step of every iteration)
        wv[m] = (w && rr[m] >= 0) ? w[sg.begin + base + rr[m]] : 1u;
        cc[m] = s_col[rr[m] < 0 ? tid : rr[m]];
        px[m][0] = (double)(int)(cc[m] & 0xff); px[m][1] = (double)(int)((cc[m] >> 8) & 0xff); px[m][2] = (double)(int)((cc[m] >> 16) & 0xff);
        bd[m] = 0.0; bd2[m] = 1.0e300;
        bc[m] = -1;
      }
#pragma unroll 1
      for (int c = 0; c < kk; c++) {
        const double c0 = s_cent[c][0], c1 = s_cent[c][1], c2 = s_cent[c][2];
#pragma unroll
        for (int m = 0; m < G; m++) {
          const double t0 = __dsub_rn(px[m][0], c0), t1 = __dsub_rn(px[m][1], c1), t2 = __dsub_rn(px[m][2], c2);
          const double sd = __fma_rn(t2, t2, __fma_rn(t1, t1, __fma_rn(t0, t0, 0.0)));
          if (bc[m] < 0 || sd < bd[m]) { bd2[m] = bc[m] < 0 ? bd2[m] : bd[m]; bd[m] = sd; bc[m] = c; }
          else if (sd < bd2[m]) bd2[m] = sd;
        }
      }
#pragma unroll
      for (int m = 0; m < G; m++) {
        const int r = rr[m];
        if (r < 0) continue;
        // single-precision roots: their error (2e-7 relative, 0.011 units at most) is far inside the margins of a whole unit
        s_u.bnd[r] = (uint32_t)min(65535, (int)(__fsqrt_rn((float)bd[m]) * (float)P3_UNIT) + 2) |
                     ((uint32_t)(bd2[m] > 1.0e12 ? 65535 : max(0, (int)(__fsqrt_rn((float)bd2[m]) * (float)P3_UNIT) - 1)) << 16);
        const int old = (int)(cc[m] >> 24);
        if (old == bc[m]) continue;
        // only a point that changes cluster touches the carried sums
        const long long wi = (long long)wv[m];
        const int pi[3] = {(int)(cc[m] & 0xff), (int)((cc[m] >> 8) & 0xff), (int)((cc[m] >> 16) & 0xff)};
        u64 *acc = &s_acc[tid & (P3_NCOPY - 1)][bc[m]][0];
        atomicAdd(&acc[3], (u64)wi);
#pragma unroll
        for (int j = 0; j < 3; j++) atomicAdd(&acc[j], (u64)(wi * pi[j]));
        if (old != 0xff) {
          u64 *oacc = &s_acc[tid & (P3_NCOPY - 1)][old][0];
          atomicAdd(&oacc[3], (u64)0 - (u64)wi);
#pragma unroll
          for (int j = 0; j < 3; j++) atomicAdd(&oacc[j], (u64)0 - (u64)(wi * pi[j]));
        }
        s_col[r] = (cc[m] & 0xffffffu) | ((uint32_t)bc[m] << 24);
        changed++;
      }
    };
    {  // 256 listed points per step while there are many, then 128, then 64: a short list costs one short step
      int e0 = 0;
      for (; nlist - e0 > 128; e0 += 256) score(std::integral_constant<int, 4>{}, e0);
      if (nlist - e0 > 64) { score(std::integral_constant<int, 2>{}, e0); e0 += 128; }
      if (nlist - e0 > 0) score(std::integral_constant<int, 1>{}, e0);
    }
    P3_STAMP(2);  // full scoring of the listed points
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o);
    if ((tid & 63) == 0 && changed) atomicAdd(&s_chg, changed);
    __syncthreads();
    P3_STAMP(3);  // waiting for the workgroup's other waves
    for (int e = tid; e < kk * 4; e += P3_NT) {
      u64 v = 0;
#pragma unroll
      for (int cp = 0; cp < P3_NCOPY; cp++) v += s_acc[cp][e >> 2][e & 3];
      if (v == 0) continue;
      if ((e & 3) == 3) atomicAdd(&st->cnts[e >> 2], v); else atomicAdd(&st->sums[e >> 2][e & 3], v);
    }
    if (tid == 0 && s_chg) atomicAdd(&st->changed[it % 3], (unsigned)s_chg);
    P3_STAMP(4);  // flush
    if (!p3_barrier(st, epoch, nbx, (unsigned)bx)) return;
    P3_STAMP(5);  // barrier of the segment's workgroups
    // (the three loads leave together: one round trip instead of three)
    const int uc = min(tid / 3, P3_MAXK - 1), uj = tid - (tid / 3) * 3;
    const unsigned tot = __hip_atomic_load(&st->changed[it % 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 cn = __hip_atomic_load(&st->cnts[uc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 sm = __hip_atomic_load(&st->sums[uc][uj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bx == 0 && tid == 0) __hip_atomic_store(&st->changed[(it + 2) % 3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // last read two barriers ago
    if (tot == 0) break;
    // new centroids: exact integer sum / weight, one IEEE division; an empty cluster keeps its centroid
    if (tid < kk * 3) {
      const int c = uc, j = uj;
      const double old = s_cent[c][j];
      double nw = old;
      if (cn > 0) nw = __ddiv_rn((double)(long long)sm, (double)(long long)cn);
      s_cent[c][j] = nw;
      const double dd = nw - old;
      s_dsq[c][j] = dd * dd;
    }
    if (tid < P3_MAXK) s_half[tid] = 0x7fffffff;
    __syncthreads();
    // what the bounds need (identical in every workgroup of the segment): how far each centroid moved, rounded up (a centroid that did
    // not move costs nothing), and half its distance to the nearest other one, rounded down
    if (tid < kk) {
      const double m2 = s_dsq[tid][0] + s_dsq[tid][1] + s_dsq[tid][2];
      s_move[tid] = m2 == 0.0 ? 0 : (int)(__fsqrt_rn((float)m2) * (float)P3_UNIT) + 2;
    }
    for (int pr = tid; pr < kk * kk; pr += P3_NT) {
      const int ca = pr / kk, cb2 = pr - ca * kk;
      if (ca >= cb2) continue;
      const double t0 = s_cent[ca][0] - s_cent[cb2][0], t1 = s_cent[ca][1] - s_cent[cb2][1], t2 = s_cent[ca][2] - s_cent[cb2][2];
      // (single-precision root, as everywhere the bounds are made: its error, 0.006 units at most, is far inside the whole unit of margin;
      // the double-precision one is a few dozen instructions on every iteration's critical path)
      const int h = max(0, (int)(0.5f * __fsqrt_rn((float)(t0 * t0 + t1 * t1 + t2 * t2)) * (float)P3_UNIT) - 1);
      atomicMin(&s_half[ca], h);
      atomicMin(&s_half[cb2], h);
    }
    __syncthreads();
    if (tid < kk) s_mh[tid] = make_int2(s_move[tid], s_half[tid]);  // (both final: the barrier above)
    if (wave == 0) {  // the largest displacement, whose it is (the first, if several), and the largest among the others: over the lanes of one
                      // wave (a thread walking the centroids read them one after the other: sixteen dependent LDS round trips per iteration)
      static_assert(P3_MAXK <= 64, "one lane per centroid");
      const int v = lane < kk ? s_move[lane] : 0;
      int m1 = v;
      for (int o = 32; o > 0; o >>= 1) m1 = max(m1, __shfl_xor(m1, o));
      const int am = __builtin_ctzll(__builtin_amdgcn_ballot_w64(v == m1 && (lane < kk || m1 == 0)));
      int m2 = lane == am ? 0 : v;
      for (int o = 32; o > 0; o >>= 1) m2 = max(m2, __shfl_xor(m2, o));
      if (lane == 0) { s_move[P3_MAXK] = m1; s_move[P3_MAXK + 1] = m2; s_move[P3_MAXK + 2] = am; }
    }
    P3_STAMP(6);  // counts + sums read back, new centroids
    it++;
    if (it >= max_iter) break;
  }
  __syncthreads();
  for (int r = tid; r < P3_ROWS; r += P3_NT)
    if (base + r < sg.count) assign[sg.begin + base + r] = (int32_t)(s_col[r] >> 24);
  if (bx == 0) {
    for (int e = tid; e < kk * 3; e += P3_NT) cent[((int64_t)seg * k + e / 3) * 3 + e % 3] = s_cent[e / 3][e % 3];
    if (tid == 0) { segs[seg].kk = kk; segs[seg].iters = it; }
  }
}

// host side of the above; *used = 0 when the shape does not fit one resident launch (the caller then takes the multi-launch path)
int kmeans3_persistent(const int32_t *pts, const uint32_t *w, const std::vector<int64_t> &seg_begin, const std::vector<int64_t> &seg_count, int k,
                              int max_iter, int32_t *assign, double *cent, std::vector<int> *host_kk, int *host_iters, hipStream_t stream, int *used,
                              double *host_cent) {
  *used = 0;
  const int nseg = (int)seg_begin.size();
  if (k > P3_MAXK) return TM_OK;
  const int cus = cu_count();
  std::vector<Seg3> hs;  // empty segments take no workgroup and are answered on the host
  std::vector<int> which;
  int nblk = 0;
  for (int s = 0; s < nseg; s++) {
    if (seg_count[s] <= 0) continue;
    Seg3 g;
    memset(&g, 0, sizeof(g));
    g.begin = seg_begin[s]; g.count = seg_count[s];
    g.blk_first = nblk;
    g.blk_count = (int)((seg_count[s] + P3_ROWS - 1) / P3_ROWS);
    nblk += g.blk_count;
    hs.push_back(g);
    which.push_back(s);
  }
  // All workgroups of a launch must be resident together: what the runtime says fits a CU (registers, LDS, the launch bound of three), not a
  // guess.  More colours than the chip holds at once (3.1 M: the motion-prediction configurations of the bench clip) go as several launches,
  // each a run of whole segments (palettes are independent), one after the other on the stream.
  std::vector<std::pair<size_t, size_t>> batches;  // [first, last) of hs
  {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_kmeans3_persistent, P3_NT, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    per_cu = std::min(per_cu, P3_WGS);
    const int capacity = per_cu * cus;
    size_t b0 = 0;
    int acc = 0;
    for (size_t i = 0; i < hs.size(); i++) {
      if (hs[i].blk_count > capacity) return TM_OK;  // one palette alone does not fit: the launches-per-iteration path
      if (acc + hs[i].blk_count > capacity) { batches.push_back({b0, i}); b0 = i; acc = 0; }
      acc += hs[i].blk_count;
    }
    if (b0 < hs.size()) batches.push_back({b0, hs.size()});
  }
  if (host_kk) host_kk->assign(nseg, 0);
  if (host_iters) *host_iters = 0;
  *used = 1;
  if (hs.empty()) return TM_OK;
  for (const auto &b : batches) {  // a launch sees its own segments only: workgroup indices from 0, the count in its first element
    const int base = hs[b.first].blk_first;
    for (size_t i = b.first; i < b.second; i++) hs[i].blk_first -= base;
    hs[b.first].nseg = (int)(b.second - b.first);
  }
  DevBuf dsegs, dstate, dcent;
  TM_TRY(dsegs.alloc(sizeof(Seg3) * hs.size()));
  TM_TRY(dstate.alloc(sizeof(Seg3State) * hs.size()));
  TM_TRY(dcent.alloc(sizeof(double) * hs.size() * k * 3));
  TM_HIP(hipMemcpyAsync(dsegs.p, hs.data(), sizeof(Seg3) * hs.size(), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemsetAsync(dstate.p, 0, sizeof(Seg3State) * hs.size(), stream));
  TM_HIP(hipMemsetAsync(dcent.p, 0, sizeof(double) * hs.size() * k * 3, stream));
  TM_CHECK(nblk >= 1 && k >= 1 && k <= P3_MAXK, TM_E_INVAL, "k-means: resident launch of %d workgroups for %d centres (at most %d)", nblk, k, P3_MAXK);
  std::unique_lock<std::mutex> resident_lock(resident_launch_lock());
  for (const auto &b : batches) {
    int grid = 0;
    for (size_t i = b.first; i < b.second; i++) grid += hs[i].blk_count;
    hipLaunchKernelGGL(k_kmeans3_persistent, dim3(grid), dim3(P3_NT), 0, stream, pts, w, dsegs.as<Seg3>() + b.first, dstate.as<Seg3State>() + b.first, k, max_iter, assign,
                       dcent.as<double>() + b.first * (size_t)k * 3);
  }
  TM_HIP(hipGetLastError());
  std::vector<Seg3State> hstate(hs.size());
  std::vector<double> hcent(hs.size() * (size_t)k * 3);
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(hs.data(), dsegs.p, sizeof(Seg3) * hs.size()));
    TM_TRY(hr_.get(hstate.data(), dstate.p, sizeof(Seg3State) * hs.size()));
    TM_TRY(hr_.get(hcent.data(), dcent.p, hcent.size() * 8));
    TM_TRY(hr_.wait());
  }
  resident_lock.unlock();
  int iters = 0;
  for (size_t i = 0; i < hs.size(); i++)
    if (hstate[i].timeout != 0) {  // a workgroup of a segment never became resident (the barrier gave up): the launches-per-iteration path instead
      fprintf(stderr, "[tm_kmeans] the resident pixel k-means gave up at its barrier (segment %zu); falling back to one launch per iteration\n", i);
      *used = 0;
      return TM_OK;
    }
  kmeans_run_stats().pixel_colour_iters = 0;
  for (size_t i = 0; i < hs.size(); i++) {
    if (host_kk) (*host_kk)[which[i]] = hs[i].kk;
    iters = std::max(iters, hs[i].iters);
    kmeans_run_stats().pixel_colour_iters += hs[i].count * (int64_t)hs[i].iters;
#if TM_KM3_STAMPS
    fprintf(stderr, "[tm_km3 stamps] segment %zu: %d workgroups, %d iterations; per iteration (s_memtime ticks): zero+thresholds %.0f, own test %.0f, scoring %.0f, "
            "workgroup sync %.0f, flush %.0f, barrier %.0f, read-back %.0f\n", i, hs[i].blk_count, hs[i].iters, (double)hstate[i].stamps[0] / std::max(1, hs[i].iters),
            (double)hstate[i].stamps[1] / std::max(1, hs[i].iters), (double)hstate[i].stamps[2] / std::max(1, hs[i].iters), (double)hstate[i].stamps[3] / std::max(1, hs[i].iters),
            (double)hstate[i].stamps[4] / std::max(1, hs[i].iters), (double)hstate[i].stamps[5] / std::max(1, hs[i].iters), (double)hstate[i].stamps[6] / std::max(1, hs[i].iters));
    fprintf(stderr, "[tm_km3 stamps]   workgroup 0: %.1f points per iteration fail the own-centroid test, %.1f are scored (whole passes)\n",
            (double)(hstate[i].stamps[7] >> 32) / std::max(1, hs[i].iters), (double)(hstate[i].stamps[7] & 0xffffffffu) / std::max(1, hs[i].iters));
#endif
  }
  if (host_iters) *host_iters = iters;
  // centroids back in the caller's [nseg][k][3] layout: on the host where the caller goes on there (no upload, nothing to wait for), else on the device
  if (host_cent) {
    std::fill(host_cent, host_cent + (size_t)nseg * k * 3, 0.0);
    for (size_t i = 0; i < hs.size(); i++) memcpy(host_cent + (size_t)which[i] * k * 3, &hcent[i * (size_t)k * 3], sizeof(double) * k * 3);
    return TM_OK;
  }
  std::vector<double> full((size_t)nseg * k * 3, 0.0);
  for (size_t i = 0; i < hs.size(); i++) memcpy(&full[(size_t)which[i] * k * 3], &hcent[i * (size_t)k * 3], sizeof(double) * k * 3);
  TM_HIP(hipMemcpyAsync(cent, full.data(), full.size() * 8, hipMemcpyHostToDevice, stream));
  TM_HIP(host_sync(stream));  // full, the upload's source, is on this frame: the copy must have read it before the frame goes
  return TM_OK;
}

}  // namespace tmx
