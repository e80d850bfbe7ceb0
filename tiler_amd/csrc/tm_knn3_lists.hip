// tm_knn3_lists.hip -- the second kernel of the third scan shape (tm_knn3.h): every query group's tile list, and the collection mode's
// bounds from its thresholds; launch_lists and launch_tau_bounds (tm_knn.h) launch them.
#include "tm_knn.h"
#include "tm_knn3_block.h"

namespace tmx {

// One workgroup (256 threads) per query group.  Runs of KNN_GROUP tiles are judged first, 16 of them at a time in outward order from the
// home run (one thread per (run, sub-tile) pair); then only the tiles of surviving runs are tested, 128 threads per run, against the
// sub-tiles that survived the run's box.  Entries collect in LDS in that order; a segment that is full (or the list's end) takes its place
// in the arena with one atomic add and is copied out, sorted by its entries' smallest bound (sort_segment; a.list_order = 0: as collected).
// The segments of a list keep the outward order among themselves.  Past the arena's capacity nothing is written and the segment's count is 0: the
// cursor keeps counting, the host sees the overflow with the scan's other counters and repeats the search with a larger arena.
__global__ __launch_bounds__(K3_LIST_NT) void k_knn_lists(const Knn3Args a) {
  constexpr int ND = KNN_ND, NT = K3_LIST_NT, LCAP = K3_LCAP;
  constexpr int RB = NT / 16, RS = NT / KNN_GROUP;  // runs per batch, runs per tile-test step
  static_assert(KNN_GROUP == 128 && RB <= 64 && RS >= 1, "run batches are compacted by one wave");
  __shared__ int s_qbox[16 * QMETA_INTS];  // the sub-tiles' qmeta records
  __shared__ unsigned s_smax[16];
  __shared__ unsigned s_rmask[RB], s_runs[RB];
  __shared__ int s_ctl[4];  // [0] entries in the buffer, [1] surviving runs of the batch, [2] arena offset of the segment being flushed
  __shared__ unsigned s_ltile[LCAP];
  __shared__ unsigned s_llbw[LCAP * 8];  // [LCAP][nsp / 2] words
  __shared__ __attribute__((aligned(4))) uint16_t s_key[LCAP];  // flush: the order the entries leave in (sort_segment)
  const int tid = threadIdx.x, lane = tid & 63;
  const int NS = a.ns, NSP = (NS + 1) & ~1, NSW = NSP / 2;
  const int64_t g = blockIdx.x, st0 = g * NS, n_ttiles = a.n_ttiles;
  const int nvalid = (int)min((int64_t)NS, a.n_qtiles - st0);
  static_assert(QMETA_INTS == 16, "a record is read as four 16-byte vectors");
  for (int i = tid; i < 16 * QMETA_INTS; i += NT) s_qbox[i] = (i >> 4) < nvalid ? a.qmeta[qmeta_at(st0 + (i >> 4), i & 15)] : 0;
  if (tid < 16) s_smax[tid] = tid < nvalid ? a.gsmax[st0 + tid] : 0u;
  if (tid == 0) s_ctl[0] = 0;
  __syncthreads();
  const int home = s_qbox[qmeta_at(0, QMETA_HOME)];
  const K3SeedWindow seeds = a.no_seeds ? K3SeedWindow{0, 0} : k3_seed_window(home, n_ttiles);  // the tiles the seed kernel scored: left out of the lists
  const int r0a = seeds.first, r0b = seeds.first + seeds.count;
  const int n_grp = (int)((n_ttiles + KNN_GROUP - 1) / KNN_GROUP), home_run = home / KNN_GROUP;
  const int total_run_slots = 2 * max(home_run, n_grp - 1 - home_run) + 1, n_run_batches = (total_run_slots + RB - 1) / RB;
  // A segment leaves in ascending order of its entries' smallest bound, equal keys in the order they came (run order): the consumer meets
  // the tiles most likely to tighten its bounds first, and may end the segment at the first entry no sub-tile wants (next_entry).  An
  // unwanted slot holds K3_LB_NONE, above every bound, and every entry has a wanted one: the key is the plain minimum of the row's sixteen
  // halves.  The words key << 10 | position (distinct, so the order is stable and a function of the list alone) go through a bitonic
  // network, EPT of them per thread: a step whose partner sits in the thread's own registers or in its wave costs no barrier (19 and 33 of
  // the 55 steps at 1 024 words); the three steps that cross waves go through s_ltile, whose words wait in registers meanwhile.  What is
  // left in LDS is s_key[rank] = position, 2 KB: the kernel stays at four workgroups per CU.  (Every entry counting the entries before it,
  // n^2 / 2 compares on broadcast reads, was measured first: 1.22 against 0.66 ms for the kernel at the bench clip's 700 entries a group.)
  auto sort_segment = [&](int n, auto ept_c) {  // (every thread calls it; n is uniform)
    constexpr int EPT = decltype(ept_c)::value, P = NT * EPT;
    static_assert(P <= LCAP && (EPT & (EPT - 1)) == 0, "the exchange buffer is s_ltile");
    unsigned v[EPT], lt[EPT];
#pragma unroll
    for (int m = 0; m < EPT; m++) {
      const int e = tid * EPT + m;
      v[m] = ~0u;  // padding: behind every entry
      lt[m] = 0;
      if (e < n) {
        unsigned k = K3_LB_NONE;
#pragma unroll
        for (int p = 0; p < 8; p++) { const unsigned w = s_llbw[e * 8 + p]; k = min(k, min(w & 0xFFFFu, w >> 16)); }
        v[m] = (k << 10) | (unsigned)e;
        lt[m] = s_ltile[e];
      }
    }
    __syncthreads();  // s_ltile's words are in registers
#pragma unroll
    for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        // word i meets word i ^ j and keeps the smaller one where (i & k) == 0 and (i & j) == 0 agree, the larger one where not
        unsigned w[EPT];
        if (j >= 64 * EPT) {
#pragma unroll
          for (int m = 0; m < EPT; m++) s_ltile[tid * EPT + m] = v[m];
          __syncthreads();
#pragma unroll
          for (int m = 0; m < EPT; m++) w[m] = s_ltile[(tid * EPT + m) ^ j];
          __syncthreads();
        } else {
#pragma unroll
          for (int m = 0; m < EPT; m++) w[m] = j < EPT ? v[m ^ (j < EPT ? j : 0)] : (unsigned)__shfl_xor((int)v[m], j / EPT);
        }
#pragma unroll
        for (int m = 0; m < EPT; m++) {
          const int i = tid * EPT + m;
          v[m] = (((i & k) == 0) == ((i & j) == 0)) ? min(v[m], w[m]) : max(v[m], w[m]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < EPT; m++) {
      const int e = tid * EPT + m;
      if (e < n) { s_ltile[e] = lt[m]; s_key[e] = (uint16_t)(v[m] & 1023u); }  // (the padding sorts behind the n entries)
    }
    __syncthreads();
  };
  int nseg = 0;
  auto flush = [&]() {  // the buffer's entries become a segment (every thread calls it; n is uniform)
    const int n = s_ctl[0];
    if (n > 0) {
      if (tid == 0) {
        const unsigned long long off = atomicAdd(a.arena_cursor, (unsigned long long)n);
        const bool fits = off + (unsigned long long)n <= a.arena_cap;
        s_ctl[2] = fits ? 1 : 0;
        s_ctl[3] = (int)(unsigned)off;  // (arena_cap < 2^32 entries: checked on the host)
        if (nseg < a.max_segs) a.segs[g * a.max_segs + nseg] = make_uint2((unsigned)off, fits ? (unsigned)n : 0u);
      }
      __syncthreads();
      if (s_ctl[2]) {
        const bool sorted = a.list_order != 0;
        if (sorted) {
          if (n <= 2 * NT) sort_segment(n, std::integral_constant<int, 2>());
          else sort_segment(n, std::integral_constant<int, LCAP / NT>());
        }
        const unsigned off = (unsigned)s_ctl[3];
        for (int i = tid; i < n; i += NT) a.ltile[off + i] = s_ltile[sorted ? (int)s_key[i] : i];
        unsigned *dst = reinterpret_cast<unsigned *>(a.llb) + (size_t)off * NSW;
        for (int i = tid; i < n * NSW; i += NT) {
          const int e = i / NSW;
          dst[i] = s_llbw[(sorted ? (int)s_key[e] : e) * 8 + (i - e * NSW)];
        }
      }
      nseg++;
      __syncthreads();
      if (tid == 0) s_ctl[0] = 0;
      __syncthreads();
    }
  };
  for (int run_batch = 0; run_batch < n_run_batches; run_batch++) {
    if (tid < RB) s_rmask[tid] = 0;
    __syncthreads();
    {
      const int jr = run_batch * RB + (tid >> 4), s = tid & 15;
      const int off = (jr + 1) >> 1, run = (jr & 1) ? home_run + off : home_run - off;
      if (jr < total_run_slots && run >= 0 && run < n_grp && s < nvalid) {
        unsigned lbq = 0;
#pragma unroll
        for (int d = 0; d < ND; d++) {
          const int tlo = a.grp_lo[d * n_grp + run], thi = a.grp_hi[d * n_grp + run];
          lbq += k3_box_gap_sq(tlo, thi, s_qbox[qmeta_at(s, QMETA_LO + d)], s_qbox[qmeta_at(s, QMETA_HI + d)]);
        }
        if (k3_box_root(lbq) <= s_smax[s]) atomicOr(&s_rmask[tid >> 4], 1u << s);  // (compared, never stored: a bound of a sub-tile is <= K3_LB_MAX, so the cap changes nothing)
      }
    }
    __syncthreads();
    if (tid < 64) {  // surviving runs of the batch, in outward order
      const int jr = run_batch * RB + lane;
      const int off = (jr + 1) >> 1, run = (jr & 1) ? home_run + off : home_run - off;
      const unsigned m = lane < RB ? s_rmask[lane] : 0u;
      const unsigned long long alive = __builtin_amdgcn_ballot_w64(m != 0);
      if (m) s_runs[__popcll(alive & ((1ull << lane) - 1ull))] = ((unsigned)run << 16) | m;
      if (lane == 0) s_ctl[1] = __popcll(alive);
    }
    __syncthreads();
    const int run_alive = s_ctl[1];
    for (int run_k = 0; run_k < run_alive; run_k += RS) {
      if (s_ctl[0] + NT > LCAP) flush();  // (uniform: every thread reads the same count behind the last barrier)
      // tile tests: RS surviving runs per step, thread = (run, tile of the run); the run's sub-tile mask is uniform in a wave
      const int k = run_k + (tid >> 7);
      const unsigned rm = k < run_alive ? s_runs[k] : 0u;
      const unsigned rmask = (unsigned)__builtin_amdgcn_readfirstlane((int)(rm & 0xFFFFu));
      const int64_t tile = (int64_t)(rm >> 16) * KNN_GROUP + (tid & 127);
      const bool valid = rmask != 0 && tile < n_ttiles && !(tile >= r0a && tile < r0b);
      // 16-bit lower bounds of this lane's tile against the 16 sub-tile slots: a 256-bit shift register, one value pushed per slot (so
      // the loop stays rolled: no run-time register index), slot s ends in bits 16 * (s & 1) of lbw[s >> 1]
      unsigned lbw[8];
#pragma unroll
      for (int p = 0; p < 8; p++) lbw[p] = 0xFFFFFFFFu;
      bool any = false;
      if (rmask) {
        int tlo[ND], thi[ND];
        const int64_t tc = valid ? tile : 0;
#pragma unroll
        for (int d = 0; d < ND; d++) { tlo[d] = a.box_lo[(int64_t)d * n_ttiles + tc]; thi[d] = a.box_hi[(int64_t)d * n_ttiles + tc]; }
#pragma unroll 1
        for (int s = 0; s < 16; s++) {
          unsigned v16 = K3_LB_NONE;
          if ((rmask >> s) & 1u) {  // uniform
            const int *const ql = &s_qbox[qmeta_at(s, QMETA_LO)], *const qh = &s_qbox[qmeta_at(s, QMETA_HI)];
            const v4i q0 = *reinterpret_cast<const v4i *>(ql), q1 = *reinterpret_cast<const v4i *>(ql + 4), q2 = *reinterpret_cast<const v4i *>(qh),
                      q3 = *reinterpret_cast<const v4i *>(qh + 4);
            const int qlo[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
            const int qhi[8] = {q2[0], q2[1], q2[2], q2[3], q3[0], q3[1], q3[2], q3[3]};
            unsigned lbq = 0;
#pragma unroll
            for (int d = 0; d < ND; d++) {
              lbq += k3_box_gap_sq(tlo[d], thi[d], qlo[d], qhi[d]);
            }
            const unsigned lb16 = k3_box_bound16(lbq);
            if (valid && lb16 <= s_smax[s]) { v16 = lb16; any = true; }
          }
#pragma unroll
          for (int p = 0; p < 7; p++) lbw[p] = __builtin_amdgcn_alignbit(lbw[p + 1], lbw[p], 16);
          lbw[7] = (lbw[7] >> 16) | (v16 << 16);
        }
      }
      {  // ordered append: the waves take their places one after the other (wave w's tiles come before wave w + 1's)
        const unsigned long long pb = __builtin_amdgcn_ballot_w64(any);
        __shared__ int s_wcnt[NT / 64];
        if (lane == 0) s_wcnt[tid >> 6] = __popcll(pb);
        __syncthreads();
        int base = s_ctl[0];
        for (int w = 0; w < (tid >> 6); w++) base += s_wcnt[w];
        const int idx = base + __popcll(pb & ((1ull << lane) - 1ull));
        if (any) {
          s_ltile[idx] = k3_entry(tile, a.thmask);  // the entry carries the tile's high-chunk mask: the consumer has it before the tile
#pragma unroll
          for (int p = 0; p < 8; p++) s_llbw[idx * 8 + p] = lbw[p];
        }
        __syncthreads();
        if (tid == 0) { int t = s_ctl[0]; for (int w = 0; w < NT / 64; w++) t += s_wcnt[w]; s_ctl[0] = t; }
        __syncthreads();
      }
    }
  }
  flush();
  if (tid == 0) a.nsegs[g] = min(nseg, a.max_segs);
}

// collection mode: the bound every sub-tile's tiles are judged against, from its queries' thresholds (what the seed kernel derives from
// the bests in the nearest-neighbour search)
__global__ __launch_bounds__(256) void k_knn_tau_bounds(const int *__restrict__ tau, int64_t nq, int64_t n_qtiles, unsigned *__restrict__ gsmax) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w * 2 < n_qtiles; w += (int64_t)gridDim.x * 4) {
    const int64_t st = w * 2 + (lane >> 5), q = st * 32 + (lane & 31);
    unsigned v = (st < n_qtiles && q < nq) ? (unsigned)(tau[q] + 1) : 0u;  // tau + 1 = the SSD bound
    for (int o = 16; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    if ((lane & 31) == 0 && st < n_qtiles) gsmax[st] = k3_bound_of(v);
  }
}

int launch_tau_bounds(const Knn3Args &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_knn_tau_bounds, dim3((unsigned)std::min<int64_t>((a.n_qtiles + 7) / 8, 2048)), dim3(256), 0, stream, a.tau, a.nq, a.n_qtiles, a.gsmax);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_lists(const Knn3Args &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_knn_lists, dim3((unsigned)a.n_groups), dim3(K3_LIST_NT), 0, stream, a);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx
