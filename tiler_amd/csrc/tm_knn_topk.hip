// tm_knn_topk.hip -- k nearest rows (ann_kdtree_short_search_multi, tilingencoder.pas:1563) on the pruned MFMA scan of tm_knn.hip.
//  1. k_topk_tau: every query's k-th smallest exact SSD among the TOPK_WINDOW database tiles around its position on the
//     curve = an upper bound tau of its true k-th smallest SSD (any k rows give one).  A large search takes its first thresholds
//     from a search of a sample of the database instead (knn_index_search_topk).
//  2. the third scan shape in collection mode (tm_knn3.h: k_knn_tau_bounds, k_knn_lists, k_knn_consume<.., TOPK = true>) with
//     those thresholds; every row with d'' <= tau lands in the query's candidate list (at most `cap` entries, the count keeps running).
//  3. k_topk_select: exact SSD (d'' + the query norm's parity bit), original row index, rank by (SSD, index), first k out.
//     A query whose list overflowed keeps the threshold the scan's ladder ended on (still a valid bound) and is
//     scanned again with the other overflowed queries.
#include <chrono>

#include "tm_knn.h"

#ifndef TM_TOPK_EST_STRIDE
#define TM_TOPK_EST_STRIDE 16  // the sample a large search's first thresholds come from: every 16th row ...
#endif
#ifndef TM_TOPK_EST_K
#define TM_TOPK_EST_K 12       // ... and the distance of its 12th nearest: about 192 rows of the whole database lie within it, give or take 55
#endif
#ifndef TM_TOPK_STEP_SHIFT
#define TM_TOPK_STEP_SHIFT 3  // a first pass's rungs (and a restart's) hang at tau >> this below the threshold
#endif
#ifndef TM_TOPK_WINDOW
#define TM_TOPK_WINDOW 32
#endif
#ifndef TM_TOPK_CAP_LATER
#define TM_TOPK_CAP_LATER 1024
#endif
#ifndef TM_TOPK_CAP_FIRST
#define TM_TOPK_CAP_FIRST 512
#endif
#ifndef TM_TOPK_CAP_FIRST_SMALLK
#define TM_TOPK_CAP_FIRST_SMALLK 512  // ... of a search for fewer than 32 rows (the sample search of knn_index_search_topk)
#endif
#ifndef TM_TOPK_BUDGET_GIB
#define TM_TOPK_BUDGET_GIB 24  // candidate lists of a pass (also capped at a third of the free device memory)
#endif

namespace tmx {

constexpr int TOPK_WINDOW_DEFAULT = TM_TOPK_WINDOW;  // tiles (of 32 rows) sampled for the first threshold (8: 1.45 s, 32: 0.99 s, 128: 1.00 s on the bench clip)

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int topk_dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}

// lane = sorted query; the window's rows are wave-uniform (scalar loads); per lane the k smallest distances in LDS [slot][lane]
__global__ __launch_bounds__(64) void k_topk_tau(const uint32_t *__restrict__ queries, const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ qkey,
                                                 int64_t nq, const uint32_t *__restrict__ db, const uint32_t *__restrict__ tperm,
                                                 const uint32_t *__restrict__ tnorm /* |row|^2 in sorted order */,
                                                 const uint32_t *__restrict__ tkey, int64_t nt, int64_t ntt, int k, int window, int *__restrict__ tau) {
  extern __shared__ uint32_t s_d[];  // [k][64]
  const int lane = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * 64, p = p0 + lane;
  const int64_t pq = min(p, nq - 1);
  const uint32_t *qrow = queries + (int64_t)qperm[pq] * 96;
  uint32_t q[96];
#pragma unroll
  for (int j = 0; j < 96; j += 4) {
    const uint4 v = *reinterpret_cast<const uint4 *>(qrow + j);
    q[j] = v.x; q[j + 1] = v.y; q[j + 2] = v.z; q[j + 3] = v.w;
  }
  uint32_t qn = 0;
#pragma unroll
  for (int j = 0; j < 96; j++) qn = (uint32_t)topk_dot2(q[j], q[j], (int)qn);
  // window: the tiles around the curve position of the wave's first query (as round 0 of the scan does for a workgroup)
  const uint32_t k0 = qkey[min(p0, nq - 1)];
  int64_t lo = 0, hi = ntt;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (tkey[mid] <= k0) lo = mid + 1; else hi = mid; }
  int64_t start = max((int64_t)0, lo - 1 - window / 2);
  start = min(start, max((int64_t)0, ntt - window));
  const int64_t r0 = start * 32, r1 = min(nt, (start + window) * 32);
  // The k smallest so far sit in LDS [slot][lane]; what decides whether a row enters is their largest.  The slots are taken in groups
  // of eight with each group's largest (and where it sits) in registers: replacing the largest re-reads ITS group only -- with 64 lanes
  // some lane replaces at almost every row, and a re-scan of all k slots per row was three quarters of this kernel.
  int cnt = 0, mslot = 0;
  uint32_t mx = 0;
  uint32_t gm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int gs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int ngr = (k + 7) >> 3;
  auto regroup = [&](int g) {  // group g's largest and its slot, then the overall ones
    uint32_t m = 0;
    int at = g * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int sl = g * 8 + i;
      const uint32_t v = sl < k ? s_d[sl * 64 + lane] : 0u;
      if (sl < k && (v > m || i == 0)) { m = v; at = sl; }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) if (j == g) { gm[j] = m; gs[j] = at; }
    mx = gm[0]; mslot = gs[0];
#pragma unroll
    for (int j = 1; j < 8; j++) if (j < ngr && gm[j] > mx) { mx = gm[j]; mslot = gs[j]; }
  };
  for (int64_t r = r0; r < r1; r++) {
    const uint32_t *row = db + (int64_t)tperm[r] * 96;
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 96; j++) acc = topk_dot2(q[j], row[j], acc);
    const uint32_t d = qn + tnorm[r] - 2u * (uint32_t)acc;
    if (cnt < k) {
      s_d[cnt * 64 + lane] = d;
      cnt++;
      if (cnt == k)
        for (int g = 0; g < ngr; g++) regroup(g);
    } else if (d < mx) {
      s_d[mslot * 64 + lane] = d;
      regroup(mslot >> 3);
    }
  }
  tau[p] = (cnt >= k && mx < 0x7fffffffu) ? (int)mx : 0x7ffffffe;  // fewer than k rows in the window: everything is a candidate
}

__global__ void k_sorted_row_norms(const int16_t *__restrict__ rows, const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ norm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int16_t *r = rows + (int64_t)perm[i] * 192;
    uint32_t s = 0;
    for (int j = 0; j < 192; j++) { const int v = r[j]; s += (uint32_t)(v * v); }
    norm[i] = s;
  }
}

// one wave per (sorted) query: rank its candidates by (SSD, original index); the first k go out in that order.  With member
// lists (grp_off != null) a candidate is a DISTINCT row standing for all its duplicates: every member has the candidate's SSD
// and its own index, so the output positions of a candidate's members start after all members of strictly nearer candidates and
// interleave by index with the members of other candidates at exactly the same SSD (rare).
__global__ __launch_bounds__(64) void k_topk_select(int64_t nq, const uint32_t *__restrict__ qperm, const uint8_t *__restrict__ qpack, int q_bytes,
                                                    const uint32_t *__restrict__ tperm, int64_t nt, const uint2 *__restrict__ cand,
                                                    const int *__restrict__ cand_cnt, int cap, int k, int *__restrict__ tau, const int *__restrict__ tau_in /* the thresholds the scan started from */,
                                                    int *__restrict__ step /* in: the pass's rung spacing; out, overflowed queries: the next pass's */,
                                                    const uint32_t *__restrict__ out_map /* null: qperm */, int32_t *__restrict__ out_idx,
                                                    uint32_t *__restrict__ out_err, uint32_t *__restrict__ ovf_list, unsigned int *__restrict__ ovf_count,
                                                    const uint32_t *__restrict__ grp_off, const uint32_t *__restrict__ grp_members, int nofilter,
                                                    uint32_t *__restrict__ unf_list /* non-null: the thresholds were ESTIMATES (topk_estimate) -- a query with fewer than k rows within its
                                                    threshold goes on this list (count: ovf_count[1]) and is searched again from a bound that holds */) {
  extern __shared__ unsigned long long s_key[];  // [cap rounded up to a power of two]
  __shared__ uint32_t s_mult[64];
  const int64_t p = blockIdx.x;
  if (p >= nq) return;
  const int lane = threadIdx.x;
  const int total = cand_cnt[p], stored = min(total, cap);
  // The scan left its final threshold in tau (it walks down the ladder while rows come in): stored candidates above it cannot be among
  // the k nearest, and dropping them before the sort shrinks it (a full list of 512 typically keeps about a hundred).
  const int th = nofilter ? INT_MAX : tau[p];
  if (total > cap) {
    // The list filled up: the query is scanned again.  Its threshold is the one the scan's ladder ended on; the next pass's ladder hangs eight
    // rungs over the bracket this pass left -- from that threshold down to the rung below it, which did not fill.  (Where the rungs hang is a
    // matter of speed only: every threshold a filled rung gives is a valid bound.  The k-th smallest of the rows that WERE stored, a bound
    // too, is no longer worked out: the first `cap` rows met say little where thousands lie within the threshold, and sorting them for it
    // was most of this kernel's time on such data.)
    if (lane == 0) {
      const int tn = min(th, 0x7ffffffe), t_in = tau_in[p], st = max(1, min(step[p], t_in >> 3));  // (the spacing as the scan clamped it)
      tau[p] = tn;
      // ... unless the threshold ended on the ladder's LOWEST rung: then nothing says how far below it the k-th nearest lies, and a ladder
      // an eighth as wide would only crawl down by its own width per pass: eighths of the threshold again
      const bool lowest = (long long)tn <= (long long)t_in - 7ll * st;
      step[p] = lowest ? max(1, tn >> TM_TOPK_STEP_SHIFT) : max(1, st >> 3);
      ovf_list[atomicAdd(ovf_count, 1u)] = (uint32_t)p;
    }
    return;
  }
  const uint32_t parity = reinterpret_cast<const uint32_t *>(qpack + (p >> 5) * (int64_t)q_bytes + knn_pack_row_terms_of(q_bytes))[p & 31] & 1u;
  int n = 0;
  // (the stored candidates are asked for eight chunks of 64 at a time: a chunk per round trip to memory was most of this kernel -- the sort
  // below is 1.5 ms of the bench clip's 23)
  for (int base0 = 0; base0 < stored; base0 += 512) {
    uint2 cbuf[8];
    uint32_t orow[8];
    bool ok[8];
#pragma unroll
    for (int u = 0; u < 8; u++) { const int i = base0 + u * 64 + lane; cbuf[u] = i < stored ? cand[p * cap + i] : make_uint2(0x7fffffffu, 0xffffffffu); }
#pragma unroll
    for (int u = 0; u < 8; u++) {  // (the original indices of the rows that pass: gathered together as well)
      const int i = base0 + u * 64 + lane;
      // signed, like the scan's own test: d'' = SSD - parity is -1 for an exact match of a query with an odd norm
      ok[u] = i < stored && (int)cbuf[u].x <= th && (int64_t)cbuf[u].y < nt;  // padded rows of the last tile replicate row nt-1: not rows
      orow[u] = ok[u] ? tperm[cbuf[u].y] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      if (base0 + u * 64 >= stored) break;  // (uniform)
      const bool valid = ok[u];
      const unsigned long long key = ((unsigned long long)(cbuf[u].x + parity) << 32) | orow[u];
      const unsigned long long m = __ballot(valid);
      if (valid) s_key[n + __popcll(m & ((1ull << lane) - 1ull))] = key;
      n += __popcll(m);
    }
  }
  if (unf_list && n < k) {  // (uniform in the wave.  n counts DISTINCT rows: with member lists k rows may need fewer, the second search only costs time)
    if (lane == 0) unf_list[atomicAdd(ovf_count + 1, 1u)] = (uint32_t)p;
    return;
  }
  if (n > 1024) {
    // the same from LDS, for the long lists the last passes give their few queries (up to 8 192 rows at, or tied with, the k-th distance)
    __syncthreads();
    uint32_t lo = 0xffffffffu, hi = 0;
    for (int i = lane; i < n; i += 64) { const uint32_t v = (uint32_t)(s_key[i] >> 32); lo = min(lo, v); hi = max(hi, v); }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, o)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, o)); }
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      int c = 0;
      for (int i0 = 0; i0 < n; i0 += 64) c += __popcll(__ballot(i0 + lane < n && (uint32_t)(s_key[min(i0 + lane, n - 1)] >> 32) <= mid));
      if (c >= k) hi = mid; else lo = mid + 1;
    }
    int m2 = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {  // in place: a chunk's survivors land at or before the chunk
      const unsigned long long key = s_key[min(i0 + lane, n - 1)];
      const bool keep = i0 + lane < n && (uint32_t)(key >> 32) <= lo;
      const unsigned long long m = __ballot(keep);
      if (keep) s_key[m2 + __popcll(m & ((1ull << lane) - 1ull))] = key;
      m2 += __popcll(m);
    }
    n = m2;
  } else if (n > 2 * k) {
    // Only the k smallest matter: the smallest SSD V with k candidates at or below it, by bisection over the values (sixteen keys a lane in
    // registers, a ballot a chunk and step), then only the candidates up to V go through the sort -- a full bitonic sort of several hundred
    // keys in LDS was this kernel's time (~1.2 microseconds of a CU's LDS bandwidth per query).
    __syncthreads();
    uint32_t ssd[16], idx[16];
    uint32_t lo = 0xffffffffu, hi = 0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = u * 64 + lane;
      const unsigned long long key = i < n ? s_key[i] : ~0ull;
      ssd[u] = (uint32_t)(key >> 32); idx[u] = (uint32_t)key;
      if (i < n) { lo = min(lo, ssd[u]); hi = max(hi, ssd[u]); }
    }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, o)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, o)); }
    const int nch = (n + 63) >> 6;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      int c = 0;
#pragma unroll
      for (int u = 0; u < 16; u++)
        if (u < nch) c += __popcll(__ballot(u * 64 + lane < n && ssd[u] <= mid));
      if (c >= k) hi = mid; else lo = mid + 1;
    }
    __syncthreads();  // every key is in registers
    int m2 = 0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
      if (u >= nch) break;  // (uniform)
      const bool keep = u * 64 + lane < n && ssd[u] <= lo;
      const unsigned long long m = __ballot(keep);
      if (keep) s_key[m2 + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)ssd[u] << 32) | idx[u];
      m2 += __popcll(m);
    }
    n = m2;
  }
  int n2 = 64;
  while (n2 < n) n2 <<= 1;
  for (int i = n + lane; i < n2; i += 64) s_key[i] = ~0ull;
  __syncthreads();
  // bitonic sort of the keys (one wave): (SSD, index of the row / of the distinct row's first occurrence) ascending
  for (int ks = 2; ks <= n2; ks <<= 1)
    for (int j = ks >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (n2 >> 1); t += 64) {  // a lane per compare-exchange: the lower element of pair t (every lane works, not every other one)
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
        const unsigned long long a = s_key[i], b = s_key[o];
        const bool up = (i & ks) == 0;
        if ((a > b) == up) { s_key[i] = b; s_key[o] = a; }
      }
      __syncthreads();
    }
  const int64_t q = out_map ? out_map[p] : qperm[p];
  // The k nearest ROWS come from the first k candidates: a member of a later candidate has at least k members before it.
  const int m = min(n, k);
  unsigned long long me = ~0ull;
  if (lane < m) me = s_key[lane];
  const bool real = me != ~0ull;
  const uint32_t ssd = (uint32_t)(me >> 32), id = (uint32_t)me;
  if (lane < 64) s_mult[lane] = real ? (grp_off ? grp_off[id + 1] - grp_off[id] : 1u) : 0u;
  __syncthreads();
  if (!real) return;
  uint32_t before = 0;  // members of strictly nearer candidates (without lists: the candidate's own rank)
  bool shared = false;  // another candidate at exactly this SSD
  for (int j = 0; j < m; j++) {
    const unsigned long long o = s_key[j];
    if (o == ~0ull) continue;
    const uint32_t os = (uint32_t)(o >> 32);
    if (grp_off) {
      if (os < ssd) before += s_mult[j];
      else if (os == ssd && j != lane) shared = true;
    } else {
      before += j < lane ? 1u : 0u;
    }
  }
  if (before >= (uint32_t)k) return;
  if (!grp_off) { out_idx[q * k + before] = (int32_t)id; out_err[q * k + before] = ssd; return; }
  const uint32_t o0 = grp_off[id], mult = s_mult[lane];
  for (uint32_t a = 0; a < mult; a++) {
    const uint32_t idx = grp_members[o0 + a];
    uint32_t pos = before + a;
    if (shared) {  // members of the other candidates at this SSD with a smaller index come first
      for (int j = 0; j < m; j++) {
        const unsigned long long o = s_key[j];
        if (j == lane || o == ~0ull || (uint32_t)(o >> 32) != ssd) continue;
        const uint32_t oo = grp_off[(uint32_t)o], om = s_mult[j];
        uint32_t lo = 0, hi = om;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (grp_members[oo + mid] < idx) lo = mid + 1; else hi = mid; }
        pos += lo;
      }
    }
    if (pos >= (uint32_t)k) { if (!shared) break; else continue; }
    out_idx[q * k + pos] = (int32_t)idx;
    out_err[q * k + pos] = ssd;
  }
}
__global__ void k_topk_fill(int32_t *__restrict__ out_idx, uint32_t *__restrict__ out_err, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) { out_idx[i] = -1; out_err[i] = 0xffffffffu; }
}

__global__ void k_topk_sorted_aux(const uint32_t *__restrict__ qperm, int64_t n, int64_t n_pad, const int *__restrict__ tau_by_row,
                                  const int *__restrict__ step_by_row, const uint32_t *__restrict__ rowmap, int *__restrict__ tau_sorted,
                                  int *__restrict__ tau_in_sorted, int *__restrict__ step_sorted, uint32_t *__restrict__ map_sorted) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n_pad; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t row = qperm[min(p, n - 1)];
    if (tau_by_row) tau_sorted[p] = tau_by_row[row];
    const int tau = tau_sorted[p];
    tau_in_sorted[p] = tau;  // (the scan overwrites tau_sorted with the thresholds it ends on)
    step_sorted[p] = step_by_row ? step_by_row[row] : (tau > 0 ? max(1, tau >> TM_TOPK_STEP_SHIFT) : 0);  // a first pass: rungs at this fraction of the threshold
    if (p < n) map_sorted[p] = rowmap ? rowmap[row] : row;
  }
}
__global__ void k_topk_gather_sub(const int16_t *__restrict__ feats, const uint32_t *__restrict__ qperm, const uint32_t *__restrict__ list, int64_t n,
                                  const int *__restrict__ tau_sorted, const int *__restrict__ step_sorted, const uint32_t *__restrict__ map_sorted,
                                  int16_t *__restrict__ sub, int *__restrict__ sub_tau, int *__restrict__ sub_step, uint32_t *__restrict__ sub_map) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * 24; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / 24;
    const int v = (int)(e - j * 24);
    const uint32_t p = list[j];
    reinterpret_cast<uint4 *>(sub)[e] = reinterpret_cast<const uint4 *>(feats + (int64_t)qperm[p] * 192)[v];
    if (v == 0) { sub_tau[j] = tau_sorted[p]; sub_step[j] = step_sorted[p]; sub_map[j] = map_sorted[p]; }
  }
}
__global__ void k_topk_scatter(const int32_t *__restrict__ idx, const uint32_t *__restrict__ err, const uint32_t *__restrict__ map, int64_t n, int k,
                               int32_t *__restrict__ out_idx, uint32_t *__restrict__ out_err) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * k; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / k;
    out_idx[(int64_t)map[j] * k + (e - j * k)] = idx[e];
    out_err[(int64_t)map[j] * k + (e - j * k)] = err[e];
  }
}

// every `stride`-th row of the database: the sample a large search takes its first thresholds from (knn_index_search_topk)
__global__ void k_topk_sample_rows(const int16_t *__restrict__ db, int64_t nt, int stride, int64_t ns, int16_t *__restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ns * 24; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / 24;
    const int v = (int)(e - j * 24);
    reinterpret_cast<uint4 *>(out)[e] = reinterpret_cast<const uint4 *>(db + min(j * stride, nt - 1) * 192)[v];
  }
}
// the sample search's ke-th distance as the full search's first threshold (0xFFFFFFFF: the sample had fewer than ke rows for this query)
__global__ void k_topk_tau_from_sample(const uint32_t *__restrict__ err, int64_t nq, int ke, int *__restrict__ tau) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t e = err[i * ke + ke - 1];
    tau[i] = e < 0x7ffffffeu ? (int)e : 0x7ffffffe;
  }
}

struct TopkExpand { const uint32_t *grp_off = nullptr, *grp_members = nullptr; const void *full_db = nullptr; int64_t full_nt = 0; };

// What one pass needs on the device beside the index: the thresholds (as the scan leaves them, and as it got them), the ladders' rung
// spacing, where each sorted query's results go, the candidate lists, and the queries select hands on (overflowed / short of an estimate).
struct TopkPass {
  int cap = 0;
  DevBuf tau, tau_in, step, map_sorted, cand, cand_cnt, ovf, counter, unf;
};

// candidates a query may store: 512 in the first pass; the passes over the overflowed queries have far fewer queries and take what 24 GB
// hold, up to 1024 -- the threshold an overflowed query leaves is the k-th smallest of what it STORED, and on data whose distances
// bunch (the literal bench clip: four in five queries overflow the first pass) 512 stored rows moved it by a third per pass; 4096 made the
// select kernel's sort the cost instead (a pass of 826 000 queries: 522 ms against 25)
// (from the fourth pass on -- a few thousand queries at most -- up to 8 192: what is left by then are queries with hundreds of rows AT their
// k-th distance, which no threshold separates; the select stage picks the k smallest of a long list by bisection)
static int topk_cap(int64_t n, int k, int depth) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)32 << 30; }
  const int64_t budget = std::max<int64_t>((int64_t)4 << 30, std::min<int64_t>((int64_t)TM_TOPK_BUDGET_GIB << 30, (int64_t)(free_b / 3)));
  return (int)std::max<int64_t>(2 * k, std::min<int64_t>(depth == 0 ? (k < 32 ? TM_TOPK_CAP_FIRST_SMALLK : TM_TOPK_CAP_FIRST) : depth < 3 ? TM_TOPK_CAP_LATER : 8192, budget / (n * 8)));
}

// the pass's buffers, and every sorted query's threshold, rung spacing and output row: the caller's (tau_by_row) or, when null, the curve
// window's bound
static int topk_thresholds(tm_knn_index_impl *ix, const int16_t *feats, int64_t n, const int *tau_by_row, const int *step_by_row, const uint32_t *rowmap, int k,
                           bool estimated, TopkPass &ps, hipStream_t stream) {
  const int64_t nqt = knn_tiles(n), ntt = knn_tiles(ix->nt), n_pad = ((nqt + 1) / 2) * 64;
  if (estimated) TM_TRY(ps.unf.alloc((size_t)n * 4));
  TM_TRY(ps.tau.alloc((size_t)n_pad * 4)); TM_TRY(ps.tau_in.alloc((size_t)n_pad * 4)); TM_TRY(ps.step.alloc((size_t)n_pad * 4)); TM_TRY(ps.map_sorted.alloc((size_t)n * 4));
  TM_TRY(ps.cand.alloc((size_t)n * ps.cap * 8)); TM_TRY(ps.cand_cnt.alloc((size_t)n * 4));
  TM_TRY(ps.ovf.alloc((size_t)n * 4)); TM_TRY(ps.counter.alloc(16));
  TM_HIP(hipMemsetAsync(ps.cand_cnt.p, 0, (size_t)n * 4, stream));
  TM_HIP(hipMemsetAsync(ps.counter.p, 0, 16, stream));
  if (!tau_by_row) {
    DevBuf tnorm;  // the plan (hence the sort order) can change between passes, so the norms are made per pass: 171 K rows, microseconds
    TM_TRY(tnorm.alloc((size_t)ix->nt * 4));
    hipLaunchKernelGGL(k_sorted_row_norms, dim3(gridn(ix->nt)), dim3(256), 0, stream, ix->db, ix->tperm.as<uint32_t>(), ix->nt, tnorm.as<uint32_t>());
    TM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_topk_tau, dim3((unsigned)(n_pad / 64)), dim3(64), (size_t)k * 64 * 4, stream, (const uint32_t *)feats, ix->qperm.as<uint32_t>(),
                       ix->qkey.as<uint32_t>(), n, (const uint32_t *)ix->db, ix->tperm.as<uint32_t>(), tnorm.as<uint32_t>(), ix->tkey.as<uint32_t>(), ix->nt, ntt, k,
                       TOPK_WINDOW_DEFAULT, ps.tau.as<int>());
    TM_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_topk_sorted_aux, dim3(gridn(n_pad)), dim3(256), 0, stream, ix->qperm.as<uint32_t>(), n, n_pad, tau_by_row, step_by_row, rowmap, ps.tau.as<int>(),
                     ps.tau_in.as<int>(), ps.step.as<int>(), ps.map_sorted.as<uint32_t>());
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// The third scan shape in collection mode (tm_knn3.h): bounds from the thresholds, tile lists judged against them (no seeds:
// every tile goes through the lists), then the consume kernel appending every row within its query's threshold.
static int topk_collect(tm_knn_index_impl *ix, int64_t n, int k, TopkPass &ps, hipStream_t stream) {
  const int64_t nqt = knn_tiles(n), ntt = knn_tiles(ix->nt);
  TM_TRY(launch_qmeta(ix, nqt, ntt, knn_boxes(ix), stream));
  TM_TRY(ix->counters.alloc(sizeof(K3Counters)));
  Knn3Args a;
  TM_TRY(scan_args(ix, n, knn3_sub_tiles_topk(ix->plan.hq), &a));
  a.no_seeds = 1;
  a.tau = ps.tau.as<int>(); a.step = ps.step.as<int>(); a.cand = ps.cand.as<uint2>(); a.cand_cnt = ps.cand_cnt.as<int>(); a.cand_cap = ps.cap; a.cand_k = k;
  // few queries left: their few workgroups would each walk most of the database one after the other -- share the tile lists
  a.split = a.n_groups >= 512 ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(64, 1024 / std::max<int64_t>(a.n_groups, 1)));
  a.grid_blocks = scan_grid_blocks(a.n_groups * a.split);
  TM_TRY(ensure_list_buffers(ix, &a));
  TM_TRY(launch_tau_bounds(a, stream));
  K3Counters *c = ix->dev_counters();
  for (int attempt = 0;; attempt++) {
    // collection lists are long (a threshold from 32 tiles of the curve is loose): twice the nearest-neighbour search's experience to begin with
    TM_TRY(ensure_arena(ix, 2.0, &a));
    TM_HIP(hipMemsetAsync(c, 0, offsetof(K3Counters, seed), stream));  // (no seed kernel runs: its stripes are left alone)
    TM_TRY(launch_lists(a, stream));
    unsigned long long cursor = 0;
    {  // the lists must fit before anything is collected through them (a second collection pass would double the candidates)
      HostRead hr_(stream);
      TM_TRY(hr_.get(&cursor, &c->stats[K3S_CURSOR], 8));
      TM_TRY(hr_.wait());
    }
    if (cursor <= ix->arena_cap) break;
    TM_TRY(arena_overflowed(ix, cursor, attempt));
  }
  return launch_collect(ix, a, stream);
}

static int topk_pow2(int v) { int r = 64; while (r < v) r <<= 1; return r; }

// rank every query's candidates, the first k out; what select could not finish comes back as counts: queries whose list overflowed (ps.ovf)
// and, with estimated thresholds, queries with fewer than k rows within theirs (ps.unf)
static int topk_select(tm_knn_index_impl *ix, int64_t n, int k, int32_t *out_idx, uint32_t *out_err, const TopkExpand &ex, bool estimated, TopkPass &ps,
                       unsigned int *novf, unsigned int *nunf, hipStream_t stream) {
  const size_t lds = (size_t)topk_pow2(ps.cap) * 8;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_topk_select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_topk_select, dim3((unsigned)n), dim3(64), lds, stream, n, ix->qperm.as<uint32_t>(), ix->qpack.as<uint8_t>(),
                     knn_pack_bytes(6 + ix->plan.hq, 0), ix->tperm.as<uint32_t>(), ix->nt, ps.cand.as<uint2>(), ps.cand_cnt.as<int>(), ps.cap, k, ps.tau.as<int>(), ps.tau_in.as<int>(), ps.step.as<int>(),
                     ps.map_sorted.as<uint32_t>(), out_idx, out_err, ps.ovf.as<uint32_t>(), ps.counter.as<unsigned int>(), ex.grp_off, ex.grp_members,
                     0, estimated ? ps.unf.as<uint32_t>() : (uint32_t *)nullptr);
  TM_HIP(hipGetLastError());
  int flag = 0;
  unsigned long long guard = 0;
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(novf, ps.counter.p, 4));
    TM_TRY(hr_.get(nunf, ps.counter.as<unsigned int>() + 1, 4));
    TM_TRY(hr_.get(&flag, ix->err_flag.p, sizeof(int)));
    TM_TRY(hr_.get(&guard, &ix->dev_counters()->stats[K3S_GUARD], 8));
    TM_TRY(hr_.wait());
  }
  TM_CHECK(guard == 0, TM_E_HIP, "knn: the collection scan met a corrupted tile list (guard word %llx)", guard);
  TM_CHECK(flag == 0, TM_E_UNSUPPORTED, "knn: feature range exceeds the exact two-digit int8 split (|v-c| >= 32640)");
  return TM_OK;
}

// the `count` queries on `list` (sorted positions) as a batch of their own: rows, thresholds, rung spacings, output rows
struct TopkSubset { DevBuf rows, tau, step, map; };
static int topk_gather(tm_knn_index_impl *ix, const int16_t *feats, const DevBuf &list, unsigned int count, const TopkPass &ps, TopkSubset &s, hipStream_t stream) {
  if (count == 0) return TM_OK;
  TM_TRY(s.rows.alloc((size_t)count * 384)); TM_TRY(s.tau.alloc((size_t)count * 4)); TM_TRY(s.step.alloc((size_t)count * 4)); TM_TRY(s.map.alloc((size_t)count * 4));
  hipLaunchKernelGGL(k_topk_gather_sub, dim3(gridn((int64_t)count * 24)), dim3(256), 0, stream, feats, ix->qperm.as<uint32_t>(), list.as<uint32_t>(),
                     (int64_t)count, ps.tau.as<int>(), ps.step.as<int>(), ps.map_sorted.as<uint32_t>(), s.rows.as<int16_t>(), s.tau.as<int>(), s.step.as<int>(), s.map.as<uint32_t>());
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// exact brute force for the queries no threshold separates
static int topk_brute(tm_knn_index_impl *ix, const TopkSubset &s, unsigned int count, int k, int32_t *out_idx, uint32_t *out_err, const TopkExpand &ex, hipStream_t stream) {
  DevBuf bi, be;
  TM_TRY(bi.alloc((size_t)count * k * 4)); TM_TRY(be.alloc((size_t)count * k * 4));
  TM_TRY(launch_knn_topk(s.rows.p, count, ex.full_db ? ex.full_db : (const void *)ix->db, ex.full_db ? ex.full_nt : ix->nt, k, bi.p, be.p, stream));
  hipLaunchKernelGGL(k_topk_scatter, dim3(gridn((int64_t)count * k)), dim3(256), 0, stream, bi.as<int32_t>(), be.as<uint32_t>(), s.map.as<uint32_t>(),
                     (int64_t)count, k, out_idx, out_err);
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(stream));
  return TM_OK;
}

// one scan of `n` query rows (feats) with thresholds (tau_by_row, or the curve-window estimate when null); results go to row
// rowmap[i] (or i) of out_idx / out_err; overflowed queries recurse with their tightened thresholds
static int topk_pass(tm_knn_index_impl *ix, const int16_t *feats, int64_t n, const int *tau_by_row, const int *step_by_row, const uint32_t *rowmap, int k,
                     int32_t *out_idx, uint32_t *out_err, int depth, hipStream_t stream, const TopkExpand &ex, bool estimated = false) {
  const auto t_start = std::chrono::steady_clock::now();
  TM_TRY(prepare_search(ix, feats, n, stream));
  TopkPass ps;
  ps.cap = topk_cap(n, k, depth);
  TM_TRY(topk_thresholds(ix, feats, n, tau_by_row, step_by_row, rowmap, k, estimated, ps, stream));
  TM_TRY(topk_collect(ix, n, k, ps, stream));
  unsigned int novf = 0, nunf = 0;
  TM_TRY(topk_select(ix, n, k, out_idx, out_err, ex, estimated, ps, &novf, &nunf, stream));
  if (knobs().knn_debug)
    fprintf(stderr, "[tm_knn] top-%d pass %d: %lld queries of %lld rows, cap %d, %u overflowed, %u fell short of their estimate, %.1f ms\n", k, depth, (long long)n,
            (long long)ix->nt, ps.cap, novf, nunf, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  if (novf == 0 && nunf == 0) return TM_OK;
  // (both subsets are gathered before either is searched: a search re-sorts the index's query side)
  TopkSubset unf, ovf;
  TM_TRY(topk_gather(ix, feats, ps.unf, nunf, ps, unf, stream));
  TM_TRY(topk_gather(ix, feats, ps.ovf, novf, ps, ovf, stream));
  ps.cand.release();  // the recursions allocate their own
  if (nunf > 0)  // from the curve window's bound (any k rows give one), as a search without estimates starts
    TM_TRY(topk_pass(ix, unf.rows.as<int16_t>(), nunf, nullptr, nullptr, unf.map.as<uint32_t>(), k, out_idx, out_err, depth + 1, stream, ex));
  if (novf == 0) return TM_OK;
  // Every pass cuts the bracket its ladder spans to an eighth (or, from the lowest rung, the threshold itself): a dozen passes take any threshold
  // down to single units.  What still overflows then has more rows at exactly the k-th distance than a list holds: exact brute force for those.
  if (depth >= 12 || (depth >= 6 && (int64_t)novf * 10 > n * 9)) return topk_brute(ix, ovf, novf, k, out_idx, out_err, ex, stream);
  return topk_pass(ix, ovf.rows.as<int16_t>(), novf, ovf.tau.as<int>(), ovf.step.as<int>(), ovf.map.as<uint32_t>(), k, out_idx, out_err, depth + 1, stream, ex);
}

int knn_index_search_topk(tm_knn_index_impl *ix, const void *queries, int64_t nq, int k, void *out_idx, void *out_err, hipStream_t stream,
                          const void *grp_off, const void *grp_members, const void *full_db, int64_t full_nt) {
  TM_CHECK(ix != nullptr, TM_E_INVAL, "knn: null index");
  TM_CHECK(k >= 1 && k <= 64, TM_E_INVAL, "top-k: k %d outside 1..64", k);
  if (nq <= 0) return TM_OK;
  hipLaunchKernelGGL(k_topk_fill, dim3(gridn(nq * k)), dim3(256), 0, stream, (int32_t *)out_idx, (uint32_t *)out_err, nq * k);
  TM_HIP(hipGetLastError());
  if (ix->nt == 0) return TM_OK;
  TopkExpand ex;
  ex.grp_off = (const uint32_t *)grp_off; ex.grp_members = (const uint32_t *)grp_members; ex.full_db = full_db; ex.full_nt = full_nt;
  // Many queries against a database of some size: the first thresholds come from a SAMPLE of the database.  The curve window's bound (the k-th
  // smallest of 1 024 rows near the query on the curve) holds but is loose -- on the literal bench clip the 512-th nearest row is 5 % farther
  // than the 64-th, a bound that is off by a factor two lets thousands of rows in, four queries in five overflowed their lists and took three
  // more passes to bracket their k-th distance.  The ke-th nearest row among every S-th row of the database is an ESTIMATE of the (ke S)-th
  // nearest row's distance whatever the distances' law is (the rows within it number ke S give or take S sqrt(ke)): no bound, so a query that
  // finds fewer than k rows within it is searched again the old way (k_topk_select's list of those), but nearly all find between k and the
  // list's capacity at once.  The sample's own search is this same function on a sixteenth of the rows (where the curve window is a third of
  // the database and its bound is good).
  const int est = knobs().topk_estimate;  // -1: by size, 0: never, 1: whenever the sample has ke rows
  constexpr int S = TM_TOPK_EST_STRIDE, KE = TM_TOPK_EST_K;
  const int64_t ns = (ix->nt + S - 1) / S;
  if (est != 0 && k >= 32 && ns >= 4 * KE && (est == 1 || (ix->nt >= 16384 && nq >= 4 * ix->nt))) {
    DevBuf srows, eidx, eerr, tau_est;
    TM_TRY(srows.alloc((size_t)ns * 384)); TM_TRY(eidx.alloc((size_t)nq * KE * 4)); TM_TRY(eerr.alloc((size_t)nq * KE * 4)); TM_TRY(tau_est.alloc((size_t)nq * 4));
    hipLaunchKernelGGL(k_topk_sample_rows, dim3(gridn(ns * 24)), dim3(256), 0, stream, ix->db, ix->nt, S, ns, srows.as<int16_t>());
    TM_HIP(hipGetLastError());
    tm_knn_index_impl *six = nullptr;
    TM_TRY(knn_index_create(srows.p, ns, stream, &six));
    // The sample's search takes its thresholds from the curve window, and on a sixteenth of the rows that bound is looser along the Hilbert order: on the
    // bench clip 1.39 of 4.32 million queries overflowed their lists of 512 and went round again, against 0.56 million along the Morton order (85 ms
    // against 61 for the sample's two passes).  Why was not found; the sample keeps the Morton order unless TM_KNN_CURVE says otherwise.
    six->curve_kind = CURVE_MORTON;
    const int rc = knn_index_search_topk(six, queries, nq, KE, eidx.p, eerr.p, stream, nullptr, nullptr, nullptr, 0);
    if (rc == TM_OK) TM_HIP(hipStreamSynchronize(stream));  // (the sample index owns scratch the stream may still read)
    knn_index_destroy(six);
    if (rc != TM_OK) return rc;
    hipLaunchKernelGGL(k_topk_tau_from_sample, dim3(gridn(nq)), dim3(256), 0, stream, eerr.as<uint32_t>(), nq, KE, tau_est.as<int>());
    TM_HIP(hipGetLastError());
    eidx.release(); srows.release();
    return topk_pass(ix, (const int16_t *)queries, nq, tau_est.as<int>(), nullptr, nullptr, k, (int32_t *)out_idx, (uint32_t *)out_err, 0, stream, ex, true);
  }
  return topk_pass(ix, (const int16_t *)queries, nq, nullptr, nullptr, nullptr, k, (int32_t *)out_idx, (uint32_t *)out_err, 0, stream, ex);
}

}  // namespace tmx
