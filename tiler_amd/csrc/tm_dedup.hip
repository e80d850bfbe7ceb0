// tm_dedup.hip -- exact tile deduplication + reindexing, A8/A16.
//
// MakeTilesUnique (tilingencoder.pas:4720-4781) sorts tile pointers by pixel content and merges equal runs
// (MergeTiles 4783-4813: sum UseCount into the run's first tile); ReindexTiles (4626-4700) then packs the tiles that
// are Active with UseCount > 0 and sorts them by UseCount descending, content ascending (CompareTileUseCountRev,
// 584-599).  Content order is CompareDWord on the 64 RGB dwords (unsigned) or CompareByte on the 64 palette
// indices (940-948).
//
// GPU form, in the order run_dedup_ex states it:
//   1. GROUP equal rows: every row's representative (the lowest index among the rows equal to it; the reference's choice among
//      byte-identical tiles is implementation defined), the group's summed use count, the list of the distinct rows.
//      The front end is a hash TABLE of 64-bit content hashes (k_dd_*: no sort).  TM_DEDUP_SORT=1 takes the hash SORT instead, a
//      stable radix sort of (hash, index) that makes equal rows neighbours, lowest index first.  Either way a row is compared IN FULL
//      with the row it would be merged with, so a hash that two different rows share cannot merge them: it raises a flag, and the
//      call groups once more the PLAIN way -- a stable merge sort of all row indices with a comparator that reads the rows (exact
//      and slow; TM_DEDUP_PLAIN=1 asks for it outright).  Use counts add up with integer atomics (order free).
//   2. ORDER the distinct rows: by content (a radix sort of 8-byte prefixes, whole rows only where prefixes tie; the comparator merge
//      sort where they tie in long runs or the rows are few), then a stable radix sort on ~UseCount.  A caller that keeps only the
//      first rows of the order (exact_first) has only the rows that can be among them sorted (k_po_*).  The by-index form ranks by row
//      number, which the table's list of distinct rows is in already: nothing is sorted then.
//   3. NUMBER the rows: every row's position is its representative's.
// rocPRIM supplies the sort and scan primitives; the hash, table, comparator, run detection, merge bookkeeping and ranking kernels
// are ours.
#include <cstring>

#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

struct RowLess {
  const uint32_t *rows;
  int dwords;
  int bytewise;  // CompareByte order: compare dwords big-endian
  __device__ int cmp(uint32_t a, uint32_t b) const {
    const uint4 *pa = reinterpret_cast<const uint4 *>(rows + (int64_t)a * dwords);
    const uint4 *pb = reinterpret_cast<const uint4 *>(rows + (int64_t)b * dwords);
    for (int i = 0; i < dwords / 4; i++) {
      const uint4 x = pa[i], y = pb[i];
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (xs[k] != ys[k]) {
          const uint32_t u = bytewise ? __builtin_bswap32(xs[k]) : xs[k];
          const uint32_t v = bytewise ? __builtin_bswap32(ys[k]) : ys[k];
          return u < v ? -1 : 1;
        }
      }
    }
    return 0;
  }
  __device__ bool operator()(const uint32_t &a, const uint32_t &b) const { return cmp(a, b) < 0; }
};

// 64-bit content hash: 16 lanes per row, one uint4 each per 256 bytes; position enters every term, the terms add up
// (`lead`: the row's first dword as lane `sub` 0 read it)
__device__ __forceinline__ unsigned long long row_hash16(const uint32_t *__restrict__ rows, int64_t row, int64_t n, int dwords, int sub, uint32_t &lead) {
  unsigned long long h = 0;
  if (row < n)
    for (int v = sub; v < dwords / 4; v += 16) {
      const uint4 x = *reinterpret_cast<const uint4 *>(rows + row * dwords + v * 4);
      if (v == 0) lead = x.x;
      unsigned long long a = ((unsigned long long)x.y << 32 | x.x) + 0x9E3779B97F4A7C15ull * (unsigned long long)(2 * v + 1);
      unsigned long long b = ((unsigned long long)x.w << 32 | x.z) + 0xC2B2AE3D27D4EB4Full * (unsigned long long)(2 * v + 2);
      a ^= a >> 32; a *= 0xD6E8FEB86659FD93ull; a ^= a >> 32;
      b ^= b >> 29; b *= 0xBF58476D1CE4E5B9ull; b ^= b >> 32;
      h += a * 0x94D049BB133111EBull + b;
    }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) h += __shfl_xor(h, o);
  return h;
}
__global__ __launch_bounds__(256) void k_row_hash(const uint32_t *__restrict__ rows, int64_t n, int dwords, int degrade, int shift,
                                                  unsigned long long *__restrict__ hash) {
  const int sub = threadIdx.x & 15;
  const int64_t stride = (int64_t)gridDim.x * 16;
  for (int64_t r0 = blockIdx.x * (int64_t)16; r0 < n; r0 += stride) {  // a block covers 16 rows per pass
    const int64_t row = r0 + (threadIdx.x >> 4);
    uint32_t lead = 0;
    const unsigned long long h = row_hash16(rows, row, n, dwords, sub, lead);
    if (row < n && sub == 0) hash[row] = degrade ? (h & 3) : (h >> shift);  // degrade: test hook that forces collisions; shift: only the top bits are kept (group_by_hash_sort)
  }
}

// ---- grouping by a hash TABLE (the default front end since round 5; the hash SORT above stays behind TM_DEDUP_SORT) ------------------------
// The sort made equal rows neighbours -- seven radix passes over (hash, index) of the clip's 4.32 M frame tiles, head marks, two scans and the
// run bookkeeping: 0.96 of Reduce's 2.2 ms -- where all that is asked is each row's group: its lowest-index member and the group's use count.
// An open-addressing table of 64-bit hashes (linear probing, at most two thirds full) gives that with one compare-and-swap per probe:
//   k_dd_insert   hashes a row (16 lanes) and claims or finds its hash's slot; the claimant leaves its index as the slot's OWNER, a row that
//                 finds the hash present lowers the slot's MINDUP (atomic minimum).  Both words of a slot lie side by side.
//   k_dd_resolve  representative = min(owner, mindup); a row that is not its own representative adds its use to the representative's count
//   k_dd_verify   ... and is compared with it IN FULL (a hash shared by different rows puts them into one slot, where at least one of them
//                 differs from the slot's lowest row: the flag sends the call down the plain path exactly as the sort's full compare did).
//   k_dd_compact  the representatives in index order (an exclusive scan of the head marks), their own use added, and what the partial order
//                 below wants of them -- use count and leading dword -- as arrays in that order (its three passes gathered both per row).
// Integer atomics only: the groups, their representatives and counts do not depend on who came first.
struct DdSlot { uint32_t owner, mindup; };
// (a workgroup hashes 256 rows sixteen at a time -- 16 lanes per row: coalesced 256-byte reads -- and then every thread takes ONE row to the
// table: with the row's first lane doing its probing the kernel had four atomics in flight per wave and took 607 us, 380 of them waiting)
__global__ __launch_bounds__(256) void k_dd_insert(const uint32_t *__restrict__ rows, int64_t n, int dwords, int degrade, int bytewise,
                                                   unsigned long long *__restrict__ tkey, DdSlot *__restrict__ tslot, uint32_t mask,
                                                   uint32_t *__restrict__ slot_of, uint32_t *__restrict__ lead_of) {
  __shared__ unsigned long long s_h[256];
  __shared__ uint32_t s_lead[256];
  const int sub = threadIdx.x & 15;
  for (int64_t c0 = blockIdx.x * (int64_t)256; c0 < n; c0 += (int64_t)gridDim.x * 256) {
    __syncthreads();  // (the previous chunk's hashes have been taken)
#pragma unroll 4
    for (int p = 0; p < 16; p++) {
      const int lr = p * 16 + (threadIdx.x >> 4);
      uint32_t lead = 0;
      const unsigned long long h = row_hash16(rows, c0 + lr, n, dwords, sub, lead);
      if (sub == 0) { s_h[lr] = h; s_lead[lr] = lead; }
    }
    __syncthreads();
    const int64_t row = c0 + threadIdx.x;
    if (row < n) {
      unsigned long long h = s_h[threadIdx.x];
      if (degrade) h &= 3;
      const unsigned long long key = h ? h : 1ull;  // (0 = an empty slot)
      uint32_t s = (uint32_t)(h ^ (h >> 32)) & mask;
      for (;;) {
        const unsigned long long old = atomicCAS(&tkey[s], 0ull, key);
        if (old == 0ull) { tslot[s].owner = (uint32_t)row; break; }  // (read by the next kernel)
        if (old == key) { atomicMin(&tslot[s].mindup, (uint32_t)row); break; }
        s = (s + 1) & mask;
      }
      slot_of[row] = s;
      const uint32_t lead = s_lead[threadIdx.x];
      lead_of[row] = bytewise ? __builtin_bswap32(lead) : lead;
    }
  }
}
// a thread per row: its representative, head mark, and a duplicate's use added to the representative's count
__global__ __launch_bounds__(256) void k_dd_resolve(int64_t n, const DdSlot *__restrict__ tslot, const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ use_in,
                                                    uint32_t *__restrict__ rep, uint32_t *__restrict__ head, uint32_t *__restrict__ use_rep) {
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
    const DdSlot sl = tslot[slot_of[row]];
    const uint32_t r = min(sl.owner, sl.mindup);
    rep[row] = r;
    head[row] = r == (uint32_t)row ? 1u : 0u;
    if (r != (uint32_t)row) {
      const uint32_t u = use_in ? use_in[row] : 1u;
      if (u) atomicAdd(&use_rep[r], u);
    }
  }
}
// every row that is not its own representative against it in full: a wave looks at 64 rows at once (one coalesced read of their
// representatives) and compares the duplicates among them four at a time, 16 lanes per row (a walk over all rows 16 lanes each was a chain of
// dependent loads: 77 us for a clip without a single duplicate)
__global__ __launch_bounds__(256) void k_dd_verify(const uint32_t *__restrict__ rows, int64_t n, int dwords, const uint32_t *__restrict__ rep, int *__restrict__ collision) {
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4, vecs = dwords / 4;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  bool diff = false;
  for (int64_t base = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nw * 64) {
    const int64_t row = base + lane;
    const uint32_t r = row < n ? rep[row] : (uint32_t)row;
    unsigned long long m = __builtin_amdgcn_ballot_w64(r != (uint32_t)row);
    while (m) {
      int mine = -1;  // this 16-lane group's duplicate of the round: the grp-th of the next four
#pragma unroll
      for (int t = 0; t < 4; t++) {
        if (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          if (t == grp) mine = b;
        }
      }
      const uint32_t rr = (uint32_t)__shfl((int)r, mine >= 0 ? mine : 0);  // (every lane takes part: the source lane may belong to a group that sits this round out)
      if (mine >= 0) {
        const uint4 *pa = reinterpret_cast<const uint4 *>(rows + (int64_t)rr * dwords);
        const uint4 *pb = reinterpret_cast<const uint4 *>(rows + (base + mine) * dwords);
        for (int v = sub; v < vecs; v += 16) {
          const uint4 x = pa[v], y = pb[v];
          diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        }
      }
    }
  }
  if (__builtin_amdgcn_ballot_w64(diff) && lane == 0) *collision = 1;
}
__global__ void k_dd_compact(int64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ head_excl, const uint32_t *__restrict__ use_in,
                             const uint32_t *__restrict__ lead_of, uint32_t *__restrict__ use_rep, uint32_t *__restrict__ uniq, uint32_t *__restrict__ cuse,
                             uint32_t *__restrict__ clead) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (head[i]) {
      const uint32_t j = head_excl[i], u = use_rep[i] + (use_in ? use_in[i] : 1u);
      use_rep[i] = u;
      uniq[j] = (uint32_t)i;
      cuse[j] = u;
      clead[j] = lead_of[i];
    }
}

// runs of equal hash: head flags as k_mark_heads writes them; a non-head row that differs from its predecessor is a collision.  16 lanes per row: a uint4 each, so a 256-byte row is one coalesced read per side (a thread
// walking both rows on its own took 0.43 ms for the bench clip's 1.08 M non-head rows)
__global__ __launch_bounds__(256) void k_mark_heads_hash(const uint32_t *__restrict__ sorted, const unsigned long long *__restrict__ hsorted, int64_t n,
                                                         RowLess less, uint32_t *__restrict__ head, uint32_t *__restrict__ headpos, int *__restrict__ collision) {
  const int sub = threadIdx.x & 15, vecs = less.dwords / 4;
  const int64_t stride = (int64_t)gridDim.x * 16;
  for (int64_t i0 = blockIdx.x * (int64_t)16; i0 < n; i0 += stride) {
    const int64_t i = i0 + (threadIdx.x >> 4);
    bool h = true, diff = false;
    if (i < n) {
      h = (i == 0) || hsorted[i] != hsorted[i - 1];
      if (!h) {
        const uint4 *pa = reinterpret_cast<const uint4 *>(less.rows + (int64_t)sorted[i - 1] * less.dwords);
        const uint4 *pb = reinterpret_cast<const uint4 *>(less.rows + (int64_t)sorted[i] * less.dwords);
        for (int v = sub; v < vecs; v += 16) {
          const uint4 x = pa[v], y = pb[v];
          diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        }
      }
      if (sub == 0) {
        head[i] = h ? 1u : 0u;
        headpos[i] = h ? (uint32_t)i : 0u;
      }
    }
    if (__builtin_amdgcn_ballot_w64(diff) && (threadIdx.x & 63) == 0) *collision = 1;
  }
}

// sort key of a distinct row: its first two dwords in comparison order ride along, so that most comparisons never touch the rows
struct PrefixKey {
  unsigned long long prefix;
  uint32_t row, pad;
};
struct PrefixLess {
  RowLess less;
  __device__ bool operator()(const PrefixKey &a, const PrefixKey &b) const {
    if (a.prefix != b.prefix) return a.prefix < b.prefix;
    return less.cmp(a.row, b.row) < 0;
  }
};
__global__ void k_prefix_keys(const uint32_t *__restrict__ uniq, int64_t nu, RowLess less, PrefixKey *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = uniq[i];
    const uint2 d = *reinterpret_cast<const uint2 *>(less.rows + (int64_t)r * less.dwords);
    const uint32_t d0 = less.bytewise ? __builtin_bswap32(d.x) : d.x, d1 = less.bytewise ? __builtin_bswap32(d.y) : d.y;
    out[i] = PrefixKey{((unsigned long long)d0 << 32) | d1, r, 0u};
  }
}
__global__ void k_prefix_rows(const PrefixKey *__restrict__ keys, int64_t nu, uint32_t *__restrict__ uniq) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) uniq[i] = keys[i].row;
}

// ---- the content sort of MANY distinct rows: by the 8-byte prefix with a radix sort, whole rows only where prefixes tie -----------------
// The comparator merge sort of (prefix, row) keys takes 2 ms for the clip's 4.32 M distinct frame tiles (a dedup without a tile budget: the
// whole order is asked for).  Most keys differ in their prefix: a radix sort of (prefix, row) pairs orders those for good, and what is left
// are short runs of equal prefixes, each put into content order by the thread at its head (insertion sort with the full comparator; a stable
// sort leaves equal prefixes in the order they came in, any order would do).  A run longer than PK_MAX_RUN rows -- flat content: thousands of
// rows may share their first pixels -- sets a flag and the call takes the comparator merge sort as before: the same result by construction
// (one total order).  Only from TM_DEDUP_RADIX_MIN keys on (default 2^20): below that the merge sort's fixed cost is small and a wasted
// radix sort is not (Reindex's 321 k palette-index rows tie in long runs on the bench clip: measured, 0.14 ms lost).
__global__ void k_pk_split(const PrefixKey *__restrict__ pk, int64_t m, unsigned long long *__restrict__ key, uint32_t *__restrict__ row) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) { key[i] = pk[i].prefix; row[i] = pk[i].row; }
}
constexpr int PK_MAX_RUN = 8;
__global__ void k_pk_ties(const unsigned long long *__restrict__ key, uint32_t *__restrict__ row, int64_t m, RowLess less, int *__restrict__ too_long) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = key[i];
    if ((i > 0 && key[i - 1] == k) || i + 1 >= m || key[i + 1] != k) continue;  // not the head of a run of two or more
    int len = 2;
    while (len <= PK_MAX_RUN && i + len < m && key[i + len] == k) len++;
    if (len > PK_MAX_RUN) { *too_long = 1; continue; }
    uint32_t r[PK_MAX_RUN];
#pragma unroll
    for (int j = 0; j < PK_MAX_RUN; j++) r[j] = j < len ? row[i + j] : 0u;
#pragma unroll
    for (int a = 1; a < PK_MAX_RUN; a++) {  // insertion sort (a register array: compile-time indices, the moves by selects)
      if (a < len) {
        const uint32_t x = r[a];
        int pos = a;
#pragma unroll
        for (int b = a - 1; b >= 0; b--)
          if (pos == b + 1 && less.cmp(x, r[b]) < 0) { r[b + 1] = r[b]; pos = b; }
#pragma unroll
        for (int b = 0; b < PK_MAX_RUN; b++) if (b == pos) r[b] = x;
      }
    }
#pragma unroll
    for (int j = 0; j < PK_MAX_RUN; j++) if (j < len) row[i + j] = r[j];
  }
}

// ---- only the first `exact_first` positions of the final order matter (Reduce keeps that many tiles): which distinct rows can be there --
// use counts of the distinct rows, clamped to 1023: a histogram per workgroup in LDS (most rows are used once: one global counter would take
// every row's atomic in turn), flushed with one atomic per occupied bin
// (the flush goes to the histogram copy of the XCD the workgroup runs on -- hist8: [8][bins], folded by k_po_fold --: every workgroup
// holds single-use rows, and 4 096 workgroups of eight XCDs adding to hist[1] passed that one word round for most of the kernel's 70 us)
__device__ __forceinline__ unsigned po_xcc() {
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  return xcc & 7u;
}
__global__ void k_po_fold(const uint32_t *__restrict__ hist8, int bins, uint32_t *__restrict__ hist) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < bins; e += gridDim.x * blockDim.x) {
    uint32_t s = 0;
#pragma unroll
    for (int x = 0; x < 8; x++) s += hist8[x * bins + e];
    hist[e] = s;
  }
}
// (cuse / clead: the distinct rows' use counts and leading dwords in uniq's order where the table front end made them; null: gathered per row)
__global__ __launch_bounds__(256) void k_po_use_hist(const uint32_t *__restrict__ uniq, int64_t nu, const uint32_t *__restrict__ use_rep, const uint32_t *__restrict__ cuse,
                                                     uint32_t *__restrict__ hist8) {
  __shared__ uint32_t s_h[1024];
  for (int e = threadIdx.x; e < 1024; e += 256) s_h[e] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) atomicAdd(&s_h[min(cuse ? cuse[i] : use_rep[uniq[i]], 1023u)], 1u);
  __syncthreads();
  uint32_t *hist = hist8 + po_xcc() * 1024;
  for (int e = threadIdx.x; e < 1024; e += 256) if (s_h[e]) atomicAdd(&hist[e], s_h[e]);
}
__device__ __forceinline__ uint32_t po_lead(const RowLess &less, uint32_t row) {  // the row's leading dword in comparison order
  const uint32_t d = less.rows[(int64_t)row * less.dwords];
  return less.bytewise ? __builtin_bswap32(d) : d;
}
// among the rows used exactly `use_star` times: a histogram of the leading dword's top 12 bits
__global__ __launch_bounds__(256) void k_po_lead_hist(const uint32_t *__restrict__ uniq, int64_t nu, const uint32_t *__restrict__ use_rep, uint32_t use_star, RowLess less,
                                                      const uint32_t *__restrict__ cuse, const uint32_t *__restrict__ clead, uint32_t *__restrict__ hist8) {
  __shared__ uint32_t s_h[4096];
  for (int e = threadIdx.x; e < 4096; e += 256) s_h[e] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    if (cuse) {
      if (cuse[i] == use_star) atomicAdd(&s_h[clead[i] >> 20], 1u);
    } else {
      const uint32_t r = uniq[i];
      if (use_rep[r] == use_star) atomicAdd(&s_h[po_lead(less, r) >> 20], 1u);
    }
  }
  __syncthreads();
  uint32_t *hist = hist8 + po_xcc() * 4096;
  for (int e = threadIdx.x; e < 4096; e += 256) if (s_h[e]) atomicAdd(&hist[e], s_h[e]);
}
// candidate = used more often than use_star, or exactly that often with a leading dword in the first buckets
__global__ void k_po_flags(const uint32_t *__restrict__ uniq, int64_t nu, const uint32_t *__restrict__ use_rep, uint32_t use_star, uint32_t last_bucket, RowLess less,
                           const uint32_t *__restrict__ cuse, const uint32_t *__restrict__ clead, uint32_t *__restrict__ flag) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t u = cuse ? cuse[i] : use_rep[uniq[i]];
    flag[i] = (u > use_star || (u == use_star && ((cuse ? clead[i] : po_lead(less, uniq[i])) >> 20) <= last_bucket)) ? 1u : 0u;
  }
}
// candidates to the front (as sort keys: ~use and the leading dword ride along), the others behind them in the order they come
__global__ void k_po_split(const uint32_t *__restrict__ uniq, int64_t nu, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t ncand,
                           const uint32_t *__restrict__ use_rep, RowLess less, const uint32_t *__restrict__ cuse, const uint32_t *__restrict__ clead,
                           PrefixKey *__restrict__ cand, uint32_t *__restrict__ order_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = uniq[i];
    if (flag[i]) cand[pos[i]] = PrefixKey{((unsigned long long)(~(cuse ? cuse[i] : use_rep[r])) << 32) | (cuse ? clead[i] : po_lead(less, r)), r, 0u};
    else order_out[ncand + (i - pos[i])] = r;
  }
}

__global__ void k_iota(uint32_t *p, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = (uint32_t)i;
}

// head[i] = 1 when sorted[i] starts a run of equal rows; headpos[i] = i at heads else 0 (for a max-scan)
__global__ void k_mark_heads(const uint32_t *__restrict__ sorted, int64_t n, RowLess less, uint32_t *__restrict__ head,
                             uint32_t *__restrict__ headpos) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool h = (i == 0) || less.cmp(sorted[i - 1], sorted[i]) != 0;
    head[i] = h ? 1u : 0u;
    headpos[i] = h ? (uint32_t)i : 0u;
  }
}

// rep[row] = first row of its run; use_rep[rep] += use_in[row]; uniq[rank of run] = rep (content order)
__global__ void k_merge_runs(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ headpos_scanned,
                             const uint32_t *__restrict__ head_excl, const uint32_t *__restrict__ head, int64_t n,
                             const uint32_t *__restrict__ use_in, uint32_t *__restrict__ rep, uint32_t *__restrict__ use_rep,
                             uint32_t *__restrict__ uniq) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x; i0 < n; i0 += stride) {  // (workgroup-uniform bound: every lane reaches the ballot)
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < n;
    const uint32_t hp = in ? headpos_scanned[i] : 0xffffffffu;
    const uint32_t row = in ? sorted[i] : 0u, r = in ? sorted[hp] : 0u;
    if (in) {
      rep[row] = r;
      if (head[i]) uniq[head_excl[i]] = r;
    }
    if (use_in) {
      // the same with counts to add up: a segmented sum over the lanes of a run (the hp of a run's rows are equal and the runs are
      // neighbours), one atomic per run and wave
      uint32_t v = in ? use_in[row] : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t ov = (uint32_t)__shfl_down((int)v, o);
        const uint32_t ohp = (uint32_t)__shfl_down((int)hp, o);
        if (lane + o < 64 && ohp == hp) v += ov;
      }
      const uint32_t prev = (uint32_t)__shfl_up((int)hp, 1);
      if (in && (lane == 0 || hp != prev) && v) atomicAdd(&use_rep[r], v);
    } else {
      // rows of a run are neighbours here, and a run's last row knows where the run began: its length is a plain store (3.2 M atomics on
      // words scattered over 17 MB, passed between the XCDs' L2s, were most of this kernel)
      if (in && (i == n - 1 || head[i + 1])) use_rep[r] = (uint32_t)(i - hp + 1);
    }
  }
}

__global__ void k_rank_keys(const uint32_t *__restrict__ uniq, int64_t nu, const uint32_t *__restrict__ use_rep, int by_index,
                            uint32_t *__restrict__ key, unsigned long long *__restrict__ live_count) {
  unsigned long long local = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t u = use_rep[uniq[i]];
    key[i] = by_index ? uniq[i] : ~u;  // ascending ~use == descending use; zero-use rows (~0) sink to the end
    local += (u > 0 || by_index) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(live_count, local);
}

__global__ void k_scatter_pos(const uint32_t *__restrict__ order, int64_t nlive, const uint32_t *__restrict__ use_rep,
                              int32_t *__restrict__ pos, uint32_t *__restrict__ use_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nlive; i += (int64_t)gridDim.x * blockDim.x) {
    pos[order[i]] = (int32_t)i;
    use_out[i] = use_rep[order[i]];
  }
}

__global__ void k_remap(const uint32_t *__restrict__ rep, const int32_t *__restrict__ pos, int64_t n, int32_t *__restrict__ remap) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) remap[i] = pos[rep[i]];
}

// ---- the host side: run_dedup_ex at the end of the file states the order of the phases below -------------------------------------------
namespace {

// one call: its arguments, its n x 4 byte scratch arrays, and what the grouping found
struct Dedup {
  const uint32_t *rows;
  int64_t n;
  int row_bytes;
  const uint32_t *use_in;
  int by_index;
  hipStream_t stream;
  RowLess less;
  DevBuf idx, sorted, head, headpos, hps, head_excl;  // the sorting front ends: 0..n-1, the sorted indices, run heads and their two scans
  DevBuf rep, use_rep, uniq;                          // what every front end leaves: row -> representative, use count at a representative, the distinct rows
  DevBuf cuse, clead;                                 // the table's extra: use count and leading dword of the distinct rows, in uniq's order
  DevBuf key, key2, ord2, pos;                        // the ranking sort's keys, the final order, row -> position
  DevBuf tmp, cnt, hflag;                             // rocPRIM's temporary, the live count, "two different rows shared a hash"
  int64_t nu = 0;                                     // distinct rows
  int alloc(bool table) {
    for (DevBuf *b : {&idx, &sorted, &head, &headpos, &head_excl, &hps, &rep, &use_rep, &uniq, &key, &key2, &ord2, &pos}) TM_TRY(b->alloc(n * 4));
    if (table) { TM_TRY(cuse.alloc(n * 4)); TM_TRY(clead.alloc(n * 4)); }
    TM_TRY(cnt.alloc(16));
    return hflag.alloc(4);
  }
};
enum Front { FRONT_TABLE, FRONT_HASH_SORT, FRONT_PLAIN };

// the one read-back of a grouping: the number of distinct rows (= head_excl[n-1] + head[n-1]) and the collision flag, one round trip for all
int read_groups(Dedup &d, bool *collision) {
  uint32_t last_excl = 0, last_head = 0;
  int flag = 0;
  HostRead hr(d.stream);
  TM_TRY(hr.get(&last_excl, d.head_excl.as<uint32_t>() + (d.n - 1), 4));
  TM_TRY(hr.get(&last_head, d.head.as<uint32_t>() + (d.n - 1), 4));
  TM_TRY(hr.get(&flag, d.hflag.p, 4));
  TM_TRY(hr.wait());
  d.nu = (int64_t)last_excl + last_head;
  *collision = flag != 0;
  return TM_OK;
}

// The three grouping front ends share one contract: rep, use_rep, uniq and nu are filled (uniq in index order after the table, in hash order
// after the hash sort, in content order after the plain sort); *collision says that two different rows shared a hash: what was filled is then not to be used.

// the table (see k_dd_insert): no sort; cuse and clead come with it.
// The table leaves uniq in ascending row order: a group's representative is its lowest row (k_dd_resolve: min(owner, mindup)), head marks
// exactly the representatives, and k_dd_compact writes uniq[head_excl[i]] = i with head_excl the exclusive scan of the marks.
int group_by_table(Dedup &d, bool *collision) {
  const int64_t n = d.n;
  int64_t slots = 1024;
  while (slots * 2 < n * 3) slots *= 2;
  DevBuf tkey, tslot, slot_of, lead_of;
  TM_TRY(tkey.alloc((size_t)slots * 8)); TM_TRY(tslot.alloc((size_t)slots * sizeof(DdSlot))); TM_TRY(slot_of.alloc(n * 4)); TM_TRY(lead_of.alloc(n * 4));
  TM_HIP(hipMemsetAsync(tkey.p, 0, (size_t)slots * 8, d.stream));
  TM_HIP(hipMemsetAsync(tslot.p, 0xff, (size_t)slots * sizeof(DdSlot), d.stream));
  TM_HIP(hipMemsetAsync(d.use_rep.p, 0, n * 4, d.stream));
  hipLaunchKernelGGL(k_dd_insert, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 256 * 8)), dim3(256), 0, d.stream, d.rows, n, d.row_bytes / 4,
                     knobs().dedup_degrade_hash ? 1 : 0, d.less.bytewise, tkey.as<unsigned long long>(), tslot.as<DdSlot>(), (uint32_t)(slots - 1), slot_of.as<uint32_t>(),
                     lead_of.as<uint32_t>());
  hipLaunchKernelGGL(k_dd_resolve, dim3(gridn(n)), dim3(256), 0, d.stream, n, tslot.as<DdSlot>(), slot_of.as<uint32_t>(), d.use_in, d.rep.as<uint32_t>(),
                     d.head.as<uint32_t>(), d.use_rep.as<uint32_t>());
  hipLaunchKernelGGL(k_dd_verify, dim3(gridn(n)), dim3(256), 0, d.stream, d.rows, n, d.row_bytes / 4, d.rep.as<uint32_t>(), d.hflag.as<int>());
  TM_TRY(with_temp(d.tmp, "dedup: scan of the table's head marks", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, d.head.as<uint32_t>(), d.head_excl.as<uint32_t>(), 0u, (size_t)n, rocprim::plus<uint32_t>(), d.stream);
  }));
  hipLaunchKernelGGL(k_dd_compact, dim3(gridn(n)), dim3(256), 0, d.stream, n, d.head.as<uint32_t>(), d.head_excl.as<uint32_t>(), d.use_in,
                     lead_of.as<uint32_t>(), d.use_rep.as<uint32_t>(), d.uniq.as<uint32_t>(), d.cuse.as<uint32_t>(), d.clead.as<uint32_t>());
  TM_HIP(hipGetLastError());
  return read_groups(d, collision);  // (a collision: about once in 2^20 calls of the bench clip's size)
}

// what the two sorting front ends share: `sorted` holds runs of equal rows, lowest index first, head / headpos mark where they begin
int merge_runs(Dedup &d, bool *collision) {
  const int64_t n = d.n;
  TM_TRY(with_temp(d.tmp, "dedup: scan of the run heads' positions", [&](void *t, size_t &b) {
    return rocprim::inclusive_scan(t, b, d.headpos.as<uint32_t>(), d.hps.as<uint32_t>(), (size_t)n, rocprim::maximum<uint32_t>(), d.stream);
  }));
  TM_TRY(with_temp(d.tmp, "dedup: scan of the run heads", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, d.head.as<uint32_t>(), d.head_excl.as<uint32_t>(), 0u, (size_t)n, rocprim::plus<uint32_t>(), d.stream);
  }));
  TM_HIP(hipMemsetAsync(d.use_rep.p, 0, n * 4, d.stream));
  hipLaunchKernelGGL(k_merge_runs, dim3(gridn(n)), dim3(256), 0, d.stream, d.sorted.as<uint32_t>(), d.hps.as<uint32_t>(), d.head_excl.as<uint32_t>(),
                     d.head.as<uint32_t>(), n, d.use_in, d.rep.as<uint32_t>(), d.use_rep.as<uint32_t>(), d.uniq.as<uint32_t>());
  TM_HIP(hipGetLastError());
  return read_groups(d, collision);
}

// the hash sort (TM_DEDUP_SORT): equal rows become neighbours by a stable radix sort of (hash, index)
int group_by_hash_sort(Dedup &d, bool *collision) {
  const int64_t n = d.n;
  DevBuf hkey, hkey2;
  TM_TRY(hkey.alloc(n * 8)); TM_TRY(hkey2.alloc(n * 8));
  // The sort only has to bring equal rows together, so the hash keeps only as many of its top bits (whole 8-bit passes of the sort) as hold
  // the chance of two different rows among n sharing them below 2^-12 -- 48 for Reindex's 321 k rows, 56 for the bench clip's 4.32 M frame tiles
  // (seven passes instead of eight).  Rows that share them and differ are caught by the full compare like any collision.
  // The kept bits are moved DOWN and sorted as bits [0, hbits): a range that ends at bit 64 without starting at 0 sends rocPRIM's
  // merge-sort path (up to ~1 M keys) through a mask built with a shift by 64 -- it then orders by the wrong bits and its merge reads out
  // of bounds (found the hard way: a memory access fault on the GPU box).
  const int degrade = knobs().dedup_degrade_hash ? 1 : 0;
  const int hbits = degrade ? 64 : std::min(64, ((int)std::ceil(2.0 * std::log2((double)std::max<int64_t>(n, 2)) + 11.0) + 7) / 8 * 8);  // n^2 / 2^(bits + 1) <= 2^-12
  const dim3 grid16((unsigned)std::min<int64_t>((n + 15) / 16, 256 * 32));  // 16 rows per workgroup and pass
  hipLaunchKernelGGL(k_row_hash, grid16, dim3(256), 0, d.stream, d.rows, n, d.row_bytes / 4, degrade, 64 - hbits, hkey.as<unsigned long long>());
  TM_TRY(with_temp(d.tmp, "dedup: radix sort of the row hashes", [&](void *t, size_t &b) {
    return rocprim::radix_sort_pairs(t, b, hkey.as<unsigned long long>(), hkey2.as<unsigned long long>(), d.idx.as<uint32_t>(), d.sorted.as<uint32_t>(), (size_t)n, 0, hbits, d.stream);
  }));
  hipLaunchKernelGGL(k_mark_heads_hash, grid16, dim3(256), 0, d.stream, d.sorted.as<uint32_t>(), hkey2.as<unsigned long long>(), n, d.less, d.head.as<uint32_t>(),
                     d.headpos.as<uint32_t>(), d.hflag.as<int>());
  return merge_runs(d, collision);  // (a collision: about once in 2^12 calls by the choice of bits above)
}

// the plain way: a stable merge sort of all row indices with a comparator that reads the rows.  No hash, nothing to collide.
int group_plain(Dedup &d, bool *collision) {
  TM_TRY(with_temp(d.tmp, "dedup: merge sort of the rows", [&](void *t, size_t &b) {
    return rocprim::merge_sort(t, b, d.idx.as<uint32_t>(), d.sorted.as<uint32_t>(), (size_t)d.n, d.less, d.stream);
  }));
  hipLaunchKernelGGL(k_mark_heads, dim3(gridn(d.n)), dim3(256), 0, d.stream, d.sorted.as<uint32_t>(), d.n, d.less, d.head.as<uint32_t>(), d.headpos.as<uint32_t>());
  bool stale;  // (the flag that comes back with the count is the front end's that sent the call here)
  TM_TRY(merge_runs(d, &stale));
  *collision = false;
  return TM_OK;
}

// m keys (prefix, row) into content order; the rows of that order to out_rows
int sort_prefix_keys(DevBuf &pk, int64_t m, const RowLess &less, uint32_t *out_rows, DevBuf &tmp, hipStream_t stream) {
  if (m <= 0) return TM_OK;
  if (m >= knobs().dedup_radix_min) {
    DevBuf k1, k2, r1, r2, flag;
    TM_TRY(k1.alloc((size_t)m * 8)); TM_TRY(k2.alloc((size_t)m * 8)); TM_TRY(r1.alloc((size_t)m * 4)); TM_TRY(r2.alloc((size_t)m * 4)); TM_TRY(flag.alloc(4));
    TM_HIP(hipMemsetAsync(flag.p, 0, 4, stream));
    hipLaunchKernelGGL(k_pk_split, dim3(gridn(m)), dim3(256), 0, stream, pk.as<PrefixKey>(), m, k1.as<unsigned long long>(), r1.as<uint32_t>());
    TM_TRY(with_temp(tmp, "dedup: radix sort of the row prefixes", [&](void *t, size_t &b) {
      return rocprim::radix_sort_pairs(t, b, k1.as<unsigned long long>(), k2.as<unsigned long long>(), r1.as<uint32_t>(), r2.as<uint32_t>(), (size_t)m, 0, 64, stream);
    }));
    hipLaunchKernelGGL(k_pk_ties, dim3(gridn(m)), dim3(256), 0, stream, k2.as<unsigned long long>(), r2.as<uint32_t>(), m, less, flag.as<int>());
    TM_HIP(hipMemcpyAsync(out_rows, r2.p, (size_t)m * 4, hipMemcpyDeviceToDevice, stream));
    TM_HIP(hipGetLastError());
    int too_long = 0;
    {
      HostRead hr(stream);
      TM_TRY(hr.get(&too_long, flag.p, 4));
      TM_TRY(hr.wait());
    }
    if (!too_long) return TM_OK;  // else a run of equal prefixes longer than k_pk_ties sorts: the comparator merge sort, the same order by construction
  }
  DevBuf pk2;
  TM_TRY(pk2.alloc((size_t)m * sizeof(PrefixKey)));
  const PrefixLess pless{less};
  TM_TRY(with_temp(tmp, "dedup: merge sort of the row prefixes", [&](void *t, size_t &b) {
    return rocprim::merge_sort(t, b, pk.as<PrefixKey>(), pk2.as<PrefixKey>(), (size_t)m, pless, stream);
  }));
  hipLaunchKernelGGL(k_prefix_rows, dim3(gridn(m)), dim3(256), 0, stream, pk2.as<PrefixKey>(), m, out_rows);
  TM_HIP(hipGetLastError());
  return TM_OK;  // pk2 goes back to the pool here; later users are ordered behind these kernels on the same stream (as with `tmp`)
}

// Only the first exact_first positions have to be right.  The order is use count descending, content ascending: a histogram of the use
// counts finds the count u* of position exact_first, a histogram of the leading dword's top bits among the rows used u* times finds
// the bucket that position falls into; rows used more often, or u* times with a leading dword up to that bucket, are the only ones
// that can come before it.  They alone are sorted (the comparator reads the rows where the keys tie); the others follow as they come.
// 3.24 M distinct rows for a budget of 321 k on the bench clip: a merge sort of a tenth of them instead of all.
// *done: ord2 holds the final order of all nu distinct rows.  Not done -- nothing written -- when the cut falls inside the clamped bin
// (1023 uses and more: the histogram cannot tell those rows apart) or no row is used at all: the caller takes the full sort.
int order_candidates(Dedup &d, bool from_table, int64_t exact_first, bool *done) {
  const int64_t nu = d.nu;
  *done = false;
  DevBuf h1, h2, h8, flag, fpos, pk;
  TM_TRY(h1.alloc(1024 * 4)); TM_TRY(h2.alloc(4096 * 4)); TM_TRY(h8.alloc(8 * 4096 * 4));
  const int po_grid = std::min(gridn(nu), 1024);  // (every workgroup flushes its bins: fewer workgroups, fewer atomics on the popular ones)
  const uint32_t *uniq = d.uniq.as<uint32_t>(), *use_rep = d.use_rep.as<uint32_t>();
  const uint32_t *cu = from_table ? d.cuse.as<uint32_t>() : nullptr, *cl = from_table ? d.clead.as<uint32_t>() : nullptr;  // (null: the kernels gather both per row)
  TM_HIP(hipMemsetAsync(h8.p, 0, 8 * 1024 * 4, d.stream));
  hipLaunchKernelGGL(k_po_use_hist, dim3(po_grid), dim3(256), 0, d.stream, uniq, nu, use_rep, cu, h8.as<uint32_t>());
  hipLaunchKernelGGL(k_po_fold, dim3(4), dim3(256), 0, d.stream, h8.as<uint32_t>(), 1024, h1.as<uint32_t>());
  TM_HIP(hipGetLastError());
  std::vector<uint32_t> hh1(1024), hh2(4096);
  {
    HostRead hr(d.stream);
    TM_TRY(hr.get(hh1.data(), h1.p, 1024 * 4));
    TM_TRY(hr.wait());
  }
  int64_t above = 0;  // rows used more often than u*
  int ustar = -1;
  for (int u = 1023; u >= 1; u--) {
    if (above + hh1[(size_t)u] >= exact_first) { ustar = u; break; }
    above += hh1[(size_t)u];
  }
  if (ustar < 1 || ustar >= 1023) return TM_OK;
  TM_HIP(hipMemsetAsync(h8.p, 0, 8 * 4096 * 4, d.stream));
  hipLaunchKernelGGL(k_po_lead_hist, dim3(po_grid), dim3(256), 0, d.stream, uniq, nu, use_rep, (uint32_t)ustar, d.less, cu, cl, h8.as<uint32_t>());
  hipLaunchKernelGGL(k_po_fold, dim3(16), dim3(256), 0, d.stream, h8.as<uint32_t>(), 4096, h2.as<uint32_t>());
  TM_HIP(hipGetLastError());
  {
    HostRead hr(d.stream);
    TM_TRY(hr.get(hh2.data(), h2.p, 4096 * 4));
    TM_TRY(hr.wait());
  }
  int64_t ncand = above;  // ... and those used u* times up to the bucket b*
  int bstar = 4095;
  for (int b = 0; b < 4096; b++) {
    ncand += hh2[(size_t)b];
    if (ncand >= exact_first) { bstar = b; break; }
  }
  TM_TRY(flag.alloc((size_t)nu * 4)); TM_TRY(fpos.alloc((size_t)nu * 4));
  hipLaunchKernelGGL(k_po_flags, dim3(gridn(nu)), dim3(256), 0, d.stream, uniq, nu, use_rep, (uint32_t)ustar, (uint32_t)bstar, d.less, cu, cl, flag.as<uint32_t>());
  TM_TRY(with_temp(d.tmp, "dedup: scan of the candidate flags", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, flag.as<uint32_t>(), fpos.as<uint32_t>(), 0u, (size_t)nu, rocprim::plus<uint32_t>(), d.stream);
  }));
  TM_TRY(pk.alloc((size_t)ncand * sizeof(PrefixKey)));
  hipLaunchKernelGGL(k_po_split, dim3(gridn(nu)), dim3(256), 0, d.stream, uniq, nu, flag.as<uint32_t>(), fpos.as<uint32_t>(), ncand, use_rep, d.less, cu, cl,
                     pk.as<PrefixKey>(), d.ord2.as<uint32_t>());
  TM_HIP(hipGetLastError());
  TM_TRY(sort_prefix_keys(pk, ncand, d.less, d.ord2.as<uint32_t>(), d.tmp, d.stream));
  *done = true;
  return TM_OK;
}

// the distinct rows, in hash or index order -> content order (what the stable ranking sort relies on)
int content_order(Dedup &d) {
  DevBuf pk;
  TM_TRY(pk.alloc((size_t)d.nu * sizeof(PrefixKey)));
  hipLaunchKernelGGL(k_prefix_keys, dim3(gridn(d.nu)), dim3(256), 0, d.stream, d.uniq.as<uint32_t>(), d.nu, d.less, pk.as<PrefixKey>());
  TM_HIP(hipGetLastError());
  return sort_prefix_keys(pk, d.nu, d.less, d.uniq.as<uint32_t>(), d.tmp, d.stream);
}

// uniq -> ord2 by a stable radix sort: on ~UseCount (content order stays within a count; *live = the rows in use, they come first), or on the
// row number (by_index: every distinct row is live)
int rank(Dedup &d, unsigned long long *live) {
  TM_HIP(hipMemsetAsync(d.cnt.p, 0, 16, d.stream));
  hipLaunchKernelGGL(k_rank_keys, dim3(gridn(d.nu)), dim3(256), 0, d.stream, d.uniq.as<uint32_t>(), d.nu, d.use_rep.as<uint32_t>(), d.by_index, d.key.as<uint32_t>(),
                     d.cnt.as<unsigned long long>());
  TM_TRY(with_temp(d.tmp, "dedup: radix sort of the ranking keys", [&](void *t, size_t &b) {
    return rocprim::radix_sort_pairs(t, b, d.key.as<uint32_t>(), d.key2.as<uint32_t>(), d.uniq.as<uint32_t>(), d.ord2.as<uint32_t>(), (size_t)d.nu, 0, 32, d.stream);
  }));
  TM_HIP(hipGetLastError());
  HostRead hr(d.stream);
  TM_TRY(hr.get(live, d.cnt.p, 8));
  return hr.wait();
}

// the final order (ord2, or uniq where it already is that order) -> the caller's arrays: a live row's position, its use count, and every
// row's position through its representative
int finish(Dedup &d, const DevBuf &final_order, int64_t live, void *remap, void *order, void *use_out) {
  TM_HIP(hipMemsetAsync(d.pos.p, 0xff, d.n * 4, d.stream));
  hipLaunchKernelGGL(k_scatter_pos, dim3(gridn(live)), dim3(256), 0, d.stream, final_order.as<uint32_t>(), live, d.use_rep.as<uint32_t>(), d.pos.as<int32_t>(), (uint32_t *)use_out);
  hipLaunchKernelGGL(k_remap, dim3(gridn(d.n)), dim3(256), 0, d.stream, d.rep.as<uint32_t>(), d.pos.as<int32_t>(), d.n, (int32_t *)remap);
  TM_HIP(hipMemcpyAsync(order, final_order.p, (size_t)live * 4, hipMemcpyDeviceToDevice, d.stream));
  TM_HIP(hipGetLastError());
  TM_HIP(host_sync(d.stream));  // the scratch DevBufs die with the caller's frame
  return TM_OK;
}

}  // namespace

// by_index = 0: the reference's ReindexTiles order (use desc, content asc), zero-use rows dropped.
// by_index = 1: representatives in ascending original index (used to search only distinct database rows; any
//               row_bytes multiple of 16, content compared as dwords).
// exact_first > 0 (only with by_index = 0 and no use_in): the caller keeps the first exact_first rows of the order and nothing of the rest but
//               their number -- those positions are exact, the ones behind them hold the remaining rows in no particular order.
int run_dedup_ex(const void *rows, int64_t n, int row_bytes, const void *use_in, void *remap, void *order, void *use_out,
                 int64_t *host_n_unique, int by_index, hipStream_t stream, int64_t exact_first) {
  TM_TRY(require_device());
  TM_CHECK(by_index ? (row_bytes > 0 && row_bytes % 16 == 0) : (row_bytes == 256 || row_bytes == 64), TM_E_INVAL,
           "dedup: row_bytes must be 256 (RGB) or 64 (palette indices)");
  TM_CHECK(n >= 0 && n < (int64_t)1 << 31, TM_E_INVAL, "dedup: row count out of range");
  if (host_n_unique) *host_n_unique = 0;
  if (n == 0) return TM_OK;
  Dedup d{(const uint32_t *)rows, n, row_bytes, (const uint32_t *)use_in, by_index, stream,
          RowLess{(const uint32_t *)rows, row_bytes / 4, (!by_index && row_bytes == 64) ? 1 : 0}};
  // 1. group: the front end the knobs name; two different rows under one hash send the call to the plain one
  Front front = knobs().dedup_plain ? FRONT_PLAIN : knobs().dedup_sort ? FRONT_HASH_SORT : FRONT_TABLE;
  TM_TRY(d.alloc(front == FRONT_TABLE));
  hipLaunchKernelGGL(k_iota, dim3(gridn(n)), dim3(256), 0, stream, d.idx.as<uint32_t>(), n);
  TM_HIP(hipMemsetAsync(d.hflag.p, 0, 4, stream));
  bool collision = false;
  TM_TRY(front == FRONT_TABLE ? group_by_table(d, &collision) : front == FRONT_HASH_SORT ? group_by_hash_sort(d, &collision) : group_plain(d, &collision));
  if (collision) {
    front = FRONT_PLAIN;
    TM_TRY(group_plain(d, &collision));
  }
  // 2. order.  The partial order wants groups that are not in content order yet, plain use counts and a cut inside the distinct rows.  Else
  //    the content order (the plain grouping left it; the by-index form ranks by row number alone: any order of the distinct rows will do),
  //    then the ranking sort.  By index from the table there is nothing to rank: uniq is in ascending row order already (group_by_table's
  //    contract) and every distinct row is live; the sorting front ends leave uniq in hash or content order and keep the sort.
  bool ordered = false;
  const bool uniq_is_final = front == FRONT_TABLE && by_index;
  unsigned long long live = 0;
  if (front != FRONT_PLAIN && !by_index && !use_in && exact_first > 0 && exact_first < d.nu && !knobs().dedup_full_order)
    TM_TRY(order_candidates(d, front == FRONT_TABLE, exact_first, &ordered));
  if (ordered || uniq_is_final) live = (unsigned long long)d.nu;
  else {
    if (front != FRONT_PLAIN && !by_index) TM_TRY(content_order(d));
    TM_TRY(rank(d, &live));
  }
  // 3. number
  TM_TRY(finish(d, uniq_is_final ? d.uniq : d.ord2, (int64_t)live, remap, order, use_out));
  if (host_n_unique) *host_n_unique = (int64_t)live;
  return TM_OK;
}

int run_dedup(const void *rows, int64_t n, int row_bytes, const void *use_in, void *remap, void *order, void *use_out,
              int64_t *host_n_unique, hipStream_t stream, int64_t exact_first) {
  return run_dedup_ex(rows, n, row_bytes, use_in, remap, order, use_out, host_n_unique, 0, stream, exact_first);
}

}  // namespace tmx
