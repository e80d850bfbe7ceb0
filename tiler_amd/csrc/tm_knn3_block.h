// tm_knn3_block.h -- the device pieces of the third scan shape (tm_knn3.h): what a wave does with one (tile, sub-tile) block and around it.
// The wave helpers, the bound rules (k3_bound_of, its inverse and the refresh, k3_within), the seed window and the box lower bound the
// seed and lists kernels must agree on, the chain, the tile loads, the looks, the mask of minima and the two epilogues.  The kernels made of
// them: tm_knn3_seed.h, tm_knn3_consume.h, tm_knn3_lists.hip.
#pragma once
#include "tm_knn3.h"

namespace tmx {

// a diagnostic build's phase stamps (TM_KNN3_STAMPS): a kernel that uses them declares st_acc[] and st_last
#if TM_KNN3_STAMPS
#define K3_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_last; st_last = t_; } while (0)
#else
#define K3_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ unsigned k3_wave_umax(unsigned x) {  // max over lanes 0..31 (every lane of a row of 16 ends with its row's)
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, true));
  x = max(x, (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xf, 0xf, true));
  return max((unsigned)__builtin_amdgcn_readlane((int)x, 0), (unsigned)__builtin_amdgcn_readlane((int)x, 16));
}

// a fresh look at an LDS word other waves update (relaxed workgroup-scope load: a plain ds_read_b32 the compiler may not cache)
__device__ __forceinline__ unsigned k3_peek(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// largest r with r * r <= x (x < 2^31): the hardware's approximate root (within one unit of the last place, i.e. well within one of
// the integer root here) set right by one step either way
__device__ __forceinline__ unsigned k3_isqrt(unsigned x) {
  unsigned r = (unsigned)__builtin_amdgcn_sqrtf((float)x);
  r += ((r + 1u) * (r + 1u) <= x) ? 1u : 0u;
  r -= (r * r > x) ? 1u : 0u;
  return r;
}

// the bound a sub-tile's tiles are judged against, from its largest best mx = d'' + 1 (an SSD bound): an upper bound of its square root
constexpr unsigned K3_BOUND_SLACK = 3u;  // what the bound stands above the hardware's approximate root of mx
__device__ __forceinline__ unsigned k3_bound_of(unsigned mx) { return mx == ~0u ? K3_LB_MAX : min(K3_LB_MAX, (unsigned)__builtin_amdgcn_sqrtf((float)mx) + K3_BOUND_SLACK); }
// ... and its inverse, for the epilogues: no best below this can have made the published bound `sm` (K3_LB_MAX stands for "some query has no
// best yet"; 0 = the caller asks for a refresh on every improvement)
// (a macro: as an inline function it moved k_knn_consume's scalar compares around the epilogue's atomic)
#define K3_BOUND_FLOOR(sm) ((sm) > K3_BOUND_SLACK ? ((sm) - K3_BOUND_SLACK) * ((sm) - K3_BOUND_SLACK) : 0u)
// A sub-tile's bound made anew from its bests (bests only go down: a late writer is only loose).  `best_hi` = the high word of this lane's
// query's best (lane & 31 = the query), `smax` = the sub-tile's bound in LDS; every lane of the wave runs it, `lane` is the caller's.
// (A macro for the same reason: the function swapped the operands of a scalar AND in k_knn_consume's block loop.)
#define K3_REFRESH_BOUND(smax, best_hi)                                   \
  do {                                                                    \
    const unsigned mx = k3_wave_umax(k3_peek(best_hi)); /* = largest d'' + 1 */ \
    if (mx != ~0u && lane == 0) atomicMin(smax, k3_bound_of(mx));         \
  } while (0)

// Can a value `look` (a lower bound of some d'' + 1) still matter against `bound` (a best d'' + 1, or a threshold + 1)?  INCLUSIVE: a row
// that only ties always passes, which the tie rule of DESIGN 27 rests on at every site.  With TD the looks are exact and the compare is the
// plain one; without, a first look can lie one below the truth -- at -1 where a query meets its own row and both norms are odd (d'' + 1 =
// 0) -- so the compare is a signed one against the bound cut to 2^31 - 1: a value that wraps goes the safe way (in).
template <bool TD>
__device__ __forceinline__ bool k3_within(unsigned look, unsigned bound) { return TD ? look <= bound : (int)look <= (int)min(bound, 0x7FFFFFFFu); }

// The seed window of a query group whose first sub-tile's home tile is `home`: the K3_SEEDS database tiles around it on the curve, clamped
// to the database.  k_knn_seed scores exactly these tiles and k_knn_lists leaves exactly these out of the lists: a tile the two disagreed
// on would be scored by nobody, and the search would stop being exact.
struct K3SeedWindow { int first, count; };  // tiles [first, first + count)
__device__ __forceinline__ K3SeedWindow k3_seed_window(int home, int64_t n_ttiles) {
  const int first = (int)max((int64_t)0, min((int64_t)home - (K3_SEEDS / 2 - 1), n_ttiles - K3_SEEDS));
  return {first, (int)min((int64_t)K3_SEEDS, n_ttiles - first)};
}

// The box lower bound of k_knn_lists: the squared gap between two boxes, dimension by dimension (halved first: the sum stays below 2^31),
// and the 16-bit form a list entry carries, 2 * floor(sqrt(sum)) <= the true distance, capped below K3_LB_NONE.
__device__ __forceinline__ unsigned k3_box_gap_sq(int tlo, int thi, int qlo, int qhi) {
  const int gap = max(0, max(tlo - qhi, qlo - thi)) >> 1;
  return (unsigned)(gap * gap);
}
__device__ __forceinline__ unsigned k3_box_root(unsigned gap_sq_sum) { return 2u * k3_isqrt(gap_sq_sum); }
__device__ __forceinline__ unsigned k3_box_bound16(unsigned gap_sq_sum) { return min(K3_LB_MAX, k3_box_root(gap_sq_sum)); }

// One block's chain: X over the digit products on one accumulator shifted between the phases; the rows' own term `cin` rides in on the
// second shift.  With TD (database digits of 2 (t - c)) cin = |t-c|^2 and the chain ends in 2 X + |t-c|^2 = d'' - qn; without, cin =
// |t-c|^2 >> 1 and it ends in Y = X + (|t-c|^2 >> 1): d'' - qn = 2 Y + (|t-c|^2 & 1), which the nearest-neighbour epilogue never makes per row
// (the minimum and its row follow from min(Y) and the parities: k3_epilogue; the collection mode makes them for the blocks that can matter).  `q` = the sub-tile's B operands in LDS at
// this lane's 16 bytes (chunk stride 1024).
// `tm` / `qm` (wave-uniform): bit kc set = high-digit chunk kc of the tile / of the sub-tile holds a non-zero digit.  A product with an
// all-zero chunk adds nothing and is skipped, its LDS read with it: the columns are packed widest first (make_plan_scaled), so a tile of
// smooth content has its high digits in the first chunk or two only.  (Measured against straight-line chains for the common mask shapes,
// picked by one or two uniform tests: a predicate per product is as fast or faster on both bench clips -- the other waves of the SIMD
// fill the matrix pipe while a product waits for its LDS read -- skips more, and needs no spilled register.)
template <int HT, int HQ, bool TD>
__device__ __forceinline__ v16i k3_chain(const v4i (&T)[6 + HT], const v16i &cin, const uint8_t *q, unsigned tm, unsigned qm) {
  constexpr int HM = HT < HQ ? HT : HQ;
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v16i acc = cin;  // a single phase: the rows' term is the chain's starting value
  if constexpr (HT + HQ > 0) {
    // No register is zeroed for a block: whatever the masks say, the chain's FIRST product is one that always runs, with the constant 0 as
    // its C operand.  That is T_H0 . Q_H0 where any T_H . Q_H product runs, and the first product of the middle phase otherwise (T_H0 . Q_L0;
    // T_L0 . Q_H0 for a database without high digits) -- a chunk its mask calls empty is all zeros (k3_load_tile_masked fills a skipped
    // chunk with them), so the product then adds nothing: a matrix instruction instead of sixteen moves.
    constexpr int FA = HT > 0 ? 6 : 0;  // the middle phase's first product: chunk FA of the tile, chunk FQ of the sub-tile
    constexpr int FQ = HT > 0 ? 0 : 6;
    bool hh = false;
    if constexpr (HM > 0) hh = (tm & qm) != 0;
    if (hh) {
      if constexpr (HM > 0) {
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], *reinterpret_cast<const v4i *>(q + 6 * 1024), zero, 0, 0, 0);                // T_H . Q_H
#pragma unroll
        for (int kc = 1; kc < HM; kc++)
          if (((tm & qm) >> kc) & 1u)
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6 + kc], *reinterpret_cast<const v4i *>(q + (6 + kc) * 1024), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = (int)((unsigned)acc[r] << 8);
      }
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[FA], *reinterpret_cast<const v4i *>(q + FQ * 1024), acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[FA], *reinterpret_cast<const v4i *>(q + FQ * 1024), zero, 0, 0, 0);
    }
#pragma unroll
    for (int kc = (HT > 0 ? 0 : 1); kc < HQ; kc++)
      if ((qm >> kc) & 1u)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[kc], *reinterpret_cast<const v4i *>(q + (6 + kc) * 1024), acc, 0, 0, 0);      // T_L . Q_H
#pragma unroll
    for (int kc = 1; kc < HT; kc++)
      if ((tm >> kc) & 1u)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6 + kc], *reinterpret_cast<const v4i *>(q + kc * 1024), acc, 0, 0, 0);        // T_H . Q_L
  }
  // the first two operands of the last phase are asked for before the shift's sixteen instructions, which hide part of their latency
  // (asked for at the very top of the chain instead: four spilled registers, 12.35 against 12.30 ms)
  v4i qa = *reinterpret_cast<const v4i *>(q), qb = *reinterpret_cast<const v4i *>(q + 1024);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (HT + HQ > 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = (int)(((unsigned)acc[r] << 8) + (unsigned)cin[r]);
  }
  // T_L . Q_L, always six products: the LDS read of product i + 1 is issued BEFORE the matrix instruction of product i (two operand
  // buffers in turn; the scheduling barriers keep the order -- left alone the compiler reads each operand into the same four registers
  // right after the instruction before it and waits out the whole LDS latency in front of every one of the six)
  {
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], qa, acc, 0, 0, 0);
    qa = *reinterpret_cast<const v4i *>(q + 2 * 1024);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[1], qb, acc, 0, 0, 0);
    qb = *reinterpret_cast<const v4i *>(q + 3 * 1024);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[2], qa, acc, 0, 0, 0);
    qa = *reinterpret_cast<const v4i *>(q + 4 * 1024);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[3], qb, acc, 0, 0, 0);
    qb = *reinterpret_cast<const v4i *>(q + 5 * 1024);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[4], qa, acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[5], qb, acc, 0, 0, 0);
  }
  return acc;
}

// matrix instructions k3_chain issues for a block with these masks
template <int HT, int HQ>
__device__ __forceinline__ int k3_chain_products(unsigned tm, unsigned qm) {
  constexpr int HM = HT < HQ ? HT : HQ;
  if (HT + HQ == 0) return 6;
  int n = 7;  // the last phase's six and the middle phase's first
  if (HM > 0 && (tm & qm)) n += 1 + __builtin_popcount((tm & qm) >> 1);
  n += HT > 0 ? __builtin_popcount(qm) + __builtin_popcount(tm >> 1) : __builtin_popcount(qm >> 1);
  return n;
}

// a tile's MFMA A operands and the rows' terms, straight into registers (global_load_dwordx4, 1 KB contiguous per instruction).  The
// pack (k_knn_pack, database side) holds per row the chain's starting value -- |t-c|^2 where the digits are those of 2 (t - c), |t-c|^2 >> 1
// where not -- and in the 15th word of the tile's box the 32 parities |t-c|^2 & 1 (bit = row); `pwh` = that word shifted so that bit
// k3_prow(r) is accumulator register r's row in this half-wave.
__device__ __forceinline__ constexpr int k3_prow(int r) { return (r & 3) + 8 * (r >> 2); }
template <int KT>
__device__ __forceinline__ void k3_load_rows(const uint8_t *tb, int half, v16i &cin, unsigned &pwh) {
#pragma unroll
  for (int q4 = 0; q4 < 4; q4++) {  // accumulator register r holds row (r&3) + 8*(r>>2) + 4*half
    const v4i x = *reinterpret_cast<const v4i *>(tb + knn_pack_row_terms(KT) + (q4 * 8 + half * 4) * 4);
    cin[q4 * 4] = x[0]; cin[q4 * 4 + 1] = x[1]; cin[q4 * 4 + 2] = x[2]; cin[q4 * 4 + 3] = x[3];
  }
  pwh = *reinterpret_cast<const unsigned *>(tb + knn_pack_parity(KT)) >> (4 * half);
}
template <int KT>
__device__ __forceinline__ void k3_load_tile(const uint8_t *tb, int lane, int half, v4i (&T)[KT], v16i &cin, unsigned &pwh) {
#pragma unroll
  for (int kc = 0; kc < KT; kc++) T[kc] = *reinterpret_cast<const v4i *>(tb + (kc * 64 + lane) * 16);
  k3_load_rows<KT>(tb, half, cin, pwh);
}

// ... leaving out the high-digit chunks the tile's mask says are all zero (the chain skips their products: bit kc clear = T[6 + kc] never
// read).  On the literal bench clip the consume kernel pulled 43.7 GB per launch through the L2s' far side -- 3.4 TB/s, the matrix pipe
// waiting on it -- and two in five of those bytes were zeros.
template <int KT>
__device__ __forceinline__ void k3_load_tile_masked(const uint8_t *tb, int lane, int half, unsigned tm, v4i (&T)[KT], v16i &cin, unsigned &pwh) {
#pragma unroll
  for (int kc = 0; kc < 6; kc++) T[kc] = *reinterpret_cast<const v4i *>(tb + (kc * 64 + lane) * 16);
#pragma unroll
  for (int kc = 6; kc < KT; kc++) {
    T[kc] = v4i{0, 0, 0, 0};
    if ((tm >> (kc - 6)) & 1u) T[kc] = *reinterpret_cast<const v4i *>(tb + (kc * 64 + lane) * 16);
  }
  k3_load_rows<KT>(tb, half, cin, pwh);
}

// ... in two parts for the first-chunk look (k3_chunk_look): chunk 0's low and high digits and row r = lane & 31's term over the chunk's
// columns (`rowp`; behind the tile's box in the pack) are all the look reads, and all k_knn_consume's look task asks for.  The rest of the
// tile is loaded by the chain task (k3_load_tile_masked, the whole tile again) when a block got past its look, which on the bench clip is one
// popped tile in nine.  (The same loads as a phase of the one block loop, look and chain registers live together: 127 registers,
// 136 bytes of scratch, 12.5 against 8.2 ms -- DESIGN 23.)
template <int KT>
__device__ __forceinline__ void k3_load_tile_chunk0(const uint8_t *tb, int lane, unsigned tm, v4i (&T)[KT], unsigned &rowp) {
  T[0] = *reinterpret_cast<const v4i *>(tb + lane * 16);
  if constexpr (KT > 6) {
    T[6] = v4i{0, 0, 0, 0};
    if (tm & 1u) T[6] = *reinterpret_cast<const v4i *>(tb + (6 * 64 + lane) * 16);
  }
  rowp = *reinterpret_cast<const unsigned *>(tb + knn_pack_first_terms(KT, 1) + (lane & 31) * 4);
}
// the minimum of the chain's sixteen values of a lane: a tree of three-way minima (five, two, one: eight instructions; pairs first cost ten)
__device__ __forceinline__ int k3_min3(int a, int b, int c) { return min(min(a, b), c); }
__device__ __forceinline__ int k3_min16(const int (&t)[16]) {
  const int a = k3_min3(t[0], t[1], t[2]), b = k3_min3(t[3], t[4], t[5]), c = k3_min3(t[6], t[7], t[8]), d = k3_min3(t[9], t[10], t[11]),
            e = k3_min3(t[12], t[13], t[14]);
  return min(k3_min3(a, b, c), k3_min3(d, e, t[15]));
}
// what a block's sixteen values say about a lane's query before anything is made of them: a LOWER bound of the smallest d'' - qn.  With
// TD the chain's values are d'' - qn themselves; without, d'' - qn = 2 Y + parity and 2 min(Y) is at most one below the smallest.
template <bool TD>
__device__ __forceinline__ int k3_first_look(const v16i &acc) {
  int y[16];
#pragma unroll
  for (int r = 0; r < 16; r++) y[r] = acc[r];
  const int ym = k3_min16(y);
  return TD ? ym : (int)((unsigned)ym << 1);
}
// Can the block matter to a query whose bound is `bound` (its best d'' + 1, or its threshold + 1)?  The test the epilogue makes itself.
template <bool TD>
__device__ __forceinline__ bool k3_may_matter(const v16i &acc, unsigned qn, unsigned bound) {
  const unsigned look = (unsigned)k3_first_look<TD>(acc) + qn + 1u;
  return k3_within<TD>(look, bound);
}
// A block judged on its first chunk before its chain runs.  The columns are packed widest first, so chunk 0 holds the 32
// widest, and the sum of squares over them is a lower bound of the sum over all: with the pack's row terms and query norms over those
// columns (`rows`: the wave's 32 row terms in LDS, in the form the full ones have -- |t-c|^2 with TD, halved without; `qnp_p`: the lane's
// query's norm, whole) the chain of the chunk's own products -- T_H0 . Q_H0, T_H0 . Q_L0, T_L0 . Q_H0, T_L0 . Q_L0, under k3_chain's
// predicates, shifted as there, the row term riding in on the second shift -- ends in the pair's SSD over the 32 columns (without TD:
// that or one less).  The invariant: what a lane compares is <= SSD over the chunk <= SSD <= d'' + 1 for every row of the block, and
// the compare against the query's best d'' + 1 is inclusive: a row that improves OR ONLY TIES a best always passes, so the bests,
// their original indices included, are those of a scan that ran every chain.  Returns whether the block can matter to this lane's query.
template <int HT, int HQ, bool TD>
__device__ __forceinline__ bool k3_chunk_look(const v4i (&T)[6 + HT], const uint8_t *rows, int half, const uint8_t *q, unsigned tm, unsigned qm, const int *qnp_p,
                                              unsigned bound) {
  constexpr int HM = HT < HQ ? HT : HQ;
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  v16i acc = zero;
  if constexpr (HT + HQ > 0) {
    constexpr int FA = HT > 0 ? 6 : 0, FQ = HT > 0 ? 0 : 6;  // (k3_chain: the product that always runs)
    bool hh = false;
    if constexpr (HM > 0) hh = (tm & qm & 1u) != 0;
    if (hh) {
      if constexpr (HM > 0) {
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], *reinterpret_cast<const v4i *>(q + 6 * 1024), zero, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = (int)((unsigned)acc[r] << 8);
      }
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[FA], *reinterpret_cast<const v4i *>(q + FQ * 1024), acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[FA], *reinterpret_cast<const v4i *>(q + FQ * 1024), zero, 0, 0, 0);
    }
    if constexpr (HM > 0)
      if (qm & 1u) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], *reinterpret_cast<const v4i *>(q + 6 * 1024), acc, 0, 0, 0);
  }
  // The row terms come out of LDS four at a time (k3_load_rows' order: accumulator register r holds row (r&3) + 8*(r>>2) + 4*half), each
  // read one group ahead of the shift that takes it in, in two buffers in turn like the chain's last operands: all sixteen asked for at
  // once were eleven more spilled registers.
  auto term = [&](int q4) { return *reinterpret_cast<const v4i *>(rows + (q4 * 8 + half * 4) * 4); };
  v4i xa = term(0), xb = term(1);
  if constexpr (HT + HQ > 0) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = (int)(((unsigned)acc[i] << 8) + (unsigned)xa[i]);
    xa = term(2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[4 + i] = (int)(((unsigned)acc[4 + i] << 8) + (unsigned)xb[i]);
    xb = term(3);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[8 + i] = (int)(((unsigned)acc[8 + i] << 8) + (unsigned)xa[i]);
    xa = *reinterpret_cast<const v4i *>(q);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[12 + i] = (int)(((unsigned)acc[12 + i] << 8) + (unsigned)xb[i]);
  } else {
    const v4i xc = term(2), xd = term(3);
#pragma unroll
    for (int i = 0; i < 4; i++) { acc[i] = xa[i]; acc[4 + i] = xb[i]; acc[8 + i] = xc[i]; acc[12 + i] = xd[i]; }
    xa = *reinterpret_cast<const v4i *>(q);
  }
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], xa, acc, 0, 0, 0);  // T_L0 . Q_L0
  const unsigned qnp = (unsigned)*qnp_p;  // (asked for behind the shifts: a register fewer across them)
  const unsigned look = (unsigned)k3_first_look<TD>(acc) + qnp;  // the SSD over the chunk (without TD: at most one below it, -1 at the least)
  return k3_within<TD>(look, bound);
}
// Two blocks of one tile judged at once: sub-tiles A and B (`qa`, `qb`: their operands) against the same chunk 0 and the same row terms,
// k3_chunk_look's arithmetic for each.  A look is one chain of dependent steps -- operand read, product, shift, product ... minimum -- and a
// wave that looks (k_knn_consume's look task) holds so little of the tile that a second accumulator fits: the two chains stand in ONE
// basic block and each fills the other's waits.  For that the products run whatever the masks say: a chunk its mask calls empty is all
// zeros, the tile's by k3_load_tile_chunk0 and the queries' in the pack, so the product adds nothing and the values are k3_chunk_look's.
template <int HT, int HQ, bool TD>
__device__ __forceinline__ void k3_chunk_look2(const v4i (&T)[6 + HT], const uint8_t *rows, int half, const uint8_t *qa, const uint8_t *qb, const int *qnpa_p,
                                               const int *qnpb_p, unsigned bounda, unsigned boundb, bool &ina, bool &inb) {
  constexpr int HM = HT < HQ ? HT : HQ;
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto opd = [](const uint8_t *q, int kc) { return *reinterpret_cast<const v4i *>(q + kc * 1024); };
  auto term = [&](int q4) { return *reinterpret_cast<const v4i *>(rows + (q4 * 8 + half * 4) * 4); };  // (k3_load_rows' order)
  const v4i la = opd(qa, 0), lb = opd(qb, 0);  // Q_L0 of either sub-tile
  const v4i r0 = term(0), r1 = term(1), r2 = term(2), r3 = term(3);
  v16i a, b;
  if constexpr (HT + HQ > 0) {
    if constexpr (HM > 0) {
      const v4i ha = opd(qa, 6), hb = opd(qb, 6);  // Q_H0
      a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], ha, zero, 0, 0, 0);
      b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], hb, zero, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; r++) a[r] = (int)((unsigned)a[r] << 8);
      a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], la, a, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; r++) b[r] = (int)((unsigned)b[r] << 8);
      b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], lb, b, 0, 0, 0);
      a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], ha, a, 0, 0, 0);
      b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], hb, b, 0, 0, 0);
    } else if constexpr (HT > 0) {  // no high digits on the query side: T_H0 . Q_L0
      a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], la, zero, 0, 0, 0);
      b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[6], lb, zero, 0, 0, 0);
    } else {  // none on the database side: T_L0 . Q_H0
      a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], opd(qa, 6), zero, 0, 0, 0);
      b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], opd(qb, 6), zero, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      a[i] = (int)(((unsigned)a[i] << 8) + (unsigned)r0[i]); a[4 + i] = (int)(((unsigned)a[4 + i] << 8) + (unsigned)r1[i]);
      a[8 + i] = (int)(((unsigned)a[8 + i] << 8) + (unsigned)r2[i]); a[12 + i] = (int)(((unsigned)a[12 + i] << 8) + (unsigned)r3[i]);
    }
    a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], la, a, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      b[i] = (int)(((unsigned)b[i] << 8) + (unsigned)r0[i]); b[4 + i] = (int)(((unsigned)b[4 + i] << 8) + (unsigned)r1[i]);
      b[8 + i] = (int)(((unsigned)b[8 + i] << 8) + (unsigned)r2[i]); b[12 + i] = (int)(((unsigned)b[12 + i] << 8) + (unsigned)r3[i]);
    }
    b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], lb, b, 0, 0, 0);
  } else {
    v16i c;
#pragma unroll
    for (int i = 0; i < 4; i++) { c[i] = r0[i]; c[4 + i] = r1[i]; c[8 + i] = r2[i]; c[12 + i] = r3[i]; }
    a = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], la, c, 0, 0, 0);
    b = __builtin_amdgcn_mfma_i32_32x32x32_i8(T[0], lb, c, 0, 0, 0);
  }
  const unsigned qnpa = (unsigned)*qnpa_p, qnpb = (unsigned)*qnpb_p;
  ina = k3_within<TD>((unsigned)k3_first_look<TD>(a) + qnpa, bounda);
  inb = k3_within<TD>((unsigned)k3_first_look<TD>(b) + qnpb, boundb);
}
template <int HT, int HQ>
__device__ __forceinline__ constexpr int k3_chunk_look2_products() {  // ... of either block
  return HT + HQ == 0 ? 1 : ((HT < HQ ? HT : HQ) > 0 ? 4 : 2);
}
// matrix instructions k3_chunk_look issues for a block with these masks
template <int HT, int HQ>
__device__ __forceinline__ int k3_chunk_look_products(unsigned tm, unsigned qm) {
  constexpr int HM = HT < HQ ? HT : HQ;
  int n = HT + HQ > 0 ? 2 : 1;
  if (HM > 0) n += ((tm & qm & 1u) ? 1 : 0) + ((qm & 1u) ? 1 : 0);
  return n;
}
// ... and the values themselves (d'' - qn of accumulator register r)
template <bool TD>
__device__ __forceinline__ void k3_values(const v16i &acc, unsigned pwh, int (&t)[16]) {
  if (!TD) asm volatile("" : "+v"(pwh));  // (the sixteen parity bits are taken out HERE, on the rare path: seen through, the compiler takes them out once per tile and keeps sixteen registers for them)
#pragma unroll
  for (int r = 0; r < 16; r++) t[r] = TD ? acc[r] : (int)(((unsigned)acc[r] << 1) | ((pwh >> k3_prow(r)) & 1u));
}

// Which of a lane's sixteen registers hold `ym`: bit k3_prow(r) for register r, the positions `pwh` keeps the rows' parities at.  A compare
// and an add-with-carry (E + E + equal: a shift that takes the compare's bit in) per register, from register 15 down, and a shift by four
// between the groups of four: 35 vector instructions.  Written out by hand because a vector compare's result may be read by a vector
// instruction only two issue slots later: left to the compiler every compare is followed by a two-cycle s_nop; here three compares are in
// flight in three scalar pairs in turn, so every add-with-carry stands two instructions behind its compare and none waits.
__device__ __forceinline__ unsigned k3_equal_mask(const v16i &acc, int ym) {
  unsigned e;
  unsigned long long c0, c1, c2;
  asm("v_cmp_eq_u32_e64 %1, %19, %20\n\t"
      "v_cmp_eq_u32_e64 %2, %18, %20\n\t"
      "v_cmp_eq_u32_e64 %3, %17, %20\n\t"
      "v_addc_co_u32_e64 %0, %1, 0, 0, %1\n\t"
      "v_cmp_eq_u32_e64 %1, %16, %20\n\t"
      "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
      "v_cmp_eq_u32_e64 %2, %15, %20\n\t"
      "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
      "v_cmp_eq_u32_e64 %3, %14, %20\n\t"
      "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
      "v_cmp_eq_u32_e64 %1, %13, %20\n\t"
      "v_lshlrev_b32_e32 %0, 4, %0\n\t"
      "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
      "v_cmp_eq_u32_e64 %2, %12, %20\n\t"
      "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
      "v_cmp_eq_u32_e64 %3, %11, %20\n\t"
      "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
      "v_cmp_eq_u32_e64 %1, %10, %20\n\t"
      "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
      "v_cmp_eq_u32_e64 %2, %9, %20\n\t"
      "v_lshlrev_b32_e32 %0, 4, %0\n\t"
      "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
      "v_cmp_eq_u32_e64 %3, %8, %20\n\t"
      "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
      "v_cmp_eq_u32_e64 %1, %7, %20\n\t"
      "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
      "v_cmp_eq_u32_e64 %2, %6, %20\n\t"
      "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
      "v_cmp_eq_u32_e64 %3, %5, %20\n\t"
      "v_lshlrev_b32_e32 %0, 4, %0\n\t"
      "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
      "v_cmp_eq_u32_e64 %1, %4, %20\n\t"
      "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"
      "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
      "v_addc_co_u32_e64 %0, %1, %0, %0, %1"
      : "=&v"(e), "=&s"(c0), "=&s"(c1), "=&s"(c2)
      : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]), "v"(acc[8]), "v"(acc[9]), "v"(acc[10]),
        "v"(acc[11]), "v"(acc[12]), "v"(acc[13]), "v"(acc[14]), "v"(acc[15]), "v"(ym));
  return e;
}

// A tile's 32 original indices into the wave's own 128 bytes of LDS (consume): one LDS-DMA load by lanes 0..31, `src` = the indices in the
// tile's pack and `lds_dst` = the slot's LDS address, both wave-uniform.  The load has no register destination -- the block loop has none to
// spare -- and the compiler does not count it: whoever reads the slot waits for it (k3_tile_idx_staged).  M0, the LDS base of
// such a load, is the compiler's and is put back.  (The wait states in front of the load cover a base the compiler may have made on the
// vector unit and M0's own.)  The wave's reads of the slot for the tile before are retired by then: each fed an atomic already issued.
__device__ __forceinline__ void k3_stage_tile_idx(const uint8_t *src, unsigned lds_dst, int lane) {
  if (lane < 32) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %3\n\t"
                 "s_nop 2\n\t"
                 "global_load_lds_dword %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane * 4), "s"(src), "s"(lds_dst)
                 : "memory");
  }
}
// ... and one of them read back by the wave that staged them.  Nothing orders an LDS read behind an LDS-DMA load but the issuing wave's own
// wait for its memory counter, so the wait stands in the statement that reads.  It waits for nothing else: the read is made behind a
// block's chain, which has taken in every load of the tile, and the next tile's are not asked for before the block loop ends.
__device__ __forceinline__ unsigned k3_tile_idx_staged(const unsigned *p) {
  unsigned v;
  asm volatile("s_waitcnt vmcnt(0)\n\t"
               "ds_read_b32 %0, %1\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(v)
               : "v"((unsigned)(size_t)(const __attribute__((address_space(3))) unsigned *)p)
               : "memory");
  return v;
}

// The survivor queue of k_knn_consume: a ring of K3_RING entries in LDS between the waves that look and the waves that run
// chains.  An entry is one 64-bit word, (ticket + 1) << 32 | list index << 16 | mask of the sub-tiles whose looks the tile got past (never
// empty: no entry's low word is 0); `head` and `tail` count the tickets taken and handed out and only grow.  A pusher claims ticket t by a
// compare-and-swap on the tail while t - head < K3_RING -- the slot's last tenant, ticket t - K3_RING, is then taken, and whoever took it
// read it before the swap that took it -- and writes the word with one store.  A popper reads the head h and the slot's word, and takes the
// entry by a compare-and-swap on the head only if the word carries ticket h: a slot not yet written, or written for another lap, reads as
// an empty queue, and a swap that fails (another wave was faster; the slot may have a new tenant by now) leaves the word read unused.
// NOBODY WAITS FOR ANOTHER WAVE.  A push is tried once: a full ring, or a tail another wave moved first, turns the entry away, and the
// pusher runs its chains itself, which costs nothing (it would as likely have popped the entry itself).  A pop is tried again only while
// an entry stands READY at the head -- every failed swap is another wave's entry taken, so the tries end with the entries (and at
// K3_RING_TRIES whatever happens); what a popper missed is picked up behind the segment's barrier.  Lane 0 acts, every lane gets the answer.
__device__ __forceinline__ unsigned k3_surv_make(int j, unsigned surv) { return ((unsigned)j << 16) | surv; }
__device__ __forceinline__ unsigned k3_surv_entry(unsigned e) { return e >> 16; }
__device__ __forceinline__ unsigned k3_surv_mask(unsigned e) { return e & 0xFFFFu; }
static_assert(K3_LCAP <= 1 << 16 && (K3_RING & (K3_RING - 1)) == 0, "a survivor entry's fields; the ring's slots by a mask");
constexpr int K3_RING_TRIES = 64;
__device__ __forceinline__ bool k3_ring_push(unsigned long long *ring, int *head, int *tail, unsigned e, int lane) {
  int ok = 0;
  if (lane == 0) {
    const unsigned t = k3_peek(reinterpret_cast<unsigned *>(tail)), h = k3_peek(reinterpret_cast<unsigned *>(head));
    // (t - h >= K3_RING: full -- or the two reads straddled other waves' work, which is taken for full)
    if (t - h < (unsigned)K3_RING && atomicCAS(reinterpret_cast<unsigned *>(tail), t, t + 1u) == t) {
      __hip_atomic_store(&ring[t & (K3_RING - 1)], ((unsigned long long)(t + 1u) << 32) | e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      ok = 1;
    }
  }
  return __builtin_amdgcn_readfirstlane(ok) != 0;
}
__device__ __forceinline__ unsigned k3_ring_pop(const unsigned long long *ring, int *head, int lane) {  // 0: nothing ready
  unsigned got = 0;
  if (lane == 0) {
    for (int tries = 0; tries < K3_RING_TRIES && !got; tries++) {
      const unsigned h = k3_peek(reinterpret_cast<unsigned *>(head));
      const unsigned long long w = __hip_atomic_load(&ring[h & (K3_RING - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if ((unsigned)(w >> 32) != h + 1u) break;  // empty, or claimed and not yet written
      if (atomicCAS(reinterpret_cast<unsigned *>(head), h, h + 1u) == h) got = (unsigned)w;
    }
  }
  return (unsigned)__builtin_amdgcn_readfirstlane((int)got);
}

// A block's epilogue: the row minimum of each query (lane & 31; the two half-waves hold 16 rows each) against its running best in LDS.
// d'' = 2 X + |t-c|^2 + 2 (|q-c|^2 >> 1) = SSD - parity.  Returns true in lanes whose improvement may have lowered the sub-tile's largest
// best (the caller refreshes the bound when any lane says so); `sm_now` = the sub-tile's published bound, or 0 to ask for a refresh on
// every improvement.
// The minimum and the rows reaching it come from the first look's own minimum ym = min Y_r.  A row's value is 2 Y_r + parity_r,
// and a row with Y_r >= ym + 1 is worth at least 2 ym + 2: so the minimum is 2 ym + p, p the smallest parity among the rows with Y_r = ym,
// and the rows reaching it are those with Y_r = ym and parity p.  With TD the values are the Y_r (p = 0).  Neither the sixteen values nor a
// second minimum are made, and the row is named by a bit scan: k3_prow grows with r, so the lowest set bit is the first register's row.
// The key's low word is the row's ORIGINAL index (`tidx`: the 32 indices of the wave's tile in LDS), so the atomic minimum settles equal
// distances by the rule of CompareEuclideanDCTPtr's callers where they meet: among a lane's rows the lowest set bit of `win` is the lowest
// index (a tile's rows ascend in it: k_knn_tile_order), the other half-wave, the other waves and the seeds meet through the atomic.
// DMA: the indices came by k3_stage_tile_idx and are waited for here (k3_tile_idx_staged).
template <bool TD, bool DMA>
__device__ __forceinline__ bool k3_epilogue(const v16i &acc, unsigned pwh, const unsigned *tidx, int half, unsigned qn, unsigned long long *best,
                                            unsigned sm_now, unsigned cur_hi /* the query's best as read BEFORE the chain: stale only on the safe side (a best only falls) */) {
  bool refresh = false;
  int y[16];
#pragma unroll
  for (int r = 0; r < 16; r++) y[r] = acc[r];
  const int ym = k3_min16(y);
  const unsigned look = (unsigned)(TD ? ym : (int)((unsigned)ym << 1)) + qn + 1u;  // k3_may_matter's test, on a minimum that is kept
  if (k3_within<TD>(look, cur_hi)) {  // (by the counters nearly half of the listed blocks improve or tie some query's best)
    const unsigned eq = k3_equal_mask(acc, ym);
    unsigned win = eq, key_hi = look;  // d'' + 1 >= 0
    if (!TD) {
      const unsigned even = eq & ~pwh;  // the rows at ym whose parity is 0
      win = even ? even : eq;
      key_hi = look + (even ? 0u : 1u);
    }
    if (key_hi <= cur_hi) {
      const int row = __builtin_ctz(win) + 4 * half;  // the first row reaching the minimum: of this lane's, the one of the lowest original index
      const unsigned idx = DMA ? k3_tile_idx_staged(tidx + row) : tidx[row];
      const unsigned long long key = ((unsigned long long)key_hi << 32) | idx;
      const unsigned long long pre = atomicMin(best, key);
      const unsigned pre_hi = (unsigned)(pre >> 32);
      // The sub-tile's largest best can only have moved if this query held it: its old best is then no smaller than what the published
      // bound was made from (K3_BOUND_FLOOR).  A refresh skipped by a race only leaves the bound loose (and is made good at the end of the
      // segment).
      const unsigned thr = K3_BOUND_FLOOR(sm_now);
      refresh = key_hi < pre_hi && pre_hi >= thr;
    }
  }
  return refresh;
}

// Collection mode's epilogue.  The query's state in LDS: `best` = (tau + 1) << 32 | step (tau: its threshold, d'' <= tau), `base` = the
// threshold it came with + 1, `lad` = 7 x 16-bit counters: rows seen with d'' + 1 <= base - j step for j = 1..7 -- the ladder's rungs hang
// below the pass's first threshold at the spacing the host chose (tau / 8 in a first pass; an eighth of the bracket the pass before left --
// its last threshold down to the rung below it that did NOT fill -- afterwards: on data whose distances bunch, a rung spacing of tau / 8
// moved the threshold by a third per pass).  Every row within the threshold is appended to the query's candidate list UNTIL THE LIST IS
// FULL (bit 31 of lad[3]: from then on the query is only counted -- it will be scanned again anyway, and its appends, a global atomic and
// eight bytes each, were most of the collection scans' time on such data); once cand_k rows lie at or below a rung, the k-th nearest is at
// most that rung + 1 and the threshold drops to it (the threshold only ever falls, every value it takes is a valid bound: the waves of a
// workgroup, and the parts of a split group, lower it on their own evidence).  Returns true in lanes that lowered a threshold the
// sub-tile's bound may hang on.
template <bool TD>
__device__ __forceinline__ bool k3_epilogue_topk(const v16i &acc, unsigned pwh, int tile, bool countable, int half, unsigned qn, unsigned long long *best,
                                                 unsigned *lad, const unsigned *base_p, bool qvalid, int64_t q, const Knn3Args &a, unsigned sm_now) {
  const unsigned tau1 = k3_peek(reinterpret_cast<unsigned *>(best) + 1);  // tau + 1
  bool refresh = false;
  // (the first look is a lower bound: a lane it lets in with no row within the threshold appends and counts nothing -- every row is tested
  // by its own value below -- and at most lowers its threshold on the rungs' counts as they stand, which is valid at any time)
  if (qvalid && k3_may_matter<TD>(acc, qn, tau1)) {
    int t[16];
    k3_values<TD>(acc, pwh, t);
    const unsigned step = k3_peek(reinterpret_cast<unsigned *>(best)), base = *base_p;
    bool full = (k3_peek(&lad[3]) >> 31) != 0, filled = false;
    unsigned c[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const unsigned d1 = (unsigned)t[r] + qn + 1u;  // d'' + 1
      if (d1 <= tau1) {
        if (!full) {
          const int slot = atomicAdd(&a.cand_cnt[q], 1);  // (ends above the capacity for a query whose list filled: how the select stage knows)
          if (slot < a.cand_cap) a.cand[q * a.cand_cap + slot] = make_uint2(d1 - 1u, (unsigned)((tile << 5) | (k3_prow(r) + 4 * half)));
          else { full = true; filled = true; }
        }
#pragma unroll
        for (int j = 1; j <= 7; j++) c[j - 1] += (countable && d1 + (unsigned)j * step <= base) ? 1u : 0u;
      }
    }
    if (filled) atomicOr(&lad[3], 0x80000000u);
    // the counters saturate where they stop mattering: a rung that has its cand_k rows takes no more (so no 16-bit field overflows
    // into its neighbour: at most cand_k + 16 rows x 2 half-waves x 16 waves land in one)
    const unsigned k = (unsigned)a.cand_k;
    unsigned cur[4];
#pragma unroll
    for (int w = 0; w < 4; w++) cur[w] = k3_peek(&lad[w]);
    unsigned add[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const unsigned have = (cur[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
      if (have < k) add[j >> 1] += c[j] << (16 * (j & 1));
    }
    unsigned now[4];
#pragma unroll
    for (int w = 0; w < 4; w++) now[w] = add[w] ? atomicAdd(&lad[w], add[w]) + add[w] : cur[w];
    now[3] &= 0x7FFFFFFFu;
    int rung = 0;
#pragma unroll
    for (int j = 1; j <= 7; j++)
      if (((now[(j - 1) >> 1] >> (16 * ((j - 1) & 1))) & 0xFFFFu) >= k) rung = j;
    // cand_k rows have d'' + 1 <= base - rung step, i.e. SSD <= that: no row beyond it can be among the k nearest
    const unsigned tnew1 = base - (unsigned)rung * step + 1u;  // (new tau = the rung's bound) + 1
    if (rung > 0 && step > 0 && tnew1 < tau1) {
      const unsigned pre = atomicMin(reinterpret_cast<unsigned *>(best) + 1, tnew1);
      const unsigned thr = K3_BOUND_FLOOR(sm_now);
      refresh = tnew1 < pre && pre >= thr;
    }
  }
  return refresh;
}

}  // namespace tmx
