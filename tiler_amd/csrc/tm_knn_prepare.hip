// tm_knn_prepare.hip -- what a KNN search does before its scan: both sides sorted along the curve (Hilbert or Morton) and packed into the scan's
// MFMA fragment order, the database's boxes (see tm_knn.hip for the scheme, tm_knn_kernel.h for the pruning).
#include <rocprim/device/device_radix_sort.hpp>

#include "tm_knn.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// Pack n rows into MFMA fragment order: per 32-row tile [kc][64 lanes][16 B] (lane = half*32 + row) followed by
// 32 u32 norms.  negate=1 (query side): digits of (c - v) and norm >> 1; negate=0 (database): digits of (v - c).
// Rows >= n replicate row n-1 (database side: the tile's box and the row terms over the first chunk's columns follow the norms, and the
// tile's last 128 bytes, the rows' original indices, are k_knn_tile_order's: the packed tile of tm_knn3.h).  err_flag is set if a digit overflows int8.
// scale (database side, KnnPlan::tscale): the digits are those of scale * (v - c); the norms stay those of v - c.
__global__ __launch_bounds__(256) void k_knn_pack(const int16_t *__restrict__ feat, int64_t n, int64_t ntiles, int hch, int negate, int scale,
                                                  const int16_t *__restrict__ centre, const int16_t *__restrict__ perm,
                                                  const uint32_t *__restrict__ rowperm, int with_box, CurveSpec cs,
                                                  int *__restrict__ box_lo, int *__restrict__ box_hi, uint8_t *__restrict__ out,
                                                  int *__restrict__ err_flag, int *__restrict__ qmeta /* query side: [ntiles][QMETA_INTS] box, home tile, high-chunk mask */,
                                                  uint8_t *__restrict__ hmask /* database side: [ntiles] which high-digit chunks of the tile hold a non-zero digit */) {
  __shared__ __attribute__((aligned(16))) int16_t s_c[192];  // centre of the column at packed position p
  __shared__ int16_t s_inv[192];                             // source column -> packed position
  __shared__ uint32_t s_norm[32];
  __shared__ unsigned s_hm;  // bit kc: high-digit chunk kc of this tile is not all zero
  __shared__ long long s_bsq[32];  // query side: squared distance of each row from the centres over the box columns
  __shared__ __attribute__((aligned(16))) int16_t s_perm[32][200];  // the tile's rows, raw values in PACKED column order (pitch 400 B)
  for (int i = threadIdx.x; i < 192; i += 256) { s_c[i] = centre[perm[i]]; s_inv[perm[i]] = (int16_t)i; }
  __syncthreads();
  const int kch = 6 + hch, tile_bytes = knn_pack_bytes(kch, with_box);
  // The 32 rows of a tile come in as 16-byte vectors (three per thread: the column permutation would otherwise turn the read into 6 144
  // two-byte loads per tile) and go into LDS already permuted, two bytes at a time to places the thread knows for good (its vectors cover the
  // same columns of every tile); digits and norms are then made from 16-byte reads of the permuted rows.  (A copy in memory order, a second,
  // centred int32 copy in packed order and a barrier between them were 38 KB of LDS -- four workgroups a CU -- and a third of a tile's time.)
  // The NEXT tile's vectors are fetched while this one is worked on, and the row numbers (curve order) of the one after: a workgroup walks
  // its tiles one after the other, and two dependent round trips to memory per tile were most of the kernel.
  int pr[3], pv[3];
  uint16_t dst[3][8];  // where the eight values of vector u go in s_perm
#pragma unroll
  for (int u = 0; u < 3; u++) {
    const int i = threadIdx.x + u * 256;
    pr[u] = i / 24; pv[u] = i - pr[u] * 24;
#pragma unroll
    for (int j = 0; j < 8; j++) dst[u][j] = (uint16_t)(pr[u] * 200 + s_inv[pv[u] * 8 + j]);
  }
  auto row_of = [&](int64_t tile, int r) -> int64_t {
    int64_t row = std::min<int64_t>(tile * 32 + r, n - 1);
    return rowperm ? (int64_t)rowperm[row] : row;  // rows are packed in curve order
  };
  int64_t nrow[3];   // rows of the tile after next
  uint4 nvec[3];     // vectors of the next tile
  {
    const int64_t t0 = blockIdx.x, t1 = (int64_t)blockIdx.x + gridDim.x;
#pragma unroll
    for (int u = 0; u < 3; u++) {
      nvec[u] = t0 < ntiles ? *reinterpret_cast<const uint4 *>(feat + row_of(t0, pr[u]) * 192 + pv[u] * 8) : make_uint4(0, 0, 0, 0);
      nrow[u] = t1 < ntiles ? row_of(t1, pr[u]) : 0;
    }
  }
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    if (threadIdx.x == 0) s_hm = 0;
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const uint32_t w[4] = {nvec[u].x, nvec[u].y, nvec[u].z, nvec[u].w};
#pragma unroll
      for (int j = 0; j < 8; j++) (&s_perm[0][0])[dst[u][j]] = (int16_t)(w[j >> 1] >> ((j & 1) * 16));
    }
    {
      const int64_t t1 = tile + gridDim.x, t2 = tile + 2 * (int64_t)gridDim.x;
#pragma unroll
      for (int u = 0; u < 3; u++) {
        if (t1 < ntiles) nvec[u] = *reinterpret_cast<const uint4 *>(feat + nrow[u] * 192 + pv[u] * 8);
        if (t2 < ntiles) nrow[u] = row_of(t2, pr[u]);
      }
    }
    __syncthreads();
    if (qmeta && threadIdx.x >= 192 && threadIdx.x < 224) {
      // the sub-tile's bounding box over the box columns, as the first scan shape computed it in its prologue: the rows are in LDS here (a
      // kernel of its own gathered six scattered columns of every row again, 0.33 ms for 3.2 M rows)
      const int r = threadIdx.x - 192;
      int lo[KNN_NC], hi[KNN_NC];
      long long boxsq = 0;
#pragma unroll
      for (int d = 0; d < KNN_NC; d++) {
        const int v = s_perm[r][s_inv[cs.col[d]]];
        lo[d] = hi[d] = v;
        const long long c = v - (int)centre[cs.col[d]];
        boxsq += c * c;
      }
      s_bsq[r] = boxsq;
      for (int o = 16; o > 0; o >>= 1)  // the six dimensions' exchanges of a step are independent: they overlap
#pragma unroll
        for (int d = 0; d < KNN_NC; d++) { lo[d] = min(lo[d], __shfl_xor(lo[d], o)); hi[d] = max(hi[d], __shfl_xor(hi[d], o)); }
      if (r == 0)
#pragma unroll
        for (int d = 0; d < KNN_NC; d++) { qmeta[qmeta_at(tile, QMETA_LO + d)] = lo[d]; qmeta[qmeta_at(tile, QMETA_HI + d)] = hi[d]; }
    }
    uint8_t *obase = out + tile * (int64_t)tile_bytes;
    bool bad = false;
    const int mult = negate ? -scale : scale;  // the digits are those of mult * (v - c)
    for (int piece = threadIdx.x; piece < kch * 64; piece += 256) {
      // a wave's 64 pieces are one chunk's (kc is the same for them, and known to be: the cases below are branches, not masks)
      const int kc = __builtin_amdgcn_readfirstlane(piece >> 6), ln = piece & 63, half = ln >> 5, r = ln & 31;
      const bool high = kc >= 6;                // a chunk of high digits, of the columns of chunk kc - 6
      const bool must_fit = !high && kc >= hch;  // columns without a high digit
      const int kp = (high ? kc - 6 : kc) * 32 + half * 16;  // packed position of the piece's first value
      // the piece's sixteen values and their centres as two 16-byte LDS reads each (the centres' are the same for the 32 rows: a broadcast)
      const int4 *src = reinterpret_cast<const int4 *>(&s_perm[r][kp]), *cen = reinterpret_cast<const int4 *>(&s_c[kp]);
      const int4 q0 = src[0], q1 = src[1], c0 = cen[0], c1 = cen[1];
      const int qw[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}, cw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      // v = mult * (value - centre), |v| < 2^18 (a 24-bit multiply is exact).  Balanced base 256, v = 256 h + l with l in [-128, 127]: l's byte
      // is v's low byte and h = (v + 128) >> 8; a digit d fits int8 where (unsigned)(d + 128) <= 255, so the OR of those sums over the piece
      // has a bit above the eighth exactly where some digit does not fit.
      uint32_t w[4] = {0, 0, 0, 0}, over = 0;
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int raw = (b & 1) ? (qw[b >> 1] >> 16) : (int)(int16_t)(qw[b >> 1] & 0xffff);
        const int c = (b & 1) ? (cw[b >> 1] >> 16) : (int)(int16_t)(cw[b >> 1] & 0xffff);
        const int v = __mul24(raw - c, mult);
        if (high) {
          const int h = (v + 128) >> 8;
          over |= (uint32_t)(h + 128);
          w[b >> 2] |= (uint32_t)(h & 255) << ((b & 3) * 8);
        } else {
          if (must_fit) over |= (uint32_t)(v + 128);
          w[b >> 2] |= (uint32_t)(v & 255) << ((b & 3) * 8);
        }
      }
      if (over > 255u) bad = true;
      *reinterpret_cast<uint4 *>(obase + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
      if (high && (w[0] | w[1] | w[2] | w[3])) atomicOr(&s_hm, 1u << (kc - 6));
    }
    {  // |v-c|^2 of every row (the kernel drops the query side's parity bit): eight lanes per row, 24 packed positions each, integer sums
       // mod 2^32 (their order does not matter; 32 threads walking 192 values each were the longest leg of a tile)
      const int r = threadIdx.x >> 3, part = threadIdx.x & 7;
      uint32_t sq = 0, sqp = 0;  // over all columns; over the first chunk's (perm[0..31], the 32 widest: k3_chunk_look's lower bound)
      const int4 *src = reinterpret_cast<const int4 *>(&s_perm[r][part * 24]), *cen = reinterpret_cast<const int4 *>(&s_c[part * 24]);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int4 q = src[k], c = cen[k];
        const int qw[4] = {q.x, q.y, q.z, q.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int p = part * 24 + k * 8 + 2 * j;
          const int v0 = (int)(int16_t)(qw[j] & 0xffff) - (int)(int16_t)(cw[j] & 0xffff), v1 = (qw[j] >> 16) - (cw[j] >> 16);
          const uint32_t s0 = (uint32_t)__mul24(v0, v0), s1 = (uint32_t)__mul24(v1, v1);  // (the low 32 bits of the product, as a 32-bit multiply's)
          sq += s0 + s1;
          if (p < 32) sqp += s0;
          if (p + 1 < 32) sqp += s1;
        }
      }
      sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4);
      sqp += __shfl_xor(sqp, 1); sqp += __shfl_xor(sqp, 2); sqp += __shfl_xor(sqp, 4);
      // what the pack keeps per row is what the scan's chain starts from (k3_chain's `cin`): the query side's |q-c|^2 (the kernel drops its
      // parity), the database side's |t-c|^2 where its digits are those of 2 (t - c), and |t-c|^2 >> 1 where not -- the parities then go
      // into the tile's box (word KNN_PACK_BOX_PARITY)
      // ... and the same over the first chunk's columns, in the same form (the query side's whole), behind the box
      if (part == 0) {
        s_norm[r] = sq;
        reinterpret_cast<uint32_t *>(knn_pack_row_terms(kch, obase))[r] = (with_box && scale == 1) ? sq >> 1 : sq;
        reinterpret_cast<uint32_t *>(knn_pack_first_terms(kch, with_box, obase))[r] = (with_box && scale == 1) ? sqp >> 1 : sqp;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (rows >= n replicate row n - 1: they add no digit the real rows do not have)
      if (hmask) hmask[tile] = (uint8_t)s_hm;
      if (qmeta) qmeta[qmeta_at(tile, QMETA_HMASK)] = (int)s_hm;
    }
    if (qmeta && threadIdx.x < 32) {  // the radial dimension of the sub-tile's box (the columns' part was done beside the centring phase)
      const int r = threadIdx.x;
      const long long n2 = (long long)(s_norm[r] & ~1u), boxsq = s_bsq[r];
      int lo = max(0, (int)floor(sqrt((double)max(0ll, n2 - boxsq))) - 1);
      int hi = (int)ceil(sqrt((double)max(0ll, n2 + 1 - boxsq))) + 1;
      for (int o = 16; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
      if (r == 0) { qmeta[qmeta_at(tile, QMETA_LO + KNN_NC)] = lo; qmeta[qmeta_at(tile, QMETA_HI + KNN_NC)] = hi; }
    }
    if (threadIdx.x < 32) {
      const uint32_t s = with_box ? s_norm[threadIdx.x] : 0u;
      if (with_box) {  // radial box dimension: |v-c| over the columns that are not box columns, rounded outwards, min/max over the rows
        int64_t row = std::min<int64_t>(tile * 32 + threadIdx.x, n - 1);
        if (rowperm) row = rowperm[row];
        long long boxsq = 0;
        for (int d = 0; d < KNN_NC; d++) { const long long c = (long long)feat[row * 192 + cs.col[d]] - centre[cs.col[d]]; boxsq += c * c; }
        const long long rest = std::max(0ll, (long long)s - boxsq);
        int lo = max(0, (int)floor(sqrt((double)rest)) - 1), hi = (int)ceil(sqrt((double)rest)) + 1;
        for (int o = 16; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
        const unsigned par = (unsigned)__builtin_amdgcn_ballot_w64((s & 1u) != 0);  // (lanes 0..31: one per row)
        if (threadIdx.x == 0) {
          int *tb = reinterpret_cast<int *>(knn_pack_box(kch, obase));
          tb[KNN_PACK_BOX_PARITY] = (int)par;
          tb[KNN_PACK_BOX_PARITY + 1] = 0;
          tb[KNN_NC] = lo;
          tb[KNN_ND + KNN_NC] = hi;
          box_lo[(int64_t)KNN_NC * ntiles + tile] = lo;
          box_hi[(int64_t)KNN_NC * ntiles + tile] = hi;
        }
      }
    }
    if (bad) atomicOr(err_flag, 1);
    if (with_box && threadIdx.x >= 64 && threadIdx.x < 64 + KNN_NC) {  // bounding box of the tile over the box columns (raw values)
      const int d = threadIdx.x - 64;
      int a = INT_MAX, b = INT_MIN;
      for (int r = 0; r < 32; r++) {
        int64_t row = tile * 32 + r;
        if (row >= n) break;
        if (rowperm) row = rowperm[row];
        const int v = feat[row * 192 + cs.col[d]];
        a = min(a, v);
        b = max(b, v);
      }
      int *tb = reinterpret_cast<int *>(knn_pack_box(kch, obase));
      tb[d] = a;
      tb[KNN_ND + d] = b;
      box_lo[(int64_t)d * ntiles + tile] = a;
      box_hi[(int64_t)d * ntiles + tile] = b;
    }
  }
}

// The rows of every tile in ascending original index.  The curve sort decides WHICH 32 rows form a tile (boxes, masks and the tiles' keys
// are functions of that set); inside the tile the order is free, and this one lets the scan settle equal distances by original index where
// it finds them: the lowest of a lane's winning rows is then the one of the lowest index (k3_epilogue).  One half-wave per tile, a bitonic
// network over its 32 lanes; the last tile's missing rows sort behind the real ones and are not written.  `pack` (the database's pack,
// tile_bytes a tile; null: none): the tile's 32 indices go into its last 128 bytes, where the scan reads the low word of its atomic minimum's
// key (k3_epilogue); a padding row carries the index of the row it replicates, row n - 1 (k_knn_pack wrote them, and needed a 129th register).
__global__ __launch_bounds__(256) void k_knn_tile_order(uint32_t *__restrict__ perm, int64_t n, int64_t ntiles, uint8_t *__restrict__ pack, int tile_bytes) {
  const int i = threadIdx.x & 31;
  for (int64_t tile = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); tile < ntiles; tile += (int64_t)gridDim.x * 8) {
    const int64_t row = tile * 32 + i;
    const int real = (int)min((int64_t)32, n - tile * 32);  // rows of the tile that exist
    uint32_t v = row < n ? perm[row] : 0xFFFFFFFFu;
#pragma unroll
    for (int k = 2; k <= 32; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, j);
        v = (((i & k) == 0) == ((i & j) == 0)) ? min(v, w) : max(v, w);
      }
    if (row < n) perm[row] = v;
    if (pack) {
      const uint32_t last = (uint32_t)__shfl((int)v, real - 1, 32);
      reinterpret_cast<uint32_t *>(pack + tile * (int64_t)tile_bytes + knn_pack_indices_of(tile_bytes))[i] = row < n ? v : last;
    }
  }
}

// second-level boxes: min / max of the tile boxes over runs of KNN_GROUP tiles, per box dimension
__global__ void k_group_boxes(const int *__restrict__ box_lo, const int *__restrict__ box_hi, int64_t ntiles, int64_t ngroups, int *__restrict__ grp_lo,
                              int *__restrict__ grp_hi) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ngroups * KNN_ND; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = i / ngroups, g = i - d * ngroups;
    int a = INT_MAX, b = INT_MIN;
    for (int64_t t = g * KNN_GROUP; t < std::min<int64_t>((g + 1) * KNN_GROUP, ntiles); t++) { a = min(a, box_lo[d * ntiles + t]); b = max(b, box_hi[d * ntiles + t]); }
    grp_lo[i] = a;
    grp_hi[i] = b;
  }
}

// R of every row, R = |v - c| over the columns that are not box columns (the radial box dimension of tm_knn_kernel.h),
// and its range over the rows (floats >= 0: their bit patterns order like the values).  8 lanes per row, 48 bytes each.
__global__ __launch_bounds__(256) void k_row_radial(const int16_t *__restrict__ feat, int64_t n, CurveSpec cs, const int16_t *__restrict__ centre,
                                                    float *__restrict__ out, unsigned int *__restrict__ range /* [0] min, [1] max */,
                                                    uint2 *__restrict__ ccol /* [n]: the row's three curve columns, for k_curve_keys */) {
  // this R only places the row on the curve (the box dimension gets its exact, outward-rounded values in k_knn_pack and in the scan's
  // prologue), so single precision is enough: the lane's 24 centres live in registers and every element is one subtract and one fma
  const int j8 = threadIdx.x & 7;
  float cen[24];
#pragma unroll
  for (int e = 0; e < 24; e++) cen[e] = (float)centre[j8 * 24 + e];
  float keep[24];  // 0 for the box columns, which do not count: a factor instead of a second, dependent round of loads
#pragma unroll
  for (int e = 0; e < 24; e++) {
    keep[e] = 1.0f;
#pragma unroll
    for (int d = 0; d < KNN_NC; d++) if (cs.col[d] == j8 * 24 + e) keep[e] = 0.0f;
  }
  unsigned int lmin = 0x7f800000u, lmax = 0u;
  constexpr int RG = 4;  // row groups of 32 per workgroup pass: 12 loads of 16 bytes in flight per lane
  for (int64_t base = (int64_t)blockIdx.x * (32 * RG); base < n; base += (int64_t)gridDim.x * (32 * RG)) {
    v4i x[RG][3];
    int16_t cc[RG][3];  // lane 0 of a row: its three curve columns (the lines are the ones the row's own loads fetch)
#pragma unroll
    for (int g = 0; g < RG; g++) {
      const int64_t i = min(base + g * 32 + (threadIdx.x >> 3), n - 1);
      const v4i *rp = reinterpret_cast<const v4i *>(feat + i * 192) + j8 * 3;
#pragma unroll
      for (int v = 0; v < 3; v++) x[g][v] = rp[v];
      if (j8 == 0)
#pragma unroll
        for (int d = 0; d < 3; d++) cc[g][d] = feat[i * 192 + cs.col[d]];
    }
#pragma unroll
    for (int g = 0; g < RG; g++) {
      const int64_t i = base + g * 32 + (threadIdx.x >> 3);
      float sq = 0.0f;
#pragma unroll
      for (int v = 0; v < 3; v++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float c0 = (float)(int16_t)(x[g][v][j] & 0xffff) - cen[v * 8 + 2 * j], c1 = (float)(x[g][v][j] >> 16) - cen[v * 8 + 2 * j + 1];
          sq = fmaf(c0 * keep[v * 8 + 2 * j], c0, fmaf(c1 * keep[v * 8 + 2 * j + 1], c1, sq));
        }
      sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4);
      if (i < n && j8 == 0) {
        const float lr = sqrtf(fmaxf(sq, 0.0f));
        out[i] = lr;
        ccol[i] = make_uint2((uint32_t)(uint16_t)cc[g][0] | ((uint32_t)(uint16_t)cc[g][1] << 16), (uint32_t)(uint16_t)cc[g][2]);
        lmin = min(lmin, __float_as_uint(lr));
        lmax = max(lmax, __float_as_uint(lr));
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { lmin = min(lmin, (unsigned)__shfl_xor((int)lmin, o)); lmax = max(lmax, (unsigned)__shfl_xor((int)lmax, o)); }
  // one pair of atomics per workgroup: the two words are the same for the whole launch, and their atomics queue up one behind the other
  __shared__ unsigned int s_rng[2][4];
  if ((threadIdx.x & 63) == 0) { s_rng[0][threadIdx.x >> 6] = lmin; s_rng[1][threadIdx.x >> 6] = lmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(&range[0], min(min(s_rng[0][0], s_rng[0][1]), min(s_rng[0][2], s_rng[0][3])));
    atomicMax(&range[1], max(max(s_rng[1][0], s_rng[1][1]), max(s_rng[1][2], s_rng[1][3])));
  }
}

// Curve key (curve_key, tm_knn_kernel.h: Hilbert or Morton order of the cells), value = row index: the three widest columns quantised over
// the union range, plus the radial coordinate over ITS range, so that the rows of a tile are alike in texture energy as well as in mean
// colour -- which is what the radial box dimension needs in order to prune (30 % fewer evaluated pairs on the bench clip than a
// 3 x 10-bit curve of the columns alone).  k_cell_keys is the key alone, on cells given (tm_stage_curve_keys: the tests' way in).
__global__ void k_curve_keys(const uint2 *__restrict__ ccol /* k_row_radial's copy of the three curve columns */, int64_t n, CurveSpec cs, const float *__restrict__ radial,
                             uint32_t *__restrict__ key, uint32_t *__restrict__ idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t q[4];
    const uint2 c3 = ccol[i];
    const int cv[3] = {(int)(int16_t)(c3.x & 0xffff), (int)(int16_t)(c3.x >> 16), (int)(int16_t)(c3.y & 0xffff)};
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const float v = d < 3 ? (float)cv[d] : (cs.rlog ? log2f(radial[i] + 1.0f) : radial[i]);
      q[d] = (uint32_t)min((float)((1u << cs.bits[d]) - 1u), max(0.0f, (v - cs.off[d]) * cs.scale[d]));
    }
    key[i] = curve_key(q, cs.bits, cs.kind);
    idx[i] = (uint32_t)i;
  }
}

__global__ void k_cell_keys(const uint32_t *__restrict__ cells /* [n][4] */, int64_t n, CurveSpec cs, uint32_t *__restrict__ key) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t q[4] = {cells[i * 4], cells[i * 4 + 1], cells[i * 4 + 2], cells[i * 4 + 3]};
    key[i] = curve_key(q, cs.bits, cs.kind);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side

// log2(R + 1) per row into `radial` and the running range into ix->rrange (two uint32, reset by the caller)
static int row_radial(tm_knn_index_impl *ix, const void *feat, int64_t n, DevBuf &radial, DevBuf &ccol, hipStream_t stream) {
  TM_TRY(radial.alloc((size_t)std::max<int64_t>(n, 1) * 4));
  TM_TRY(ccol.alloc((size_t)std::max<int64_t>(n, 1) * 8));
  if (n <= 0) return TM_OK;
  hipLaunchKernelGGL(k_row_radial, dim3((unsigned)std::min<int64_t>((n + 127) / 128, 2048)), dim3(256), 0, stream, (const int16_t *)feat, n, ix->curve,
                     ix->plan_dev.as<int16_t>(), radial.as<float>(), ix->rrange.as<unsigned int>(), ccol.as<uint2>());
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_curve_keys(const uint32_t *cells, int64_t n, const int bits[4], int kind, uint32_t *keys, hipStream_t stream) {
  if (n <= 0) return TM_OK;
  CurveSpec cs = {};
  for (int d = 0; d < 4; d++) cs.bits[d] = bits[d];
  cs.kind = kind;
  hipLaunchKernelGGL(k_cell_keys, dim3(gridn(n)), dim3(256), 0, stream, cells, n, cs, keys);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// rows sorted along the curve: perm (row order) and the sorted keys
static int sort_by_curve(tm_knn_index_impl *ix, const DevBuf &ccol, int64_t n, const DevBuf &radial, DevBuf &perm, DevBuf &keys_sorted, hipStream_t stream) {
  TM_TRY(ix->skey.alloc((size_t)n * 4)); TM_TRY(ix->sidx.alloc((size_t)n * 4));
  TM_TRY(perm.alloc((size_t)n * 4)); TM_TRY(keys_sorted.alloc((size_t)n * 4));
  hipLaunchKernelGGL(k_curve_keys, dim3(gridn(n)), dim3(256), 0, stream, ccol.as<uint2>(), n, ix->curve, radial.as<float>(),
                     ix->skey.as<uint32_t>(), ix->sidx.as<uint32_t>());  // (n >= 1: no search gets here with an empty side)
  TM_TRY(with_temp(ix->sort_tmp, "knn: radix sort of the curve keys", [&](void *t, size_t &b) {
    return rocprim::radix_sort_pairs(t, b, ix->skey.as<uint32_t>(), keys_sorted.as<uint32_t>(), ix->sidx.as<uint32_t>(), perm.as<uint32_t>(), (size_t)n, 0, 32, stream);
  }));
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_tile_order(uint32_t *perm, int64_t n, hipStream_t stream, uint8_t *pack, int tile_bytes) {
  if (n <= 0) return TM_OK;
  const int64_t ntiles = knn_tiles(n);
  hipLaunchKernelGGL(k_knn_tile_order, dim3((unsigned)std::min<int64_t>((ntiles + 7) / 8, 2048)), dim3(256), 0, stream, perm, n, ntiles, pack, tile_bytes);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

static int run_pack(tm_knn_index_impl *ix, const void *feat, int64_t n, int negate, int hch, const DevBuf &perm, int with_box,
                    DevBuf &out, hipStream_t stream) {
  const int scale = negate ? 1 : ix->plan.tscale;
  const int64_t ntiles = (n + 31) / 32;
  TM_TRY(out.alloc((size_t)ntiles * knn_pack_bytes(6 + hch, with_box)));
  TM_TRY(ix->err_flag.alloc(sizeof(int)));
  if (negate) TM_TRY(ix->qmeta.alloc((size_t)std::max<int64_t>(ntiles, 1) * QMETA_INTS * 4));
  else TM_TRY(ix->thmask.alloc((size_t)std::max<int64_t>(ntiles, 1)));
  int grid = (int)std::min<int64_t>(ntiles, 4096);
  hipLaunchKernelGGL(k_knn_pack, dim3(grid), dim3(256), 0, stream, (const int16_t *)feat, n, ntiles, hch, negate, scale,
                     ix->plan_dev.as<int16_t>(), ix->plan_dev.as<int16_t>() + 192, perm.as<uint32_t>(), with_box, ix->curve,
                     ix->box_lo.as<int>(), ix->box_hi.as<int>(), out.as<uint8_t>(), ix->err_flag.as<int>(), negate ? ix->qmeta.as<int>() : nullptr,
                     negate ? nullptr : ix->thmask.as<uint8_t>());
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// the queries' column ranges: kept by their producer (query_colmm, device [384]) or computed here
static int query_ranges(tm_knn_index_impl *ix, const void *queries, int64_t nq, const void *query_colmm, ColStats *qs, hipStream_t stream) {
  if (query_colmm) return read_col_ranges(query_colmm, qs, stream);
  return col_stats(queries, nq, qs, ix->scratch, stream);
}

// exactness domain: all arithmetic is mod 2^32 and compared as signed, which needs every SSD < 2^31.  Tile features
// satisfy it by construction (<= 1.35e9); arbitrary int16 data may not.
static int check_exact_domain(const ColStats &ts, const ColStats &qs) {
  long long bound = 0;
  for (int c = 0; c < 192; c++) {
    const long long lo = std::min(ts.mn[c], qs.mn[c]), hi = std::max(ts.mx[c], qs.mx[c]);
    if (hi > lo) bound += (hi - lo) * (hi - lo);
  }
  TM_CHECK(bound < (1ll << 31) - 2, TM_E_UNSUPPORTED,
           "knn: column ranges allow an SSD of %lld >= 2^31, outside the exact domain of the int8/int32 kernel", bound);
  return TM_OK;
}

// a digit plan for the database and this batch, on the device
static int new_plan(tm_knn_index_impl *ix, const ColStats &qs, int64_t nq, hipStream_t stream) {
  TM_TRY(make_plan(ix->tstats, qs, &ix->plan));
  TM_CHECK(plan_covers(ix->plan, ix->tstats, ix->plan.ht, ix->plan.tscale) && plan_covers(ix->plan, qs, ix->plan.hq), TM_E_UNSUPPORTED,
           "knn: feature range exceeds the exact two-digit int8 split");
  if (knobs().knn_debug)
    fprintf(stderr, "[tm_knn] nq=%lld nt=%lld big columns: database %d (digits x%d), queries %d -> HT=%d HQ=%d K=%d bytes\n", (long long)nq,
            (long long)ix->nt, ix->plan.nbig_t, ix->plan.tscale, ix->plan.nbig_q, ix->plan.ht, ix->plan.hq, knn_kbytes(ix->plan));
  return upload_plan(ix, stream);
}

// The curve of an index (fixed until its plan changes): the KNN_ND widest columns of the union are the box columns, the first three
// drive the curve order; the radial coordinate of every database row and of this batch of queries is computed on the way, its range
// scales the key's radial bits.
#ifndef TM_KNN_CURVE_BITS
#define TM_KNN_CURVE_BITS 8, 7, 7, 8  // (a measuring build sets another split: tools/build_variant.sh NAME -DTM_KNN_CURVE_BITS=8,8,8,8)
#endif
static int choose_curve(tm_knn_index_impl *ix, const void *queries, int64_t nq, const ColStats &qs, hipStream_t stream) {
  CurveSpec &cs = ix->curve;
  int order[192];
  for (int c = 0; c < 192; c++) order[c] = c;
  auto urange = [&](int c) {
    const int lo = std::min(ix->tstats.mn[c], qs.mn[c]), hi = std::max(ix->tstats.mx[c], qs.mx[c]);
    return hi >= lo ? hi - lo : 0;
  };
  std::stable_sort(order, order + 192, [&](int a, int b) { return urange(a) > urange(b); });
  for (int d = 0; d < KNN_NC; d++) cs.col[d] = order[d];
  for (int d = 0; d < 3; d++) {
    const int c = order[d];
    cs.lo[d] = std::min(ix->tstats.mn[c], qs.mn[c]);
    cs.range[d] = std::max(1, urange(c));
  }
  TM_TRY(ix->rrange.alloc(8));
  const unsigned int init[2] = {0x7f800000u, 0u};
  TM_HIP(hipMemcpyAsync(ix->rrange.p, init, 8, hipMemcpyHostToDevice, stream));
  TM_TRY(row_radial(ix, ix->db, ix->nt, ix->tradial, ix->tccol, stream));
  TM_TRY(row_radial(ix, queries, nq, ix->qradial, ix->qccol, stream));
  unsigned int rr[2];
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(rr, ix->rrange.p, 8));
    TM_TRY(hr_.wait());
  }
  float rlo, rhi;
  memcpy(&rlo, &rr[0], 4); memcpy(&rhi, &rr[1], 4);
  if (!(rhi > rlo)) { rlo = 0.0f; rhi = 1.0f; }
  // Measured on the bench clip (column ranges 20262 / 13399 / 13118, R in 2566..5284): every dimension over its own range with
  // 8, 7, 7, 8 bits and log2 R -- R cells of 0.3 % -- evaluates 15.3 G pairs (scan 18.4 ms); 8, 8, 8, 8: 14.7 G but 20.0 ms;
  // isotropic cells (9, 8, 8, 6 bits, linear R): 18.6 G, 21.4 ms; columns only (10, 10, 10): 28.9 G, 30.2 ms.
  // The k-nearest scans use the same curve (measured after their kernel stopped spilling: first collection pass of the
  // extended-palette run 112 ms on this curve, 146 ms on 10, 10, 10 bits of the columns alone).
  // (Those figures are round 1's kernel on the Morton order.  DESIGN.md section 36 has the two orders on today's scan.)
  const int nb[4] = {TM_KNN_CURVE_BITS};
  cs.rlog = 1;
  cs.kind = knobs().knn_curve >= 0 ? knobs().knn_curve : ix->curve_kind;  // TM_KNN_CURVE: the nearest-neighbour search and the k-nearest collection share the curve and both follow it
  for (int d = 0; d < 3; d++) { cs.bits[d] = nb[d]; cs.off[d] = (float)cs.lo[d]; cs.scale[d] = (float)((1 << nb[d]) - 1) / (float)cs.range[d]; }
  cs.bits[3] = nb[3]; cs.off[3] = log2f(rlo + 1.0f);
  cs.scale[3] = ((float)(1 << nb[3]) - 0.001f) / std::max(1e-6f, log2f(rhi + 1.0f) - log2f(rlo + 1.0f));
  if (knobs().knn_debug)
    fprintf(stderr, "[tm_knn] curve: column ranges %d %d %d, radial %.1f..%.1f -> bits %d %d %d %d (%s, %s order)\n", cs.range[0], cs.range[1], cs.range[2], rlo, rhi,
            cs.bits[0], cs.bits[1], cs.bits[2], cs.bits[3], "own ranges, log radial", cs.kind == CURVE_HILBERT ? "Hilbert" : "Morton");
  return TM_OK;
}

// the database sorted along the curve and packed under the plan, its tiles' keys and boxes and the boxes of runs of KNN_GROUP tiles
static int build_database_side(tm_knn_index_impl *ix, hipStream_t stream) {
  const int64_t ntt = knn_tiles(ix->nt);
  TM_TRY(sort_by_curve(ix, ix->tccol, ix->nt, ix->tradial, ix->tperm, ix->skey2, stream));
  ix->tccol.release();
  ix->tradial.release();
  TM_TRY(ix->tkey.alloc((size_t)ntt * 4));
  TM_HIP(hipMemcpy2DAsync(ix->tkey.p, 4, ix->skey2.p, 128, 4, (size_t)ntt, hipMemcpyDeviceToDevice, stream));  // each tile's smallest key (the sorted keys stay in curve order)
  TM_TRY(ix->tpack.alloc((size_t)ntt * knn_pack_bytes(6 + ix->plan.ht, 1)));  // (the pack's own allocation below finds it there)
  TM_TRY(launch_tile_order(ix->tperm.as<uint32_t>(), ix->nt, stream, ix->tpack.as<uint8_t>(), knn_pack_bytes(6 + ix->plan.ht, 1)));
  TM_TRY(ix->box_lo.alloc((size_t)ntt * KNN_ND * 4));
  TM_TRY(ix->box_hi.alloc((size_t)ntt * KNN_ND * 4));
  TM_TRY(run_pack(ix, ix->db, ix->nt, 0, ix->plan.ht, ix->tperm, 1, ix->tpack, stream));
  const int64_t ng = (ntt + KNN_GROUP - 1) / KNN_GROUP;
  TM_TRY(ix->grp_lo.alloc((size_t)ng * KNN_ND * 4)); TM_TRY(ix->grp_hi.alloc((size_t)ng * KNN_ND * 4));
  hipLaunchKernelGGL(k_group_boxes, dim3((unsigned)std::min<int64_t>((ng * KNN_ND + 255) / 256, 1024)), dim3(256), 0, stream, ix->box_lo.as<int>(),
                     ix->box_hi.as<int>(), ntt, ng, ix->grp_lo.as<int>(), ix->grp_hi.as<int>());
  TM_HIP(hipGetLastError());
  ix->packed = true;
  return TM_OK;
}

int prepare_search(tm_knn_index_impl *ix, const void *queries, int64_t nq, hipStream_t stream, const void *query_colmm) {
  ColStats qs;
  TM_TRY(query_ranges(ix, queries, nq, query_colmm, &qs, stream));
  TM_TRY(ix->err_flag.alloc(sizeof(int)));
  TM_HIP(hipMemsetAsync(ix->err_flag.p, 0, sizeof(int), stream));  // both pack passes below report into it
  TM_TRY(check_exact_domain(ix->tstats, qs));
  if (!ix->packed || !plan_covers(ix->plan, qs, ix->plan.hq)) {  // a first batch, or one the kept plan cannot represent: plan and database side anew
    TM_TRY(new_plan(ix, qs, nq, stream));
    TM_TRY(choose_curve(ix, queries, nq, qs, stream));  // (leaves the queries' radial coordinates as well)
    TM_TRY(build_database_side(ix, stream));
  } else {
    TM_TRY(row_radial(ix, queries, nq, ix->qradial, ix->qccol, stream));  // a later batch on a built index (its range result is not used)
  }
  TM_TRY(sort_by_curve(ix, ix->qccol, nq, ix->qradial, ix->qperm, ix->qkey, stream));
  TM_TRY(run_pack(ix, queries, nq, 1, ix->plan.hq, ix->qperm, 0, ix->qpack, stream));
  return TM_OK;
}

}  // namespace tmx
