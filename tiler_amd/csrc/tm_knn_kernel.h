// tm_knn_kernel.h -- what the KNN stage's kernels and its host code share (see tm_knn.hip for the scheme, tm_knn3.h for the scan).
#pragma once
#include <climits>
#include <cstdint>
#include <type_traits>

#include "tm_common.h"

namespace tmx {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Database tiles (32 rows): [6 low chunks | HT high chunks] x [64 lanes] x 16 B, then 32 u32 norms |t-c|^2, then the tile's box.
// Query tiles (32 queries): [6 low chunks | HQ high chunks] of the NEGATED centred values, then 32 u32 (|q-c|^2 >> 1).
// Columns are permuted so that the columns carrying a high digit are a prefix on each side (nested sets), widest first.
//   X = 65536 T_H . Q_H (m = min(HT, HQ) chunks) + 256 (T_L[:HQ] . Q_H + T_H . Q_L[:HT]) + T_L . Q_L (6 chunks)
//   d''  = |t-c|^2 + 2 X + 2 (|q-c|^2 >> 1) = SSD - (|q-c|^2 & 1), exact mod 2^32.
//
// Pruning.  Both sides arrive sorted along a space-filling curve (curve_key below: Hilbert by default) of the three widest feature columns (the Y/U/V DC terms for tile features) and
// the radial coordinate below, so 32 consecutive rows form a compact box.  For ND dimensions the database keeps per-tile bounding boxes
// (and boxes of runs of KNN_GROUP tiles); the squared box-to-box distance is a lower bound of every SSD between a query sub-tile's
// queries and a tile's rows.  Exactness: the minimum VALUE is exact (a tile is only skipped when bound > best + 1), and a row that
// only ties a best is never skipped either: the scan's atomic minimum, keyed by (value, original index), settles the lowest-index rule.
constexpr int KNN_NC = 6;        // bounding-box columns
// One more box dimension, radial: R = |v - c| over all the OTHER columns.  |R(q) - R(t)|^2 <= the squared distance over those
// columns (reverse triangle inequality), so its gap adds to the lower bound like a column's; it tells a noisy tile from a smooth
// one of the same mean colour, which the widest (low-frequency) columns cannot.  Stored as integers rounded outwards.
constexpr int KNN_ND = KNN_NC + 1;
constexpr int KNN_GROUP = 128;   // tiles per second-level box

struct KnnBoxes {
  const int *lo, *hi;   // [KNN_ND][n_ttiles] bounding boxes of the database tiles
  const int *glo, *ghi; // [KNN_ND][ceil(n_ttiles / KNN_GROUP)] boxes of runs of KNN_GROUP tiles: a run no sub-tile can use is skipped whole
  const uint32_t *tkey; // [n_ttiles] each tile's smallest curve key: that of its first row in curve order (ascending)
  int col[KNN_NC];      // source feature column of each box dimension
  int cen[KNN_NC];      // the digit plan's centre of that column (the radial dimension is measured from the centres)
};

constexpr int CURVE_MORTON = 0, CURVE_HILBERT = 1;  // CurveSpec::kind (TM_KNN_CURVE)

// where a row lies on the space-filling curve both sides are sorted along (k_row_radial, k_curve_keys), and the box columns (k_knn_pack)
struct CurveSpec {
  int col[KNN_NC];
  int lo[3], range[3];      // the three curve columns: union range
  float scale[4], off[4];   // quantised coordinate of dimension d (three columns, radial) = (value - off) * scale, clamped to its bits
  int bits[4];
  int rlog;                 // radial coordinate taken as log2(R + 1) instead of R
  int kind;                 // CURVE_MORTON or CURVE_HILBERT: how curve_key orders the cells
};

// The key of the cell q (q[d] < 2^bits[d]) on the curve; both sides are sorted by it, and nothing downstream reads more from a key than its
// order (the sort, the copies tkey / qkey, the binary searches of k_knn_qmeta and k_topk_tau).
//   CURVE_MORTON   the coordinates' bits interleaved from the top: bit b of every dimension that has more than b bits, b descending, so a
//                  dimension with more bits splits first.  One step in 16 along this order crosses a 2^4-cell boundary, one in 256 the next
//                  level's, and a run of 32 rows that straddles such a jump gets a box that spans both sides of it.
//   CURVE_HILBERT  the Hilbert index of the cell on a grid of B = max(bits) bits per axis, by Skilling's transpose form (J. Skilling,
//                  "Programming the Hilbert curve", AIP Conf. Proc. 707, 2004: axes to transposed index, then the interleave).  An axis
//                  with fewer bits is shifted left by B - bits[d]: its resolution stays what it is, the key has 4 B bits (B <= 8).
//                  Consecutive cells of this order are always neighbours: one step on one axis.
__host__ __device__ inline uint32_t curve_key(const uint32_t q[4], const int bits[4], int kind) {
  uint32_t k = 0;
  if (kind == CURVE_MORTON) {
    for (int b = 15; b >= 0; b--)
#pragma unroll
      for (int d = 0; d < 4; d++)
        if (bits[d] > b) k = (k << 1) | ((q[d] >> b) & 1u);
    return k;
  }
  int nb = 1;
#pragma unroll
  for (int d = 0; d < 4; d++) nb = bits[d] > nb ? bits[d] : nb;
  uint32_t x[4];
#pragma unroll
  for (int d = 0; d < 4; d++) x[d] = q[d] << (nb - bits[d]);
  const uint32_t top = 1u << (nb - 1);
  for (uint32_t bit = top; bit > 1; bit >>= 1) {  // inverse undo
    const uint32_t low = bit - 1;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      if (x[d] & bit) x[0] ^= low;  // invert the low bits of axis 0
      else { const uint32_t t = (x[0] ^ x[d]) & low; x[0] ^= t; x[d] ^= t; }  // exchange the low bits of axes 0 and d
    }
  }
#pragma unroll
  for (int d = 1; d < 4; d++) x[d] ^= x[d - 1];  // Gray encode
  uint32_t t = 0;
  for (uint32_t bit = top; bit > 1; bit >>= 1)
    if (x[3] & bit) t ^= bit - 1;
#pragma unroll
  for (int d = 0; d < 4; d++) x[d] ^= t;
  for (int b = nb - 1; b >= 0; b--)  // the transposed index read out: axis 0 carries the highest bit of every group of four
#pragma unroll
    for (int d = 0; d < 4; d++) k = (k << 1) | ((x[d] >> b) & 1u);
  return k;
}

}  // namespace tmx
