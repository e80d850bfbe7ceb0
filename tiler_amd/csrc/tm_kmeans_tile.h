// tm_kmeans_tile.h -- what the three D = 192 files share (tm_kmeans_assign192.hip, tm_kmeans_skip.hip, tm_kmeans_resident.hip); nobody else
// includes it.  Every rule the skipping iterations' bit-exactness rests on is stated here once: the margins and the bound rules (the
// first look's rule is in tm_kmeans.h).  What the other k-means files call of these three is in tm_kmeans.h.
#pragma once
#include "tm_kmeans.h"

namespace tmx {

constexpr int T_ROW = 193;  // a centroid's row of carried sums in LDS: 192 sums and the count (as doubles, in k_h_update: an odd pitch)

// the most dynamic LDS a kernel here asks for: the CU's, less what the kernels keep as static arrays
constexpr size_t DYN_LDS_CEILING = (size_t)CU_LDS_BYTES - 2048;

// ---- iterations that skip what cannot change (Hamerly's bounds, made exact) ---------------------------------------------------------
// After a few full iterations most tiles sit firmly in their cluster and the centroids barely move, yet the assignment step costs
// the same 16 x 192 double-precision distance terms per tile every time.  Per point two Euclidean bounds are kept: ub >= its distance
// to its own centroid, lb <= its distance to every other one; a centroid update moves them by the centroids' displacements.  While
//      ub < max(lb, half the distance from the own centroid to the nearest other one)
// holds WITH a relative margin of KM_ETA on both sides, the own centroid is strictly the nearest by a margin six orders of magnitude above
// the rounding of the distance arithmetic (192 fused multiply-adds: relative error below 1e-13) and of the bound bookkeeping (every
// step rounds the safe way, with margins of H_ROOT), so the assignment the full computation would make -- computed distances, ties to
// the lowest index -- is the one the point already has: it is skipped.  Otherwise the distance to the own centroid is computed
// (tightening ub), and if the test still fails the point is listed and goes through k_assign192 itself, which reads its rows through the list.
// The result is therefore bit for bit that of the plain iterations (and of the oracle); only the work differs.
constexpr double KM_ETA = 1e-9;    // the margin of every comparison that decides: the skip test, the first look; and of what is computed of the centroids alone
constexpr double H_ROOT = 1e-12;   // a root of a summed distance, moved outwards: far above the sum's own error, 2.2e-14 whatever the order of its terms
constexpr double H_STEP = 1e-15;   // a bound moved by a displacement, rounded outwards: nine roundings of an addition

// the skip test: the bounds prove that the point stays with its centroid (`half`: half the distance from it to the nearest other one).
// (A macro: as an inlined function the operands are all read before the first product, and that order reaches the schedules of k_h_bounds and
// k_h_resident.)
#define H_PROVEN(u, half, l) ((u) * (1.0 + KM_ETA) < fmax((half), (l)) * (1.0 - KM_ETA))
// bounds from a chain's sums: ub from the smallest (or from the sum to the own centroid, the recheck's), lb from the second smallest
__device__ __forceinline__ double h_ub_of_sum(double sum) { return sqrt(sum) * (1.0 + H_ROOT); }
__device__ __forceinline__ double h_lb_of_sum(double sum2) { return sqrt(sum2) * (1.0 - H_ROOT); }
// bounds moved by the centroids' displacements: the own one's loosens ub; lb bounds the OTHER centroids, so the largest displacement loosens
// it, or the second largest where the own centroid is the largest mover.  Not yet rounded: h_round_up / h_round_down for bounds kept as
// doubles, the resident kernel's hr_up / hr_down for its Singles.
__device__ __forceinline__ double h_ub_moved(double u, double own_move) { return u + own_move; }
__device__ __forceinline__ double h_lb_moved(double l, bool own_moved_most, double dmax, double dmax2) { return l - (own_moved_most ? dmax2 : dmax); }
__device__ __forceinline__ double h_round_up(double x) { return x * (1.0 + H_STEP); }       // (x >= 0)
__device__ __forceinline__ double h_round_down(double x) { return x - fabs(x) * H_STEP; }
// of the centroids alone: a displacement from its squared length, rounded up; half the distance to the nearest other centroid from the
// smallest squared distance (its bit pattern: the kernels take the minimum with integer atomics), rounded down.
// (The sums behind both only feed the bounds, with margins of KM_ETA: their order is free.)
__device__ __forceinline__ double h_displacement(double sum) { return sqrt(sum) * (1.0 + KM_ETA); }
__device__ __forceinline__ double h_half_distance(unsigned long long min_sum_bits) { return 0.5 * sqrt(__longlong_as_double((long long)min_sum_bits)) * (1.0 - KM_ETA); }
constexpr double H_ALONE = 1.0e300;  // the half-distance of the only centroid

}  // namespace tmx
