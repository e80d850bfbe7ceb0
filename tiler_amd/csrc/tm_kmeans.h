// tm_kmeans.h -- what the k-means files share (tm_kmeans.hip, tm_kmeans_pixel.hip, tm_palettize.hip and the three D = 192 files behind
// tm_kmeans_tile.h); nobody else includes it.  The callers' prototypes are in tm_internal.h.
#pragma once
#include <cstring>
#include <algorithm>
#include <climits>
#include <mutex>
#include <vector>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

typedef unsigned long long u64;

struct Seg {      // per segment state, device resident
  int64_t begin;  // first point
  int64_t count;  // number of points
  int kk;         // live centroids so far
  int init_done;
  int64_t cur;    // point index chosen as the newest centroid
  int changed;
  int nseg;       // element 0 only: number of segments
  int blk_first;  // 1-D grids: first workgroup of this segment and how many it owns (proportional to its size)
  int blk_count;
};

// 1-D grid -> (segment, workgroup index inside it, workgroups it owns)
__device__ __forceinline__ int find_seg(const Seg *__restrict__ segs, int &bx, int &nbx) {
  int lo = 0, hi = segs[0].nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].blk_first <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  bx = (int)blockIdx.x - segs[lo].blk_first;
  nbx = segs[lo].blk_count;
  return lo;
}

// best key: larger mindist wins, then lower index.  mindist can reach 2^38 (D=192), indices 2^31: two words.  (Wavelet features,
// DitheringMode = pvsWavelets, stay far below: |coefficient| <= 8 x the largest Lab plane magnitude, 8 x 331 < 2 650, so mindist < 2^33.)
struct BestKey { long long dist; long long negidx; };
__device__ __forceinline__ bool better(const BestKey &a, const BestKey &b) {
  return a.dist > b.dist || (a.dist == b.dist && a.negidx > b.negidx);
}

constexpr int KCH = 16;     // centroids scored per pass (register accumulators)
constexpr int H_MAXK = 64;  // centroids kept in LDS by the skipping kernels
constexpr int CU_LDS_BYTES = 160 * 1024;  // a compute unit's LDS

// ---- the barrier of the resident kernels (k_h_resident: the whole grid; k_kmeans3_persistent: the workgroups of one segment) -----------
// Arrivals are counted in eight shards (workgroup g on shard g % 8: atomics on one word take their turns, ~12 ns each); the last arrival of
// a shard adds one to each of the eight replicas of `top` (one instruction, eight lanes); a waiting workgroup polls its shard's replica
// until all shards are in (loads on one word queue up like atomics do: 32 pollers a line).  A round trip to the memory side is about a
// microsecond here, so the count of dependent ones is the barrier's price: arrival, replica add, poll.  Every word on a 128-byte line of its own.
struct alignas(128) BarrierLine { unsigned v; unsigned pad[31]; };

// No fence: everything that crosses workgroups in these kernels is an agent-scope atomic on both sides (adds and maxima, relaxed loads,
// relaxed stores to clear), every wave drains its vmcnt before its workgroup arrives, every load of the data comes behind a workgroup
// barrier behind the poll -- the hand-off form of MI355X_MICROARCH.md "Valid forms" that needs no L2 write-back and no L1 invalidate
// (1.7 us each, twice per iteration, before).  That form is not the language's release / acquire: it leans on how these two targets'
// caches treat agent-scope atomics, so another target has to be looked at before it is built for.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "the resident kernels' fence-free barrier was written for gfx942 / gfx950: check the hand-off against the new target's caches first"
#endif
// every thread of the workgroup calls it; st: the kernel's state with BarrierLine bar[8], top[8] and unsigned timeout, zeroed before the
// launch; `g` of `nblk`: the workgroup's place among those that meet; false: the spin gave up after SPIN_LIMIT polls (a workgroup is not
// resident) or another workgroup raised st->timeout, the caller leaves
template <unsigned SPIN_LIMIT, class State>
__device__ __forceinline__ bool grid_barrier(State *st, unsigned &epoch, unsigned nblk, unsigned g, int *s_ok) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's atomics and stores have been performed
  __syncthreads();
  if (threadIdx.x < 64) {
    epoch++;
    int ok = 1;
    if (nblk > 1) {
      const unsigned sh = g & 7u, nsh = nblk < 8u ? nblk : 8u;
      const unsigned mine = (nblk - sh + 7u) >> 3;  // workgroups on this shard
      bool last = false;
      if (threadIdx.x == 0) last = __hip_atomic_fetch_add(&st->bar[sh].v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == epoch * mine;
      last = __builtin_amdgcn_readfirstlane((int)last) != 0;
      if (last && threadIdx.x < 8) __hip_atomic_fetch_add(&st->top[threadIdx.x].v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // one instruction, eight lines
      if (threadIdx.x == 0)
      for (unsigned spins = 1; __hip_atomic_load(&st->top[sh].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch * nsh; spins++) {
        __builtin_amdgcn_s_sleep(1);
        if ((spins & 255u) == 0 && (spins > SPIN_LIMIT || __hip_atomic_load(&st->timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {  // (a second round trip: rarely)
          __hip_atomic_store(&st->timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = 0;
          break;
        }
      }
    }
    if (threadIdx.x == 0) *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// One resident launch at a time per process and device (see tm_kmeans.hip); held from the launch to the read-back that ends it.
std::mutex &resident_launch_lock();

inline int cu_count() {  // compute units of the current device
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}

// tm_kmeans.hip: batched k-means over nseg contiguous segments.  seg_begin / seg_count are host arrays.  Outputs assign (global point
// order), cent [nseg][k][d], host_kk[nseg] live centroid counts.  init_idx / dev_init_idx (optional, host / device): the caller's own
// initial centres instead of the farthest-first picks, k point indices per segment (relative to the segment), -1 = none.
// host_cent (optional, host, [nseg][k][d]): the centroids come to the host with the clustering's own read-back; where the clustering holds
// them on the host already (the resident pixel launch) the device copy `cent` is then NOT written: no upload, no wait for one.
int kmeans_batched(const int32_t *pts, const uint32_t *w, int d, const std::vector<int64_t> &seg_begin, const std::vector<int64_t> &seg_count, int k,
                   int max_iter, int32_t *assign, double *cent, std::vector<int> *host_kk, int *host_iters, hipStream_t stream,
                   const int64_t *init_idx = nullptr, const long long *dev_init_idx = nullptr, double *host_cent = nullptr);

// tm_kmeans_pixel.hip: the whole D = 3 clustering in resident launches; *used = 0 when the shape does not fit (the caller then takes the
// launches-per-iteration path).  host_cent: as above.
int kmeans3_persistent(const int32_t *pts, const uint32_t *w, const std::vector<int64_t> &seg_begin, const std::vector<int64_t> &seg_count, int k,
                       int max_iter, int32_t *assign, double *cent, std::vector<int> *host_kk, int *host_iters, hipStream_t stream, int *used,
                       double *host_cent = nullptr);

// ---- D = 192 (tm_kmeans_tile.h has the rules the three files share) -----------------------------------------------------------------
// tm_kmeans_assign192.hip: the plain iterations' assignment step
void launch_chunk_major(const int32_t *pts, int64_t n, int32_t *out, hipStream_t stream);  // [n][192] -> [24][n][8]

// ---- the first look of the plain iterations: decide in single precision, the double-precision chain only where in doubt ----------------
// The assignment step needs the DECISIONS of the reference's 192-term double-precision chains, not their values.  Per point p (an int32
// row) and centroid c (doubles), with c^ the Single nearest to c in every coordinate:
//   s(c)  = the Single sum over the dimensions of (float(p_j) - c^_j)^2: one subtraction and one fused multiply-add per term, in any
//           order and any number of partial sums.  Its terms are non-negative, so its relative error against the exact sum over (p_j - c^_j)^2
//           is below (2 + 192) * 2^-24 = 194 * 2^-24 when every float(p_j) is exact; the Single root adds 2^-24 and halves the rest.
//           FL_GAMMA = 2^-16 is taken as the bound on the ROOT's relative error, more than twice what it needs.
//   E(c)  = FL_CENT * |c| = 2^-23 |c| >= |c^ - c| (rounding a coordinate to Single moves it by at most 2^-24 of itself; no centroid of
//           integer rows leaves Single's normal range: a quotient of an int64 sum and a count, zero or at least 2^-64 in magnitude),
//           computed in double and rounded up.  By the triangle inequality | |p - c^| - |p - c| | <= E(c).
// The true distance d(c) therefore lies in [lo(c), hi(c)] = [sqrt(s(c)) (1 - FL_GAMMA) - E(c), sqrt(s(c)) (1 + FL_GAMMA) + E(c)].
// With c* the Single argmin, a point is DECIDED iff lo(c) (1 - KM_ETA) > hi(c*) (1 + KM_ETA) for every other c: the reference's computed
// squared distances (within 1e-13 of the true ones) are then strictly ordered the same way, no tie can occur, c* is the reference's
// answer.  Otherwise, or when some |p_j| >= 2^24 (its conversion may round), the point is IN DOUBT and goes through the chain itself:
// double, terms in order, ties to the lowest index, against all its centroids (those that are no contenders lie strictly behind c*, so
// scoring them as well changes nothing).
// Bounds for the skipping iterations: ub = hi(c*), lb = the smallest lo(c) among the others, each moved outwards by KM_ETA (the one margin, tm_kmeans_tile.h); the exact
// roots with k_assign192's own margins where the chain ran.
constexpr double FL_GAMMA = 1.0 / 65536.0;    // 2^-16
constexpr double FL_CENT = 1.0 / 8388608.0;   // 2^-23
constexpr float FL_INT_EXACT = 16777216.0f;    // 2^24: below it int32 -> Single is exact

// k_assign192's launch: slices of the largest segment sized so that one round of workgroups fills the chip evenly
struct Assign192Shape { int ppt, nblk, rows, lds_delta; size_t lds; };
Assign192Shape assign192_shape(int64_t maxcount, int nseg, int k, int cus);
// what a launch of k_assign192 works on.  ub, lb: where it leaves the bounds the skipping iterations start from, or null.  look_stats: two
// counters on the device (point-scorings looked at, those that went to the chain) the launch adds to, or null; the first look itself is taken
// unless TM_KM_FIRST_LOOK=0
struct Assign192Args {
  const int32_t *pts, *ptsc;  // rows, and the same chunk-major
  int64_t ntot;
  const uint32_t *w;
  Seg *ds;
  int k;
  const double *cent;
  int32_t *assign;
  u64 *sums, *cnts;
  const int *quiet;
  double *ub = nullptr, *lb = nullptr;
  u64 *look_stats = nullptr;
};
void launch_assign192(const Assign192Shape &sh, int nseg, hipStream_t stream, const Assign192Args &a);

// ---- tm_kmeans_resident.hip
// Would one segment of n points and k centroids go through k_h_resident on a device of `cus` compute units?  rounds == 0: no.
struct ResidentPlan { int grid, rounds; size_t lds; };
ResidentPlan resident_plan(int64_t n, int k, int cus);

// ---- tm_kmeans_skip.hip
// One clustering of one D = 192 segment with at most H_MAXK centroids, as kmeans_batched hands it to the skipping iterations: after
// H_WARM plain iterations the assignment step only touches the points whose bounds do not prove their assignment.
constexpr int H_WARM = 5;
struct TileRun {
  const int32_t *pts, *ptsc;  // rows, and the same chunk-major
  const uint32_t *w;
  int64_t n;
  int k, max_iter;
  Seg *ds;
  double *cent;
  int32_t *assign;
  u64 *sums, *cnts;
  int *quiet;
  u64 *look = nullptr;  // the first look's two counters (launch_assign192)
  Assign192Shape a192;
  hipStream_t stream;
  // the skipping iterations' own state (tile_skip_setup)
  DevBuf ub, lb, cent_t, move, half, need, cnt;
  int kt;        // row pitch of the transposed centroids (cent_t)
  Assign192Args assign192_args(double *ub_out = nullptr, double *lb_out = nullptr) const { return {pts, ptsc, n, w, ds, k, cent, assign, sums, cnts, quiet, ub_out, lb_out, look}; }
};
int tile_skip_setup(TileRun &t);
void tile_skip_iteration(TileRun &t, int iter, int *pin_dev);  // iteration `iter` (plain below H_WARM) and its update
// tm_kmeans_resident.hip again, on a TileRun:
enum class Resident { done, gave_up, not_applicable };
// the H_WARM plain iterations, then all skipping iterations in one launch of k_h_resident; done: *iters is set.  host_seg / host_look
// (optional): the segment's table entry and the first look's two counters as the launch leaves them, fetched with the launch's own read-back
int tile_resident(TileRun &t, const ResidentPlan &plan, Resident *verdict, int *iters, Seg *host_seg = nullptr, u64 *host_look = nullptr);

}  // namespace tmx
