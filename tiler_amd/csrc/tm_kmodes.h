// tm_kmodes.h -- what the k-modes files share (tm_kmodes.hip, tm_kmodes_init.hip, tm_kmodes_iter.hip; the map is at the head of
// tm_kmodes.hip); nobody else includes it.  The callers' prototype is in tm_internal.h.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

typedef unsigned long long u64;
constexpr int KM_ATTRS = 80, KM_WORDS = 20;
// the shape experiments of tools/build_variant.sh: how many owners share the clusters, how many of their keys the walker asks for at once
#ifndef TM_KM_OWNERS
#define TM_KM_OWNERS 64
#endif
#ifndef TM_KM_WALKER_BATCH
#define TM_KM_WALKER_BATCH 64
#endif
constexpr int KM_BIN = 960, KM_WT = 1024, KM_MAX_OWNERS = TM_KM_OWNERS, KM_STAGE = 768;
constexpr int KM_MLIST_CAP = 2 * KM_BIN + 8;  // a bin's move list: every point may move and every move may be followed by a repair
constexpr int KM_FAST_STOPS = 4;              // stops of the fast leg in one iteration before the bin-by-bin launches finish it

__device__ __forceinline__ unsigned km_dissim(const uint32_t *__restrict__ a, const uint32_t (&b)[KM_WORDS]) {
  unsigned sad = 0, zero_bytes = 0;
#pragma unroll
  for (int w = 0; w < KM_WORDS; w++) {
    const uint32_t x = a[w], y = b[w];
    sad = __builtin_amdgcn_sad_u8(x, y, sad);
    const uint32_t d = x ^ y;
    // 0x80 in every byte of d that is zero
    zero_bytes += __builtin_popcount(~(((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d | 0x7f7f7f7fu));
  }
  return sad + ((unsigned)(KM_ATTRS - zero_bytes) << 11);  // at most 80 * (255 + 2048): 32 bits are plenty
}

// row i of `rows` (80 bytes, 16-byte aligned) into twenty registers by five 16-byte loads
__device__ __forceinline__ void km_load_row(uint32_t (&p)[KM_WORDS], const uint32_t *__restrict__ rows, int64_t i) {
#pragma unroll
  for (int w = 0; w < KM_WORDS; w += 4) {
    const uint4 v = *reinterpret_cast<const uint4 *>(rows + i * KM_WORDS + w);
    p[w] = v.x; p[w + 1] = v.y; p[w + 2] = v.z; p[w + 3] = v.w;
  }
}

__host__ __device__ inline uint32_t rand_int(uint32_t range, uint32_t &seed) {  // kmodes.pas:88-92
  seed = (uint32_t)((int32_t)(seed * 0x08088405u) + 1);
  return (uint32_t)(((uint64_t)seed * (uint64_t)range) >> 32);
}

// ---- an owner's best (distance, cluster) for a point as one word, so that the walker's minimum over the owners' words is the reference's
// arg-min: the smallest distance, and among equal distances the LAST cluster (kmodes.pas:272, 414)
constexpr int KM_CLUSTER_BITS = 12, KM_MAX_CLUSTERS = 1 << KM_CLUSTER_BITS;
static_assert(KM_ATTRS * (255 + 2048) < (1 << 20), "a distance has at most 20 bits");
static_assert(20 + KM_CLUSTER_BITS <= 32, "distance and cluster share one 32-bit key");
__device__ __forceinline__ unsigned km_key_pack(unsigned distance, int cluster) { return (distance << KM_CLUSTER_BITS) | (unsigned)(KM_MAX_CLUSTERS - 1 - cluster); }
__device__ __forceinline__ unsigned km_key_distance(unsigned key) { return key >> KM_CLUSTER_BITS; }
__device__ __forceinline__ int km_key_cluster(unsigned key) { return KM_MAX_CLUSTERS - 1 - (int)(key & (unsigned)(KM_MAX_CLUSTERS - 1)); }

// ---- the clustering's state lives in HBM: memberships, member counts, the per-(cluster, attribute) histograms of
// MovePointCat (k x 80 x num_modalities counters), the modes, the LCG's seed, the iteration's cost and move counters
struct KmState {
  int32_t *memb, *clust;      // [n]
  unsigned *dis;              // [n]
  int32_t *members;           // [k]
  int32_t *freq;              // [k][80][nmod]
  uint8_t *cent;              // [k][80]
  uint32_t *seed;             // [1]
  unsigned long long *cost;   // [1] of the running iteration
  unsigned *moves;            // [1]
  int3 *mlist;                // the bin's moves in order: (point, to, from), at most KM_MLIST_CAP
  unsigned *nmoves;           // [1]
  int *bad;                   // [1] set when something that cannot happen did (no donor for a repair)
};
// the scalars KmState points at, one block the host reads back after every iteration
struct KmScalars {
  uint32_t seed;
  uint32_t mode_words_changed;  // counted by a TM_KM_COUNT_MODE_CHANGES build only
  unsigned long long cost;      // cost and moves are the iteration's: cleared together before each
  unsigned moves, nmoves;
  int bad;
};
static_assert(offsetof(KmScalars, seed) == 0, "km_scalars finds the block through KmState::seed");
static_assert(offsetof(KmScalars, moves) == offsetof(KmScalars, cost) + sizeof(unsigned long long), "cost and moves are cleared by one memset");
__host__ __device__ inline KmScalars *km_scalars(const KmState &st) { return reinterpret_cast<KmScalars *>(st.seed); }

// the two bin numbers that pass between the fast leg, the host and the iteration's graph
struct KmHandover {
  long long fast_stop;    // k_kmodes_fast: the first bin it did not walk
  long long graph_start;  // the bin the graph's work starts at (its launches for earlier bins return at once); 0 between iterations
};

// ---- k_kmodes_owner's dynamic LDS, in 4-byte words, for k clusters dealt to G owners: the kernel carves it, the host sizes it
struct KmOwnerLds {
  int max_own;  // clusters of the owner that holds most: w, w + G, w + 2 G, ...
  __host__ __device__ KmOwnerLds(int k, int G) : max_own((k + G - 1) / G) {}
  __host__ __device__ int mode() const { return 0; }                                         // uint32_t [max_own][20]: the owned modes
  __host__ __device__ int touch() const { return max_own * KM_WORDS; }                       // int [max_own]: a move of the previous bin enters or leaves the cluster
  __host__ __device__ int rel() const { return touch() + max_own; }                          // int3 [KM_MLIST_CAP]: those moves, in order
  __host__ __device__ int rows() const { return (rel() + 3 * KM_MLIST_CAP + 3) & ~3; }       // uint4 [KM_STAGE][5]: their points' rows
  __host__ __device__ size_t bytes() const { return (size_t)rows() * 4 + (size_t)KM_STAGE * KM_ATTRS; }
};

// ---- a histogram row (the nmod <= 256 counters of one (cluster, attribute) pair) held by a wave, four entries per lane: entry = lane + 64 slot
__device__ __forceinline__ void km_hist_load(int (&t)[4], const int32_t *freq, int64_t pair, int nmod, int lane) {
#pragma unroll
  for (int sl = 0; sl < 4; sl++) t[sl] = lane + 64 * sl < nmod ? freq[pair * nmod + lane + 64 * sl] : 0;
}
__device__ __forceinline__ void km_hist_store(int32_t *freq, int64_t pair, const int (&t)[4], int nmod, int lane) {
#pragma unroll
  for (int sl = 0; sl < 4; sl++) if (lane + 64 * sl < nmod) freq[pair * nmod + lane + 64 * sl] = t[sl];
}
// GetMaxValueIndex (kmodes.pas:155-167): the FIRST largest counter of the row, the same in every lane; `unique` (optional): no other
// counter equals it.  The wave's largest value by a butterfly of values alone, then a ballot per slot of who holds it: the entries ascend
// with the slot and, inside a slot, with the lane, so the first holder is the lowest lane of the lowest slot that has one.
__device__ __forceinline__ int km_first_largest(const int (&t)[4], int nmod, int lane, bool *unique = nullptr) {
  int mx = INT_MIN;
#pragma unroll
  for (int s = 0; s < 4; s++) if (lane + 64 * s < nmod) mx = max(mx, t[s]);
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  int first = 0, holders = 0;
#pragma unroll
  for (int s = 3; s >= 0; s--) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(lane + 64 * s < nmod && t[s] == mx);
    if (m) first = 64 * s + __builtin_ctzll(m);
    holders += __popcll(m);
  }
  if (unique) *unique = holders == 1;
  return first;
}

// ---- host side: one call's problem and everything it keeps on the device (tm_kmodes.hip allocates and fills it once)
struct KmBuffers {
  const uint8_t *rows;  // [n][80]
  int64_t n, nbins;
  int k, nmod;
  int G;                // owners: clusters dealt round-robin
  int ff_blocks;        // k_kmodes_ff's grid
  hipStream_t stream;
  DevBuf clust, dis, memb, members, freq, cent, scal, mlist;  // what st points at
  DevBuf used, mind, ff_partial, which;                       // farthest-first: picked points, min-distances, a candidate per block, the k picks
  std::vector<u64> ff_partial_host;                           // the last two as the host sees them; which_host is read by an
  std::vector<int64_t> which_host;                            // asynchronous copy: initial_assignment's end waits for it
  DevBuf keys;                                                // [G][KM_BIN] the owners' keys for the walker
  DevBuf handover;                                            // KmHandover
  DevBuf best_memb, best_cent;                                // the run's best iteration
  KmState st;
  KmHandover *hand() const { return static_cast<KmHandover *>(handover.p); }
  int alloc(const uint8_t *rows_, int64_t n_, int k_, int nmod_, hipStream_t stream_);
};

// tm_kmodes_init.hip
int validate_values(const KmBuffers &b);                     // launch only: st.bad = 1 when a byte of the rows is not below nmod
int score_prepare(int k);                                    // once per call, before the first score
int score(const KmBuffers &b, int64_t first, int64_t last);  // clust / dis of points [first, last) against the modes as they stand
int farthest_first(KmBuffers &b, int64_t start);             // InitFarthestFirst from point `start`: the k picked rows are the modes
int initial_assignment(const KmBuffers &b);                  // memberships, counts, histograms and modes from the first scores; waits for them

// tm_kmodes_iter.hip
// One iteration bin by bin is 2 * bins + 1 dependent launches with the same arguments every time: a graph, built once per call and replayed
// (the host's share of a launch is then paid once, not 3 400 times per iteration)
class IterGraph {
 public:
  IterGraph() = default;
  IterGraph(const IterGraph &) = delete;
  IterGraph &operator=(const IterGraph &) = delete;
  ~IterGraph();
  int build(const KmBuffers &b);
  int launch_from(const KmBuffers &b, int64_t bin);  // the iteration from bin `bin` on; bin > 0: no move is pending (the fast leg left none)
 private:
  hipGraph_t g = nullptr;
  hipGraphExec_t exec = nullptr;
};
// k_kmodes_fast from bin `bin` on (the points behind it scored already); *stop = the first bin it did not walk
int fast_leg(const KmBuffers &b, int64_t bin, int64_t *stop);

}  // namespace tmx
