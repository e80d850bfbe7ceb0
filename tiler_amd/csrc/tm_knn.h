// tm_knn.h -- what the KNN stage's host files share (tm_knn.hip, tm_knn_plan.hip, tm_knn_prepare.hip, tm_knn_topk.hip); nobody else
// includes it.  The callers' prototypes are in tm_internal.h, the kernels' argument structs and the layouts both sides agree on in
// tm_knn_kernel.h and tm_knn3.h (the packed tile: knn_pack_bytes and its parts).
#pragma once
#include <cstring>

#include <algorithm>
#include <climits>
#include <cstdlib>

#include "tm_common.h"
#include "tm_internal.h"
#include "tm_knn_kernel.h"
#include "tm_knn3.h"

namespace tmx {

struct ColStats { int mn[192], mx[192]; };  // per-column range of one side's rows (mn > mx: no rows)

struct KnnPlan {
  int ht = 6, hq = 6;     // 32-column chunks that carry a high digit on the database / query side (0..6)
  int16_t centre[192];    // per source column
  int16_t perm[192];      // packed position -> source column (columns with high digits first, nested sets)
  int nbig_t = 192, nbig_q = 192;
  int tscale = 1;         // database digits are those of tscale * (t - c): 2 lets the scan's chain deliver 2 X without a final doubling
};
inline int knn_kbytes(const KnnPlan &p) { return 192 + 32 * (p.ht + p.hq + std::min(p.ht, p.hq)); }  // K of the distance GEMM

// what the last nearest-neighbour search's counters said (K3Counters, read once per attempt)
struct KnnCounts {
  unsigned long long blocks = 0, tiles = 0, pairs = 0;           // the consume kernel's
  unsigned long long seed_blocks = 0, seed_tiles = 0, seed_pairs = 0;  // the seed kernel's, summed over its stripes
  unsigned long long listed = 0, popped = 0, cursor = 0;         // list entries written / taken off / asked of the arena
  unsigned long long stopped = 0, stopped_pairs = 0;             // blocks the first-chunk look stopped, and their pairs
  unsigned long long nosurv = 0, pushed = 0, ringfull = 0, whole = 0;      // popped tiles none of whose blocks got past its look; survivor entries queued / turned away by the full ring
  unsigned long long mfma = 0, guard = 0;
  unsigned long long stamps[6] = {}, stamps_in[3] = {}, seed_stamps[7] = {};  // a diagnostic build's (TM_KNN3_STAMPS)
};

struct tm_knn_index_impl {
  const int16_t *db = nullptr;  // borrowed, like ann_kdtree_create borrows its rows (tilingencoder.pas:4600, 4615-4624)
  int64_t nt = 0;
  ColStats tstats;
  KnnPlan plan;
  bool packed = false;
  DevBuf tpack, qpack, plan_dev, scratch, best_key, best_tile, err_flag;
  DevBuf tperm, tkey, box_lo, box_hi, grp_lo, grp_hi;  // database sorted along the curve, per-tile boxes, boxes of runs of KNN_GROUP tiles
  DevBuf qperm, qkey, skey, skey2, sidx, sort_tmp;  // queries sorted along the curve
  DevBuf rrange, tradial, qradial;                  // radial coordinate of the rows (curve key) and its range
  CurveSpec curve;
  int curve_kind = CURVE_HILBERT;                   // the order an index takes where TM_KNN_CURVE is not set (choose_curve)
  DevBuf counters;                                  // one K3Counters (tm_knn3.h)
  DevBuf tccol, qccol;                              // the rows' three curve columns (k_row_radial -> k_curve_keys)
  DevBuf qmeta;                                     // per query sub-tile: box, home tile, high-chunk mask
  // third scan shape: what the seed kernel leaves for the other two (bests, bounds) and the groups' tile lists
  DevBuf gbest, gsmax, segs, nsegs, arena_tile, arena_lb;
  DevBuf thmask;                                    // per database tile: which of its high-digit chunks are not all zero
  uint64_t arena_cap = 0, arena_want = 0;           // list entries the arena holds / the largest cursor a search has reported
  hipEvent_t ev_seed = nullptr, ev_lists = nullptr;
  double last_seed_ms = 0, last_lists_ms = 0, last_consume_ms = 0;
  int64_t last_blocks = 0, last_loads = 0, last_listed = 0, last_popped = 0;
  double last_ms = 0;
  int last_kbytes = 0;
  int64_t last_pairs = 0, last_seed_pairs = 0, last_mfma = 0;
  int64_t last_consume_tiles = 0, last_no_survivor = 0, last_pushed = 0, last_ring_full = 0, last_whole = 0, last_completed = 0;  // the consume kernel's survivor queue (tm_knn3.h)
  int64_t last_chunk_looked = 0, last_chunk_stopped = 0, last_stopped_pairs = 0;  // listed blocks judged on their first chunk, and those it stopped
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  K3Counters *dev_counters() const { return counters.as<K3Counters>(); }  // (a device address: only its members' addresses are taken on the host)
  ~tm_knn_index_impl() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_seed) (void)hipEventDestroy(ev_seed);
    if (ev_lists) (void)hipEventDestroy(ev_lists);
  }
};

inline int64_t knn_tiles(int64_t rows) { return (rows + 31) / 32; }

// tm_knn_plan.hip: column ranges and the digit plan
int read_col_ranges(const void *dev_ranges /* [384]: 192 minima, 192 maxima */, ColStats *out, hipStream_t stream);
int col_stats(const void *feat, int64_t n, ColStats *out, DevBuf &scratch, hipStream_t stream);
int make_plan(const ColStats &ts, const ColStats &qs, KnnPlan *plan);
bool plan_covers(const KnnPlan &plan, const ColStats &st, int hch, int scale = 1);
int upload_plan(tm_knn_index_impl *ix, hipStream_t stream);

// tm_knn_prepare.hip: everything a search needs before the scan -- digit plan (database repacked if the batch widens it), both sides
// sorted along the curve and packed in MFMA fragment order
int prepare_search(tm_knn_index_impl *ix, const void *queries, int64_t nq, hipStream_t stream, const void *query_colmm = nullptr);

// tm_knn.hip: the scan's host side, shared by the nearest-neighbour search and the collection passes of tm_knn_topk.hip
KnnBoxes knn_boxes(const tm_knn_index_impl *ix);
int launch_qmeta(tm_knn_index_impl *ix, int64_t nqt, int64_t ntt, const KnnBoxes &bx, hipStream_t stream);
// the part of the scan's arguments both modes share, from the index as it stands (ns: sub-tiles per group of the mode)
int scan_args(tm_knn_index_impl *ix, int64_t nq, int ns, Knn3Args *a);
int ensure_list_buffers(tm_knn_index_impl *ix, Knn3Args *a);
int ensure_arena(tm_knn_index_impl *ix, double factor, Knn3Args *a);
int arena_overflowed(tm_knn_index_impl *ix, unsigned long long cursor, int attempt);
int scan_grid_blocks(int64_t units);
int launch_collect(tm_knn_index_impl *ix, const Knn3Args &a, hipStream_t stream);

// tm_knn3_lists.hip: the lists kernel and the collection mode's bounds
int launch_tau_bounds(const Knn3Args &a, hipStream_t stream);
int launch_lists(const Knn3Args &a, hipStream_t stream);

}  // namespace tmx
