// tm_knn.hip -- exact nearest-neighbour search of int16[192] tile features as an int8 MFMA distance GEMM.
//
// Replaces ann_kdtree_short_{create,search} (extern.pas:182-184) as used by PrepareReconstruct (tilingencoder.pas:
// 4566-4613) and TFrame.Reconstruct.DoXY (1534-1557): for every query row find the database row minimising
// CompareEuclideanDCTPtr (utils.pas:541-557).  Brute force, bit-exact, ties -> lowest database index.
//
// Scheme (DESIGN.md "KNN"):
//   SSD(q,t) = |q-c|^2 + |t-c|^2 - 2 (q-c).(t-c) for any per-column centre c.  On each SIDE (database, queries) a
//   column whose centred values stay within +-127 fits one int8 digit; the others ("big": data dependent, DC/low
//   frequencies for source tiles, many more for dithered tiles) get a balanced base-256 split v = 256 h + l.  Columns
//   are permuted so each side's big columns are a prefix (the smaller set nested in the larger), HT / HQ chunks of 32:
//      X = 65536 * (T_H . Q_H)[:min] + 256 * (T_L[:HQ] . Q_H + T_H . Q_L[:HT]) + T_L . Q_L
//   = three int32 MFMA accumulators fed by v_mfma_i32_32x32x32_i8, K = 192 + 32 (HT + HQ + min(HT,HQ)) <= 768 bytes.
//   The query digits are stored NEGATED, so one lane computes, with nq2 = 2 * (|q-c|^2 >> 1),
//      d'' = |t-c|^2 + 2 * (acc2<<16 + acc1<<8 + acc0) + nq2  ==  SSD - (|q-c|^2 & 1)   (exact mod 2^32, SSD < 2^31)
//   with three v_lshl_add_u32 + one add per element, and keeps a running (min d'', lowest original index) per query.  Database
//   rows ride the MFMA A operand (accumulator rows), queries the B operand (accumulator columns = lanes), so the argmin of a
//   query never leaves its lane until the 64-bit atomic minimum where the half-waves, the waves and the seeds meet.  A second
//   tiny kernel puts (index, error) back in the caller's order.
//
// Files: tm_knn_plan.hip (column ranges, digit plan), tm_knn_prepare.hip (curve order, packs, boxes), this file (the index, the scan's
// host side, the nearest-neighbour search), tm_knn_topk.hip (the k nearest rows); tm_knn.h is what the four share.  The scan's kernels:
// tm_knn3.h (what they share with the host), tm_knn3_lists.hip and tm_knn3_k<HT>.hip.
#include <atomic>

#include "tm_knn.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// What the scan leaves per sorted query -- d'' = SSD - (|q-c|^2 & 1) and the winner's ORIGINAL index, equal distances already settled to the
// lowest one inside the scan (k3_epilogue) -- back in the caller's order, the parity put back.
__global__ __launch_bounds__(256) void k_knn_refine(int64_t nq, const uint32_t *__restrict__ qperm, const uint8_t *__restrict__ qpack, int q_bytes,
                                                    const int *__restrict__ best_key, const int *__restrict__ best_idx,
                                                    int *__restrict__ out_idx, uint32_t *__restrict__ out_err) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nq; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t nqv = reinterpret_cast<const uint32_t *>(qpack + (p >> 5) * (int64_t)q_bytes + knn_pack_row_terms_of(q_bytes))[p & 31];
    const int64_t q = qperm[p];
    out_idx[q] = best_idx[p];
    out_err[q] = (uint32_t)best_key[p] + (nqv & 1u);
  }
}

// per query sub-tile: the database tile its first query falls into on the curve (the sub-tile's box is written by k_knn_pack)
__global__ __launch_bounds__(256) void k_knn_qmeta(const uint32_t *__restrict__ qkey, int64_t n_qtiles, KnnBoxes bx, int64_t n_ttiles, int *__restrict__ qmeta) {
  for (int64_t st = (int64_t)blockIdx.x * 256 + threadIdx.x; st < n_qtiles; st += (int64_t)gridDim.x * 256) {
    const uint32_t k0 = qkey[st * 32];  // last tile whose first key <= the sub-tile's first key
    int64_t lo = 0, hi = n_ttiles;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (bx.tkey[mid] <= k0) lo = mid + 1; else hi = mid; }
    qmeta[qmeta_at(st, QMETA_HOME)] = (int)max((int64_t)0, lo - 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side: the index

int knn_index_create(const void *db, int64_t nt, hipStream_t stream, tm_knn_index_impl **out) {
  TM_TRY(require_device());
  TM_CHECK(nt >= 0, TM_E_INVAL, "knn: negative row count");
  auto *ix = new tm_knn_index_impl();
  ix->db = (const int16_t *)db;
  ix->nt = nt;
  int rc = col_stats(db, nt, &ix->tstats, ix->scratch, stream);
  if (rc == TM_OK && (hipEventCreate(&ix->ev0) != hipSuccess || hipEventCreate(&ix->ev1) != hipSuccess || hipEventCreate(&ix->ev_seed) != hipSuccess ||
                      hipEventCreate(&ix->ev_lists) != hipSuccess)) {
    set_error("hipEventCreate failed");
    rc = TM_E_HIP;
  }
  if (rc != TM_OK) { delete ix; return rc; }
  *out = ix;
  return TM_OK;
}

void knn_index_destroy(tm_knn_index_impl *ix) { delete ix; }

// ---------------------------------------------------------------------------------------------------------------
// host side: the third scan shape (tm_knn3.h): seeds -> lists -> consume, all queued on the caller's stream

#define TM_KNN3_BY_HT(FN)                                          \
  switch (ht) {                                                      \
    case 0: FN<0>(hq, a, stream); break;                             \
    case 1: FN<1>(hq, a, stream); break;                             \
    case 2: FN<2>(hq, a, stream); break;                             \
    case 3: FN<3>(hq, a, stream); break;                             \
    case 4: FN<4>(hq, a, stream); break;                             \
    case 5: FN<5>(hq, a, stream); break;                             \
    default: FN<6>(hq, a, stream); break;                            \
  }
static void launch_seed3(int ht, int hq, const Knn3Args &a, hipStream_t stream) { TM_KNN3_BY_HT(knn3_launch_seed_ht) }
static void launch_consume3(int ht, int hq, const Knn3Args &a, hipStream_t stream) { TM_KNN3_BY_HT(knn3_launch_consume_ht) }
static void launch_collect3(int ht, int hq, const Knn3Args &a, hipStream_t stream) { TM_KNN3_BY_HT(knn3_launch_collect_ht) }

// diagnostics for the tests (tm_knn_last_plan): the digit plan and mode of the calling thread's last scan (which instantiation of the
// kernels ran), and how many times a scan of this process was repeated because its tile lists outgrew the arena
struct KnnLastPlan { int ht = -1, hq = -1, topk = 0; };
static thread_local KnnLastPlan t_last_plan;
static std::atomic<long long> g_arena_retries{0};
void knn_last_plan(int *ht, int *hq, int *topk, long long *arena_retries) {
  if (ht) *ht = t_last_plan.ht;
  if (hq) *hq = t_last_plan.hq;
  if (topk) *topk = t_last_plan.topk;
  if (arena_retries) *arena_retries = g_arena_retries.load();
}

static int device_cus() {  // compute units of the current device (persistent kernels launch one workgroup per CU)
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    ncu = std::max(1, prop.multiProcessorCount);
  }
  return ncu;
}
int scan_grid_blocks(int64_t units) { return (int)std::min<int64_t>(units, (int64_t)device_cus() * K3_WGS); }  // the consume kernel's persistent workgroups

KnnBoxes knn_boxes(const tm_knn_index_impl *ix) {
  KnnBoxes bx;
  bx.lo = ix->box_lo.as<int>();
  bx.hi = ix->box_hi.as<int>();
  bx.glo = ix->grp_lo.as<int>();
  bx.ghi = ix->grp_hi.as<int>();
  bx.tkey = ix->tkey.as<uint32_t>();
  for (int d = 0; d < KNN_NC; d++) { bx.col[d] = ix->curve.col[d]; bx.cen[d] = ix->plan.centre[ix->curve.col[d]]; }
  return bx;
}

int launch_qmeta(tm_knn_index_impl *ix, int64_t nqt, int64_t ntt, const KnnBoxes &bx, hipStream_t stream) {
  hipLaunchKernelGGL(k_knn_qmeta, dim3(gridn(nqt)), dim3(256), 0, stream, ix->qkey.as<uint32_t>(), nqt, bx, ntt, ix->qmeta.as<int>());  // (nqt >= 1)
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// What both modes hand the scan's kernels, from the index as it stands: the packs, the boxes, the group geometry, the buffers between the
// kernels and the counters.  The mode's own fields stay zero (nearest neighbour: mode, first_chunk, the bests and the seed counters;
// collection: no_seeds, split, the thresholds and the candidate lists) and grid_blocks is the caller's (scan_grid_blocks).
int scan_args(tm_knn_index_impl *ix, int64_t nq, int ns, Knn3Args *out) {
  const int64_t nqt = knn_tiles(nq), ntt = knn_tiles(ix->nt);
  TM_CHECK(ntt < K3_ENTRY_TILES, TM_E_UNSUPPORTED, "knn: %lld database tiles exceed the list entries' 24-bit tile index", (long long)ntt);
  Knn3Args &a = *out;
  memset(&a, 0, sizeof(a));
  a.tpack = ix->tpack.as<uint8_t>(); a.n_ttiles = ntt; a.nt_rows = ix->nt;
  a.box_lo = ix->box_lo.as<int>(); a.box_hi = ix->box_hi.as<int>(); a.grp_lo = ix->grp_lo.as<int>(); a.grp_hi = ix->grp_hi.as<int>();
  a.qpack = ix->qpack.as<uint8_t>(); a.n_qtiles = nqt; a.nq = nq; a.qmeta = ix->qmeta.as<int>();
  a.thmask = ix->thmask.as<uint8_t>();
  a.ns = ns; a.mode = K3_MODE_LISTS; a.tdouble = ix->plan.tscale == 2;
  a.list_order = knobs().knn_list_order ? 1 : 0;
  a.n_groups = (nqt + ns - 1) / ns;
  a.max_segs = (int)(ntt / (K3_LCAP - K3_LIST_NT) + 2);  // every segment but a list's last holds more than K3_LCAP - K3_LIST_NT entries
  a.gsmax = ix->gsmax.as<unsigned>(); a.segs = ix->segs.as<uint2>(); a.nsegs = ix->nsegs.as<int>();
  a.ltile = ix->arena_tile.as<unsigned>(); a.llb = ix->arena_lb.as<uint16_t>(); a.arena_cap = ix->arena_cap;
  K3Counters *c = ix->dev_counters();
  a.stats = c->stats; a.arena_cursor = &c->stats[K3S_CURSOR]; a.tickets = c->tickets();
  return TM_OK;
}

// the buffers the lists kernel writes for the consume kernel: every sub-tile's bound, every group's segments
int ensure_list_buffers(tm_knn_index_impl *ix, Knn3Args *a) {
  TM_TRY(ix->gsmax.alloc((size_t)a->n_qtiles * 4));
  TM_TRY(ix->segs.alloc((size_t)a->n_groups * a->max_segs * 8)); TM_TRY(ix->nsegs.alloc((size_t)a->n_groups * 4));
  a->gsmax = ix->gsmax.as<unsigned>(); a->segs = ix->segs.as<uint2>(); a->nsegs = ix->nsegs.as<int>();
  return TM_OK;
}

// The list arena is sized from experience: factor x the entries per group the process's searches have needed so far (+ 30 %; 640 to begin
// with, the bench clip needs ~400 -- an index lives for one Reconstruct, the experience is kept beside it), TM_KNN_ARENA_ENTRIES instead
// where set (tests: a tiny arena, so that the repeat-with-the-counted-size path runs), and never below what an overflowed search of this
// index asked for.  The allocations are no-ops while they are large enough.
static std::atomic<double> g_list_entries_per_group{640.0};
int ensure_arena(tm_knn_index_impl *ix, double factor, Knn3Args *a) {
  const uint64_t first = knobs().knn_arena_entries > 0 ? (uint64_t)knobs().knn_arena_entries
                                                       : std::max<uint64_t>(1u << 16, (uint64_t)((double)a->n_groups * factor * g_list_entries_per_group.load()));
  const uint64_t want = std::max<uint64_t>(ix->arena_want, first);
  TM_CHECK(want < (1ull << 32), TM_E_UNSUPPORTED, "knn: %llu list entries exceed the arena's 32-bit offsets", (unsigned long long)want);
  const int nsp = (a->ns + 1) & ~1;
  TM_TRY(ix->arena_tile.alloc((size_t)want * 4)); TM_TRY(ix->arena_lb.alloc((size_t)want * nsp * 2));
  ix->arena_cap = want;
  a->ltile = ix->arena_tile.as<unsigned>(); a->llb = ix->arena_lb.as<uint16_t>(); a->arena_cap = ix->arena_cap;
  return TM_OK;
}

// A scan whose lists did not fit is told so by the cursor the host reads back: the next ensure_arena of this index holds what the cursor
// asked for and a quarter more.  Two repeats at most.
int arena_overflowed(tm_knn_index_impl *ix, unsigned long long cursor, int attempt) {
  TM_CHECK(attempt < 2, TM_E_HIP, "knn: the list arena overflowed again after growing to %llu entries", (unsigned long long)ix->arena_cap);
  if (knobs().knn_debug) fprintf(stderr, "[tm_knn] list arena: %llu entries needed, %llu held -- searching again\n", cursor, (unsigned long long)ix->arena_cap);
  ix->arena_want = cursor + cursor / 4;
  g_arena_retries.fetch_add(1);
  return TM_OK;
}

// remember what the lists needed (never below the starting guess: a small search says little about the next)
static void note_list_entries(unsigned long long cursor, int64_t n_groups) {
  const double per = 1.3 * (double)cursor / (double)std::max<int64_t>(1, n_groups);
  double cur = g_list_entries_per_group.load();
  while (per > cur && !g_list_entries_per_group.compare_exchange_weak(cur, per)) {}
}

int launch_collect(tm_knn_index_impl *ix, const Knn3Args &a, hipStream_t stream) {
  t_last_plan.ht = ix->plan.ht; t_last_plan.hq = ix->plan.hq; t_last_plan.topk = 1;
  launch_collect3(ix->plan.ht, ix->plan.hq, a, stream);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// The nearest-neighbour scan; the host looks at nothing in between.  A search whose lists did not fit is told so by the cursor it reads
// back with its other counters (knn_index_search) and runs again.
static int launch_scan3(tm_knn_index_impl *ix, int64_t nq, int prune, hipStream_t stream) {
  Knn3Args a;
  TM_TRY(scan_args(ix, nq, knn3_sub_tiles(ix->plan.hq), &a));
  a.mode = prune ? K3_MODE_LISTS : K3_MODE_DENSE;
  a.first_chunk = knobs().knn_first_chunk ? 1 : 0;
  if (prune) {
    TM_TRY(ix->gbest.alloc((size_t)a.n_qtiles * 32 * 8));
    TM_TRY(ensure_list_buffers(ix, &a));
    TM_TRY(ensure_arena(ix, 1.0, &a));
  }
  a.gbest = ix->gbest.as<unsigned long long>();
  a.best_key = ix->best_key.as<int>(); a.best_tile = ix->best_tile.as<int>();
  a.seed_stats = &ix->dev_counters()->seed[0][0];
  a.grid_blocks = scan_grid_blocks(a.n_groups);
  if (prune) {
    launch_seed3(ix->plan.ht, ix->plan.hq, a, stream);
    TM_HIP(hipGetLastError());
    TM_HIP(hipEventRecord(ix->ev_seed, stream));
    TM_TRY(launch_lists(a, stream));
    TM_HIP(hipEventRecord(ix->ev_lists, stream));
  } else {
    TM_HIP(hipEventRecord(ix->ev_seed, stream));
    TM_HIP(hipEventRecord(ix->ev_lists, stream));
  }
  t_last_plan.ht = ix->plan.ht; t_last_plan.hq = ix->plan.hq; t_last_plan.topk = 0;
  launch_consume3(ix->plan.ht, ix->plan.hq, a, stream);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// host side: the nearest-neighbour search

// one read of the whole counter block (and the packs' overflow flag) behind everything queued so far
static int read_counts(tm_knn_index_impl *ix, KnnCounts *n, int *flag, hipStream_t stream) {
  K3Counters c;
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(flag, ix->err_flag.p, sizeof(int)));
    TM_TRY(hr_.get(&c, ix->counters.p, sizeof(c)));
    TM_TRY(hr_.wait());
  }
  *n = KnnCounts();
  n->blocks = c.stats[K3S_BLOCKS]; n->tiles = c.stats[K3S_TILES]; n->pairs = c.stats[K3S_PAIRS];
  n->listed = c.stats[K3S_LISTED]; n->popped = c.stats[K3S_POPPED]; n->cursor = c.stats[K3S_CURSOR];
  n->stopped = c.stats[K3S_STOPPED]; n->stopped_pairs = c.stats[K3S_STOPPED_PAIRS];
  n->nosurv = c.stats[K3S_NOSURV]; n->pushed = c.stats[K3S_PUSHED]; n->ringfull = c.stats[K3S_RINGFULL]; n->whole = c.stats[K3S_WHOLE];
  n->mfma = c.stats[K3S_MFMA]; n->guard = c.stats[K3S_GUARD];
  for (int i = 0; i < 64; i++) { n->seed_blocks += c.seed[i][K3SEED_BLOCKS]; n->seed_tiles += c.seed[i][K3SEED_TILES]; n->seed_pairs += c.seed[i][K3SEED_PAIRS]; }
  for (int i = 0; i < 6; i++) n->stamps[i] = c.stats[K3S_STAMPS + i];
  for (int i = 0; i < 3; i++) n->stamps_in[i] = c.stats[K3S_STAMPS_IN + i];
  for (int i = 0; i < 7; i++) n->seed_stamps[i] = c.stats[K3S_SEED_STAMPS + i];
  return TM_OK;
}

// what the stats getters report of the last search
static int record_counts(tm_knn_index_impl *ix, const KnnCounts &n, int prune) {
  float ms = 0, a_ = 0, b_ = 0, c_ = 0;  // the scan, and its three kernels on their own (ev0 | seeds | ev_seed | lists | ev_lists | consume | ev1)
  TM_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
  TM_HIP(hipEventElapsedTime(&a_, ix->ev0, ix->ev_seed));
  TM_HIP(hipEventElapsedTime(&b_, ix->ev_seed, ix->ev_lists));
  TM_HIP(hipEventElapsedTime(&c_, ix->ev_lists, ix->ev1));
  ix->last_ms = ms; ix->last_seed_ms = a_; ix->last_lists_ms = b_; ix->last_consume_ms = c_;
  ix->last_kbytes = knn_kbytes(ix->plan);
  // pairs actually evaluated: exact (real query, real row) pairs.  (The pairs of the listed blocks the first-chunk look stopped were judged, by a
  // lower bound over 32 columns, not evaluated: they are part of what last_stats reports, as the pairs of a block that ended at its first look always
  // were, and are taken out of what the roofline prices: knn_index_kernel_split)
  ix->last_stopped_pairs = (int64_t)n.stopped_pairs;
  ix->last_pairs = (int64_t)(n.pairs + n.seed_pairs + n.stopped_pairs);
  ix->last_seed_pairs = (int64_t)n.seed_pairs;
  ix->last_mfma = (int64_t)n.mfma;
  ix->last_blocks = (int64_t)(n.blocks + n.seed_blocks); ix->last_loads = (int64_t)(n.tiles + n.seed_tiles);
  ix->last_listed = (int64_t)n.listed; ix->last_popped = (int64_t)n.popped;
  ix->last_consume_tiles = (int64_t)n.tiles; ix->last_no_survivor = (int64_t)n.nosurv; ix->last_pushed = (int64_t)n.pushed; ix->last_ring_full = (int64_t)n.ringfull; ix->last_whole = (int64_t)n.whole; ix->last_completed = (int64_t)n.blocks;
  ix->last_chunk_stopped = (int64_t)n.stopped; ix->last_chunk_looked = prune && knobs().knn_first_chunk ? (int64_t)(n.blocks + n.stopped) : 0;
  return TM_OK;
}

static void print_counts(const tm_knn_index_impl *ix, const KnnCounts &n, int64_t nq, int64_t groups) {
  const int64_t ntt = knn_tiles(ix->nt);
  fprintf(stderr, "[tm_knn] first chunk: %lld of %lld listed blocks stopped (%.1f %%); %llu of %llu popped tiles with no block past its look (%.1f %%)\n", (long long)ix->last_chunk_stopped,
          (long long)ix->last_chunk_looked, 100.0 * (double)ix->last_chunk_stopped / (double)std::max<int64_t>(1, ix->last_chunk_looked), n.nosurv, n.tiles,
          100.0 * (double)n.nosurv / (double)std::max<unsigned long long>(1, n.tiles));
  fprintf(stderr, "[tm_knn] survivor queue: %llu entries pushed, %llu more run in place (ring full), %llu tiles loaded whole; %llu blocks completed\n", n.pushed, n.ringfull, n.whole, n.blocks);
  fprintf(stderr, "[tm_knn] seeds %.3f ms, lists %.3f ms (%.1f entries per group, arena %.0f %% full), consume %.3f ms, %.2f of %d matrix instructions per block\n", ix->last_seed_ms, ix->last_lists_ms,
          (double)n.cursor / (double)groups, 100.0 * (double)n.cursor / (double)std::max<uint64_t>(1, ix->arena_cap), ix->last_consume_ms,
          (double)n.mfma / (double)std::max<unsigned long long>(1, n.blocks + n.stopped), knn_kbytes(ix->plan) / 32);
  fprintf(stderr, "[tm_knn] scan %.3f ms, evaluated %.3f%% of %lld x %lld pairs (%lld blocks; workgroups read %.3f%% of tiles, %.1f per group; %.1f list entries per group, %.1f popped)\n",
          ix->last_ms, 100.0 * (double)(ix->last_pairs - ix->last_stopped_pairs) / ((double)nq * (double)ix->nt), (long long)nq, (long long)ix->nt, (long long)ix->last_blocks,
          100.0 * (double)ix->last_loads / ((double)groups * (double)ntt), (double)ix->last_loads / (double)groups, (double)ix->last_listed / (double)groups, (double)ix->last_popped / (double)groups);
}

#if TM_KNN3_STAMPS
static void print_stamps(const KnnCounts &n, int64_t groups) {
  static const char *names3[6] = {"prologue + results", "segment load", "consume", "end-of-segment wait", "waiting for the tile", "total"};
  for (int i = 0; i < 6; i++) fprintf(stderr, "[tm_knn3 stamps] %-24s %6.2f %% of the consume kernel's wave time\n", names3[i], 100.0 * (double)n.stamps[i] / (double)n.stamps[5]);
  static const char *names3b[3] = {"  of consume: pick", "  of consume: chain", "  of consume: epilogue"};
  for (int i = 0; i < 3; i++) fprintf(stderr, "[tm_knn3 stamps] %-24s %6.2f %% (%.0f ticks per block)\n", names3b[i], 100.0 * (double)n.stamps_in[i] / (double)n.stamps[5], (double)n.stamps_in[i] / (double)std::max<unsigned long long>(1, n.blocks));
  static const char *names_s[7] = {"set-up", "wait: first slice + tile", "wait: later slices", "blocks", "end barrier", "results", "total"};
  for (int i = 0; i < 7; i++) fprintf(stderr, "[tm_knn3 stamps] seeds: %-24s %6.2f %% of wave time (%.0f clock ticks per wave)\n", names_s[i], 100.0 * (double)n.seed_stamps[i] / (double)n.seed_stamps[6],
                                      (double)n.seed_stamps[i] / (8.0 * (double)groups));
}
#endif

// one attempt: the scan between its events, then its results in the caller's order
static int search_attempt(tm_knn_index_impl *ix, int64_t nq, void *out_idx, void *out_err, int prune, hipStream_t stream) {
  K3Counters *c = ix->dev_counters();
  TM_HIP(hipMemsetAsync(c, 0, sizeof(K3Counters), stream));
  TM_HIP(hipEventRecord(ix->ev0, stream));
  TM_TRY(launch_scan3(ix, nq, prune, stream));
  TM_HIP(hipEventRecord(ix->ev1, stream));
  hipLaunchKernelGGL(k_knn_refine, dim3(gridn(nq)), dim3(256), 0, stream, nq, ix->qperm.as<uint32_t>(), ix->qpack.as<uint8_t>(), knn_pack_bytes(6 + ix->plan.hq, 0),
                     ix->best_key.as<int>(), ix->best_tile.as<int>(), (int *)out_idx, (uint32_t *)out_err);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int knn_index_search(tm_knn_index_impl *ix, const void *queries, int64_t nq, void *out_idx, void *out_err, hipStream_t stream, const void *query_colmm) {
  TM_CHECK(ix != nullptr, TM_E_INVAL, "knn: null index");
  TM_CHECK(nq >= 0, TM_E_INVAL, "knn: negative query count");
  if (nq == 0) return TM_OK;
  if (ix->nt == 0) {  // ANN on an empty tree: the caller treats idx outside [0,T) as "none" (tilingencoder.pas:1549-1557)
    TM_HIP(hipMemsetAsync(out_idx, 0xff, (size_t)nq * 4, stream));
    TM_HIP(hipMemsetAsync(out_err, 0xff, (size_t)nq * 4, stream));
    return TM_OK;
  }
  TM_TRY(prepare_search(ix, queries, nq, stream, query_colmm));
  const int64_t nqt = knn_tiles(nq), ntt = knn_tiles(ix->nt);
  TM_TRY(ix->best_key.alloc((size_t)nqt * 32 * 4));
  TM_TRY(ix->best_tile.alloc((size_t)nqt * 32 * 4));
  TM_TRY(ix->counters.alloc(sizeof(K3Counters)));
  const int prune = knobs().knn_noprune ? 0 : 1;  // diagnostic: full scan with the same kernel (bench.py roofline_dense)
  const KnnBoxes bx = knn_boxes(ix);
  TM_TRY(launch_qmeta(ix, nqt, ntt, bx, stream));
  const int ns = knn3_sub_tiles(ix->plan.hq);
  const int64_t groups = (nqt + ns - 1) / ns;
  int flag = 0;
  KnnCounts n;
  for (int attempt = 0;; attempt++) {
    TM_TRY(search_attempt(ix, nq, out_idx, out_err, prune, stream));
    TM_TRY(read_counts(ix, &n, &flag, stream));
    if (prune) note_list_entries(n.cursor, groups);
    TM_CHECK(n.guard == 0, TM_E_HIP, "knn: the scan met a corrupted tile list (guard word %llx)", n.guard);
    if (!prune || n.cursor <= ix->arena_cap) break;
    TM_TRY(arena_overflowed(ix, n.cursor, attempt));  // the tile lists did not fit the arena: the cursor says what they need
  }
  TM_CHECK(flag == 0, TM_E_UNSUPPORTED, "knn: feature range exceeds the exact two-digit int8 split (|v-c| >= 32640)");
  TM_TRY(record_counts(ix, n, prune));
  if (knobs().knn_debug) print_counts(ix, n, nq, groups);
#if TM_KNN3_STAMPS
  print_stamps(n, groups);
#endif
  return TM_OK;
}

int knn_index_row_order(tm_knn_index_impl *ix, void *out_rows, hipStream_t stream) {
  TM_CHECK(ix != nullptr && ix->packed, TM_E_INVAL, "knn: the index has not searched yet");
  HostRead hr_(stream);
  TM_TRY(hr_.get(out_rows, ix->tperm.p, (size_t)ix->nt * 4));
  return hr_.wait();
}

void knn_index_kernel_split(tm_knn_index_impl *ix, double ms[3], int64_t pairs[3]) {
  ms[0] = ix->last_seed_ms; ms[1] = ix->last_lists_ms; ms[2] = ix->last_consume_ms;
  pairs[0] = ix->last_seed_pairs; pairs[2] = ix->last_mfma;
  pairs[1] = ix->last_pairs - ix->last_seed_pairs - ix->last_stopped_pairs;  // the consume kernel's blocks that ran to completion: what a roofline may price
}

void knn_index_stats(tm_knn_index_impl *ix, double *ms, int *kbytes, int64_t *pairs) {
  if (ms) *ms = ix->last_ms;
  if (kbytes) *kbytes = ix->last_kbytes;
  if (pairs) *pairs = ix->last_pairs;
}

void knn_index_survivor_counts(tm_knn_index_impl *ix, int64_t *tiles, int64_t *no_survivor, int64_t *pushed, int64_t *ring_full, int64_t *whole, int64_t *completed) {
  if (whole) *whole = ix->last_whole;
  if (completed) *completed = ix->last_completed;
  if (tiles) *tiles = ix->last_consume_tiles;
  if (no_survivor) *no_survivor = ix->last_no_survivor;
  if (pushed) *pushed = ix->last_pushed;
  if (ring_full) *ring_full = ix->last_ring_full;
}

void knn_index_chunk_counts(tm_knn_index_impl *ix, int64_t *looked, int64_t *stopped) {
  if (looked) *looked = ix->last_chunk_looked;
  if (stopped) *stopped = ix->last_chunk_stopped;
}

void knn_index_list_counts(tm_knn_index_impl *ix, int64_t *listed, int64_t *popped) {
  if (listed) *listed = ix->last_listed;
  if (popped) *popped = ix->last_popped;
}

int knn3_sub_tiles(int hq) { return k3_ns(6 + std::min(std::max(hq, 0), 6)); }
int knn3_sub_tiles_topk(int hq) { return k3_ns_topk(6 + std::min(std::max(hq, 0), 6)); }

}  // namespace tmx
