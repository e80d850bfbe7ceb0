// tm_knn3.h -- the nearest-neighbour scan of the KNN stage, third shape ("KNN"): what its host files and its kernels
// share, and no device code.  Shape constants, the kernels' arguments and counters, the layouts both sides must agree on (the packed tile,
// the qmeta record, the list entry word), the consume kernel's LDS budget, and the launch prototypes.
//
// The second shape (round 2-3) did everything in one persistent kernel: a workgroup loaded its 384 queries, scored the
// tiles around its position on the curve, built tile lists with all 1024 threads, consumed them, built the next ... and its phase stamps
// showed 21 % of the wave time in phases where the matrix pipe has nothing to do (list building 10.8 %, the wait for the slowest wave at
// every list's end 6.8 %, prologue 3.7 %).  Here each phase is a kernel of its own, shaped for what it does:
//   1. k_knn_seed    (tm_knn3_seed.h) every query sub-tile against the K3_SEEDS database tiles around its group's position on the curve:
//                    bests (one 64-bit word per query) and the sub-tile's bound sqrt(largest best) -- MFMA work with no list in sight,
//                    several workgroups per CU.
//   2. k_knn_lists   (tm_knn3_lists.hip) the tile list of every query group, judged against the seeds' bounds: runs of KNN_GROUP tiles first,
//                    then the tiles of surviving runs; per entry the box lower bound of each (tile, sub-tile) pair as a 16-bit square root.
//                    No MFMA, no query operands: small workgroups, many per CU, whose global loads hide behind each other.  Lists go to an
//                    arena in HBM in segments of <= K3_LCAP entries, each sorted by its entries' smallest bound.
//   3. k_knn_consume (tm_knn3_consume.h) persistent workgroups (one per CU, 16 waves): a group's query operands and its seeds' bests into LDS,
//                    then one list segment after the other: copied into LDS, consumed by the waves on their own (pop an entry, re-judge it
//                    against the sub-tiles' bounds AS THEY ARE NOW, one MFMA chain per sub-tile that wants the tile).  An entry judged with
//                    the seeds' bound instead of a later, tighter one costs one pop, not a block; a sorted segment ends at the first entry
//                    whose smallest bound lies above every sub-tile's bound.  A block is judged on its first chunk of columns, the 32
//                    widest, before its chain runs, and ends there nine times in ten (k3_chunk_look).  The two jobs
//                    are two tasks: a wave either LOOKS -- the popped tile's chunk 0 only, two sub-tiles at a time,
//                    the next tile's chunk 0 asked for before -- or RUNS THE CHAINS of a tile some look let through, taken from a survivor
//                    queue in LDS and loaded whole then; nine popped tiles in ten never are.  The collection mode keeps the one loop that
//                    loads every popped tile whole.
// The device pieces the three are made of are in tm_knn3_block.h; tm_knn3_kernels.h is what a tm_knn3_k<HT>.hip includes.
// Arithmetic, operands, boxes, curve and the exactness argument are those of the earlier shapes: a pair is skipped only when its lower
// bound exceeds the sub-tile's largest best + 1 (both sides of the 16-bit compare rounded the safe way), the minimum VALUE is exact, and
// among the rows reaching it the lowest ORIGINAL index wins inside the scan: a query's best is (d'' + 1) << 32 | original index, every row
// that reaches or ties it arrives at k3_epilogue's 64-bit atomic minimum (k3_within: the inclusive compares of next_entry, pick,
// k3_chunk_look and the epilogue), and a tile's rows stand in ascending original index (k_knn_tile_order), so a lane's lowest winning row
// is its lowest index.
#pragma once
#include <cstddef>
#include "tm_knn_kernel.h"

namespace tmx {

// ------------------------------------------------------------------------------------------------------------------ shape
#ifndef TM_KNN3_WAVES
#define TM_KNN3_WAVES 16  // consume: 16 = one workgroup per CU; 8 = two (half the LDS each, fewer sub-tiles per group)
#endif
constexpr int K3_NW = TM_KNN3_WAVES;
constexpr int K3_NT = K3_NW * 64;
constexpr int K3_WGS = 16 / K3_NW;       // consume workgroups per CU (they split its LDS)
constexpr int K3_LDS = 163840 / K3_WGS;
constexpr int K3_LCAP = 1024;            // entries of a list segment (what the consume kernel holds in LDS at a time)
#ifndef TM_KNN3_SEEDS
#define TM_KNN3_SEEDS 8
#endif
constexpr int K3_SEEDS = TM_KNN3_SEEDS;  // tiles around the group's position on the curve, scored first by every sub-tile
#ifndef TM_KNN3_REFRESH_EVERY
#define TM_KNN3_REFRESH_EVERY 64         // consume: list entries between two full refreshes of the sub-tiles' bounds (a power of two; 0 = never)
#endif
#ifndef TM_KNN3_STAMPS
#define TM_KNN3_STAMPS 0                 // diagnostic build: s_memtime spans of the seed and consume kernels' phases, summed over all waves
#endif
constexpr int K3_LIST_NT = 256;          // threads of a list-building workgroup

enum { K3_MODE_LISTS = 0, K3_MODE_DENSE = 1 };

// ------------------------------------------------------------------------------------------------------------------ the packed tile
// A pack (k_knn_pack) is a row of tiles of 32 rows each.  A tile of `chunks` operand chunks (6 low + HT or HQ high) holds, in this order:
//   operands      chunks x 1 KB: [chunk][64 lanes][16 B] in MFMA fragment order
//   row terms     32 words: the chain's starting value per row -- database: |t-c|^2 where the digits are those of 2 (t - c), |t-c|^2 >> 1
//                 where not; queries: |q-c|^2 (the scan drops its parity, k_knn_refine and k_topk_select put it back)
//   box           database only (with_box), 16 words: lows at 0.., highs at KNN_ND.., the 32 rows' parities |t-c|^2 & 1 in word
//                 KNN_PACK_BOX_PARITY (bit = row), a zero word behind it
//   first terms   32 words: the row terms over the first chunk's columns, in the row terms' form (queries: whole)
//   indices       database only, 32 words: the rows' original indices, ascending (k_knn_tile_order); padding rows carry the last real row's
// Every part's function gives its offset in bytes from the tile's start, or, handed the tile's address as `at`, its address; the functions
// take compile-time and run-time arguments alike.
constexpr int KNN_PACK_CHUNK = 1024;      // bytes of an operand chunk
constexpr int KNN_PACK_WORDS = 32 * 4;    // bytes of a part that holds one word per row
constexpr int KNN_PACK_BOX = 16 * 4;      // bytes of a database tile's box
constexpr int KNN_PACK_BOX_PARITY = 14;   // the box's word of row parities
static_assert(2 * KNN_ND == KNN_PACK_BOX_PARITY, "the parities stand behind the box's highs");
template <class P = int> __host__ __device__ constexpr P knn_pack_row_terms(int chunks, P at = 0) { return at + chunks * KNN_PACK_CHUNK; }
template <class P = int> __host__ __device__ constexpr P knn_pack_box(int chunks, P at = 0) { return knn_pack_row_terms(chunks, at) + KNN_PACK_WORDS; }
template <class P = int> __host__ __device__ constexpr P knn_pack_parity(int chunks, P at = 0) { return knn_pack_box(chunks, at) + KNN_PACK_BOX_PARITY * 4; }
template <class P = int> __host__ __device__ constexpr P knn_pack_first_terms(int chunks, int with_box, P at = 0) { return knn_pack_box(chunks, at) + (with_box ? KNN_PACK_BOX : 0); }
template <class P = int> __host__ __device__ constexpr P knn_pack_indices(int chunks, P at = 0) { return knn_pack_first_terms(chunks, 1, at) + KNN_PACK_WORDS; }
__host__ __device__ constexpr int knn_pack_bytes(int chunks, int with_box) { return knn_pack_first_terms(chunks, with_box) + KNN_PACK_WORDS + (with_box ? KNN_PACK_WORDS : 0); }
// ... and for the kernels that are handed a tile's size, not its chunks: the same two parts counted from the tile's end
__host__ __device__ constexpr int knn_pack_indices_of(int t_bytes) { return t_bytes - KNN_PACK_WORDS; }        // database side
__host__ __device__ constexpr int knn_pack_row_terms_of(int q_bytes) { return q_bytes - 2 * KNN_PACK_WORDS; }  // query side
constexpr bool knn_pack_ends_agree(int chunks) {
  return knn_pack_indices_of(knn_pack_bytes(chunks, 1)) == knn_pack_indices(chunks) && knn_pack_row_terms_of(knn_pack_bytes(chunks, 0)) == knn_pack_row_terms(chunks);
}
static_assert(knn_pack_ends_agree(6) && knn_pack_ends_agree(7) && knn_pack_ends_agree(8) && knn_pack_ends_agree(9) && knn_pack_ends_agree(10) &&
                  knn_pack_ends_agree(11) && knn_pack_ends_agree(12),
              "a pack's parts counted from its end");

// ------------------------------------------------------------------------------------------------------------------ the qmeta record
// Per query sub-tile, QMETA_INTS ints (k_knn_pack writes all of it but the home tile, which is k_knn_qmeta's): the sub-tile's box as KNN_ND
// lows and KNN_ND highs, the database tile its first query falls into on the curve, the mask of its non-zero high-digit chunks.  (The lows
// and the highs each start a 32-byte half: k_knn_lists reads a record as four 16-byte vectors.)
constexpr int QMETA_INTS = 16, QMETA_LO = 0, QMETA_HOME = 7, QMETA_HI = 8, QMETA_HMASK = 15;
static_assert(QMETA_LO + KNN_ND <= QMETA_HOME && QMETA_HI + KNN_ND <= QMETA_HMASK, "the record's fields");
template <class I> __host__ __device__ constexpr I qmeta_at(I sub_tile, int field) { return sub_tile * QMETA_INTS + field; }

// ------------------------------------------------------------------------------------------------------------------ the list entry word
// tile << 8 | mask of the tile's non-zero high-digit chunks (`thmask`: the mask of every database tile): the consumer has the mask before
// the tile.
constexpr int K3_ENTRY_MASK_BITS = 8;
constexpr int64_t K3_ENTRY_TILES = (int64_t)1 << (32 - K3_ENTRY_MASK_BITS);  // tiles an entry can name (scan_args checks)
template <class I> __host__ __device__ constexpr unsigned k3_entry(I tile, const uint8_t *thmask) { return ((unsigned)tile << K3_ENTRY_MASK_BITS) | (unsigned)thmask[tile]; }
// The tile comes out by a SHIFT.  (An earlier layout, tile | mask << 24 with `tile = word & 0xFFFFFF`, met a compiler combine that treats
// the 64-bit multiply by the tile size as a 24-bit multiply, drops the AND as redundant for one, and then selects a full 32-bit
// v_mad_u64_u32: the loads went to word * 12 KB -- a memory aperture violation on the GPU box.)
__host__ __device__ constexpr unsigned k3_entry_tile(unsigned entry) { return entry >> K3_ENTRY_MASK_BITS; }
__host__ __device__ constexpr unsigned k3_entry_mask(unsigned entry) { return entry & ((1u << K3_ENTRY_MASK_BITS) - 1u); }
// ... and the 16-bit bounds an entry carries per sub-tile slot (Knn3Args::llb), which the sub-tiles' own bounds (::gsmax) are compared with
constexpr unsigned K3_LB_MAX = 0xFFFEu;  // the largest 16-bit bound, of a box or of a sub-tile (a sub-tile's: some query has no best yet)
constexpr unsigned K3_LB_NONE = 0xFFFFu; // a list entry's slot for a sub-tile that does not want the tile: above every bound

// ------------------------------------------------------------------------------------------------------------------ LDS budget
// (per sub-tile: operands, norms, bests, box, the norms over the first chunk's columns; per wave: its tile's 32 row terms over them and its
// 32 original indices)
// ... and the survivor queue between the consume kernel's looks and its chains: a ring of 8-byte entries
constexpr int K3_RING = 128;             // entries (a power of two)
constexpr int K3_RING_BYTES = K3_RING * 8;
constexpr int K3_CTL_HEAD = 4, K3_CTL_TAIL = 5;  // the ring's tickets: words of the kernel's s_ctl (taken / handed out; they only grow)
constexpr int k3_lds_bytes(int ns, int kq) {
  return ns * (kq * 1024 + 576) + 64 + 64 + 64 + K3_NW * (128 + 128) + K3_LCAP * (4 + 2 * ((ns + 1) & ~1)) + K3_RING_BYTES;
}
constexpr int k3_ns(int kq) {  // sub-tiles per query group
  int ns = 16;
  while (ns > 1 && k3_lds_bytes(ns, kq) > K3_LDS) ns--;
  return ns;
}
static_assert(K3_NW != 16 || k3_ns(10) == 12, "the bench's plan <5, 4> keeps its 12 sub-tiles per group beside the ring");
constexpr int k3_ns_topk(int kq) { return k3_ns(kq) > 1 ? k3_ns(kq) - 1 : 1; }  // collection mode: one fewer pays for the ladder's counters

// ------------------------------------------------------------------------------------------------------------------ arguments
struct Knn3Args {
  const uint8_t *tpack; int64_t n_ttiles, nt_rows;
  const int *box_lo, *box_hi, *grp_lo, *grp_hi;  // database tile boxes [KNN_ND][n_ttiles], boxes of runs of KNN_GROUP tiles
  const uint8_t *qpack; int64_t n_qtiles, nq;
  const int *qmeta;             // [n_qtiles][QMETA_INTS]: box lo[7], home tile, box hi[7], mask of the sub-tile's non-zero high-digit chunks
  const uint8_t *thmask;        // [n_ttiles] the same mask for every database tile
  int ns;                       // sub-tiles per group (k3_ns of the queries' digit plan)
  int mode;                     // consume: K3_MODE_LISTS / K3_MODE_DENSE (every tile, every sub-tile; no seeds, no lists)
  int tdouble;                  // the database pack holds the digits of 2 (t - c)
  // between the kernels (HBM)
  unsigned long long *gbest;    // [n_qtiles * 32] (d'' + 1) << 32 | original index
  unsigned *gsmax;              // [n_qtiles] upper bound of sqrt(largest best + 1) of the sub-tile, K3_LB_MAX = some query has none
  uint2 *segs;                  // [n_groups][max_segs] (first entry, entries) of each list segment
  int *nsegs;                   // [n_groups]
  int max_segs;
  unsigned *ltile;              // arena [arena_cap] k3_entry of the tile, per entry
  uint16_t *llb;                // arena [arena_cap][nsp] lower bounds per sub-tile slot
  unsigned long long arena_cap; // entries
  unsigned long long *arena_cursor;  // entries handed out (keeps counting past the capacity: the host sizes the next arena from it)
  int *best_key, *best_tile;
  // collection mode (the k nearest rows, ann_kdtree_short_search_multi, tilingencoder.pas:1563): see k_knn_consume<.., TOPK = true>
  int *tau;                     // [n_qtiles * 32] every sorted query's threshold (d'' <= tau); the scan leaves its final one
  const int *step;              // [n_qtiles * 32] the spacing of its ladder's rungs below the threshold (null: tau / 8)
  uint2 *cand;                  // [nq][cand_cap] (d'', sorted row) of every row within the threshold
  int *cand_cnt;                // [nq] rows appended (keeps counting past cand_cap)
  int cand_cap, cand_k;
  int split;                    // workgroups that share one group's tile list (entry j goes to part j mod split)
  int no_seeds;                 // lists: no seed kernel ran (collection mode), so no tile is left out of the lists
  int first_chunk;              // consume, nearest-neighbour lists: a block is judged on its first chunk's columns before its chain runs (k3_chunk_look; 0: every block runs its chain)
  int list_order;               // lists: a segment leaves sorted by its entries' smallest bound; consume: a segment ends at the first entry nobody can want (0: run order, no stop)
  unsigned long long *stats;    // K3Counters::stats, indexed by K3Stat
  unsigned long long *seed_stats;  // K3Counters::seed: [64][4] striped by workgroup: blocks, tiles read, pairs of the seed kernel
  int64_t n_groups;
  int grid_blocks;              // consume: persistent workgroups
  unsigned *tickets;            // [8] zeroed before the consume launch: next run-slot of each XCD's share of the groups
};

// The counter block of a search: one buffer the host zeroes before the scan and reads back after it.  The kernels reach it through
// Knn3Args::stats (+ a K3Stat), ::arena_cursor, ::tickets and ::seed_stats; the host through this struct and nothing else.
enum K3Stat {
  K3S_BLOCKS = 0,          // consume: blocks evaluated
  K3S_TILES = 1,           // consume: tiles read
  K3S_PAIRS = 2,           // consume: exact (query, row) pairs
  K3S_LISTED = 3,          // list entries listed
  K3S_STAMPS = 4,          // [4..9] a diagnostic build's (TM_KNN3_STAMPS) spans of the consume kernel's phases, the last one the total
  K3S_STAMPS_IN = 10,      // [10..12] ... and inside "consume": pick, chain, epilogue
  K3S_STOPPED_PAIRS = 13,  // (query, row) pairs of the blocks the first chunk stopped
  K3S_TICKETS = 14,        // [14..17] these 32 bytes are Knn3Args::tickets: eight u32
  K3S_CURSOR = 18,         // Knn3Args::arena_cursor
  K3S_MFMA = 19,           // matrix instructions issued
  K3S_SEED_STAMPS = 20,    // [20..26] a diagnostic build's spans of the seed kernel's phases, the last one the total
  K3S_GUARD = 27,          // consume: a tile index or a segment out of range (0: none)
  K3S_POPPED = 28,         // entries the waves took off their lists: short of K3S_LISTED by what the stops left behind
  K3S_STOPPED = 29,        // blocks the first chunk stopped
  K3S_NOSURV = 30,         // popped tiles none of whose blocks got past its first-chunk look
  K3S_PUSHED = 31,         // survivor entries pushed to the ring: tiles with a block past its look, loaded whole by whoever took the entry
  K3S_RINGFULL = 32,       // ... and those the queue turned away (the ring full, or the tail lost to another wave's push): the looker ran their chains itself
  K3S_WHOLE = 33,          // chain tasks run: tiles loaded whole (= pushed + turned away: the queue loses and doubles nothing)
  K3S_COUNT = 34
};
enum K3SeedStat { K3SEED_BLOCKS = 0, K3SEED_TILES = 1, K3SEED_PAIRS = 2, K3SEED_WORDS = 4 };  // a stripe of the seed kernel's counters (the fourth word is spare)
struct K3Counters {
  unsigned pad_[4];
  unsigned long long stats[K3S_COUNT];
  unsigned long long seed[64][K3SEED_WORDS];  // the seed kernel's, striped by workgroup
  unsigned *tickets() { return reinterpret_cast<unsigned *>(stats + K3S_TICKETS); }
};
static_assert(offsetof(K3Counters, stats) == 16 && offsetof(K3Counters, seed) == 288 && sizeof(K3Counters) == 2336, "the counter block's layout");

// ------------------------------------------------------------------------------------------------------------------ launches
// one per HT, defined in tm_knn3_k<HT>.hip (tm_knn3_kernels.h)
template <int HT> void knn3_launch_seed_ht(int hq, const Knn3Args &a, hipStream_t stream);
template <int HT> void knn3_launch_consume_ht(int hq, const Knn3Args &a, hipStream_t stream);
template <int HT> void knn3_launch_collect_ht(int hq, const Knn3Args &a, hipStream_t stream);  // k_knn_consume<.., TOPK = true>
int knn3_sub_tiles(int hq);       // NS of the queries' digit plan
int knn3_sub_tiles_topk(int hq);  // ... in collection mode
// (launch_lists and launch_tau_bounds, of tm_knn3_lists.hip, return the host side's error codes: tm_knn.h)

}  // namespace tmx
