// tm_internal.h -- launcher prototypes shared between the kernel files, the stage ABI and the encoder.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "tm_common.h"

namespace tmx {

// tm_load.hip: the load stage (A1-A3)
int launch_load(const void *frames, int nframes, int img_w, int img_h, int tm_w, int tm_h, void *tiles, void *flags,
                void *lab_means, hipStream_t stream);
int launch_rgb_to_lab(const void *rgb, int64_t n, void *out, hipStream_t stream);
int launch_pearson(const void *lab, int nframes, int per, void *correl, hipStream_t stream);

// tm_features.hip: the int16 features of tiles (A4 + A5)
int launch_features_rgb(const void *tiles, int64_t n, const void *mirror_flags, int mode, int use_lab, void *out, hipStream_t stream);
// colmm (optional): [384] ints on the device, mn[192] preset to INT_MAX and mx[192] to INT_MIN: the kernel folds the output columns' ranges in
int launch_features_rgb_rows(const void *tiles, const void *rows, int64_t n, int mode, int use_lab, void *out, hipStream_t stream, void *colmm = nullptr);
int launch_features_pal(const void *pal_px, const void *pal_idx, int64_t n, const void *palettes, int pal_size, int mode, void *out,
                        hipStream_t stream);
// int16 features of the (tile, palette) pairs pairs[i] = tile << 32 | palette (the rows the extended-palette re-rank asks for)
int launch_features_pairs(const void *pal_px, const void *pairs, int64_t n, const void *palettes, int pal_size, void *out, hipStream_t stream);
int launch_features_table(const void *pal_px, int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, hipStream_t stream);

// tm_features_cluster.hip: the clustering's int32 features (A6)
int launch_features_cluster(const void *tiles, int64_t n, int mode, void *out, hipStream_t stream);

// tm_window_dcts.hip: the features of every 8 x 8 window of a frame buffer (motion prediction)
int launch_window_dcts(const void *fb, int w, int h, void *out, hipStream_t stream, const int *only_if = nullptr);
// The windows' features straight into the matrix layout of the motion search (tm_motion.hip: what k_mo_pack_win makes of the int16 rows) -- the
// int16 rows are then never written.  Per block of 32 consecutive window positions of a row: [12 chunks][64 lanes][16 B] digits (low digits of the
// 160 plain coefficients + the 16 of b5 + b6, then the high digits), 32 norms, block 7 of the first half raw.  `flag` (device int, preset 0) is
// raised when a coefficient of the windows or of the `ntiles` tiles `cur` (their int16 features) lies beyond the range in which the matrix form is exact.
constexpr int MM_CH = 6;                                             // 32-wide chunks of the 160 plain coefficients + 16 of block 6 + 16 of padding
constexpr int MM_DIG = 2 * MM_CH * 1024, MM_NORM = MM_DIG, MM_QUIRK = MM_DIG + 128;
constexpr int MM_BLK_BYTES = MM_QUIRK + 32 * 16;                     // 12928
constexpr int MM_LIMIT6 = 10922;                                     // |coefficient| bound of blocks 5 and 6 under which a6 - b5 - b6 cannot saturate
constexpr int MM_LIMIT = 16383;                                      // |coefficient| bound under which no plain difference saturates
int launch_window_dcts_packed(const void *fb, int w, int h, const void *cur, int ntiles, void *packed, int *flag, hipStream_t stream);

// tm_epu.hip: FrameTilingExtendedPaletteUsage (tilingencoder.pas:1559-1610)
int launch_knn_topk(const void *queries, int64_t nq, const void *db, int64_t nt, int k, void *out_idx, void *out_err, hipStream_t stream);
int launch_epu_rerank_ondemand(const void *queries, int64_t nq, const void *knn_idx, int k, const void *tile_pal, int64_t ntiles, const void *pal_px,
                               const void *palettes, int npal, int pal_size, void *out_tile, void *out_pal, void *out_err, hipStream_t stream);
int launch_epu_rerank(const void *queries, int64_t nq, const void *knn_idx, int k, const void *tile_pal, int64_t ntiles, int npal,
                      const void *table, void *out_tile, void *out_pal, void *out_err, hipStream_t stream);

// tm_knn.hip (index, nearest neighbour, the stats of the last search) and tm_knn_topk.hip (k nearest rows); tm_knn.h is their own header
struct tm_knn_index_impl;
int knn_index_create(const void *db, int64_t nt, hipStream_t stream, tm_knn_index_impl **out);
void knn_index_destroy(tm_knn_index_impl *ix);
// query_colmm (optional): the queries' column ranges as launch_features_rgb_rows leaves them (device, [384]) -- saves the search its own pass
int knn_index_search(tm_knn_index_impl *ix, const void *queries, int64_t nq, void *out_idx, void *out_err, hipStream_t stream, const void *query_colmm = nullptr);
void knn_index_stats(tm_knn_index_impl *ix, double *ms, int *kbytes, int64_t *pairs);
void knn_index_list_counts(tm_knn_index_impl *ix, int64_t *listed, int64_t *popped);
void knn_index_chunk_counts(tm_knn_index_impl *ix, int64_t *looked, int64_t *stopped);
void knn_index_survivor_counts(tm_knn_index_impl *ix, int64_t *tiles, int64_t *no_survivor, int64_t *pushed, int64_t *ring_full, int64_t *whole, int64_t *completed);
void knn_last_plan(int *ht, int *hq, int *topk, long long *arena_retries);
// diagnostics for the tests: the database's row order as the scan sees it (host, [nt]: tile t holds rows out[32 t ..]), of an index that has searched
int knn_index_row_order(tm_knn_index_impl *ix, void *out_rows, hipStream_t stream);
// tm_knn_prepare.hip: every run of 32 entries of perm (device, [n]) into ascending order, in place (what a built index does to its curve order;
// pack: the database's pack, whose tiles' last 128 bytes take the ordered indices)
int launch_tile_order(uint32_t *perm, int64_t n, hipStream_t stream, uint8_t *pack = nullptr, int tile_bytes = 0);
// tm_knn_prepare.hip: curve_key (tm_knn_kernel.h) of n cells (device, [n][4], cell d below 2^bits[d]) into keys (device, [n]); kind: CURVE_MORTON 0, CURVE_HILBERT 1
int launch_curve_keys(const uint32_t *cells, int64_t n, const int bits[4], int kind, uint32_t *keys, hipStream_t stream);
// the last search's three kernels on their own: ms of seeds / lists / consume; pairs evaluated by seeds / consume, matrix instructions the consume kernel issued
void knn_index_kernel_split(tm_knn_index_impl *ix, double ms[3], int64_t pairs[3]);
// grp_off / grp_members (optional): the index was built over DISTINCT rows; results are expanded to the original rows (member lists
// as build_groups makes them), full_db = all rows, for the brute-force fallback
int knn_index_search_topk(tm_knn_index_impl *ix, const void *queries, int64_t nq, int k, void *out_idx, void *out_err, hipStream_t stream,
                          const void *grp_off = nullptr, const void *grp_members = nullptr, const void *full_db = nullptr, int64_t full_nt = 0);

// tm_dither.hip
int launch_dither(const void *tiles, const void *flags, const void *pal_idx, int64_t n, const void *palettes, int npal, int pal_size,
                  int use_tk, int y2_mixed, void *out_pal_px, hipStream_t stream, int64_t *pairs_planned = nullptr,
                  const void *pair_keys = nullptr, int64_t n_pair_keys = 0);
// pair_keys (optional): the distinct pixel keys palette << 24 | G << 16 | R << 8 | B of exactly these tiles (or a superset), as run_quantize_palettes
// leaves them -- saves Dither its own pass over the pixels

// tm_dedup.hip
int run_dedup(const void *rows, int64_t n, int row_bytes, const void *use_in, void *remap, void *order, void *use_out,
              int64_t *host_n_unique, hipStream_t stream, int64_t exact_first = 0);
int run_dedup_ex(const void *rows, int64_t n, int row_bytes, const void *use_in, void *remap, void *order, void *use_out,
                 int64_t *host_n_unique, int by_index, hipStream_t stream, int64_t exact_first = 0);

// tm_lists.hip
int build_groups(const void *remap, int64_t n, const void *counts, int64_t ngroups, void *off, void *members, hipStream_t stream);
int compact_kept(const void *keep, int64_t n, void *out_idx, void *pos, int64_t *host_count, hipStream_t stream);

// tm_motion.hip: motion prediction (tilingencoder.pas:1154-1282, 1496-1654) and Reduce's tile-count search (4014-4046)
int launch_motion_search(const void *cur, int tm_w, int tm_h, const void *win, int radius, void *best_err, void *px, void *py,
                         hipStream_t stream);
// the encoder's form: window features of the frame buffer `fb` (tm_w * 8 x tm_h * 8) and the search in one go -- the windows are made in the
// search's matrix layout at once (launch_window_dcts_packed); `win` ((tm_w*8-7) * (tm_h*8-7) * 384 B) is written only by the fallback (a frame
// whose coefficients leave the matrix form's exact range, or TM_MOTION_VALU=1) and by TM_MOTION_PACK_SEPARATE=1 (the two-pass form, for A/B runs)
int launch_motion_search_fb(const void *cur, int tm_w, int tm_h, const void *fb, void *win, int radius, void *best_err, void *px, void *py,
                            hipStream_t stream);
int launch_tiles_to_screen(const void *tiles, const void *flags, int tm_w, int tm_h, void *screen, hipStream_t stream);
int launch_recon_decide(int tm_w, int per, int pal_from_map, const void *mp_err, const void *fflags, const void *gpal_idx, const void *gpal_px,
                        const void *palettes, int pal_size, const void *back, void *front, void *tm_tile, void *tm_pal, void *tm_err,
                        const void *px, const void *py, void *pred, hipStream_t stream);
int solve_tile_count(const void *group, int64_t ngroups, const void *pm_err, const void *frame_is_kf, int per, int64_t q, double target,
                     void *pred, void *keep, double *x_out, int *probes_out, hipStream_t stream);
// STCGREval's marking at one threshold x (4024-4031): pred / keep of every item, as after the search's last probe
int mark_at_threshold(const void *pm_err, const void *frame_is_kf, int per, int64_t q, double x, void *pred, void *keep, hipStream_t stream);
float euclidean_to_psnr(uint32_t e);

// tm_render.hip: the decoded frames (Render, tilingencoder.pas:3455-3640, the constructor's defaults) and their quality against the source
struct RenderMap {  // the output picture: tile maps [frames][tm_h * tm_w] from frame 0, tiles, palettes (0x00BBGGRR)
  const int32_t *tile, *pal;
  const uint8_t *mir;                 // bit 0 H mirror, bit 1 V mirror
  const uint8_t *pred;                // predicted where pred[i] & pred_mask (null: none is)
  int pred_mask;
  const int8_t *px, *py;
  const uint8_t *pal_px;              // [ntiles][64]
  int64_t ntiles;
  const int32_t *palettes;            // [npal][pal_size]
  int npal, pal_size, tm_w, tm_h;
};
struct RenderInput {  // the source picture: frame tiles (canonical orientation, 0x00BBGGRR) and their mirror flags, from frame 0
  const uint32_t *tiles;
  const uint8_t *flags;
  int tm_w, tm_h;
};
// frames [first, first + count) as [count][tm_h * 8][tm_w * 8] 0x00RRGGBB
int launch_render_output(const RenderMap &m, int first, int count, void *out, hipStream_t stream);
int launch_render_input(const RenderInput &in, int first, int count, void *out, hipStream_t stream);
// per frame of [first, first + count): SSE of R, G, B (uint64 [count][3]) and the SSIM of GenerateY4M's luma (double [count]), output against source
int launch_quality_render(const RenderInput &in, const RenderMap &m, int first, int count, void *sse, void *ssim, hipStream_t stream);
// the same for two stacks of 0x00RRGGBB frames [n][h][stride_px] (w, h: multiples of 4, at least 8)
int launch_quality_frames(const void *a, const void *b, int n, int w, int h, int64_t stride_px, void *sse, void *ssim, hipStream_t stream);

// tm_yuv_out.hip: decoded frames delivered as YUV.  check_yuv_out makes every check of a destination without a device
// call and says what its planes look like; the resolved colour rule travels with the plan.
struct YuvOutPlan {
  int w = 0, h = 0, cw = 0, ch = 0, chroma = 0, samples = 0, depth = 8, mode = 0, bytes = 1, nplanes = 1;  // nplanes: 1 mono, 2 Y + pairs, 3 planar
  bool pairs = false;
  int64_t row_bytes[3] = {0, 0, 0};  // of Y, U (or the pairs), V
  int rows[3] = {0, 0, 0};
  int64_t plane_bytes(int i) const { return row_bytes[i] * rows[i]; }
  int64_t frame_bytes() const { int64_t n = 0; for (int i = 0; i < nplanes; i++) n += plane_bytes(i); return n; }
};
struct YuvDst { uint8_t *p[3]; int64_t row[3], frame[3]; };  // device planes, strides in bytes
int check_yuv_out(const tm_yuv_out *d, int width, int height, int mode, YuvOutPlan *out);
int yuv_out_is_device(const tm_yuv_out &d, int device);  // TM_E_INVAL unless every plane is memory of that device
YuvDst yuv_dst_of(const tm_yuv_out &d, int64_t frame0);  // the caller's planes from frame0 on
// a packed chunk of `cap` frames at base -- [cap frames of Y][of U or the pairs][of V], frame_bytes() * cap bytes -- from frame0 on
YuvDst yuv_dst_packed(const YuvOutPlan &p, uint8_t *base, int cap, int frame0);
// rgb: [nframes][h][stride_px] 0x00RRGGBB on the device
int launch_rgb32_to_yuv(const YuvOutPlan &p, const void *rgb, int64_t stride_px, int nframes, const YuvDst &d, hipStream_t stream);
int yuv_copy_out(const YuvOutPlan &p, const uint8_t *packed, int cap, const tm_yuv_out &d, int64_t frame0, int nf, hipStream_t stream);

// tm_png.hip (host only): inflate of a zlib stream, the PNG reader (8-bit, non-interlaced; pixels 0x00RRGGBB; out null: the size only)
uint32_t crc32_ieee(const uint8_t *p, size_t n);
int inflate_zlib(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n);
int read_png(const char *path, uint32_t *out, int64_t cap_px, int *w, int *h);

// tm_input.h: Load's input -- InputInfo and probe_input, the staging helpers (PinnedBuf, StagingRing), the YUV planes' way in (InputTables)

// tm_resample.hip (host only): the rule's tables, shared by tm_yuv_in.hip (YUV planes in) and tm_scale.hip (RGB32 frames out).
// The resampling tables of one conversion on the device: per axis first [m], count [m], coef [tap][m] (the lanes of a wave read neighbouring
// words); a vertical axis also has, per tile of th output rows, the source rows its samples reach as (first row, number of rows)
struct AxisTaps { const int32_t *first, *count, *coef; const int2 *span; };
int resample_taps(int n, int m, int np, int s, int o_halves, int32_t *first, int32_t *count, int32_t *coef, int64_t *sum_abs_max);
constexpr int RESAMPLE_TH_MAX = 16;  // output rows per workgroup, at most
struct AxisTable {  // one axis on the host: first / count [m], coef [m][TM_RESAMPLE_MAX_TAPS], the largest sum of |coefficients| of a sample
  int m = 0;
  int64_t amax = 0;
  std::vector<int32_t> first, count, coef;
  int make(int n, int m_out, int np, int s, int o_halves);      // resample_taps
  void trim();                                                  // a sample's window shrinks to its coefficients that are not 0
  std::vector<int32_t> tile_spans(int th, int *widest) const;   // per tile of th samples: (first source sample, number of them)
};
int check_resample_sums(const AxisTable &h, const AxisTable &v, int src_w, int src_h, int dst_w, int dst_h);  // the vertical sum fits 32 bits
int resample_tile_rows(const AxisTable *const *vertical, int nplanes, int max_rows);  // th (0: not even one row's taps fit)
// the axes in the device layout above; odd ones are vertical and get the spans of tiles of th rows (none may reach more than max_rows)
int upload_axis_tables(const AxisTable *const *axes, int naxes, int th, int max_rows, DevBuf *dev, AxisTaps *out, hipStream_t stream);

// tm_scale.hip: RGB32 frames [n][h][stride] 0x00RRGGBB at another size.  probe_scale: the sizes and the filter;
// check_scale_args: those, the pointers, the strides in pixels and the overlap -- neither makes a device call.
int probe_scale(int src_w, int src_h, int dst_w, int dst_h, int filter);
int check_scale_args(const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, int src_w, int src_h, const void *dst, int64_t dst_stride_px,
                     int64_t dst_frame_px, int dst_w, int dst_h, int filter);
constexpr int SC_TW = 64, SC_HROWS = 80;  // a Lanczos workgroup's tile width, and the most source rows its tile may reach (ScaleTables::th is chosen for it)
struct ScaleTables {  // the tables of one (source size, output size, filter), kept until another is asked for
  int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0, filter = 0, th = 0;  // th: output rows per workgroup
  bool ready = false, on_device = false;
  AxisTable h, v;  // TM_SCALE_LANCZOS3 only
  DevBuf dev;
  AxisTaps taps_h{}, taps_v{};
  int prepare(int src_w, int src_h, int dst_w, int dst_h, int filter);  // host: every refusal of the size pair, no device call
  int upload(hipStream_t stream);                                       // drains the stream when there is something to upload
};
int launch_scale_rgb32(const ScaleTables &t, const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, void *dst, int64_t dst_stride_px,
                       int64_t dst_frame_px, hipStream_t stream);

// One process per GPU: the collectives a step needs between its kernels, handed in by the host (tm_set_collective).  The calls
// are made on the caller's thread with the encoder's stream idle, and return with the result in place.
struct Collectives {
  int rank = 0, world = 1;
  // the transport (kind: TM_COLL_*): an all-reduce works in place on send (recv null), an all-gather puts world x count bytes into recv
  std::function<int(int kind, const void *send, void *recv, int64_t count)> call;
  int allreduce_sum_i32(void *buf, int64_t count) const { return call(TM_COLL_ALLREDUCE_SUM_I32, buf, nullptr, count); }
  int allreduce_max_i32(void *buf, int64_t count) const { return call(TM_COLL_ALLREDUCE_MAX_I32, buf, nullptr, count); }
  int allreduce_sum_i64(void *buf, int64_t count) const { return call(TM_COLL_ALLREDUCE_SUM_I64, buf, nullptr, count); }
  int allgather(const void *send, void *recv, int64_t bytes_per_rank) const {  // recv: world x bytes_per_rank, rank order
    return call(TM_COLL_ALLGATHER_BYTES, send, recv, bytes_per_rank);
  }
};

// tm_group.hip: the in-process communicator of a device group (tm_set_devices).  Shard `rank` calls these from its own host thread with
// its own stream; they drain the stream, wait for the other shards at host barriers and return with the result in place.
constexpr int GROUP_MAX = 32;
struct GroupComm;
GroupComm *group_comm_create(const std::vector<int> &devices);
void group_comm_destroy(GroupComm *g);
void group_comm_reset(GroupComm *g);            // before a step, every shard idle: forget a failure of the last one
void group_comm_abort(GroupComm *g, int rank);  // shard `rank` failed: every barrier of the group gives up at once
int group_comm_broken_by(GroupComm *g);         // the shard that broke the group first, -1 if none
int group_allreduce(GroupComm *g, int rank, int kind, void *buf, int64_t count, hipStream_t stream);   // kind: TM_COLL_ALLREDUCE_*
int group_allgather(GroupComm *g, int rank, const void *send, void *recv, int64_t bytes, hipStream_t stream);
// dst[i] = sum / max over the nsrc sources' element i (TM_COLL_ALLREDUCE_* kinds; int32 sums wrap around); dst may be one of the sources
int launch_group_reduce(int kind, const void *const *srcs, int nsrc, int64_t n_elem, void *dst, hipStream_t stream);

// tm_palettize.hip (PreparePalettes) and tm_kmeans.hip (run_kmeans, run_kmeans_seeded, kmeans_run_stats)
// DoPalettization over `world` processes: every process holds the points of its own tile range (global index of the first:
// global_begin); the farthest-first picks are settled by an all-gather of one candidate per process, the Lloyd iterations by
// an all-reduce of the exact integer sums, so every process ends with the same centroids and with the assignment of its own
// range (out_pal_idx: n_local entries, already ranked by global tile count).
int run_palettize_dist(const void *feat_local, const void *use_local, int64_t n_local, int64_t global_begin, int npal, int max_iter,
                       void *out_pal_idx_local, const Collectives &co, hipStream_t stream);
int run_kmeans(const void *pts, const void *weights, int64_t n, int d, int k, int max_iter, void *assign, void *centroids, int *host_k,
               int *host_iters, hipStream_t stream);
// the same Lloyd iterations from the caller's own initial centres (k point indices, -1 = none) instead of the farthest-first picks
int run_kmeans_seeded(const void *pts, const void *weights, int64_t n, int d, int k, const int64_t *host_init_idx, int max_iter, void *assign, void *centroids,
                      int *host_k, int *host_iters, hipStream_t stream);
// keep_keys / keep_n (optional): the sorted distinct pixel keys palette << 24 | G << 16 | R << 8 | B the quantisation found, for Dither (u64 each)
// host_palettes (optional): the palettes go to this host array [npal][pal_size] INSTEAD of out_palettes (which may then be null): no upload, and
// the call does not wait for one
struct DevBuf;
int run_quantize_palettes(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter, void *out_palettes,
                          hipStream_t stream, DevBuf *keep_keys = nullptr, int64_t *keep_n = nullptr, int32_t *host_palettes = nullptr);
// the same for the palettes p with p % pal_world == pal_rank only (independent tasks, one thread per palette in the reference:
// tilingencoder.pas:1864); the other palettes' rows come back as zeros, so that an all-reduce(SUM) assembles the set
int run_quantize_palettes_part(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter, void *out_palettes,
                               int pal_rank, int pal_world, hipStream_t stream, DevBuf *keep_keys = nullptr, int64_t *keep_n = nullptr,
                               int32_t *host_palettes = nullptr);
int run_palettize(const void *feat, const void *use, int64_t n, int npal, int max_iter, void *out_pal_idx, hipStream_t stream);
// the seeding of that clustering alone: the k picked indices to the host (-1 beyond the centres found), *out_kk = centres found
int run_pp_seeds(const void *feat, const void *use, int64_t n, int k, int64_t *out_seeds_host, int *out_kk, hipStream_t stream);
bool palettize_resident(int64_t n, int npal);  // the clustering above would take the resident launch (then several processes each run it whole)
// tm_reduce_keys.hip, Reduce over several processes (see there): a 16-byte key per distinct tile (rows[idx[r]], use[r]) and, on the gathered keys of
// all processes, the tiles that can be among the first `target` of the merged order (in_s: uint32 flags)
int reduce_make_keys(const void *rows, const void *idx, const void *use, int64_t n, int row_bytes, void *keys_out /* n x 16 bytes */, hipStream_t stream);
int reduce_select_candidates(const void *keys, int64_t n, int64_t target, void *in_s, hipStream_t stream);
// tm_dl3.hip: dl3quant on device pointers (blocking)
int run_dl3quant(const void *dev_rgb, int64_t npixels, int quant_to, int lookup_bpc, void *dev_pal, int *out_colors, hipStream_t stream);
// what the calling thread's last tile -> palette clustering and last colour quantisation ran through (tm_get_kmeans_iters)
struct KmeansRunStats { int resident = 0 /* the last k-means of all ran in a resident launch to its end */; int tile_iters = 0; int64_t tile_points = 0; int pixel_iters = 0; int64_t pixel_colours = 0, pixels = 0, pixel_colour_iters = 0; int64_t look_scored = 0, look_exact = 0 /* the last D = 192 clustering's first look: point-scorings looked at, and those of them the double-precision chain settled */; };
KmeansRunStats &kmeans_run_stats();

// tm_kmodes.hip (the driver of tm_kmodes_init.hip and tm_kmodes_iter.hip): A17, TKModes.ComputeKModes (kmodes.pas:923-1094); host pointers
int run_kmodes(const uint8_t *rows, int64_t n, int k, int num_init, int nmod, int max_iter, int32_t *labels_out, uint8_t *cent_out, uint64_t *cost_out,
               int *iters_out, hipStream_t stream);

// tm_optpal.hip (host only)
int optimize_palettes_host(std::vector<int32_t> &pals, int pal_count, int pal_size, int *sweeps_out);

// tm_gtm.h: the .gtm container, write_gtm / read_gtm / probe_gtm, lz_compress / lz_decompress; tm_player.h: the player's host side

}  // namespace tmx
