// tm_encoder.h -- the encoder object behind tm_create / tm_run, shared by tm_encoder.hip, the steps (tm_steps.h), tm_shard.hip, the input
// side (tm_input.hip, tm_input_clip.hip, tm_input_files.hip) and what leaves the encoder (tm_gtm_api.hip, tm_render_api.hip, tm_export.hip).
#pragma once
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "tm_common.h"
#include "tm_internal.h"
#include "tm_input.h"

struct ncclComm;  // (RCCL's header: tm_shard.hip only)
struct tm_encoder;
void comm_abort(tm_encoder *e);  // tm_shard.hip: the native communicator, if any, goes without the collective handshake

namespace tmx {

struct Settings {
  std::string InputFileName, OutputFileName;
  int StartFrame = 0, FrameCount = 0;
  double Scaling = 1.0;
  int MotionPredictRadius = 32;
  bool GlobalTilingUseTargetPSNR = false;
  double GlobalTilingTargetPSNR = 20.0, GlobalTilingQualityBasedTileCount = 7.0;
  int GlobalTilingTileCount = 0;
  int PaletteSize = 16, PaletteCount = 1024;
  int DitheringMode = TM_PVS_WEIGHTED_SPE_DCT;
  bool DitheringUseThomasKnoll = true;
  int DitheringYliluoma2MixedColors = 4;
  bool FrameTilingExtendedPaletteUsage = true;
  int MaxThreadCount = 1;
  double ShotTransMaxSecondsPerKF = 15.0, ShotTransMinSecondsPerKF = 1.0, ShotTransCorrelLoThres = 0.8;
};

}  // namespace tmx

using namespace tmx;

struct tm_encoder {
  Settings s;
  int device = 0;
  hipStream_t stream = nullptr;
  tm_progress_cb cb = nullptr;
  void *cb_user = nullptr;
  // video (ReframeUI, tilingencoder.pas:2631-2638)
  int width = 0, height = 0, tm_w = 0, tm_h = 0, nframes = 0;
  double fps = 24.0;
  bool auto_tile_count = true;
  // device state
  DevBuf frames_owned;
  const void *frames = nullptr;  // [nframes][height][width] RGB32
  // the frame source "file" (tm_open_input): Load decodes InputFileName into a clip the encoder owns (tm_input.hip and its two source files, tm_input.h)
  InputInfo input;
  int input_yuv = TM_YUV_AUTO;
  InputTables input_tables;
  ScaleTables rgb_in_tables;         // the same for an RGB clip lent at another size (tm_set_frames_rgb)
  PinnedBuf input_pinned[2];         // the two staging buffers of a Y4M file's chunks
  std::vector<uint32_t> input_clip;  // a PNG sequence, decoded on the host, until Load has uploaded it
  const void *frames_host = nullptr;  // the same in HOST memory (tm_set_frames_host): Load copies it over in chunks beside its own kernel
  hipStream_t copy_stream = nullptr;
  // Clips that come from host memory land in one of two device buffers: the one the last Load read, and the one a prefetch
  // (tm_prefetch_frames_host) is filling for the next Load while this clip's later steps run.
  struct HostClip {
    DevBuf buf;
    const void *host = nullptr;       // the host clip it holds (or is being filled with)
    std::vector<hipEvent_t> events;   // one per chunk, recorded on the copy stream
    int chunk = 0, nchunks = 0;
    bool pending = false;             // filled (or being filled) by a prefetch that no Load has adopted yet
    uint64_t seq = 0;                 // order of the prefetches
  } hclip[2];
  int hclip_cur = -1;                 // the buffer `frames` points into, if any
  uint64_t hclip_seq = 0;
  // Load's inter-frame correlation is a chain of additions per frame (0.86 ms at 720p x 300) that nothing before the key frames' first
  // use waits for: it runs on a stream of its own beside Reduce, and its host tail (square roots, FindKeyFrames) is taken when somebody
  // asks (load_tail): a later step, a getter, the next Load
  hipStream_t stream_aux = nullptr;
  hipEvent_t ev_tiles = nullptr;
  DevBuf dcorrel;
  bool load_tail_pending = false;
  double kf_lo_thres = 0, kf_min_s = 0, kf_max_s = 0, kf_fps = 0;  // ShotTrans* and the frame rate at the time of that Load
  bool kf_manual = false;               // that Load read a PNG sequence: the key frames are the .kf files' (FindKeyFrames(AManualMode), 3380-3384)
  std::vector<int32_t> kf_manual_list;
  DevBuf ftiles, fflags, flab;   // frame tiles (canonical), mirror flags, Lab means
  DevBuf gtiles, gflags, guse, gpal_idx, gpal_px, palettes_dev;  // global tiles
  DevBuf tm_tile, tm_pal, tm_err;  // tile map, frame-major: TileIdx, PalIdx, error behind PSNR (KNN or motion)
  DevBuf pm_err, tm_px, tm_py, tm_pred;  // motion prediction: PredictMotion's best error, PredictedX/Y (int8), IsPredicted (uint8)
  bool has_pm = false;                   // PredictMotion ran with a radius > 0: Reduce and Reconstruct take their motion branches
  double reduce_threshold = 0;           // last PSNR threshold SolveTileCount evaluated
  int reduce_probes = 0;
  int64_t q = 0, t = 0;
  bool has_pal_px = false, reconstructed = false;
  bool gtiles_have_rgb = false;  // false after ReloadGTM until Reduce has run again
  // host state
  std::vector<float> correl;
  std::vector<int32_t> kf_start;
  std::vector<int32_t> palettes_host;
  std::vector<uint8_t> h_fflags;
  double stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  tm_save_stats save_stats{};  // of the last Save (tm_get_save_stats)
  bool has_save_stats = false;
  tm_png_options png_options{0, TM_PNG_FILTER_AUTO};  // what GeneratePNGs writes (tm_set_png_options); level 0: stored blocks
  tm_export_stats export_stats{};                      // of the last GeneratePNGs (tm_get_export_stats)
  bool has_export_stats = false;
  tm_jpeg_options jpeg_options{90, TM_JPEG_420, 1};    // what GenerateJPEGs / GenerateMJPEG write (tm_set_jpeg_options)
  tm_jpeg_export_stats jpeg_export_stats{};            // of the last of them (tm_get_jpeg_export_stats)
  bool has_jpeg_export_stats = false;
  tm_gif_options gif_options{TM_GIF_COLOURS_AUTO, 256, 1, 4096, 0, 0};  // what GenerateGIF writes (tm_set_gif_options)
  tm_gif_export_stats gif_export_stats{};                                // of the last GenerateGIF (tm_get_gif_export_stats)
  bool has_gif_export_stats = false;
  tm_webp_options webp_options{1, TM_WEBP_PALETTE_AUTO, 1, 4096, 0, 0};  // what GenerateWebP writes (tm_set_webp_options)
  tm_webp_export_stats webp_export_stats{};                              // of the last GenerateWebP (tm_get_webp_export_stats)
  bool has_webp_export_stats = false;
  int gif_decode = TM_PNG_DECODE_AUTO;  // where a GIF input is decoded (tm_set_gif_decode); TM_GIF_DECODE overrides
  int gif_background = -1;              // the canvas colour of a GIF input (tm_set_gif_background); -1: the file's
  int jpeg_decode = TM_PNG_DECODE_AUTO; // where a JPEG input is decoded (tm_set_jpeg_decode); TM_JPEG_DECODE overrides
  int png_decode = TM_PNG_DECODE_AUTO;  // where a PNG input is decoded (tm_set_png_decode); TM_PNG_DECODE overrides
  tm_input_stats input_stats{};          // of the last Load that read a PNG input (tm_get_input_stats)
  bool has_input_stats = false;
  int shard_first = 0, shard_count = -1;  // query frames this process matches in Reconstruct (multi-GPU: one shard per rank)
  DevBuf pair_keys;          // the distinct pixel keys PreparePalettes' quantisation sorted out, for Dither (valid while pair_keys_n > 0:
  int64_t pair_keys_n = 0;   // every step that rewrites the global tiles zeroes it)
  int64_t dither_pairs = 0;  // distinct (palette, colour) pairs the last Dither planned (0: every pixel on its own)
  int dither_rank = 0, dither_world = 1;  // tiles this process dithers: [t * rank / world, t * (rank + 1) / world)
  // one process per GPU (tm_set_collective): the steps shard their work over `world` processes and merge through the host's collectives
  tm_collective_cb coll_cb = nullptr;
  void *coll_user = nullptr;
  bool coll_stream_ordered = false;  // the callback enqueues on e->stream (tm_set_collective_mode): no drain before, no wait after
  Collectives co;
  bool load_sharded = false;     // Load only filled the frame tiles of this process's frames (and of the frame before them)
  bool src_tiles = false;        // the frame tiles are the current video's source (Load ran; ReloadGTM clears it): the input render's data
  int load_first = 0, load_count = 0;
  int64_t coll_calls[4] = {0, 0, 0, 0}, coll_bytes = 0;  // per kind, and the bytes this process put through them (tm_get_collective_stats)
  // the native communicator (tm_comm_init): RCCL linked into the library, the collectives queued on the encoder's stream
  ncclComm *comm = nullptr;
  bool force_dist = false;  // a one-rank communicator walks the sharded paths too (TM_COMM_FORCE_DIST=1: tests on a one-GPU box)
  // One process, several devices (tm_set_devices): the front encoder is shard 0 and owns the group; every shard's collectives go through
  // the group's in-process communicator (tm_group.hip), co.rank / co.world are its place in the group.
  struct Group *grp = nullptr;
  GroupComm *gcomm = nullptr;
  int pp_whole = -1;                // PreparePalettes' branch as the group decided it for all shards (-1: this encoder decides)
  const void *frames_peer = nullptr;  // tm_set_frames_device of a group whose clip lives on another device: Load pulls what it reads
  int frames_peer_dev = -1;
  bool dist() const { return (coll_cb != nullptr || comm != nullptr || gcomm != nullptr) && (co.world > 1 || force_dist); }
  // Query features of Reconstruct's first chunk, computed AHEAD on a second (non-blocking) stream: they depend on the frame tiles only.
  // Launched when PreparePalettes hands over to the host (OptimizePalettes' 2-5 ms search, then Dither's start), the one stretch where
  // the GPU idles; launched earlier they only trade time with the k-means kernels (measured: +3.8 ms there for -3.7 ms here).
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_qf = nullptr;
  DevBuf qf_pre;
  DevBuf qf_colmm;  // the prefetched distinct rows' column ranges (the feature kernel keeps them; Reconstruct's search reads them)
  int qf_f0 = -1, qf_nf = 0, qf_epu = -1;
  bool qf_valid = false;
  // Reduce's exact grouping of the frame tiles (motion prediction off, one process): group of every tile-map item and the first item of
  // every group.  Items of one group have the same pixels, hence the same features and the same nearest database row: Reconstruct
  // searches once per GROUP (3.2 of 4.3 million on the bench clip) and hands the answer to the group's items.
  DevBuf q_group, q_rep;
  int64_t q_groups = 0;
  bool qf_distinct = false;  // the prefetched features are the groups' (not a frame range's)
  void drop_prefetch() {  // never frees under a running kernel
    if (stream2) (void)hipStreamSynchronize(stream2);
    qf_valid = false;
    qf_pre.release();
  }
  ~tm_encoder() {
    drop_prefetch();
    comm_abort(this);
    if (ev_qf) (void)hipEventDestroy(ev_qf);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream_aux) { (void)hipStreamSynchronize(stream_aux); (void)hipStreamDestroy(stream_aux); }
    if (ev_tiles) (void)hipEventDestroy(ev_tiles);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    for (HostClip &c : hclip)
      for (hipEvent_t ev : c.events) (void)hipEventDestroy(ev);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
  }
  double knn_ms = 0;   // device time of the distance kernel, summed over launches of the last Reconstruct
  int64_t knn_pairs = 0;
  int knn_launches = 0, knn_kbytes = 0;
  double knn_split_ms[3] = {0, 0, 0};  // seeds / lists / consume kernels of those launches
  int64_t knn_split_pairs[3] = {0, 0, 0};
  KmeansRunStats km_stats;  // of the last PreparePalettes (single process: the sharded path runs its own loops)
  int64_t knn_db_rows = 0;  // distinct database rows actually searched
  int64_t knn_queries = 0;  // queries of the last Reconstruct's searches (distinct frame tiles when Reduce's groups are used)
  int steps_done = 0;  // bit per step

  int64_t tm_size() const { return (int64_t)tm_w * tm_h; }
};

inline void progress(tm_encoder *e, int step, int pos, int max) {
  if (e->cb) e->cb(e->cb_user, step, pos, max, 0);
}
inline int need(tm_encoder *e, int step_bit, const char *what) {
  TM_CHECK(e->steps_done & (1 << step_bit), TM_E_INVAL, "step order: %s has not been run", what);
  return TM_OK;
}

// tm_encoder.hip
void recompute_auto_tile_count(tm_encoder *e);
std::string settings_text(const Settings &s);

// tm_steps.hip (what the steps' three files share among themselves: tm_steps.h)
int run_step(tm_encoder *e, int step);
int load_tail(tm_encoder *e, hipStream_t st = nullptr);
int queue_host_clip(tm_encoder *e, int slot, const void *host);

// tm_input.hip
int load_from_input(tm_encoder *e);
// tm_input_clip.hip: frames [a, b) of a clip in memory or of a raw file into the encoder's device clip
int decode_y4m(tm_encoder *e, int a, int b);
int convert_yuv_clip(tm_encoder *e, int a, int b);
int convert_rgb_clip(tm_encoder *e, int a, int b);
int play_gtm(tm_encoder *e, int a, int b);
// tm_input_files.hip: the same of coded files (decode_pngs: the whole sequence on the host, into input_clip), and where each kind is decoded
int decode_pngs(tm_encoder *e);
int decode_pngs_device(tm_encoder *e, int a, int b);
int decode_jpegs(tm_encoder *e, int a, int b);
int decode_gif(tm_encoder *e, int a, int b);
int png_decode_where(const tm_encoder *e);
int jpeg_decode_where(const tm_encoder *e);
int gif_decode_where(const tm_encoder *e);

// tm_shard.hip
void share_of(int64_t n, int rank, int world, int64_t *lo, int64_t *hi);
int gather_var(tm_encoder *e, const void *send, int64_t count, int item, DevBuf &out, std::vector<int64_t> *counts);
int group_each(tm_encoder *e, const std::function<int(tm_encoder *)> &fn);
int group_run_step(tm_encoder *e, int step);
void group_teardown(tm_encoder *e);
struct Piece { int first = 0, count = 0; };
std::vector<Piece> group_pieces(tm_encoder *e, int first, int count);

// tm_gtm_api.hip
int save_to(tm_encoder *e, const char *path);

// tm_render_api.hip
// what the device renders check and read (tm_render_frames and its kin there, the exports, the views of tm_render_view.hip); no device call
int render_range_ok(tm_encoder *e, int first, int count);
int render_output_map(tm_encoder *e, RenderMap *m);
int render_input_src(tm_encoder *e, int first, int count, RenderInput *in);
// the source of a render: the source frames (input) or the decoded ones.  prepare makes the checks for frames [first, +count), draw launches
struct RenderSource {
  bool input = false;
  RenderMap m{};
  RenderInput in{};
  int prepare(tm_encoder *e, int first, int count) { return input ? render_input_src(e, first, count, &in) : render_output_map(e, &m); }
  int draw(int first, int nf, void *dst, hipStream_t stream) const {
    return input ? launch_render_input(in, first, nf, dst, stream) : launch_render_output(m, first, nf, dst, stream);
  }
};
// the frames a render chunk holds, of `frame_count` asked for: at most 32 frames or 256 MB of its larger frame, and at least one
inline int render_chunk_frames(int frame_count, size_t frame_bytes) {
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(frame_count, 32), ((size_t)256 << 20) / frame_bytes));
}
