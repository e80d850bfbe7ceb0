/*
 * tilemotion.h -- C ABI of libtilemotion.so: the MI355X (gfx950) implementation of the TileMotion
 * encoder's per-frame tile pipeline (gligli/tiler: tilingencoder.pas / utils.pas / extern.pas).
 *
 * Plain pointers and sizes only; every function returns 0 on success or a negative TM_E_* code, never
 * throws or aborts across the boundary.  tm_last_error() gives the message of the calling thread's last
 * failure.  There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 * TM_E_NODEVICE.
 *
 * Three layers, each replacing a reference seam (file:line in the reference tree):
 *   1. Coarse seam  tm_encoder_*  == TTilingEncoder's public surface (tilingencoder.pas:486-568):
 *      Create/Destroy, settings properties (3745-3770, clamps 2919-3047), frame callback contract of
 *      TFFMPEGFrameCallback (extern.pas:149), Run(step) with TEncoderStep values (tilingencoder.pas:18),
 *      read-only Tiles/Frames/Palettes views (509-512).
 *   2. Stage seam   tm_stage_*    == the per-step workers behind Run, on DEVICE pointers, so a host that
 *      owns several processes/GPUs (bench.py, tiler_amd.distributed) can put RCCL collectives between them.
 *   3. Fine seam    ann_kdtree_* / yakmo_* / bico_*  == the DLL imports of extern.pas:178-223, same
 *      per-call semantics, plus *_batch twins (per-call GPU use is latency bound; kept for compatibility).
 *
 * Several GPUs, two ways.  (a) One process, several devices: tm_set_device_mask / tm_set_devices right after tm_create make the encoder a
 * group of shards, one per listed device, and Run(step) shards and merges inside the library; the reference's single control thread
 * (tiler.lpr:64-70) needs that one call and nothing else.  The surveyed objections, answered: the group does
 * not use RCCL, which assumes a process per device -- its collectives are the library's own in-process ones (host barriers, peer copies
 * and a reduce kernel); the steps' host tails (OptimizePalettes, the key-frame logic, LZMA) do not queue on one thread -- every device
 * gets a host thread of its own; a fault or an out-of-memory on one device still takes the other shards with it -- that is the caller's
 * choice to make.  (b) One process per device, for those who want that isolation: N encoders become one job through tm_comm_init (RCCL
 * inside the library) or tm_set_collective (the host's own communicator), each process with a rank.
 *
 * Environment switches.  All are optional; they are sampled at the API boundary (tm_create, tm_run, every tm_stage_* and fine-seam entry)
 * and never read inside a step.  Set and not "0" = on.
 *   TM_KNN_DEBUG            one line per search on stderr: the three kernels' times, pairs evaluated, list sizes, matrix instructions
 *   TM_KNN_NOPRUNE          the nearest-neighbour scan evaluates every (query, row) pair (bench.py's dense diagnostic launch)
 *   TM_KNN_LIST_ORDER=0     the scan's tile lists stay in run order and are consumed to their ends (default: every list segment sorted by
 *                           its entries' smallest bound, and ended at the first entry no query can want; A/B runs and tests)
 *   TM_KNN_FIRST_CHUNK=0    the scan runs every listed block's whole chain (default: a block is judged on its 32 widest columns first and
 *                           ends there when no query of it can gain or tie; A/B runs and tests)
 *   TM_KNN_CURVE=morton|hilbert the order both sides of a KNN search (nearest neighbour and k nearest) are sorted in before they are cut into
 *                           tiles: the Hilbert index of a row's four quantised coordinates, or their interleaved bits.  The results are the same
 *                           either way; the boxes, and with them the work, are not (A/B runs and tests).  Not set: Hilbert,
 *                           except for the sampled rows the k-nearest search estimates its first thresholds from, which stay in Morton order
 *   TM_KNN_ARENA_ENTRIES=<n> first size of the scan's tile-list arena (tests: a tiny one, so that a search is repeated with the counted size)
 *   TM_TOPK_BRUTE           the k-nearest search by the VALU brute force (tests compare the pruned scan with it)
 *   TM_EPU_TABLE_GIB=<x>    above this size the (tile, palette) feature table is not built, the pairs asked for are (default 6)
 *   TM_NO_QUERY_GROUPS      Reconstruct searches once per tile-map item instead of once per distinct frame tile (tests)
 *   TM_DITHER_OWN_KEYS      Dither collects its (palette, colour) pairs itself instead of taking PreparePalettes' keys (tests)
 *   TM_DITHER_NO_DEDUP      Dither plans every pixel on its own (tests); TM_DITHER_LITERAL: every tile through the literal-sort kernel
 *   TM_DEDUP_PLAIN          exact dedup by the comparator sort alone; TM_DEDUP_SORT: equal rows grouped by the radix sort of their hashes
 *                           (the front end of rounds 1-4) instead of the hash table; TM_DEDUP_RADIX_MIN=n: the distinct rows go into content
 *                           order by a radix sort of their 8-byte prefixes (whole rows compared only within short runs of equal prefixes;
 *                           the comparator merge sort where a run is long) from n rows on (default 2^20; tests: 1); TM_DEDUP_DEGRADE_HASH: a 2-bit hash, so that every group
 *                           collides (tests); TM_DEDUP_FULL_ORDER: the whole order, not only the rows that can survive the budget (tests)
 *   TM_MOTION_VALU          the motion search's VALU kernel only (tests drive both kernels)
 *   TM_FEATURES_PLAIN       the int16 DCT features sum every coefficient in the reference's order (no separable first look; the tests
 *                           compare the two forms)
 *   TM_KM_LAUNCHES          the tile -> palette k-means runs its skipping iterations as three launches each instead of one resident launch
 *                           for all of them (tests compare the two)
 *   TM_KM_FIRST_LOOK=0      the plain iterations of the tile -> palette k-means score every point with the double-precision chain -- without
 *                           the single-precision first look that leaves the chain to the points it cannot decide (A/B runs; tests compare the two)
 *   TM_KMODES_BINWISE       every k-modes iteration bin by bin (two launches per 960 points) -- without the leg that scores all remaining points
 *                           at once and walks the bins in one launch for as long as no mode changes (tests compare the two);
 *                           TM_KMODES_FAST_ALWAYS: that leg is tried in every iteration after the first, also behind an iteration that moved many
 *                           points (tests: its stops and the hand-over to the bin-by-bin launches in the middle of an iteration)
 *   TM_FEATURES_BY_TILE     the int16 features of RGB tiles by the tile-at-a-time kernel (k_features_i16<0>) instead of eight tiles a wave
 *                           (k_features_tiles8; tests compare the two)
 *   TM_MOTION_PACK_SEPARATE the encoder's motion search as three launches per frame (int16 window features, their packing, the search) instead of
 *                           window features made in the search's layout at once (A/B runs, tests)
 *   TM_MOTION_FORCE_FLAG    treat every frame as beyond the matrix search's exact range: the fallback (int16 windows + VALU search) runs (tests)
 *   TM_TOPK_ESTIMATE        0: the k-nearest search never takes its first thresholds from a sample of the database (the curve window's bound instead);
 *                           1: whenever the database has rows enough for a sample (default: many queries against >= 16 384 rows)
 *   TM_KM_RESIDENT_FAIL     the resident launch of the tile k-means is treated as if its barrier had given up: the clustering is repeated from its
 *                           seeds through the launches (tests: the fallback's result must be the same)
 *   TM_WINDOW_DCTS_BY_TILE  the sliding-window features of motion prediction a window at a time (k_features_i16<2>) instead of by strips that share
 *                           the colour conversion and the row transforms between windows (tests compare the two)
 *   TM_PP_SHARDED           several processes: the tile -> palette clustering stays data-parallel (an all-reduce per Lloyd iteration) even where
 *                           every process could run it whole in one resident launch (tests, A/B)
 *   TM_PP_DEBUG             PreparePalettes prints its sub-steps' wall times (adds synchronisations)
 *   TM_COMM_FORCE_DIST      a one-process communicator still walks the sharded code paths (tests on a one-GPU box)
 *   TM_COMM_TIMEOUT_S=<s>   how long tm_comm_init (and a collective of the library's own communicator, or of a device group) waits for the
 *                           other processes or shards (120)
 *   TM_GROUP_FAIL_SHARD=<r> shard r of a device group fails with TM_E_INVAL ("forced") at the start of its next step, before it queues any work
 *                           (tests: the other shards must leave their collectives at once)
 *   TM_INPUT_CHUNK_FRAMES=<n> Load reads a Y4M file, or stages a lent YUV or RGB clip, n frames at a time instead of 16 MB worth (tests: 1, so that
 *                           a small clip walks the two staging buffers many times)
 *   TM_PNG_DECODE=host|device where the Load of a PNG sequence or of lent PNG files decodes, whatever tm_set_png_decode said;
 *                           with `device`, TM_INPUT_CHUNK_FRAMES=<n> is also the number of files a chunk holds
 *   TM_RECON_CHUNK_FRAMES=<n> Reconstruct computes and searches its query features n frames at a time instead of 8 GiB worth (2 GiB with the
 *                           extended palette usage); the features computed ahead during PreparePalettes are then those of the first n frames
 *                           (tests: a small clip takes several chunks)
 *   TM_PLAYER_NO_WORKER     tm_player_*: the next key frame is decoded when the last one has been played, on the calling thread, instead of
 *                           by a worker thread beside the playing (measurements: what the overlap buys)
 *   TM_PLAYER_CHUNK_FRAMES=<n> tm_player_*: item records go to the device n frames at a time instead of 8 MB worth, at most 16 (tests: 1 or 2,
 *                           so that a small clip walks the two staging buffers many times)
 *   TM_POOL_GIB=<x>         cap of the device-memory pool a thread keeps (96); TM_HOST_THREADS=<n>: OptimizePalettes' helper threads
 *                           (both read once per process)
 *   TM_HOST_THREADS=<n>     also: the threads Save codes its key frames' streams on, at most one per key frame and at most 16 (default: the
 *                           machine's, at most 16); this use is read at each Save.  1: one stream after the other on the calling thread
 *   TM_SAVE_FINDER=host|device  where Save's coder takes its match lists from: its own finder on the parser threads, or the device finder
 *                           (tm_lz_matches.hip) on the encoder's device with the parsers one window behind; read at each Save.  The file
 *                           is the same bytes either way.  Default: device for tm_save_gtm / esSave, host for tm_write_gtm_host (no device)
 *   TM_LZ_WINDOW=<n>        the device finder works in windows of n positions instead of 262144; read at each call (tests: small, so that
 *                           window edges fall inside matches)
 */
#ifndef TILEMOTION_H
#define TILEMOTION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TM_API __attribute__((visibility("default")))

enum {
  TM_OK = 0,
  TM_E_INVAL = -1,     /* bad argument / bad state (the reference would Assert) */
  TM_E_NODEVICE = -2,  /* no HIP device, or kernels for gfx950 cannot run here */
  TM_E_HIP = -3,       /* a HIP runtime call failed */
  TM_E_NOMEM = -4,
  TM_E_IO = -5,
  TM_E_UNSUPPORTED = -6, /* reference feature outside the hot path */
  TM_E_INTERNAL = -7     /* the library contradicted itself (a bug: the message says where); nothing was written */
};

/* TEncoderStep, tilingencoder.pas:18 */
enum { TM_STEP_ALL = -1, TM_STEP_LOAD = 0, TM_STEP_PREDICT_MOTION = 1, TM_STEP_REDUCE = 2, TM_STEP_PREPARE_PALETTES = 3,
       TM_STEP_DITHER = 4, TM_STEP_RECONSTRUCT = 5, TM_STEP_REINDEX = 6, TM_STEP_SAVE = 7 };

/* TPsyVisMode, tilingencoder.pas:21 */
enum { TM_PVS_DCT = 0, TM_PVS_WEIGHTED_DCT = 1, TM_PVS_WAVELETS = 2, TM_PVS_SPE_DCT = 3, TM_PVS_WEIGHTED_SPE_DCT = 4 };

#define TM_NULL_COLOR ((int32_t)0xffff00ff) /* cDitheringNullColor, utils.pas:45 */

/* TTile header, packed, 20 bytes (tilingencoder.pas:116-121).  Flags bits: 0 Active, 1 HasRGBPixels,
 * 2 HasPalPixels, 3 HMirror_Initial, 4 VMirror_Initial (FPC set, 4 bytes). */
#pragma pack(push, 1)
typedef struct { uint32_t UseCount; int32_t TmpIndex; int32_t MergeIndex; int32_t PalIdx_Initial; uint32_t Flags; } tm_tile_hdr;
/* TTileMapItem, packed, 18 bytes (tilingencoder.pas:178-184).  Flags bits: 0 HMirror, 1 VMirror, 2 Predicted. */
typedef struct { int32_t TileIdx; int32_t PalIdx; int8_t PredictedX; int8_t PredictedY; float PSNR; uint32_t Flags; } tm_tilemap_item;
#pragma pack(pop)

TM_API const char *tm_last_error(void);
TM_API int tm_device_count(void);           /* usable gfx950 devices, 0 if none */
TM_API const char *tm_version(void);
/* The peaks a roofline divides by, measured on this device: a bare loop of the int8 MFMA the KNN kernel issues
 * (two waves per SIMD, operands in registers; about `seconds_hint` seconds) in TOP/s, and a stream triad a = b + s c over three
 * arrays of `bytes_per_array` in GB/s.  Diagnostics for bench.py; nothing in the product path calls them. */
TM_API int tm_probe_mfma_i8(double seconds_hint, double *tops);
TM_API int tm_probe_hbm_triad(int64_t bytes_per_array, double *gb_per_s);
/* The all-reduce of a device group (tm_set_devices): mean wall time in us of `iters` int32 sum all-reduces of `bytes` between n shards
 * on `devices` (one host thread each, the stream drained before and after, as a step sees it).  A diagnostic for tools/group_bench.py. */
TM_API int tm_probe_group_allreduce(const int *devices, int n, int64_t bytes, int iters, double *us_per_call);

/* ======================================================================================= coarse seam */
typedef struct tm_encoder tm_encoder;
typedef void (*tm_progress_cb)(void *user, int step, int position, int max, int hourglass); /* OnProgress, :304 */

TM_API tm_encoder *tm_create(void);                 /* TTilingEncoder.Create, :5484; NULL on failure */
TM_API void tm_destroy(tm_encoder *);               /* Destroy, :5516 */
TM_API int tm_set_device(tm_encoder *, int device); /* which HIP device this encoder (process) drives */
/* One process, several devices: the encoder becomes a group of shards, one per listed device, each with its own host thread; Run(step)
 * shards and merges inside the library exactly as N processes under tm_comm_init do, and ends every step with the single encoder's state.
 * Only before tm_set_video; settings already made carry over to every shard.  A list of one device is tm_set_device.  TM_E_INVAL: mask 0, a
 * device outside 0 .. tm_device_count()-1, n < 1 or n > 32, an encoder with video, tm_set_collective or tm_comm_init; those two calls,
 * tm_set_query_shard and tm_set_dither_shard then refuse the group (it owns the sharding).  TM_E_UNSUPPORTED: two listed devices cannot
 * reach each other's memory.  The group is used from one host thread like any encoder; progress callbacks come from shard 0 only, on it. */
TM_API int tm_set_device_mask(tm_encoder *, uint32_t mask);              /* bit d = HIP device d */
TM_API int tm_set_devices(tm_encoder *, const int *devices, int n);     /* a device may repeat: several shards on one device */
/* Settings: keys are the INI names of SaveSettings (:3745-3770); setters clamp like :2919-3047. */
TM_API int tm_load_default_settings(tm_encoder *);  /* LoadDefaultSettings, :3817-3845 */
TM_API int tm_load_settings_ini(tm_encoder *, const char *path); /* LoadSettings, :3777 */
TM_API int tm_save_settings_ini(tm_encoder *, const char *path); /* SaveSettings, :3738-3775: the text a .gtm embeds (:5331-5335), CR LF line ends */
/* LoadSettings followed by SaveSettings on text (host only, no device): `ini_text` through the setters' clamps, back as the INI text
 * SaveSettings would write; *out_len = its length, `out` (may be NULL) receives up to cap - 1 bytes and a terminator. */
TM_API int tm_settings_text_host(const char *ini_text, char *out, int64_t cap, int64_t *out_len);
TM_API int tm_set_int(tm_encoder *, const char *key, int64_t v);
TM_API int tm_set_float(tm_encoder *, const char *key, double v);
TM_API int tm_set_bool(tm_encoder *, const char *key, int v);
TM_API int tm_set_str(tm_encoder *, const char *key, const char *v);
TM_API int tm_get_int(tm_encoder *, const char *key, int64_t *v);
TM_API int tm_get_float(tm_encoder *, const char *key, double *v);
TM_API int tm_set_progress_cb(tm_encoder *, tm_progress_cb cb, void *user);
/* Video: what FFMPEG_Open + ReframeUI + InitFrames establish (:1772-1776, :2631, :2661). */
TM_API int tm_set_video(tm_encoder *, int width, int height, double fps, int frame_count);
/* One decoded frame, AV_PIX_FMT_RGB32 (uint32 0xAARRGGBB), as TFFMPEGFrameCallback hands it (extern.pas:149);
 * read during the call only.  stride_px = pixels per row. */
TM_API int tm_push_frame_rgb32(tm_encoder *, int index, const uint32_t *pixels, int stride_px);
/* Same, but the frames already sit in device memory as [frame_count][height][width] uint32 (bench path). */
TM_API int tm_set_frames_device(tm_encoder *, const void *dev_frames);
/* Same, with the whole clip in HOST memory as [frame_count][height][width] uint32 (the batch form of the frame callback for a
 * host that holds the decoded clip).  The next Load moves it across PCIe in chunks, each chunk's copy running beside the Load
 * kernel of the chunk before; page-locked memory makes the copies asynchronous.  The clip is BORROWED until that Load has
 * returned; from then on the encoder reads its own device copy (a later Run(esLoad) without new frames reads that copy), and
 * the host may free or reuse the memory. */
TM_API int tm_set_frames_host(tm_encoder *, const uint32_t *host_frames);
/* Start moving the clip the NEXT Load will read while the current clip's steps still run (a second device buffer, the copy
 * stream): call it before tm_run of the current clip, then tm_set_frames_host with the same pointer before the next one -- that
 * Load adopts the copies instead of issuing its own, so back-to-back clips pay PCIe beside the compute, not before it.
 * Borrowed until the adopting Load has returned.  At most one clip can wait beside the one in flight (TM_E_INVAL otherwise);
 * with both buffers taken the clip of the LAST Load gives way, after which a Load without new frames fails ("no frames"). */
TM_API int tm_prefetch_frames_host(tm_encoder *, const uint32_t *host_frames);
/* The probe half of Load (:1764-1820): reads InputFileName, StartFrame, FrameCount and Scaling, does what tm_set_video(DstWidth, DstHeight,
 * fps, frames) does and makes the file the encoder's frame source; tm_run(TM_STEP_LOAD) then decodes it into a device clip the encoder owns
 * and goes on as if that clip had been set with tm_set_frames_device (a second Load without a new tm_open_input reads that clip again).
 * With no video described yet and InputFileName set, Load calls it itself.  tm_set_video, tm_push_frame_rgb32 and tm_set_frames_* (_device,
 * _host, _yuv, _rgb) switch the source back to memory (and the key frames back to the automatic rule).
 *   An existing file must be Y4M ('YUV4MPEG2 '): W, H, F num:den (fps = num / den), I and C tags, XCOLORRANGE=FULL|LIMITED; frames are
 * found by walking their 'FRAME...' headers, a last frame cut short does not count.  8-bit C444, C422, C420jpeg (also no C tag), C420mpeg2,
 * Cmono; Ip, I? or no I tag.  Anything else -- other layouts, deeper samples, interlaced video, a file that is not Y4M (FFmpeg stays out of
 * scope: DESIGN.md sections 9, 17; convert with `ffmpeg -i ... -f yuv4mpegpipe`) -- is TM_E_UNSUPPORTED with the tag in the message.
 * DstWidth = Round(W * Scaling), DstHeight = Round(H * Scaling), at least 1 (extern.pas:780-781); frames = the file's - StartFrame, or
 * FrameCount when > 0 (:1778-1782); a range that runs past the file is TM_E_INVAL.  The planes are uploaded as they are; chroma
 * upsampling, the Lanczos-3 resize (this build's integer rule, DESIGN.md section 17, in place of libswscale's: extern.pas:837-840) and
 * YUV -> RGB run on the device (tm_stage_yuv_to_rgb32).
 *   An existing file that starts with 'GTMv' is a .gtm stream: Load plays frames [StartFrame, StartFrame + FrameCount) with the player
 * (tm_player_*) into the device clip; the video is tm_w*8 x tm_h*8 at the stream's rate.  Key frames follow the automatic rule: the stream's
 * own are not taken over.  Scaling != 1 is TM_E_UNSUPPORTED (played frames are not resampled on the way in), refused here, before the stream is read.
 *   Otherwise the name is a Format pattern with one %d or %.Nd (%% = '%'): the PNG sequence Format(name, [i + StartFrame])
 * (LoadInputVideo, :3340-3353), fps 24 (:1791), FrameCount <= 0 counts files up to the first gap (:1797-1806), the size is the first
 * file's (:1813-1814; a later file of another size: TM_E_INVAL at Load), Scaling is ignored (:3347-3348).  Key frames are manual: frame 0
 * and every frame i for which Format(ChangeFileExt(name, '.kf'), [i + StartFrame]) exists (FindKeyFrames(AManualMode), :3380-3384). */
TM_API int tm_open_input(tm_encoder *);
TM_API int tm_get_video(tm_encoder *, int *width, int *height, double *fps, int *frames); /* as tm_set_video / tm_open_input left them; any pointer may be NULL */
/* How a Y4M clip's samples become RGB (not a settings key: the INI text is the reference's).  AUTO: BT601_FULL under XCOLORRANGE=FULL, else
 * BT601_LIMITED (what FFmpeg assumes for an untagged file).  TILER: YUVToRGB(Y, U - 128, V - 128) (utils.pas:492-509), for files of
 * tm_generate_y4m.  BT709_LIMITED / BT709_FULL: the matrix of HD sources (Kr = 0.2126, Kb = 0.0722), never chosen by AUTO -- name it.  With
 * D = U - 128, E = V - 128 and every channel clamped to 0 .. 255:
 *   BT709_LIMITED, C = Y - 16:  R = (298C + 459E + 128) >> 8,  G = (298C - 55D - 136E + 128) >> 8,  B = (298C + 541D + 128) >> 8
 *   BT709_FULL:  R = (65536Y + 103206E + 32768) >> 16,  G = (65536Y - 12276D - 30679E + 32768) >> 16,  B = (65536Y + 121609D + 32768) >> 16
 * (round(k 2^n) of the matrix; the limited rule scales luma by 255/219 and chroma by 255/224). */
enum { TM_YUV_AUTO = 0, TM_YUV_BT601_LIMITED = 1, TM_YUV_BT601_FULL = 2, TM_YUV_TILER = 3, TM_YUV_BT709_LIMITED = 4, TM_YUV_BT709_FULL = 5 };
TM_API int tm_set_input_yuv(tm_encoder *, int mode);
enum { TM_INPUT_Y4M = 1, TM_INPUT_PNGS = 2, TM_INPUT_GTM = 4 };
/* chroma layouts: where the U / V samples sit among the luma samples (420jpeg: centred in both axes; 420mpeg2 and 422: on the even luma
 * columns, 420mpeg2 centred vertically); odd luma sizes give planes of (n + 1) / 2 samples */
enum { TM_CHROMA_444 = 0, TM_CHROMA_422 = 1, TM_CHROMA_420JPEG = 2, TM_CHROMA_420MPEG2 = 3, TM_CHROMA_MONO = 4 };
/* A YUV clip LENT in memory, as a decoder leaves it: planar (yuv420p and its kin), or with U and V interleaved (NV12, P010, P016), 8-bit or
 * 9 .. 16-bit samples in little-endian words, in host memory or on a device.  U16_LOW holds the sample in the low `depth` bits of the word
 * (yuv420p10le), U16_HIGH in the high bits (P010, P016).  A deep sample becomes a byte where it is fetched, and everything after that is the
 * 8-bit rule bit for bit:
 *   p_d = word & (2^d - 1) (U16_LOW: the bits above the depth are ignored),  p_d = word >> (16 - d) (U16_HIGH: the low bits are ignored)
 *   p = min(255, (p_d + 2^(d-9)) >> (d - 8))                                 (10-bit limited range 64 .. 940 lands on 16 .. 235)
 * With v == NULL the plane u has cw (U, V) pairs per row: U is sample 2k, V sample 2k + 1 of the row; nothing else differs from two planes.
 * Strides are in bytes.  The struct is 120 bytes: y 0, u 8, v 16, the six strides 24 .. 64, width 72, height 76, frames 80, fps 88, chroma 96,
 * samples 100, depth 104, full_range 108, memory 112. */
enum { TM_SAMPLES_U8 = 0, TM_SAMPLES_U16_LOW = 1, TM_SAMPLES_U16_HIGH = 2 };
enum { TM_MEM_HOST = 0, TM_MEM_DEVICE = 1 };
typedef struct {
  const void *y, *u, *v;          /* v == NULL: u holds interleaved (U, V) pairs, U first (NV12, P010, P016) */
  int64_t y_row, y_frame, u_row, u_frame, v_row, v_frame;   /* bytes */
  int width, height, frames; double fps;
  int chroma;                     /* TM_CHROMA_*; MONO: u, v unused */
  int samples, depth;             /* U8: depth 8.  U16_*: little-endian words, depth 9..16 */
  int full_range;                 /* what XCOLORRANGE says for a file: feeds TM_YUV_AUTO */
  int memory;                     /* TM_MEM_* */
} tm_yuv_clip;
/* What tm_open_input does for a file, for a clip in memory: reads Scaling, describes the video as Round(width Scaling) x Round(height Scaling)
 * (each at least 1; shrinking by more than 8 is TM_E_UNSUPPORTED) with the struct's fps and frame count, and makes the clip the frame source
 * of the next tm_run(TM_STEP_LOAD), which converts it on the device as it does a Y4M file's planes.  StartFrame and FrameCount do not apply;
 * the key frames follow the automatic rule.  The planes are BORROWED until that Load has returned; from then on the encoder reads its own
 * RGB32 clip: a second Load with the same tm_set_input_yuv mode reads that clip again, one with another mode (or a larger share of the frames)
 * is TM_E_INVAL -- lend the clip again.  tm_set_video, tm_push_frame_rgb32, tm_set_frames_* (tm_set_frames_rgb among them) and tm_open_input
 * switch the source away.
 *   Planes on the encoder's own device (TM_MEM_DEVICE; the owner is asked of the runtime) are converted where they are.  Planes in host
 * memory or on another device of a group go through two staging buffers in chunks (TM_INPUT_CHUNK_FRAMES applies), straight from page-locked
 * memory, through the encoder's own page-locked buffers from pageable memory.
 *   TM_E_INVAL, before anything is stored and before any device call: a null struct or y; chroma missing for a layout that has it, or v
 * without u; width or height outside 1 .. 65536; frames < 1; fps <= 0; an unknown chroma, samples or memory value; depth != 8 with U8 or
 * outside 9 .. 16 with U16_*; a row stride shorter than the plane's row in bytes (interleaved rows are twice as long); an odd pointer or
 * stride with 16-bit samples; a negative frame stride.  A refused call leaves the encoder as it was.
 *   tm_probe_yuv_clip_host is the host-only seam: the same checks and the size tm_set_frames_yuv would describe (pointers may be NULL). */
TM_API int tm_set_frames_yuv(tm_encoder *, const tm_yuv_clip *clip);
TM_API int tm_probe_yuv_clip_host(const tm_yuv_clip *clip, double scaling, int *dst_width, int *dst_height);
/* An RGB clip LENT in memory, as its producer leaves it (tm_rgb_in.hip): three pointers and one step describe every
 * layout -- RGB24 (g = r + 1, b = r + 2, step 3), BGRA (b = base, g = base + 1, r = base + 2, step 4), RGB48 (step 6, words), gbrp (three
 * planes, step 1), [N,3,H,W] (pointers one plane apart, frame = three planes), grey (r = g = b).  Alpha and padding bytes are never read as
 * samples.
 *   Sample: the sample of channel c at (f, y, x) is the byte or word at c + f frame + y row + x step; words become bytes by tm_yuv_clip's
 * rule, bit for bit: U16_LOW p_d = word & (2^d - 1), U16_HIGH p_d = word >> (16 - d), then p = min(255, (p_d + 2^(d-9)) >> (d - 8)).
 *   Pixel: the unscaled pixel is R << 16 | G << 8 | B, top byte 0.
 *   Size: the video is Round(width Scaling) x Round(height Scaling), as tm_set_frames_yuv describes it.  At that size equal to the source's
 * the clip is the unscaled pixels; otherwise every frame is TM_SCALE_LANCZOS3 of the unscaled frame, exactly as tm_scale_rgb32_host computes it.
 * The struct is 88 bytes: r 0, g 8, b 16, step 24, row 32, frame 40, width 48, height 52, frames 56, fps 64, samples 72, depth 76, memory 80. */
typedef struct {
  const void *r, *g, *b;      /* the R, G, B sample of pixel (0, 0) of frame 0; may be equal (grey) */
  int64_t step, row, frame;   /* bytes from a channel's sample to its right neighbour, to the row below, to the next frame; shared by the three channels */
  int width, height, frames; double fps;
  int samples, depth;         /* TM_SAMPLES_U8: depth 8.  TM_SAMPLES_U16_LOW / _HIGH: little-endian words, depth 9 .. 16 */
  int memory;                 /* TM_MEM_HOST, TM_MEM_DEVICE */
} tm_rgb_clip;
/* tm_set_frames_yuv's twin in every respect but the samples: reads Scaling, describes the video, and makes the clip the frame source of the
 * next tm_run(TM_STEP_LOAD).  StartFrame and FrameCount do not apply; the key frames follow the automatic rule.  The clip is BORROWED until
 * that Load has returned; a second Load reads the encoder's own RGB32 clip again, one that needs a larger share of the frames is TM_E_INVAL
 * -- lend the clip again.  tm_set_input_yuv plays no part.  tm_set_video, tm_push_frame_rgb32, tm_set_frames_* and tm_open_input switch the
 * source away.  A clip on the encoder's own device is converted where it is; host memory and other devices go through the two staging
 * buffers (TM_INPUT_CHUNK_FRAMES applies): an interleaved clip -- the three pointers within one step of the lowest -- as one plane from the
 * lowest pointer, otherwise every distinct channel pointer as a plane of its own.
 *   TM_E_INVAL, before anything is stored and before any device call: a null struct or channel; width or height outside 1 .. 65536;
 * frames < 1; fps <= 0; an unknown samples or memory value; depth != 8 with U8 or outside 9 .. 16 with words; step < bytes per sample;
 * row < (width - 1) step + bytes; a negative frame; an odd pointer, step or stride with words.  TM_MEM_DEVICE pointers that are not device
 * memory are TM_E_INVAL at Load.  TM_E_UNSUPPORTED: a shrink beyond 8.  A refused call leaves the encoder as it was.
 *   tm_probe_rgb_clip_host: the same checks and the size, with no device; pointers are only compared, never read.  tm_rgb_to_rgb32_host:
 * the rule in plain loops on host memory -- frames [first_frame, +frame_count) unpacked, then scaled as tm_scale_rgb32_host scales them,
 * into out [frame_count][dst_h][dst_w].  tm_stage_rgb_to_rgb32 (k_rgb_unpack / k_rgb_to_rgb32): the kernel alone on device pointers, every
 * frame of the clip, on the current device, queued on `stream`; it returns after the launch at equal size and drains the stream otherwise. */
TM_API int tm_set_frames_rgb(tm_encoder *, const tm_rgb_clip *clip);
TM_API int tm_probe_rgb_clip_host(const tm_rgb_clip *clip, double scaling, int *dst_width, int *dst_height);
TM_API int tm_rgb_to_rgb32_host(const tm_rgb_clip *clip, int first_frame, int frame_count, int dst_w, int dst_h, uint32_t *out);
TM_API int tm_stage_rgb_to_rgb32(const tm_rgb_clip *clip, int dst_w, int dst_h, void *out_rgb32, void *stream);
/* ---- Frames delivered as YUV (tm_yuv_out.hip): the mirror image of the above ----------------------------------------
 * A destination has tm_yuv_clip's field layout (same offsets, 120 bytes); its plane pointers are WRITTEN.  `frames` is its capacity, fps is
 * not read, v == NULL means u takes interleaved (U, V) pairs, memory is TM_MEM_HOST or TM_MEM_DEVICE (the device of the player / encoder).
 * width and height must equal the frames being delivered (tm_w*8 x tm_h*8); odd sizes give chroma planes of (n + 1) / 2 samples.
 *   The rule.  For BT601_LIMITED / _FULL and BT709_LIMITED / _FULL the forward matrix follows from Kr, Kb (0.299 / 0.114, 0.2126 / 0.0722):
 * Y = (Kr, Kg, Kb) ys, U = (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)) cs, V = (1 - Kr, -Kg, -Kb) / (2 (1 - Kr)) cs; limited: ys = 219/255, cs = 224/255.
 * The constants are round(k 65536), the G coefficient of a row absorbing the rounding so that the Y row sums to round(ys 65536) and the U and
 * V rows to 0 (grey stays grey); tm_yuv_out_matrix_host gives them (rows Y, U, V; columns R, G, B).  A sample at depth d is
 *   ((c . S + half) >> s) + off, clamped to 0 .. 2^d - 1;   s = 16 - (d - 8) + lw, half = 1 << (s - 1)
 * with S the weighted sum of R, G, B over the sample's footprint (weights totalling 2^lw) and off = 16 << (d - 8) for limited luma, 0 for
 * full luma, 128 << (d - 8) for chroma.  Footprints: the pixel itself for luma and 4:4:4 chroma; the 2 x 2 block for 420JPEG; columns 2k - 1,
 * 2k, 2k + 1 with weights 1, 2, 1 for 422; those columns on rows 2j and 2j + 1 for 420MPEG2.  Coordinates outside the picture repeat the edge
 * pixel.  MONO writes luma only.  U16_LOW stores the d-bit value in the low bits, U16_HIGH shifted left by 16 - d (d = 9 .. 16).
 *   Only the limited rules take deep samples (scale 2^(d-8): 64 .. 940 at 10 bits).  A full-range rule with deep samples is
 * TM_E_UNSUPPORTED: its standard scale, (2^d - 1) / 255, is not a shift, and nothing here consumes it.  TM_YUV_TILER is tm_generate_y4m's
 * arithmetic bit for bit (RGBToYUV, utils.pas:478-490: double products narrowed once to Single, + 128 in Single, round half to even, clamp),
 * defined for 8-bit 4:4:4 and MONO only: anything else with it is TM_E_INVAL.  TM_YUV_AUTO: BT601_FULL when full_range is set, else
 * BT601_LIMITED.
 *   TM_E_INVAL, before any device call and with nothing written: a null struct or y; chroma pointers missing for a layout that has them (or v
 * without u); a size that differs from the frames'; frames < 1 or fewer than the call delivers; unknown chroma, samples, memory or mode
 * values; depth != 8 with U8 or outside 9 .. 16 with words; a row stride shorter than the row (pairs: twice as long); an odd pointer or
 * stride with words; a negative frame stride.  U8 planes may sit at any byte address; 16-byte aligned rows get the widest stores.
 * tm_probe_yuv_out_host makes these checks and nothing else. */
typedef struct {
  void *y, *u, *v;                /* v == NULL: u takes interleaved (U, V) pairs, U first (NV12, P010, P016) */
  int64_t y_row, y_frame, u_row, u_frame, v_row, v_frame;   /* bytes */
  int width, height, frames; double fps;
  int chroma;                     /* TM_CHROMA_*; MONO: u, v unused */
  int samples, depth;             /* U8: depth 8.  U16_*: little-endian words, depth 9..16 */
  int full_range;                 /* feeds TM_YUV_AUTO */
  int memory;                     /* TM_MEM_* */
} tm_yuv_out;
TM_API int tm_probe_yuv_out_host(const tm_yuv_out *dst, int width, int height, int mode);
/* Host seams of the pixel rule (no device): the integer matrix of a mode (TM_E_INVAL for AUTO and TILER), and n pixels 0x00RRGGBB through the
 * one-pixel footprint at `depth` (8 .. 16; the d-bit values, unshifted; AUTO = BT601_LIMITED; any of y, u, v may be NULL). */
TM_API int tm_yuv_out_matrix_host(int mode, int32_t m[9]);
TM_API int tm_rgb32_to_yuv_host(const uint32_t *rgb, int64_t n, int mode, int depth, uint16_t *y, uint16_t *u, uint16_t *v);
/* Host-only seams of the above (no device needed).  tm_probe_input_host: what tm_open_input would find (kind: TM_INPUT_*; width, height:
 * the file's; any pointer may be NULL).  tm_read_png_host: a non-interlaced 8-bit PNG (grey, grey + alpha, RGB, RGBA, palette; alpha
 * dropped; CRCs and Adler-32 checked) as 0x00RRGGBB; out_rgb32 NULL gives the size only.  tm_inflate_host: one zlib stream (stored, fixed
 * and dynamic blocks); TM_E_INVAL for a damaged or truncated stream or one longer than cap.  tm_resample_taps_host: the resampling table
 * of one axis -- n luma samples in, m out, a plane of np samples at luma positions s k + o_halves / 2 (s 1 or 2) -- as the first tap,
 * the number of taps and the coefficients in 1/16384 (64 per output sample, unused ones 0); TM_E_UNSUPPORTED when n / m / s > 8. */
#define TM_RESAMPLE_MAX_TAPS 64
TM_API int tm_probe_input_host(const char *name, int start_frame, int frame_count, double scaling, int *kind, int *width, int *height, int *dst_width,
                               int *dst_height, double *fps, int *frames, int *chroma);
TM_API int tm_read_png_host(const char *path, uint32_t *out_rgb32, int64_t cap_px, int *width, int *height);
TM_API int tm_inflate_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n);
TM_API int tm_resample_taps_host(int n, int m, int np, int s, int o_halves, int32_t *first /* [m] */, int32_t *count /* [m] */, int32_t *coef /* [m][64] */);
TM_API int tm_run(tm_encoder *, int step);          /* Run(AStep), :5529-5554; blocking */
/* read-back views (copy-out) */
TM_API int tm_get_counts(tm_encoder *, int64_t *tiles, int *frames, int *palettes, int *tm_w, int *tm_h, int *keyframes);
TM_API int tm_get_tile(tm_encoder *, int64_t i, tm_tile_hdr *hdr, uint8_t pal_px[64], uint32_t rgb_px[64]);
TM_API int tm_get_tiles(tm_encoder *, int64_t first, int64_t count, tm_tile_hdr *hdrs, uint8_t *pal_px, uint32_t *rgb_px);
TM_API int tm_get_tilemap(tm_encoder *, int frame, tm_tilemap_item *items /* tm_w*tm_h */);
/* Frames[first_frame .. first_frame+frame_count-1].TileMap in one call (tilingencoder.pas:178-184, 509-512): the packed 18-byte items are
 * put together on the device and cross PCIe in one copy (at the link's rate when `items` is page-locked memory); the per-frame form above is
 * this with frame_count = 1. */
TM_API int tm_get_tilemaps(tm_encoder *, int first_frame, int frame_count, tm_tilemap_item *items /* frame_count*tm_w*tm_h */);
TM_API int tm_get_palette(tm_encoder *, int i, int32_t *rgb /* PaletteSize */);
TM_API int tm_get_keyframes(tm_encoder *, int32_t *start_frames /* keyframes */);
TM_API int tm_get_frame_correlations(tm_encoder *, float *correl /* frames */);
/* TKeyFrame.LogPSNR (:1006-1028): mean "PSNR-HVS (by tile)" of every key frame (the items' PSNR summed in a Double, divided by tile-map
 * size x frames of the key frame) and of the whole clip; what the reference prints after Reconstruct.  Either pointer may be NULL. */
TM_API int tm_get_psnr(tm_encoder *, double *per_keyframe /* keyframes */, double *global_mean);
TM_API int tm_get_stage_ms(tm_encoder *, double ms[8]); /* wall ms of the last run of each step (ProgressRedraw, :3925) */
TM_API int tm_save_gtm(tm_encoder *, const char *path);  /* Save, :2040 -> SaveStream, :5177 */
/* The same writer on HOST arrays (no device needed): tiles in their final (Reindex) order with use counts, palettes
 * [pal_count][pal_size], tile maps [nframes][tm_h*tm_w].  What SaveStream reads from FTiles/FPalettes/FFrames. */
TM_API int tm_write_gtm_host(const char *path, int tm_w, int tm_h, int nframes, double fps, const int32_t *kf_start, int nkf,
                             const uint8_t *pal_px, const uint32_t *use, int64_t ntiles, const int32_t *palettes, int pal_count,
                             int pal_size, const tm_tilemap_item *tilemap, const char *settings_text);
/* LZCompress, extern.pas:420-439 (LZMA-alone: lc 8, lp 0, pb 2, 4 MiB dictionary, unknown size, end marker), host
 * buffers.  *out_n = compressed size; TM_E_INVAL (with *out_n set) when cap is too small. */
TM_API int tm_lz_compress_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n);
/* The coder's match finder on its own.  The list of position i of a stream is a function of (src, n, i): the
 * records of the running maximum of the match length over the nearest earlier position with the same two bytes, the nearest with the same
 * 3-byte hash, then up to 96 positions of the 4-byte hash chain, nearest first, all within 4 MiB; lengths strictly increase, end at
 * min(273, n - i), and a list holds at most 98 pairs.  A table of lists is CSR: a uint8 count per position, the pairs of all positions in a row.
 * tm_lz_matches_host: the lists of positions [first, first + count); *npairs = pairs needed/written, TM_E_INVAL (with *npairs set) when
 * cap_pairs is too small, TM_E_UNSUPPORTED for n >= 2^31.
 * tm_lz_compress_from_matches_host: the parser and range coder of tm_lz_compress_host on lists the caller supplies for all n positions
 * (the same capacity convention); with the finder's lists it writes tm_lz_compress_host's bytes. */
typedef struct tm_lz_pair {
  uint16_t len;
  uint16_t zero; /* padding, written as 0 */
  uint32_t dist; /* distance - 1 */
} tm_lz_pair;
TM_API int tm_lz_matches_host(const uint8_t *src, size_t n, size_t first, size_t count, uint8_t *counts_u8, tm_lz_pair *pairs, size_t cap_pairs,
                              size_t *npairs);
TM_API int tm_lz_compress_from_matches_host(const uint8_t *src, size_t n, const uint8_t *counts_u8, const tm_lz_pair *pairs, uint8_t *dst, size_t cap,
                                            size_t *out_n);
/* The same finder on the device (tm_lz_matches.hip: three stable key sorts of the positions, then one lane per position over its chain's
 * stretch of the sorted order).  tm_stage_lz_matches: dev_src = the stream's n bytes in DEVICE memory; the counts and pairs of positions
 * [first, first + count) into DEVICE memory, exactly tm_lz_matches_host's; *host_npairs = pairs needed/written, TM_E_INVAL (with
 * *host_npairs set, nothing written to dev_pairs) when cap_pairs is too small, TM_E_UNSUPPORTED for n >= 2^31.  It returns synchronised.
 * tm_stage_lz_compress: HOST bytes in, tm_lz_compress_host's bytes out (the same capacity convention): the bytes are uploaded, the device
 * finder runs window by window and the host parser follows one window behind on a helper thread.  TM_LZ_WINDOW=<n> (read at each call)
 * sets the window to n positions instead of 262144 (tests: small, so that window edges fall inside matches). */
TM_API int tm_stage_lz_matches(const uint8_t *dev_src, size_t n, size_t first, size_t count, uint8_t *dev_counts_u8, tm_lz_pair *dev_pairs,
                               size_t cap_pairs, size_t *host_npairs, void *stream);
TM_API int tm_stage_lz_compress(const uint8_t *host_src, size_t n, uint8_t *dst, size_t cap, size_t *out_n);
/* What the encoder's last Save did (tm_save_gtm): TM_E_INVAL before the first one.  Save codes the key frames' streams side by side on up
 * to min(key frames, TM_HOST_THREADS, 16) helper threads, with the match lists from the device finder (TM_SAVE_FINDER=device, the default:
 * DESIGN.md section 33 has the measurement behind it) or from the coder's own (TM_SAVE_FINDER=host); both switches are read at each Save,
 * and TM_SAVE_FINDER=host with TM_HOST_THREADS=1 is the one-thread writer of before.  The file is the same bytes in every case. */
typedef struct tm_save_stats {
  int64_t raw_bytes, comp_bytes; /* the sums of the GTMk entries */
  int32_t key_frames, threads;   /* threads: the parser threads that ran */
  int32_t finder, reserved;      /* TM_SAVE_FINDER_* */
  double ms_commands;            /* building the command bytes */
  double ms_finder;              /* the device finder: upload, sorts, windows, read-back, each timed behind a synchronise (0 with the host finder) */
  double ms_parse;               /* parser + range coder (with the host finder: its finder too), summed over the threads */
  double ms_wall;                /* the whole Save */
} tm_save_stats;
enum { TM_SAVE_FINDER_HOST = 0, TM_SAVE_FINDER_DEVICE = 1 };
TM_API int tm_get_save_stats(tm_encoder *, tm_save_stats *out);
/* LZDecompress, extern.pas:441-458: one stream; *out_n = decoded size (set even when cap is too small -> TM_E_INVAL),
 * *consumed (optional) = bytes of src the stream occupied, so that the next key frame's stream can follow. */
TM_API int tm_lz_decompress_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n, size_t *consumed);
/* GenerateY4M (:2126-2199) and GeneratePNGs (:2075-2124): the frames as Render draws them with the constructor's defaults
 * (predicted items copied from the previous output frame, tiles through the item's palette and mirrors; :3573-3640, :5505-5507), or the
 * source frames (input != 0).  Y4M: 'YUV4MPEG2 W.. H.. F..:1000000 Ip C444', full-resolution Y, U + 128, V + 128 planes from RGBToYUV
 * (utils.pas:478-490), rounded and clamped.  PNGs: <OutputFileName without extension>_NNNN.png (24-bit RGB) + <...>.txt with the
 * palettes, one 'FFBBGGRR' line per colour.  Host code (export tooling); the Y4M planes are made on the device (TM_YUV_TILER) and cross as 3 bytes a pixel. */
TM_API int tm_generate_y4m(tm_encoder *, const char *path, int input);
TM_API int tm_generate_pngs(tm_encoder *, int input);
/* ---- Compressed PNG export: row filters and deflate on the device (tm_png_out.hip; the rule: tm_deflate.h) ----------
 * level 0 (the default) writes the picture in stored blocks, the bytes GeneratePNGs has always written.  level 1 codes the filtered rows --
 * colour type 2, 8 bits, one IDAT -- in segments of 32768 stream bytes: per position the longest match among the 32 nearest earlier
 * positions with the same three bytes within 32768 bytes (never past the segment's end; a match of 3 further than 4096 back is dropped), a
 * greedy parse, and per segment one dynamic-Huffman block (length-limited codes) or a stored block when that is no larger, an empty
 * stored block between segments.  The file is a function of the pixels and the options alone: the device form (filter, key sort, match,
 * parse, histograms, pack and compaction in kernels; the code lengths on up to min(TM_HOST_THREADS, 16) host threads, one round trip per
 * chunk of frames) and the host twin write the same bytes.
 *   filter: NONE = type 0 on every row; ADAPTIVE = per row the type 0..4 with the least sum of |(int8) byte| (ties to the lowest type);
 * SMALLER = both are coded, the shorter file is kept (a tie: NONE); AUTO = NONE for the Output page, ADAPTIVE for the Input page, resolved
 * by tm_generate_pngs -- the seams below take AUTO as NONE.
 *   tm_set_png_options: what tm_generate_pngs writes from then on (TM_E_INVAL: null, unknown level or filter).  tm_get_export_stats: the
 * last tm_generate_pngs (TM_E_INVAL before the first): ms_device = render, coding and read-back, ms_write = the files (at level 0 with
 * the host's packing of the pixels into them), both inside ms_wall.
 *   tm_png_bound_host: an upper bound of one file's size for any options (TM_E_INVAL: w or h outside 1 .. 32768, a stream of 2^31 bytes or more).
 *   tm_stage_png_encode: nframes pictures [h][w] of 0x00RRGGBB in DEVICE memory, rows stride_px apart, frames frame_px apart (pixels), as
 * files laid one behind the other in HOST memory host_out, file f at [offsets[f], offsets[f + 1]).  tm_png_encode_host: the same from HOST
 * frames without a device, byte for byte.  tm_stage_zlib_compress / tm_zlib_compress_host: the stream coder alone, n bytes to one zlib
 * stream.  Refusals, TM_E_INVAL before any device call and with nothing written: a null pointer, an unknown level or filter, w or h
 * outside 1 .. 32768, n >= 2^31, nframes < 0, a row stride shorter than the row with more than one row, a frame stride shorter than a
 * frame with more than one frame.  A cap too small is TM_E_INVAL too, with offsets[nframes] (or *out_n) set to the bytes needed and
 * host_out untouched; it can only be known once the pictures are coded, and the coded files are dropped: size host_out by
 * tm_png_bound_host (nframes times it for tm_stage_png_encode, n + 10 (n / 32768 + 1) + 6 for a stream) and the call is made once.
 * The stage calls return synchronised.
 *   tm_png_filter_rows_host: the stream the coder sees, h (1 + 3 w) bytes (filter NONE or ADAPTIVE).  tm_deflate_code_lengths_host: the
 * rule's length-limited code lengths of nsym (2 .. 288) frequencies, max_bits 1 .. 15 with 2^max_bits >= nsym. */
enum { TM_PNG_FILTER_AUTO = 0, TM_PNG_FILTER_NONE = 1, TM_PNG_FILTER_ADAPTIVE = 2, TM_PNG_FILTER_SMALLER = 3 };
typedef struct tm_png_options {
  int32_t level;  /* 0: stored blocks, today's bytes (default); 1: the rule above */
  int32_t filter; /* TM_PNG_FILTER_*; level 0 ignores it */
} tm_png_options;
typedef struct tm_export_stats {
  int64_t frames, file_bytes; /* files written and the sum of their sizes */
  int32_t level, filter;      /* the options that held (level 1: AUTO resolved; level 0: the filter as set, it is not used) */
  double ms_device;           /* render, coding and read-back of the chunks, each behind a synchronise */
  double ms_write;            /* writing the files (level 0: packing the pixels into them too) */
  double ms_wall;             /* the whole call */
} tm_export_stats;
TM_API int tm_set_png_options(tm_encoder *, const tm_png_options *opt);
TM_API int tm_get_png_options(tm_encoder *, tm_png_options *opt);
TM_API int tm_get_export_stats(tm_encoder *, tm_export_stats *out);
TM_API int tm_png_bound_host(int w, int h, int64_t *bytes);
TM_API int tm_stage_png_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt,
                               uint8_t *host_out, int64_t cap, int64_t *offsets /* nframes + 1 */, void *stream);
TM_API int tm_png_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt,
                              uint8_t *out, int64_t cap, int64_t *offsets /* nframes + 1 */);
TM_API int tm_stage_zlib_compress(const uint8_t *dev_src, int64_t n, uint8_t *host_out, int64_t cap, int64_t *out_n, void *stream);
TM_API int tm_zlib_compress_host(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_n);
TM_API int tm_png_filter_rows_host(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, uint8_t *stream);
TM_API int tm_deflate_code_lengths_host(const uint32_t *freq, int nsym, int max_bits, uint8_t *lens);
/* ---- PNG input on the device: inflate and unfilter (tm_png_in.hip; the rule: tm_inflate.h) -------------------------
 * The export's mirror image.  A zlib stream (RFC 1950 / 1951: stored, fixed and dynamic blocks, Adler-32) is accepted exactly when
 * tm_inflate_host accepts it and then yields the same bytes; a refused stream ends with a status and never with an access outside its
 * buffers.  A stream's input is a list of spans of one blob (the IDAT payloads of a file are not joined; a span may be empty and a split may
 * fall inside a code); its output goes to dst + dst_off, at most dst_cap bytes.  The status is per stream: code (TM_INF_*, 0 = accepted),
 * the input byte position reached and the bytes written (0 unless accepted).
 *   Device form: k_inflate, one wave per stream and all streams of a batch in one launch -- decode state the same in every lane; tables, a
 * stage of input bytes and the 32 KiB window in LDS (37 KB a workgroup: four and more streams to a compute unit); a match copied LDS to LDS
 * by the whole wave; output in 16-byte stores; Adler-32 summed as the output leaves and compared on the device.  k_png_unfilter, one wave
 * per picture, lanes on 64 consecutive rows one pixel apart (lane l at pixel x - l): `up` and `up-left` come from lane l - 1 by a
 * cross-lane move, the filter type is read per row, and the 0x00RRGGBB pixel -- grey replicated, alpha dropped, a palette index looked up
 * -- is written straight into the destination frame.
 *   tm_inflate_streams_host / tm_stage_inflate: the rule on host memory with no device call / the kernel on a batch from HOST memory into
 * DEVICE memory dev_dst (status: HOST).  They return TM_OK whenever the batch was well formed (refusals: a null pointer, a span outside the
 * blob, a stream's spans outside the list or 4 GiB and more in sum, a destination outside dst_bytes); what became of each stream is its status.
 *   tm_png_decode_host / tm_stage_png_decode: nfiles PNG files in HOST memory, each of w x h, into frames [h][w] of 0x00RRGGBB, frame_px
 * pixels apart, in HOST / DEVICE memory.  The accepted set is tm_read_png_host's: 8 bits per sample, colour types 0, 2, 3, 4, 6,
 * non-interlaced.  What the container walk refuses (signature, CRC, IHDR, PLTE, a size other than w x h) fails the call with
 * tm_read_png_host's code, naming the file's index, before anything is decoded; what only decoding finds is the file's status[]: a
 * TM_INF_* code, TM_PNG_BAD_SIZE (not h (1 + row bytes) bytes of data), TM_PNG_BAD_FILTER (a row's filter type above 4), TM_PNG_BAD_INDEX
 * (a palette index beyond PLTE) -- the first in tm_read_png_host's order: stream, then rows top to bottom, a row's type before its pixels.
 *   tm_set_png_decode: where the Load of a PNG sequence (tm_open_input) or of lent PNG files (tm_set_frames_png) decodes.  HOST: the files
 * are decoded by tm_read_png_host's reader on host threads and the RGB32 clip is uploaded.  DEVICE: the files' bytes and a descriptor per
 * frame are uploaded chunk by chunk (TM_INPUT_CHUNK_FRAMES frames; otherwise as many as 2 GiB of inflated rows and 512 MiB of files hold: a stream is one wave's work) and the two kernels write the encoder's clip; a
 * refused file fails tm_run(TM_STEP_LOAD) with the host path's code, naming the file.  AUTO is DEVICE (it was the faster on both measured
 * sequences: DESIGN.md section 35), and HOST for pictures of 4 GiB of rows and more.  The environment variable TM_PNG_DECODE=host|device overrides what was set.
 *   tm_set_frames_png: PNG files LENT in host memory until the next Load has returned, as tm_set_frames_rgb lends pixels: the size is the
 * first file's (Scaling is ignored, as for a PNG sequence), a file of another size is TM_E_INVAL (at Load for all files but the first), the
 * key frames follow the automatic rule, StartFrame and FrameCount do not apply.  tm_probe_png_clip_host: the refusals and the size with no
 * device -- TM_E_INVAL for a null list, pointer or size, nframes < 1, fps <= 0; the first file's container refusals as tm_read_png_host
 * makes them.
 *   tm_get_input_stats: the last Load that read an input (TM_E_INVAL before the first): ms_read = the files into host memory (DEVICE) or
 * read and decoded (HOST), ms_device = upload and kernels, each behind a synchronise, both inside ms_wall. */
enum {
  TM_INF_OK = 0, TM_INF_TOO_SHORT = 1, TM_INF_BAD_HEADER = 2, TM_INF_DICT = 3, TM_INF_TRUNCATED = 4, TM_INF_BLOCK_TYPE = 5, TM_INF_STORED_LEN = 6,
  TM_INF_DYN_HEADER = 7, TM_INF_CL_CODE = 8, TM_INF_LENGTHS = 9, TM_INF_NO_EOB = 10, TM_INF_OVER_SUBSCRIBED = 11, TM_INF_BAD_CODE = 12,
  TM_INF_BAD_SYMBOL = 13, TM_INF_DISTANCE = 14, TM_INF_OVERFLOW = 15, TM_INF_NO_CHECKSUM = 16, TM_INF_ADLER = 17, TM_INF_BAD_SPAN = 18,
  TM_PNG_BAD_SIZE = 32, TM_PNG_BAD_FILTER = 33, TM_PNG_BAD_INDEX = 34
};
enum { TM_PNG_DECODE_AUTO = 0, TM_PNG_DECODE_HOST = 1, TM_PNG_DECODE_DEVICE = 2 };
typedef struct tm_inflate_span { uint64_t off; uint32_t len, reserved; } tm_inflate_span;   /* bytes [off, off + len) of the blob */
typedef struct tm_inflate_stream {
  uint64_t dst_off;                /* where the stream's output starts in the destination */
  uint32_t dst_cap;                /* the most it may write */
  uint32_t first_span, span_count; /* its input: spans [first_span, + span_count) in order */
  uint32_t reserved;
} tm_inflate_stream;
typedef struct tm_inflate_status { int32_t code; uint32_t in_pos, out_n; } tm_inflate_status;
typedef struct tm_input_stats {
  int64_t frames, file_bytes, bytes_uploaded; /* frames this Load read; the sum of their files' sizes; bytes sent to the device for them */
  int32_t where, kind;                         /* TM_PNG_DECODE_HOST / _DEVICE (what held); TM_INPUT_PNGS or 6 for lent PNG files */
  double ms_read, ms_device, ms_wall;
} tm_input_stats;
TM_API int tm_inflate_streams_host(const uint8_t *blob, size_t blob_bytes, const tm_inflate_span *spans, int nspans, const tm_inflate_stream *streams,
                                   int nstreams, uint8_t *dst, size_t dst_bytes, tm_inflate_status *status /* nstreams */);
TM_API int tm_stage_inflate(const uint8_t *blob, size_t blob_bytes, const tm_inflate_span *spans, int nspans, const tm_inflate_stream *streams,
                            int nstreams, uint8_t *dev_dst, size_t dst_bytes, tm_inflate_status *status /* nstreams, host */, void *stream);
TM_API int tm_png_decode_host(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint32_t *out, int64_t frame_px,
                              int32_t *status /* nfiles */);
TM_API int tm_stage_png_decode(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint32_t *dev_out, int64_t frame_px,
                               int32_t *status /* nfiles, host */, void *stream);
TM_API int tm_set_png_decode(tm_encoder *, int where);
TM_API int tm_get_png_decode(tm_encoder *, int *where);
TM_API int tm_set_frames_png(tm_encoder *, const void *const *files, const size_t *sizes, int nframes, double fps);
TM_API int tm_probe_png_clip_host(const void *const *files, const size_t *sizes, int nframes, double fps, int *width, int *height);
TM_API int tm_get_input_stats(tm_encoder *, tm_input_stats *out);
/* ---- JPEG input on the device (the rule: tiler_amd/csrc/tm_jpeg.h).
 *   Accepted: baseline JPEG -- SOF0, or SOF1 with 8-bit samples; one component, or three (YCbCr) with chroma 1x1 and luma 1x1 (4:4:4), 2x1
 * (4:2:2) or 2x2 (4:2:0); one interleaved scan with Ss 0, Se 63, Ah = Al = 0; DQT with 8- or 16-bit entries; DHT tables 0..3 per class,
 * and a file with no DHT at all decodes with the tables of T.81 Annex K.3 (the frames of an MJPEG capture); DRI / RSTn; APPn and COM of
 * any size and fill bytes before a marker are skipped; what follows EOI is ignored.  The EXIF orientation is ignored.
 *   The container walk (host) refuses, naming the marker or field, before anything is decoded: TM_E_UNSUPPORTED for SOF2 (progressive),
 * SOF3 and SOF5..SOF15, a precision other than 8, 2 or 4 components, any other sampling, more than one scan, APP14 (Adobe) transform 0 on
 * three components (RGB), DNL or a height of 0; TM_E_IO for a file without SOI, a segment that runs past the file, a scan that names a
 * missing table or component, a DHT whose counts over-subscribe the code space or name more than 256 symbols.
 *   The walk cuts the scan at every RSTn into segments of restart_interval MCUs, each an independent chain; what only decoding finds is
 * the file's status: TM_JPG_TRUNCATED (a symbol needs bits beyond its segment), TM_JPG_BAD_CODE (bits that are no code), TM_JPG_BAD_RUN (a
 * zero run past coefficient 63), TM_JPG_BAD_MAGNITUDE (a DC category above 11, an AC category above 10), TM_JPG_BAD_RESTART (an RSTn
 * missing or out of sequence: the file is not decoded) -- the first in segment order, then MCU order.  TM_JPG_BAD_DESC is the kernel's
 * refusal of a descriptor that points outside what the launch was given; the entry points below never make one.
 *   The samples: coefficient x quantiser, the "islow" integer inverse DCT (13-bit constants, columns then rows, descaled by 11 and by 18),
 * + 128, clamped -- in wrapping 32-bit arithmetic, the same on the host and on the device; for files written from 8-bit samples these are
 * libjpeg's planes bit for bit.  Chroma planes are ceil(w / 2) wide and, for 4:2:0, ceil(h / 2) high.
 *   tm_probe_jpeg_host: the walk alone, no device: the size, the components, the luma sampling factors, the restart interval (0: none),
 * the number of segments, the SOF kind (0 or 1), the TM_CHROMA_* layout of the planes (4:2:2 is sited between the luma pairs, as JFIF
 * has it, which no public layout names: it reports TM_CHROMA_422) and status (0 or TM_JPG_BAD_RESTART).
 *   tm_jpeg_decode_host / tm_stage_jpeg_decode: nfiles files in HOST memory into planes in HOST / DEVICE memory.  File i's planes start
 * i frame strides into y, u, v and have the file's own size, which may be anything up to w x h: strides = {y_row, y_frame, u_row,
 * u_frame, v_row, v_frame} in bytes (HOST array); u and v may be null when every file has one component.  The walk's refusals fail the
 * call, naming the file's index; so do (TM_E_INVAL) a null pointer, a file larger than w x h, strides shorter than a file's planes.
 * Otherwise they return TM_OK and what became of each file is its status; a refused file never causes an access outside its own planes,
 * and both forms leave the same bytes in them.
 *   tm_set_frames_jpeg: JPEG files LENT in host memory until the next Load has returned, as tm_set_frames_png lends PNG files: the size
 * and sampling are the first file's, a file of another size or sampling is TM_E_INVAL at Load, Scaling is ignored, the key frames follow
 * the automatic rule, StartFrame and FrameCount do not apply.  tm_probe_jpeg_clip_host: its refusals and the size with no device.
 *   A pattern whose first file starts with FF D8 is a JPEG sequence for tm_open_input / tm_probe_input_host (kind TM_INPUT_JPEGS), with a
 * PNG sequence's rules: 24 frames a second, files counted to the first gap, key frames where a .kf file exists, Scaling ignored.
 *   The decoded planes become RGB32 through the YUV input rule (k_yuv_to_rgb32): JFIF is full-range BT.601, so TM_YUV_AUTO is
 * TM_YUV_BT601_FULL; a mode set with tm_set_input_yuv is honoured.
 *   tm_set_jpeg_decode: where Load decodes.  DEVICE: the files and a descriptor per frame go up chunk by chunk (TM_INPUT_CHUNK_FRAMES
 * files; otherwise as many as 1 GiB of planes and 512 MiB of files hold) and k_jpeg_decode writes the planes.  HOST: the reader threads
 * decode with the host form and the planes are uploaded.  AUTO goes by the first file, whose segments are the lanes it keeps busy:
 * DEVICE when it has four restart segments or more, else HOST.  Measured at 720p x 300 with 1, 2, 4, 8, 16, 30 and 45 segments a file: the
 * host is faster at 1 and 2 (138 ms against 227 ms, 142 against 150), the device from 4 on (96 ms against 142 ms; 26 against 139 at 45);
 * three segments were not measured.  TM_JPEG_DECODE=host|device overrides.
 * tm_get_input_stats reports kind 8 for a sequence and 12 for lent files. */
enum { TM_JPG_TRUNCATED = 48, TM_JPG_BAD_CODE = 49, TM_JPG_BAD_RUN = 50, TM_JPG_BAD_MAGNITUDE = 51, TM_JPG_BAD_RESTART = 52, TM_JPG_BAD_DESC = 53 };
enum { TM_INPUT_JPEGS = 8 };
typedef struct tm_jpeg_info {
  int32_t width, height, components, h_samp, v_samp, restart_interval, segments, sof, chroma, status;
} tm_jpeg_info;
TM_API int tm_probe_jpeg_host(const void *file, size_t size, tm_jpeg_info *out);
TM_API int tm_jpeg_decode_host(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint8_t *y, uint8_t *u, uint8_t *v,
                               const int64_t *strides /* 6 */, int32_t *status /* nfiles */);
TM_API int tm_stage_jpeg_decode(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint8_t *dev_y, uint8_t *dev_u, uint8_t *dev_v,
                                const int64_t *strides /* 6, host */, int32_t *status /* nfiles, host */, void *stream);
TM_API int tm_set_jpeg_decode(tm_encoder *, int where /* TM_PNG_DECODE_* */);
TM_API int tm_get_jpeg_decode(tm_encoder *, int *where);
TM_API int tm_set_frames_jpeg(tm_encoder *, const void *const *files, const size_t *sizes, int nframes, double fps);
TM_API int tm_probe_jpeg_clip_host(const void *const *files, const size_t *sizes, int nframes, double fps, int *width, int *height);
/* ---- GIF input on the device (the rule: tiler_amd/csrc/tm_gif.h).
 *   An existing file that starts with GIF87a / GIF89a is an animated GIF for tm_open_input / tm_probe_input_host (kind TM_INPUT_GIF): the
 * size is the logical screen's, the rate the file's, StartFrame and FrameCount apply (the frames before StartFrame are decoded and
 * composited, not delivered), the key frames follow the automatic rule, Scaling != 1 is TM_E_UNSUPPORTED.
 *   The container walk (host) refuses before anything is decoded: TM_E_UNSUPPORTED for a file without the signature or of 4 GiB or more;
 * TM_E_IO for a block or sub-block that runs past the end of the file, an unknown block introducer, a file with no image, a screen or a
 * rectangle of width or height 0, a minimum code size outside 2..8 (1 is refused, not read as 2: Pillow reads such a file with a
 * two-symbol alphabet at two bits, so data written for 2 comes out differently there and there is no one reading to agree with), an
 * image with neither a local nor a global colour table.  Graphic
 * control (disposal, transparent index, delay; for the next image only) and the NETSCAPE2.0 loop count are read; every other extension is
 * skipped sub-block by sub-block; what follows the trailer is ignored; a file that ends without a trailer behind a whole image is read.
 *   LZW: codes LSB first from min + 1 bits, clear = 1 << min, eoi = clear + 1, first free entry clear + 2, wider when the next free entry
 * reaches 1 << width, up to 12; a full table goes on at 12 bits and adds nothing; a clear resets; the code behind a clear adds no entry; a
 * missing initial clear is accepted; decoding stops at w x h indices (eoi is not required, what follows is not looked at).  Per image:
 * TM_GIF_TRUNCATED (the data or an eoi ends it early), TM_GIF_BAD_CODE (a code above the next free entry, or a non-literal behind a clear).
 * TM_GIF_BAD_DESC is the kernel's refusal of a descriptor that points outside what the launch was given; the entry points never make one.
 *   Frames: the canvas is the logical screen, filled with bg = the caller's colour, else the global table's entry at the background index
 * when that index lies in the table, else 0x000000.  Before frame i > 0 the rectangle of frame i - 1 (clipped to the screen) is set to bg
 * (disposal 2) or to what the canvas held before frame i - 1 was drawn (disposal 3); any other disposal leaves it.  Then frame i's
 * indices other than its transparent index are drawn through its local table, else the global one (an index past the table: 0x000000);
 * a rectangle that leaves the screen is clipped; interlaced rows are stored in the four-pass order.  The canvas is the frame, 0x00RRGGBB.
 *   Rate: a delay (1/100 s) of 0 or 1 counts as 10; fps = 100 n / sum of the delays of all n frames; uniform_delay: all equal.  Frames are
 * never repeated or dropped.
 *   tm_probe_gif_host / tm_gif_frames_host: the walk alone (no device); *nframes is the file's count, at most cap entries are written.
 *   tm_gif_lzw_streams_host / tm_stage_gif_lzw: the LZW rule on a batch.  Stream s reads the sub-block chain (length bytes included) at
 * [src_off, src_off + src_bytes) of blob (HOST) and writes at most npix indices at dst_off of dst (HOST / DEVICE); the end of the span ends
 * the data like a terminator.  TM_E_INVAL for a stream outside blob or dst or a min_code_size outside 2..8; otherwise TM_OK and a status
 * per stream: {code, payload bytes of the codes read, indices written}.  A refused stream writes only inside its own npix.
 *   tm_gif_decode_host / tm_stage_gif_decode: frames [first, first + count) of a file in HOST memory as [count] frames of frame_px pixels in
 * HOST / DEVICE memory; background -1: the file's.  status: first + count entries (HOST), one per image from image 0 on.  The walk's
 * refusals fail the call; otherwise TM_OK, and nothing is delivered from the first image with a status on.  The device form goes chunk by
 * chunk (TM_INPUT_CHUNK_FRAMES images, otherwise what 1 GiB of stored indices holds); where the chunks end changes no byte.
 *   tm_set_frames_gif: one GIF file LENT in host memory until the next Load has returned; fps <= 0: the file's.  Scaling, StartFrame and
 * FrameCount do not apply.  tm_probe_gif_clip_host: its refusals, size, frames and rate with no device.
 *   tm_set_gif_decode: where Load decodes (TM_PNG_DECODE_*; TM_GIF_DECODE=host|device overrides).  HOST: the reader threads run the LZW
 * image by image, the frames are composited on the host and the RGB32 clip is uploaded.  DEVICE: the file and a descriptor per chunk go up,
 * k_gif_lzw (a wave per image) and k_gif_compose (a lane per four canvas pixels) write the encoder's clip.  AUTO is DEVICE.  Measured on
 * two clips of 480 x 270 x 120 written by Pillow, OpenInput + Load from a memory-backed directory, median of 7 passes (range): the bench
 * clip in 256 colours 24.4 ms (24.3 - 25.0) on the device against 32.8 ms (31.7 - 35.6) on the host, a flat 16-colour one 2.19 ms (2.16 -
 * 2.24) against 24.5 ms (24.3 - 24.7); the ranges meet on neither.
 * tm_set_gif_background: -1 (the file's) or 0x00RRGGBB.  tm_get_input_stats reports kind 16 for a file and 20 for a lent file. */
enum { TM_GIF_TRUNCATED = 64, TM_GIF_BAD_CODE = 65, TM_GIF_BAD_DESC = 66 };
enum { TM_INPUT_GIF = 16 };
typedef struct tm_gif_info {
  int32_t width, height, frames, uniform_delay, loop_count /* -1: no loop extension */, global_table_size, background_index, version /* 87, 89 */;
  uint32_t background; /* resolved, 0x00RRGGBB */
  int32_t reserved;
  double fps;
} tm_gif_info;
typedef struct tm_gif_frame {
  int32_t left, top, width, height, delay /* 1/100 s, as stored */, disposal, transparent /* index, or -1 */, interlaced;
  int32_t table_size, local_table /* 1: its own table */, min_code_size, reserved;
  uint64_t data_off, data_bytes; /* the sub-block chain in the file, terminator included */
} tm_gif_frame;
typedef struct tm_gif_stream { uint64_t src_off, dst_off; uint32_t src_bytes, npix, min_code_size, reserved; } tm_gif_stream;
typedef struct tm_gif_status { int32_t code; uint32_t in_pos, out_n; } tm_gif_status;
TM_API int tm_probe_gif_host(const void *file, size_t size, tm_gif_info *out);
TM_API int tm_gif_frames_host(const void *file, size_t size, tm_gif_frame *out, int cap, int *nframes);
TM_API int tm_gif_lzw_streams_host(const uint8_t *blob, size_t blob_bytes, const tm_gif_stream *streams, int nstreams, uint8_t *dst, size_t dst_bytes, tm_gif_status *status);
TM_API int tm_stage_gif_lzw(const uint8_t *blob, size_t blob_bytes, const tm_gif_stream *streams, int nstreams, uint8_t *dev_dst, size_t dst_bytes,
                            tm_gif_status *status /* host */, void *stream);
TM_API int tm_gif_decode_host(const void *file, size_t size, int first, int count, int background /* -1: the file's */, uint32_t *out, int64_t frame_px,
                              int32_t *status /* first + count */);
TM_API int tm_stage_gif_decode(const void *file, size_t size, int first, int count, int background, uint32_t *dev_out, int64_t frame_px,
                               int32_t *status /* first + count, host */, void *stream);
TM_API int tm_set_gif_decode(tm_encoder *, int where /* TM_PNG_DECODE_* */);
TM_API int tm_get_gif_decode(tm_encoder *, int *where);
TM_API int tm_set_gif_background(tm_encoder *, int background /* -1, or 0x00RRGGBB */);
TM_API int tm_get_gif_background(tm_encoder *, int *background);
TM_API int tm_set_frames_gif(tm_encoder *, const void *file, size_t size, double fps /* <= 0: the file's */);
TM_API int tm_probe_gif_clip_host(const void *file, size_t size, double fps, int *width, int *height, int *frames, double *out_fps);
/* ---- JPEG export on the device: forward DCT and Huffman coding; MJPEG (tm_jpeg_out.hip; the rule: tm_jpeg_out.h) ----
 * The input's mirror image.  The files are libjpeg's baseline files byte for byte: quantisers = the Annex K.1 tables scaled by quality
 * (scale = q < 50 ? 5000 / q : 200 - 2 q; clamp((base scale + 50) / 100, 1, 255)); JFIF's YCbCr in 16-bit fixed point; chroma box-averaged
 * with libjpeg's alternating bias, edges repeated; the "islow" integer forward DCT; quantisation by integer division; the Huffman tables
 * of Annex K.3 (not optimised); SOI, APP0 JFIF 1.01, DQT per table, SOF0, DHT per table (DC0, AC0, DC1, AC1), DRI, SOS, the scan, EOI.
 * The file is a function of the pixels and the options alone: the device form (transform, bit counts, scans, bit packing, byte stuffing
 * and compaction in kernels; only file bytes cross to the host, one size read-back and one copy per chunk of frames) and the host twin
 * write the same bytes.
 *   quality 1 .. 100 (default 90); sampling TM_JPEG_420 (default), _422, _444 or _GREY (Y alone); restart_rows: 0 = no DRI, one entropy
 * segment; n > 0 = a restart interval of n MCU rows (default 1: the file tm_open_input decodes on the device, section 39.3).
 *   tm_set_jpeg_options: what tm_generate_jpegs / tm_generate_mjpeg write from then on (TM_E_INVAL: null, quality outside 1 .. 100,
 * unknown sampling, restart_rows < 0, restart_rows times the MCUs of a row above 65535 is refused by the call that learns the width).
 *   tm_generate_jpegs: <OutputFileName without extension>_NNNN.jpg, one per frame, of the frames tm_generate_pngs writes (the Output page
 * with the constructor's defaults, or the source frames: input != 0); no .txt.  tm_generate_mjpeg: the same files one behind another in
 * `path`.  Both refuse what tm_generate_pngs refuses and, in a device group, read shard 0.  tm_get_jpeg_export_stats: the last of either
 * (TM_E_INVAL before the first), with tm_export_stats' meanings; tm_export_stats and tm_get_export_stats are not touched by them.
 *   tm_jpeg_bound_host: an upper bound of one file's size for any pixels.  tm_jpeg_quant_tables_host: the two quantiser tables of a
 * quality in natural (row-major) order.
 *   tm_stage_jpeg_encode: nframes pictures [h][w] of 0x00RRGGBB in DEVICE memory, rows stride_px apart, frames frame_px apart (pixels), as
 * files laid one behind the other in HOST memory host_out, file f at [offsets[f], offsets[f + 1]).  tm_jpeg_encode_host: the same from
 * HOST frames without a device, byte for byte.  Refusals, TM_E_INVAL before any device call and with nothing written: a null pointer,
 * options tm_set_jpeg_options refuses, w or h outside 1 .. 32768, a restart interval above 65535 MCUs, nframes < 0, a row stride shorter
 * than the row with more than one row, a frame stride shorter than a frame with more than one frame.  A cap too small is TM_E_INVAL too,
 * with offsets[nframes] set to the bytes needed and host_out untouched: size host_out by nframes times tm_jpeg_bound_host and the call is
 * made once.  The stage call returns synchronised. */
enum { TM_JPEG_420 = 0, TM_JPEG_422 = 1, TM_JPEG_444 = 2, TM_JPEG_GREY = 3 };
typedef struct tm_jpeg_options {
  int32_t quality;      /* 1 .. 100 (default 90) */
  int32_t sampling;     /* TM_JPEG_* (default TM_JPEG_420) */
  int32_t restart_rows; /* 0: none; n: RSTn every n MCU rows (default 1) */
} tm_jpeg_options;
typedef struct tm_jpeg_export_stats {
  int64_t frames, file_bytes;               /* pictures written and the sum of their sizes */
  int32_t quality, sampling, restart_rows;  /* the options that held */
  int32_t reserved;
  double ms_device;                         /* render, coding and read-back of the chunks, each behind a synchronise */
  double ms_write;                          /* writing the files */
  double ms_wall;                           /* the whole call */
} tm_jpeg_export_stats;
TM_API int tm_set_jpeg_options(tm_encoder *, const tm_jpeg_options *opt);
TM_API int tm_get_jpeg_options(tm_encoder *, tm_jpeg_options *opt);
TM_API int tm_generate_jpegs(tm_encoder *, int input);
TM_API int tm_generate_mjpeg(tm_encoder *, const char *path, int input);
TM_API int tm_get_jpeg_export_stats(tm_encoder *, tm_jpeg_export_stats *out);
TM_API int tm_jpeg_bound_host(int w, int h, const tm_jpeg_options *opt, int64_t *bytes);
TM_API int tm_jpeg_quant_tables_host(int quality, uint16_t *luma /* 64 */, uint16_t *chroma /* 64 */);
TM_API int tm_stage_jpeg_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt,
                                uint8_t *host_out, int64_t cap, int64_t *offsets /* nframes + 1 */, void *stream);
TM_API int tm_jpeg_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt,
                               uint8_t *out, int64_t cap, int64_t *offsets /* nframes + 1 */);
/* ---- GIF export on the device: colour tables, LZW coding in segments (tm_gif_out.hip; the rule: tm_gif_out.h) ----
 * One animated GIF89a of the frames tm_generate_pngs writes.  A decoded frame is a paletted picture, so with PaletteCount x PaletteSize <=
 * 256 the file is lossless.  No global table; NETSCAPE2.0 as `loop` says; per frame a graphic control (disposal 1, no transparency, the
 * delay), an image descriptor with a local table of the next power of two >= the colours (at least 2, padded with black), the minimum
 * code size max(2, bits of the table size), the data in sub-blocks of 255 and a last shorter one, a 0; the trailer.  The delay is delay_cs,
 * or max(2, floor(100 / fps + 0.5)) (the reader and browsers take 0 and 1 as 10); above 65535: TM_E_INVAL.
 *   diff 1: frame 0 whole, frame i the bounding box of the pixels whose 0x00RRGGBB differs from frame i - 1's, an unchanged frame the 1 x 1
 * rectangle at (0, 0).  Table and indices per frame over the rectangle's pixels.  Exact (the distinct colours number <= max_colours): the
 * distinct colours ascending, a pixel's index is its colour's rank, a reader shows the source.  Quantised (more colours under
 * TM_GIF_COLOURS_AUTO, every frame under _QUANTISE; under _EXACT such a frame is TM_E_UNSUPPORTED): a median cut in integers over 15-bit
 * cells (tm_gif_out.h states every tie), a pixel's index is its cell's box, no dithering.
 *   LZW: the rectangle's indices in row order are cut into segments of segment_pixels; each is coded on its own from a clear (greedy longest
 * match, an entry per code, a clear when the table fills), the clear that opens the next segment is written at the width its segment ended
 * on, the last segment ends with eoi.  The file is a function of the pixels, the rate and the options alone: the device form (a wave per
 * segment, every segment of a chunk of frames in one launch; the bits joined by a scan and a shifted copy) and the host twin write the same
 * bytes, and where the chunks end changes no byte.
 *   tm_set_gif_options: TM_E_INVAL for null, unknown colours, max_colours outside 2 .. 256, diff other than 0 / 1, segment_pixels other
 * than 0 or >= 256, loop outside -1 .. 65535, delay_cs 1 or outside 0 .. 65535.  tm_generate_gif refuses what tm_generate_pngs refuses,
 * before any file is opened, and in a device group reads shard 0.  tm_get_gif_export_stats: of the last tm_generate_gif.
 *   tm_stage_gif_encode: nframes pictures [h][w] of 0x00RRGGBB in DEVICE memory as one file in HOST memory `out`; chunk_frames <= 0: the
 * writer's own.  tm_gif_encode_host: the same from HOST frames with no device; canvas (or null): [nframes][h][w], what a reader shows.
 * TM_E_INVAL before any device call: null pointers, options as above, w or h < 1, nframes < 1, strides shorter than a row / a frame, a
 * delay above 65535; TM_E_UNSUPPORTED: a side above 65535, a frame above 2^28 pixels.  A cap too small is TM_E_INVAL with *bytes set to
 * the bytes needed and `out` untouched; tm_gif_bound_host bounds any file of that shape.  stats may be null.
 *   tm_stage_gif_lzw_pack / tm_gif_lzw_pack_host: n indices (DEVICE / HOST) below 1 << min_code as the payload before sub-blocks.
 * tm_stage_gif_palettise / tm_gif_palettise_host: one frame as table (256 entries), colour count, exact-or-not and indices [h][w] (HOST). */
enum { TM_GIF_COLOURS_AUTO = 0, TM_GIF_COLOURS_EXACT = 1, TM_GIF_COLOURS_QUANTISE = 2 };
typedef struct tm_gif_options {
  int32_t colours;        /* TM_GIF_COLOURS_* (default AUTO) */
  int32_t max_colours;    /* 2 .. 256 (default 256) */
  int32_t diff;           /* 0: whole frames; 1: the changed rectangle (default) */
  int32_t segment_pixels; /* 0: one segment per image; else indices per segment, >= 256 (default 4096: DESIGN.md section 43.3) */
  int32_t loop;           /* -1: no NETSCAPE block; 0: for ever (default); n: n times */
  int32_t delay_cs;       /* 0: from the rate (default); else 1/100 s per frame */
} tm_gif_options;
typedef struct tm_gif_export_stats {
  int64_t frames, frames_exact, frames_quantised, segments, file_bytes;
  double ms_colours; /* rectangles, distinct colours and histograms on the device, their read-back */
  double ms_tables;  /* the host: sorting, the median cut */
  double ms_lzw;     /* mapping and coding, the bit counts' read-back */
  double ms_emit;    /* joining the bits, the container, the bytes' read-back */
  double ms_device;  /* render and all of the above */
  double ms_write;   /* writing the file */
  double ms_wall;    /* the whole call */
} tm_gif_export_stats;
TM_API int tm_set_gif_options(tm_encoder *, const tm_gif_options *opt);
TM_API int tm_get_gif_options(tm_encoder *, tm_gif_options *opt);
TM_API int tm_generate_gif(tm_encoder *, const char *path, int input);
TM_API int tm_get_gif_export_stats(tm_encoder *, tm_gif_export_stats *out);
TM_API int tm_gif_bound_host(int w, int h, int nframes, const tm_gif_options *opt, int64_t *bytes);
TM_API int tm_stage_gif_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt,
                               int chunk_frames, uint8_t *out, int64_t cap, int64_t *bytes, tm_gif_export_stats *stats, void *stream);
TM_API int tm_gif_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt,
                              uint8_t *out, int64_t cap, int64_t *bytes, uint32_t *canvas, tm_gif_export_stats *stats);
TM_API int tm_stage_gif_lzw_pack(const uint8_t *dev_indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes, void *stream);
TM_API int tm_gif_lzw_pack_host(const uint8_t *indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes);
TM_API int tm_stage_gif_palettise(const uint32_t *dev_frame, int64_t stride_px, int w, int h, const tm_gif_options *opt, uint32_t *table /* 256 */, int *colours,
                                  int *exact, uint8_t *indices /* host, h * w */, void *stream);
TM_API int tm_gif_palettise_host(const uint32_t *frame, int64_t stride_px, int w, int h, const tm_gif_options *opt, uint32_t *table /* 256 */, int *colours, int *exact,
                                 uint8_t *indices /* h * w */);
/* ---- WebP export on the device: lossless VP8L frames, one animated file (tm_webp_out.hip; the rule: tm_webp_out.h) ----
 * One animated WebP of the frames tm_generate_pngs writes, every frame a lossless VP8L image: exact at any number of colours.  RIFF / WEBP
 * with VP8X (animation flag only), ANIM (background 0, `loop`), and per frame an ANMF (x / 2, y / 2, width - 1, height - 1, the duration,
 * flags 0x02: no blending, no disposal) holding one VP8L chunk.  The duration is duration_ms, or max(1, floor(1000 / fps + 0.5)); above
 * 2^24 - 1: TM_E_INVAL.
 *   diff 1: frame 0 whole, frame i the bounding box of the pixels whose 0x00RRGGBB differs from frame i - 1's with its left and top lowered
 * to even, an unchanged frame the 1 x 1 rectangle at (0, 0).  Per frame over the rectangle's pixels: with at most 256 distinct colours
 * under TM_WEBP_PALETTE_AUTO a colour-indexing transform (the distinct colours ascending, a pixel's index is its colour's rank, 8 / 4 / 2
 * / 1 indices to a coded pixel for <= 2 / 4 / 16 / more colours, lowest bits first; the table coded as differences with literals only),
 * otherwise the subtract-green transform.  The coded pixels (alpha 0xFF) in row order are cut into segments of segment_pixels.
 *   LZ77, greedy from a segment's first pixel: the candidates of a position are the earlier positions of the image whose three pixels hash
 * alike, nearest first, at most 8 visited, none further than 2^20 - 120 back; the length is the common run capped at min(4096, what is
 * left of the segment); the longest wins, the nearest among equals; below 3, or 3 and further than 512 back: no match, a literal.  A
 * match never crosses its segment's end; its source may lie anywhere before it.  A distance d is written as the code d + 120.
 *   One group of five prefix codes per image from the histograms of its tokens: lengths by tm_deflate_code_lengths_host (15 bits; 7 for
 * the code of the lengths, whose zero runs use 17 and 18); an alphabet with at most two used symbols, all below 256, is a simple code.
 * No colour cache, no predictor or colour transform, no meta codes, no alpha.  The file is a function of the pixels, the rate and the
 * options alone: the device form and the host twin write the same bytes, and where the chunks end changes no byte.
 *   tm_set_webp_options: TM_E_INVAL for null, diff or lz77 other than 0 / 1, an unknown palette, segment_pixels < 0, loop outside 0 ..
 * 65535, duration_ms outside 0 .. 2^24 - 1.  tm_generate_webp refuses what tm_generate_pngs refuses, before any file is opened, and in a
 * device group reads shard 0.  tm_get_webp_export_stats: of the last tm_generate_webp.
 *   tm_stage_webp_encode: nframes pictures [h][w] of 0x00RRGGBB in DEVICE memory as one file in HOST memory `out`; chunk_frames <= 0: the
 * writer's own (at most 32).  tm_webp_encode_host: the same from HOST frames with no device; canvas (or null): [nframes][h][w], what a
 * reader shows.  TM_E_INVAL before any device call: null pointers, options as above, w or h < 1, nframes < 1, strides shorter than a row /
 * a frame, a rate that gives no duration; TM_E_UNSUPPORTED: a side above 16384.  A cap too small is TM_E_INVAL with *bytes set to the
 * bytes needed and `out` untouched; tm_webp_bound_host bounds any file of that shape.  stats may be null. */
enum { TM_WEBP_PALETTE_AUTO = 0, TM_WEBP_PALETTE_OFF = 1 };
typedef struct tm_webp_options {
  int32_t diff;           /* 0: whole frames; 1: the changed rectangle (default) */
  int32_t palette;        /* TM_WEBP_PALETTE_* (default AUTO) */
  int32_t lz77;           /* 0: literals only; 1: matches (default) */
  int32_t segment_pixels; /* 0: one segment per image; else coded pixels per segment (default 4096: DESIGN.md section 44.3) */
  int32_t loop;           /* 0: for ever (default); n: n times */
  int32_t duration_ms;    /* 0: from the rate (default); else ms per frame */
} tm_webp_options;
typedef struct tm_webp_export_stats {
  int64_t frames, frames_indexed, segments, tokens, matches, file_bytes;
  double ms_colours; /* rectangles and distinct colours on the device, their read-back, the host's tables */
  double ms_match;   /* coded pixels, the key sort and the links */
  double ms_parse;   /* the parse, the histograms and their read-back */
  double ms_codes;   /* the host: code lengths and every image's header bits */
  double ms_emit;    /* packing and joining the bits, the container, the bytes' read-back */
  double ms_device;  /* render and all of the above */
  double ms_write;   /* writing the file */
  double ms_wall;    /* the whole call */
} tm_webp_export_stats;
TM_API int tm_set_webp_options(tm_encoder *, const tm_webp_options *opt);
TM_API int tm_get_webp_options(tm_encoder *, tm_webp_options *opt);
TM_API int tm_generate_webp(tm_encoder *, const char *path, int input);
TM_API int tm_get_webp_export_stats(tm_encoder *, tm_webp_export_stats *out);
TM_API int tm_webp_bound_host(int w, int h, int nframes, const tm_webp_options *opt, int64_t *bytes);
TM_API int tm_stage_webp_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt,
                                int chunk_frames, uint8_t *out, int64_t cap, int64_t *bytes, tm_webp_export_stats *stats, void *stream);
TM_API int tm_webp_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt,
                               uint8_t *out, int64_t cap, int64_t *bytes, uint32_t *canvas, tm_webp_export_stats *stats);
/* The same pictures rendered on the device (Render :3455-3640, Output tab with the constructor's defaults; or the Input tab: input != 0):
 * frames [first_frame, first_frame+frame_count) as [frame_count][tm_h*8][tm_w*8] uint32 0x00RRGGBB (the format frames are pushed in; the
 * input render is every pushed frame cropped to tm_w*8 x tm_h*8 with alpha 0).  A predicted item is frame f-1's output at its offset,
 * clamped to the picture; a range starting inside a key frame's group gives what the whole clip gives.  out: a device pointer on the
 * encoder's device (out_on_device != 0) or host memory (one DMA when page-locked).  Blocking.  TM_E_INVAL when the output has not been
 * reconstructed or reloaded, when the source frames are not in memory (input: after ReloadGTM without Load, or frames a sharded Load
 * did not keep), or when the range is out of bounds. */
TM_API int tm_render_frames(tm_encoder *, int first_frame, int frame_count, int input, void *out, int out_on_device);
/* The same frames as YUV (tm_yuv_out above): frame first_frame + i goes to frame i of dst, converted on the device behind the render; a
 * device destination is written in place, a host destination receives 1 to 6 bytes a pixel instead of 4.  Refuses what tm_render_frames
 * refuses, and what tm_probe_yuv_out_host refuses (frame_count > dst->frames included), before any device call.  In a device group it
 * reads shard 0, like the exports -- one refusal more than tm_render_frames: with input != 0 after a sharded Load, a range outside the
 * frames shard 0 loaded is TM_E_INVAL (tm_render_frames gathers such a range from every shard's piece).  Blocking. */
TM_API int tm_render_frames_yuv(tm_encoder *, int first_frame, int frame_count, int input, const tm_yuv_out *dst, int mode);
/* ---- Decoded frames at a caller's size: RGB32 frames resampled on the device (tm_scale.hip) -----------------------
 * A frame is uint32 0x00RRGGBB; R, G and B are three planes at luma positions (s = 1, o = 0 in tm_resample_taps_host's terms).
 *   TM_SCALE_LANCZOS3  each channel through the rule of tm_stage_yuv_to_rgb32, unchanged: tables of tm_resample_taps_host(n, m, n, 1, 0),
 *                      horizontal pass first, h = (sum c p + 64) >> 7, then v = clamp((sum c h + 2^20) >> 21, 0, 255).  At equal size one tap
 *                      of 16384 is left: the output is the input.  Shrinking an axis by more than 8 is TM_E_UNSUPPORTED (the tables' limit).
 *   TM_SCALE_NEAREST   output sample j of m takes source sample ((2 j + 1) n) / (2 m), in integer division, per axis.  No shrink limit.
 * The output's top byte is 0, whatever the source's top byte holds.  Refusals, all before any device call and with nothing written:
 * TM_E_INVAL for a size below 1, an unknown filter, a null (or not 4-byte aligned) pointer, a row stride shorter than the row (a frame
 * stride shorter than the frame, with more than one), source and destination ranges that overlap; TM_E_UNSUPPORTED for a Lanczos shrink
 * beyond 8 on either axis and for any of the four sizes above TM_SCALE_MAX_SIZE.
 *   tm_probe_scale_host makes the size and filter checks and nothing else.  tm_scale_rgb32_host is the rule in plain loops, one frame, no
 * device.  tm_stage_scale_rgb32 (k_scale_rgb32_lanczos3 / k_scale_rgb32_nearest): nframes frames, strides in pixels, both on the current
 * device; 16-byte stores where dst is 16-byte aligned and dst_w and the destination strides are multiples of 4, 4-byte stores otherwise.
 * Bytes outside the rows are not touched.  Queued on `stream`; the Lanczos filter waits for it (the tables are the call's). */
#define TM_SCALE_LANCZOS3 0
#define TM_SCALE_NEAREST  1
#define TM_SCALE_MAX_SIZE 32768
TM_API int tm_probe_scale_host(int src_w, int src_h, int dst_w, int dst_h, int filter);
TM_API int tm_scale_rgb32_host(const uint32_t *src, int64_t src_stride_px, int src_w, int src_h,
                               uint32_t *dst, int64_t dst_stride_px, int dst_w, int dst_h, int filter);
TM_API int tm_stage_scale_rgb32(const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, int src_w, int src_h,
                                void *dst, int64_t dst_stride_px, int64_t dst_frame_px, int dst_w, int dst_h, int filter, void *stream);
/* tm_render_frames / tm_render_frames_yuv at another size: the same frames, resampled (out: [frame_count][out_h][out_w]; for the YUV call
 * dst->width and dst->height give the size).  The frames are drawn at tm_w*8 x tm_h*8 in chunks of at most 32 frames or 256 MB, scaled
 * behind the render, then delivered or converted.  The refusals of the unscaled calls and of tm_probe_scale_host apply, before any device
 * call; a device group reads what the unscaled twin reads.  Blocking. */
TM_API int tm_render_frames_scaled(tm_encoder *, int first_frame, int frame_count, int input, int out_w, int out_h, int filter,
                                   void *out, int out_on_device);
TM_API int tm_render_frames_yuv_scaled(tm_encoder *, int first_frame, int frame_count, int input, const tm_yuv_out *dst, int mode, int filter);
/* Pixel-domain quality of the decoded output against the source, frames [first_frame, first_frame+frame_count), over tm_w*8 x tm_h*8:
 * sse [count][3] exact squared errors of R, G, B; psnr [count] = 10 log10(3 W H 255^2 / (SSE_R+SSE_G+SSE_B)), +inf for SSE 0;
 * ssim_y [count] = mean SSIM of the 8x8 windows on a 4-pixel grid of GenerateY4M's Y plane (c1 = (64*0.01*255)^2, c2 = (64*0.03*255)^2 on
 * the windows' integer sums); clip_psnr from the range's summed SSE, clip_ssim_y the mean of the frames'.  The render is fused with the
 * sums: no frame is materialised.  Any pointer may be NULL.  Errors as tm_render_frames (both renders are needed). */
TM_API int tm_get_frame_quality(tm_encoder *, int first_frame, int frame_count, uint64_t *sse /* [count][3] */, double *psnr /* [count] */,
                                double *ssim_y /* [count] */, double *clip_psnr, double *clip_ssim_y);
/* ---- Render's other views (Render :3455-3736 with its switches; tm_render_view.hip) ---------------------------------
 * tm_render_frames draws with the constructor's switches.  A tm_render_view names the others: the page, and FRenderPredicted,
 * FRenderMirrored, FRenderOutputDithered, FRenderUseGamma, FRenderPaletteIndex and RenderGammaValue.  Pixels are 0x00RRGGBB, background
 * is 0 (the GUI's hatched brush, its motion-vector lines and its texts are not drawn).  THE RULE:
 *   DrawTile (:3457-3506).  The colour starts as magenta, 0x00FF00FF.  With a palette and the tile's HasPalPixels flag it is
 * palette[pal_px[mirrored (ty, tx)]] with R and B swapped -- 0 for a colour index at or beyond the palette size; without a palette and with
 * the tile's HasRGBPixels flag it is the tile's RGB pixel with R and B swapped.  Then, with use_gamma, every channel c becomes lut[c]
 * (tm_render_gamma_lut_host; also the magenta and the 0 of a colour index out of range: they are DrawTile's).  Background and aqua are not
 * DrawTile's and stay as they are.  The Output page ignores the tile's Active flag, as tm_render_frames does; the Tiles page honours it
 * (an inactive tile is magenta).
 *   Output page (:3574-3634), per item.  Predicted and view.predicted: the previous frame's picture under the same view at the offset,
 * clamped per pixel (before frame 0: background).  Otherwise -- predicted items too when view.predicted is 0 -- the item is drawn as its
 * stored TileIdx / PalIdx say: a TileIdx out of range is background; dithered and palette_index < 0: the item's own palette, a PalIdx out
 * of range is background; dithered and palette_index >= 0: drawn where PalIdx == palette_index, background elsewhere; dithered 0: no
 * palette and no filter, the tile's RGB pixels.  mirrored 0 drops the item's two mirror flags.  A predicted pixel follows its chain to
 * the first drawn item and takes that item's colour under the view (background where the filter skips it), so gamma is applied once.
 *   Input page (:3538-3570).  The frame tiles, un-mirrored by their initial flags (mirrored) or in their stored orientation (mirrored 0);
 * gamma applies; every other switch is ignored.
 *   Tiles page (:3678-3707).  Page p is a picture of the frame's size whose cell (sy, sx) shows tile tm_w*sy + sx + tm_w*tm_h*p, aqua
 * (0x0000FFFF) beyond the last tile; ceil(tiles / (tm_w*tm_h)) pages.  With dithered and at least one palette the palette is
 * palette_index if >= 0, else max(0, PalIdx_Initial) -- background where that is beyond the palettes (the reference would index past
 * FPalettes); otherwise the RGB pixels.  Mirrors are the tile's HMirror_Initial / VMirror_Initial when mirrored is set.
 * With tm_render_view_default the Output page is tm_render_frames(input = 0) bit for bit and the Input page is input = 1. */
enum { TM_RENDER_PAGE_INPUT = 0, TM_RENDER_PAGE_OUTPUT = 1, TM_RENDER_PAGE_TILES = 2 };   /* TRenderPage: rpInput, rpOutput, rpTilesPalette */
typedef struct {
  int32_t page;           /* TM_RENDER_PAGE_* */
  int32_t predicted;      /* FRenderPredicted */
  int32_t mirrored;       /* FRenderMirrored */
  int32_t dithered;       /* FRenderOutputDithered */
  int32_t use_gamma;      /* FRenderUseGamma */
  int32_t palette_index;  /* FRenderPaletteIndex; < 0: every palette */
  double  gamma;          /* RenderGammaValue = FGamma[1]; the constructor's 0.6 */
} tm_render_view;         /* 32 bytes; offsets 0, 4, 8, 12, 16, 20, 24 */
/* Host only, no device.  tm_render_view_default: the constructor's values (:5495-5509) -- page OUTPUT, predicted, mirrored and dithered 1,
 * gamma off at 0.6, palette_index -1.  tm_probe_render_view_host: TM_E_INVAL for a null struct, an unknown page, a NaN gamma, or
 * palette_index >= pal_count (the reference would index past FPalettes there); a negative gamma is not refused, it counts as 0
 * (SetRenderGammaValue, :3024-3027).  tm_render_gamma_lut_host: the table DrawTile applies (:3490-3495 with InitLuts :1689-1694),
 * lut[i] = RoundHalfEven(pow(i / 255.0, max(0, gamma)) * 255.0) in double; gamma 1 is the identity, gamma 0 is 255 everywhere
 * (pow(0, 0) = 1).  The device only looks the table up. */
TM_API int tm_render_view_default(tm_render_view *view);
TM_API int tm_probe_render_view_host(const tm_render_view *view, int pal_count);
TM_API int tm_render_gamma_lut_host(double gamma, uint8_t lut[256]);
/* Pages INPUT and OUTPUT of frames [first_frame, first_frame+frame_count): out, out_on_device and the refusals as tm_render_frames, plus
 * the probe's (pal_count = the encoder's palettes); page TILES here is TM_E_INVAL.  tm_render_tile_pages: pages [first_page,
 * first_page+page_count) of the Tiles page, [page_count][tm_h*8][tm_w*8]; the tiles must exist (after Reduce or ReloadGTM), a page range
 * outside tm_get_tile_page_count's is TM_E_INVAL; view->page is not looked at.  All refusals come before any device call and write
 * nothing.  In a device group the calls read shard 0, like the exports and tm_render_frames_yuv (page INPUT: a range shard 0 did not load
 * is TM_E_INVAL).  After tm_reload_gtm the tiles carry no RGB pixels (HasRGBPixels false): an undithered view is magenta where an item
 * is drawn, as in the reference.  Blocking. */
TM_API int tm_render_view_frames(tm_encoder *, const tm_render_view *view, int first_frame, int frame_count, void *out, int out_on_device);
TM_API int tm_render_tile_pages(tm_encoder *, const tm_render_view *view, int first_page, int page_count, void *out, int out_on_device);
TM_API int tm_get_tile_page_count(tm_encoder *, int *pages);
/* ReloadGTM, :2059 -> LoadStream, :4880-5175: replaces the encoder's tiles (palette indices only), palettes, tile maps and key
 * frames with the file's; the video set with tm_set_video must match the file's header (:5021-5032) or TM_E_INVAL comes back.
 * Afterwards the read-back views and tm_save_gtm work on the loaded state. */
TM_API int tm_reload_gtm(tm_encoder *, const char *path);
/* ---- The .gtm player: an object of its own, no encoder behind it (tm_player.hip, tm_player_parse.hip, tm_play_frame.hip) --------------------------------
 * tm_player_open reads the GTMv header and the GTMk index and decodes the FIRST key frame's stream only (it carries the settings text,
 * SetDimensions, the TileSet and the palettes); frames then come out in order, key frame by key frame, each frame one kernel launch that
 * reads the frame before it.  A frame is, bit for bit, what tm_render_frames(first, count, input = 0) gives after tm_reload_gtm of the same
 * file: a drawn item is palette[PalIdx][tile[mirrored (ty, tx)]] with R and B swapped (0 for a colour index >= the palette size, for a
 * tile or palette index out of range); a predicted item is the previous output frame at (clamp(y + PredictedY), clamp(x + PredictedX)),
 * clamped per pixel; SkipBlock items are predicted with offset (0, 0); before frame 0 the picture is 0.  An intra tile travels with its
 * item.  Two differences, neither reachable with a stream tm_save_gtm writes: a ShortShort / LongShort / LongLong item that names a tile at
 * or beyond the end of the TileSet draws 0 (after tm_reload_gtm it draws whatever intra tile of the WHOLE file landed in that slot), and
 * after tm_player_seek a predicted item in a key frame's first frame reads 0 instead of the key frame before.
 *   Memory does not depend on the clip's length beyond the index (28 bytes per key frame).  Host: the records of two key frames (the one
 * playing, the one a worker thread decodes ahead: 8 bytes per item + 64 per intra item) and two page-locked chunks.  Device: the TileSet,
 * the palettes, two chunks of records, one kept frame, and -- for host destinations and seeks -- a ring of two chunks of frames.
 *   Refusals, all before any device call: TM_E_UNSUPPORTED for a file without the GTMv header (tm_reload_gtm reads those; without the index
 * there is no seek and no frame count); TM_E_IO for a truncated or damaged file, index or command stream, a key frame whose decoded size
 * or frame count differs from its GTMk entry, a SetDimensions that is not the header's picture size (or more than 2^24 items a frame), an
 * incomplete tile map at FrameEnd, a tile set beyond the declared tile count;
 * TM_E_INVAL for a seek out of range. */
typedef struct tm_player tm_player;
typedef struct {
  int32_t width, height, tm_w, tm_h, frames, keyframes;   /* pixels: tm_w * 8 x tm_h * 8 is what tm_player_read delivers */
  int32_t tile_count, tileset_tiles, pal_size, pal_count, encoder_version;
  uint32_t avg_bytes_per_s, kf_max_bytes_per_s;            /* the header's two byte rates */
  double fps;                                              /* 1e9 / SetDimensions' nanoseconds per frame */
  int64_t host_bytes, device_bytes;                        /* what the player holds now (high-water marks of its buffers) */
} tm_gtm_info;
TM_API int tm_player_open(const char *path, int device, tm_player **out);
TM_API int tm_player_info(tm_player *, tm_gtm_info *info);
TM_API int tm_player_keyframes(tm_player *, int32_t *start_frames /* keyframes */);
TM_API int tm_player_settings_text(tm_player *, char *buf, size_t cap, size_t *n);  /* *n = the text's length; buf may be NULL */
/* the next `count` frames as [count][tm_h*8][tm_w*8] uint32 0x00RRGGBB, into device memory of the player's device (16-byte aligned; frame i
 * of a call reads frame i - 1 of the same buffer, the last frame is also kept by the player, so the buffer is the caller's again on return)
 * or host memory (one copy per chunk; a single DMA each when page-locked).  *got < count only at the end of the stream.  Blocking.
 *   The player writes on a non-blocking stream of its own, which waits for nobody else's work: whatever the caller has queued that reads or
 * writes `out` must have completed before the call.  Every player call leaves the calling thread's current device as it found it.
 *   A later key frame that cannot be read (TM_E_IO) ends the call at the frame before it: *got frames have been delivered and are right,
 * the position stands at the damaged key frame, and a seek elsewhere goes on playing. */
TM_API int tm_player_read(tm_player *, int count, void *out, int out_on_device, int *got);
/* tm_player_read with a YUV destination (tm_yuv_out, see tm_probe_yuv_out_host): position, *got, errors and seeks behave as above; frame i
 * of the call goes to frame i of dst.  The player plays into its own RGB ring (a predicted item needs the previous RGB frame) and converts
 * each frame behind its k_play_frame on the same stream: device planes are written in place, host planes through a packed device ring, one
 * copy per plane and chunk (a 2-D copy where rows have padding).  A refused descriptor (TM_E_INVAL / TM_E_UNSUPPORTED; also when the call
 * would deliver more than dst->frames frames: min(count, frames left)) leaves position and destination untouched. */
TM_API int tm_player_read_yuv(tm_player *, int count, const tm_yuv_out *dst, int mode, int *got);
/* the next read starts at `frame` (0 .. frames; frames = the end): restarts at the key frame at or before it and plays forward without delivering */
/* The size frames are delivered at (0, 0: the stream's own, the default; filter: TM_SCALE_*).  May be called between any two reads; the
 * position does not move.  Refuses what tm_probe_scale_host refuses (and a size of which only one part is 0: TM_E_INVAL) and then leaves
 * the setting as it was.  With a size set, tm_player_read delivers [count][height][width] and tm_player_read_yuv wants a tm_yuv_out of
 * that width and height.  The player goes on playing at the stream's size into a ring of its own (a predicted item reads the previous
 * native frame; the kept last frame stays native) and scales a chunk behind its frames on the same stream, in one launch: straight into a
 * device destination, through a ring of two scaled chunks (one copy per chunk) into a host destination, through the scaled ring into the
 * YUV conversion.  A seek's catching up scales nothing.  tm_player_info keeps reporting the stream's size. */
TM_API int tm_player_set_output(tm_player *, int width, int height, int filter);
TM_API int tm_player_get_output(tm_player *, int *width, int *height, int *filter);  /* 0, 0: none set */
TM_API int tm_player_seek(tm_player *, int frame);
TM_API int tm_player_tell(tm_player *);  /* the frame the next read starts at */
/* wall ms since open, summed: LZMA decode, command parse (both on the worker thread when there is one), record staging + upload calls,
 * waits for the worker, kernel launches (host side); and ms from open's entry to the first delivered frame's completion */
TM_API int tm_player_timings(tm_player *, double ms[5], double *first_frame_ms);
TM_API void tm_player_close(tm_player *);
/* Host-only seams (no device).  tm_player_probe_host: header and index of a file as tm_player_open checks them (kf: [cap_kf][4] = first
 * frame, raw size, compressed size, milliseconds; *nkf = the file's count).  tm_player_parse_host: one key frame's decoded command bytes
 * into the player's records -- per frame tm_w * tm_h records of 8 bytes {uint32 a; uint16 pal; uint8 flags; uint8 0}: flags bit 0 / 1 H / V
 * mirror, bit 2 predicted (a = (uint8) PredictedX | (uint8) PredictedY << 8), bit 3 intra (a = index of its 64 index bytes among the
 * frame's intra tiles), else a = tile index -- and the frames' intra tiles (intra_first[f] = index of frame f's first one, [frames + 1]).
 * tm_w / tm_h / tile_count are what SetDimensions of the first key frame said (a SetDimensions in the stream itself must agree or they
 * must be 0).  Capacities count frames and tiles; *frames / *nintra are set even when a capacity is too small (TM_E_INVAL). */
TM_API int tm_player_probe_host(const char *path, tm_gtm_info *info, int32_t *kf, int cap_kf, int *nkf);
TM_API int tm_player_parse_host(const uint8_t *raw, size_t n, int tm_w, int tm_h, int64_t tile_count, uint64_t *records, int cap_frames,
                                uint8_t *intra, int64_t cap_intra, int64_t *intra_first, int *frames, int64_t *nintra);
/* One frame with the player's kernel on caller-held device arrays: records [tm_w*tm_h] (above), intra [nintra][64] (an index beyond: 0), tiles [ntiles][64],
 * palettes i32 [npal][pal_size] 0x00BBGGRR, prev (NULL: black) and out u32 [tm_h*8][tm_w*8] 0x00RRGGBB, 16-byte aligned. */
TM_API int tm_stage_play_frame(const void *records, const void *intra, int64_t nintra, const void *tiles, const void *palettes, const void *prev, void *out,
                               int tm_w, int tm_h, int pal_size, int64_t ntiles, int npal, void *stream);
/* Multi-GPU (one process per GPU): this process matches only frames [first, first+count) in Reconstruct (frames are
 * independent in the KNN branch, DoXY :1464); the host then merges the per-frame results of all processes with an
 * all-reduce(MAX) over the arrays below (other shards hold -1) and calls tm_sync_tilemap before Reindex.
 * PredictMotion honours the same range (its frames are independent, :1982-1985); with motion prediction on, the range
 * given for Reconstruct must start on a key frame (frames chain inside a key frame, :1496). */
enum { TM_ARRAY_TILEMAP_TILE = 0, TM_ARRAY_TILEMAP_ERR = 1, TM_ARRAY_TILEMAP_PAL = 2,
       /* with motion prediction: uint8 IsPredicted, int8 PredictedX, int8 PredictedY (1 byte per item; other shards hold 0: merge with SUM) */
       TM_ARRAY_TILEMAP_PRED = 3, TM_ARRAY_TILEMAP_PX = 4, TM_ARRAY_TILEMAP_PY = 5,
       TM_ARRAY_PM_ERR = 6 /* uint32 best error of PredictMotion per item; other shards hold 0 */,
       TM_ARRAY_TILE_PALPX = 7 /* uint8 [tiles][64] dithered palette indices (DitherTile's output, :2690-2724); tiles of other
                                  dither shards hold 0: merge with SUM, as bytes or as count/4 32-bit words (count is a multiple of 64) */ };
TM_API int tm_set_query_shard(tm_encoder *, int first_frame, int frame_count /* <0: to the end */);
/* One process per GPU with the merges INSIDE the steps: the host hands the encoder its rank, the number of processes and a
 * callback that performs a collective over them (the host's own communicator -- RCCL through torch.distributed in bench.py, gloo in the
 * CPU tests; the library ALSO links RCCL and can carry the collectives itself, tm_comm_init below, which bench.py takes with
 * TM_BENCH_NATIVE=1).  The callback runs on the caller's thread with the encoder's stream idle; it returns 0 once the result is in place.
 *   kind: TM_COLL_ALLREDUCE_SUM_I32 / _MAX_I32 / _SUM_I64: `count` elements in `dev_buf`, in place;
 *         TM_COLL_ALLGATHER_BYTES: `count` bytes from `dev_buf` of every process into `dev_recv` (world x count bytes, rank order).
 * With it set, Run(step) shards by itself: Load by frame (motion prediction off), Reduce as a local exact dedup + an all-gather of
 * the distinct tiles + a dedup of the union, PreparePalettes as data-parallel Lloyd (all-reduce of the integer sums per
 * iteration) and palette-parallel colour quantisation, Dither by global tile, Reconstruct with the database rows built per share
 * and all-gathered and the query frames of tm_set_query_shard.  Every process ends each step with the same global tiles,
 * palettes and merged tile maps as a single-process run. */
enum { TM_COLL_ALLREDUCE_SUM_I32 = 0, TM_COLL_ALLREDUCE_MAX_I32 = 1, TM_COLL_ALLREDUCE_SUM_I64 = 2, TM_COLL_ALLGATHER_BYTES = 3 };
typedef int (*tm_collective_cb)(void *user, int kind, void *dev_buf, void *dev_recv, int64_t count);
TM_API int tm_set_collective(tm_encoder *, int rank, int world, tm_collective_cb cb, void *user);
/* The HIP stream (hipStream_t) every step of this encoder is queued on, and the callback's contract with it.  Mode 0 (default): the
 * library drains the stream before each callback and the callback returns with the result in place (any communicator, any stream).
 * Mode 1, stream-ordered: the callback ENQUEUES the collective on that stream (RCCL: ncclAllReduce(..., stream), or a
 * torch.distributed call made with the stream current) and returns at once; the library neither drains before nor waits after --
 * the ~80 collectives of a step (one per Lloyd iteration among them) then cost no host round trip each. */
TM_API void *tm_get_stream(tm_encoder *);
TM_API int tm_set_collective_mode(tm_encoder *, int stream_ordered);
/* The native form of the above -- what a FreePascal host needs for N GPUs and nothing else: RCCL is linked into the library, one
 * process per GPU.  One process obtains an id (tm_comm_unique_id = ncclGetUniqueId), hands its 128 bytes to the others by any
 * means (a file, an environment variable, a pipe), and every process calls tm_comm_init(enc, id, rank, world) on an encoder whose
 * device has been chosen (tm_set_device).  From then on Run(step) shards and merges as described for tm_set_collective, with the
 * four collective kinds issued as ncclAllReduce / ncclAllGather on the encoder's own stream: no callback, no host round trip.
 * tm_comm_init is collective (ncclCommInitRank: it returns once all `world` processes have called it).  Sits where the
 * reference's Run (tilingencoder.pas:5529-5554) sits: the host's code above it does not change with the number of GPUs. */
#define TM_COMM_ID_BYTES 128
TM_API int tm_comm_unique_id(uint8_t id[TM_COMM_ID_BYTES]);
TM_API int tm_comm_init(tm_encoder *, const uint8_t id[TM_COMM_ID_BYTES], int rank, int world);
TM_API int tm_comm_destroy(tm_encoder *);
/* Collectives this process has issued since the last reset, by kind (index = TM_COLL_*), and the bytes it put through them
 * (all-reduce: the buffer; all-gather: world x the piece) -- whichever of the two paths above carries them. */
TM_API int tm_get_collective_stats(tm_encoder *, int64_t calls[4], int64_t *bytes, int reset);
/* Dither (DoDither :1873-1907, one independent DitherTile per global tile): this process dithers tiles
 * [T * rank / world, T * (rank + 1) / world) only (T = global tiles after Reduce) and zeroes the rest; the host merges
 * TM_ARRAY_TILE_PALPX with an all-reduce(SUM) before Reconstruct.  (0, 1) = every tile (default). */
TM_API int tm_set_dither_shard(tm_encoder *, int rank, int world);
TM_API int tm_get_device_array(tm_encoder *, int which, void **dev_ptr, int64_t *count /* elements: int32 for 0-2 and 6, bytes for 3-5 and 7 */);
TM_API int tm_sync_tilemap(tm_encoder *);
/* device time (HIP events on the encoder's stream) of the KNN distance kernel over the last Reconstruct */
/* pairs = (query, distinct database row) pairs the kernel evaluated; db_rows = distinct rows searched (<= global tiles) */
TM_API int tm_get_knn_stats(tm_encoder *, double *kernel_ms, int64_t *pairs, int *launches, int *k_bytes, int64_t *db_rows);
/* the same launches kernel by kernel (the scan is three kernels): device ms of k_knn_seed / k_knn_lists / k_knn_consume,
 * the (query, row) pairs the seed and the consume kernel evaluated, and the 32x32x32 int8 matrix instructions the consume kernel issued for them
 * (a chain has 6 + HT + HQ + min(HT, HQ); products with an all-zero high-digit chunk are skipped); kernel_ms above is the sum of the three
 * times, pairs the sum of the two counts */
TM_API int tm_get_knn_kernel_split(tm_encoder *, double ms[3], int64_t pairs[3]);
/* queries of the last Reconstruct's searches: the DISTINCT frame tiles when Reduce's exact groups can be used (one process, motion
 * prediction off), every tile-map item otherwise */
TM_API int64_t tm_get_knn_queries(tm_encoder *);
/* the last Dither: the distinct (palette, colour) pairs it planned once each (pixels look their pair up), 0 when every pixel was planned on
 * its own (few duplicates, the Yliluoma ditherer, few tiles for the number of palettes) */
TM_API int64_t tm_get_dither_pairs(tm_encoder *);
/* What the last PreparePalettes ran through (single process): Lloyd iterations and points of the tile -> palette clustering
 * (DoPalettization, tilingencoder.pas:4105-4245; yakmo's cap is cYakmoMaxIterations = 300) and, for the colour quantisation
 * (QuantizeUsingYakmo, :4434-4532), the iterations of the slowest palette, the distinct colours clustered, the pixels they stand for and
 * the sum over the palettes of (distinct colours x iterations). */
TM_API int tm_get_kmeans_iters(tm_encoder *, int *tile_iters, int64_t *tile_points, int *pixel_iters, int64_t *pixel_colours, int64_t *pixels,
                               int64_t *pixel_colour_iters);

/* ======================================================================================= stage seam
 * All pointers are DEVICE pointers unless named host_*.  `stream` is a hipStream_t (NULL = default stream).
 * Tiles are [n][64] uint32 0x00BBGGRR in the reference's canonical (mirrored) orientation. */

/* A1+A2+A3: TFrame.LoadFromImage (:1293) + PrepareInterFrameData (:1329) + mirror canonicalisation (:1393-1411).
 * frames: [nframes][img_h][img_w] RGB32.  Outputs: tiles [nframes*tm_w*tm_h][64], flags u8 (bit0 H, bit1 V),
 * lab_means f32 [ntiles][3]. */
TM_API int tm_stage_load(const void *frames, int nframes, int img_w, int img_h, int tm_w, int tm_h,
                         void *tiles, void *flags, void *lab_means, void *stream);

/* PearsonCorrelation (:2201-2228) of consecutive frames, the correlation Load finds its key frames with, in two seams.
 * tm_pearson_finish_host (host only, no device call): its last lines (:2221-2227) on the raw sums (num, sum dx^2, sum dy^2) of n frames ->
 * correl[f] = num / (sqrt(sum dx^2) * sqrt(sum dy^2)) in IEEE Single arithmetic, 1 where that denominator is 0; correl[0] = 0 (frame 0
 * has no predecessor; its sums are not read).  Load's own tail calls it.
 * tm_stage_pearson: the sums of [nframes][per] Singles in DEVICE memory (per >= 1: Load passes 3 x the tile count), read back and finished
 * with the function above -> HOST float32 [nframes].  Blocking. */
TM_API int tm_pearson_finish_host(const float *sums /* [n][3] */, int n, float *correl /* [n] */);
TM_API int tm_stage_pearson(const void *lab_f32, int nframes, int per, void *correl_f32_host, void *stream);

/* Planes of 8-bit Y, U, V -> RGB32 frames [nframes][dst_h][dst_w] 0x00RRGGBB, the format frames are pushed in: chroma upsampling, the
 * Lanczos-3 resize to dst_w x dst_h and the colour conversion in one kernel (what tm_open_input's Load runs per chunk of frames).  strides
 * (HOST array): row and frame stride in bytes of y, u, v -- {y_row, y_frame, u_row, u_frame, v_row, v_frame}; chroma: TM_CHROMA_* (MONO: u,
 * v unused, U = V = 128); yuv_mode: TM_YUV_* (AUTO = BT601_LIMITED here: there is no header).  The rule, bit for bit (DESIGN.md section
 * 17): separable, horizontal first; per axis r = n / m, f = max(1, r / s), u_j = ((j + 0.5) r - 0.5 - o) / s, taps ceil(u_j - 3f) ..
 * floor(u_j + 3f) inside the plane, c_k = RoundHalfEven(16384 w_k / sum w) with w_k = sinc(t) sinc(t / 3), t = (k - u_j) / f, the
 * remainder to the largest tap; h = (sum c p + 64) >> 7, v = clamp((sum c h + 2^20) >> 21, 0, 255).  BT601_LIMITED: C = Y - 16,
 * R = (298C + 409E + 128) >> 8, G = (298C - 100D - 208E + 128) >> 8, B = (298C + 516D + 128) >> 8; BT601_FULL: libjpeg's 16-bit
 * constants 91881, 22554, 46802, 116130.  Blocking (builds and frees the tap tables). */
TM_API int tm_stage_yuv_to_rgb32(const void *y, const void *u, const void *v, const int64_t *host_strides /* [6] */, int nframes, int src_w, int src_h,
                                 int chroma, int dst_w, int dst_h, int yuv_mode, void *out_rgb32, void *stream);
/* The same for every sample format of tm_yuv_clip (see there for the depth rule and the interleaved layout): v == NULL means (U, V) pairs in
 * u; samples: TM_SAMPLES_*; depth: 8, or 9 .. 16 for words.  With TM_SAMPLES_U8, depth 8 and three planes it is tm_stage_yuv_to_rgb32.
 * yuv_mode also takes TM_YUV_BT709_LIMITED / _FULL, as the call above does. */
TM_API int tm_stage_yuv_to_rgb32_fmt(const void *y, const void *u, const void *v /* NULL: pairs in u */, const int64_t *host_strides /* [6], bytes */,
                                     int nframes, int src_w, int src_h, int chroma, int samples, int depth,
                                     int dst_w, int dst_h, int yuv_mode, void *out_rgb32, void *stream);
/* The way back (k_rgb32_to_yuv, tm_yuv_out.hip): frames [nframes][h][stride_px] 0x00RRGGBB -> planes as tm_yuv_out describes them (rule,
 * footprints and refusals: see tm_probe_yuv_out_host; AUTO = BT601_LIMITED).  v == NULL: pairs in u.  Any w, h >= 1; U8 planes at any byte
 * address.  Bytes outside the rows are not touched.  Queued on `stream`, not blocking. */
TM_API int tm_stage_rgb32_to_yuv_fmt(const void *rgb32, int64_t stride_px, int nframes, int w, int h, void *y, void *u, void *v /* NULL: pairs in u */,
                                     const int64_t *host_strides /* [6], bytes */, int chroma, int samples, int depth, int mode, void *stream);

/* RGBToLAB (utils.pas:374-410) of n colours 0x00RRGGBB -> float [n][3] (L, a, b): the colour conversion the load and feature kernels
 * share, as an operator of its own (the whole 24-bit domain is checked against the oracle through it). */
TM_API int tm_stage_rgb_to_lab(const void *rgb, int64_t n, void *out_lab, void *stream);

/* A4+A5: ConvertToCpnPixels (:3049) + ComputeCpnPixelsPsyVisFeatures (:3103) -> int16 [n][192].
 * mirror_flags may be NULL (no un-mirroring). */
TM_API int tm_stage_features_rgb(const void *tiles, int64_t n, const void *mirror_flags, int mode, int use_lab,
                                 void *out_i16, void *stream);
/* The same for a list of rows, as Reconstruct asks for its queries: out row i = the features of tile rows[i] (i32 [n], repeats allowed; no
 * un-mirroring).  colmm may be NULL; else i32 [384] on the device, preset by the caller to 192 x INT_MAX, then 192 x INT_MIN: the minimum and the
 * maximum of each of the 192 output columns are folded in (what the nearest-neighbour search's digit plan reads). */
TM_API int tm_stage_features_rgb_rows(const void *tiles, const void *rows, int64_t n, int mode, int use_lab, void *out_i16,
                                      void *colmm_or_null, void *stream);
/* FromPal=True variant (PrepareReconstruct.DoPsyV, :4570-4583): pal_px u8 [n][64], pal_idx i32 [n],
 * palettes i32 [npal][pal_size]. */
TM_API int tm_stage_features_pal(const void *pal_px, const void *pal_idx, int64_t n, const void *palettes, int pal_size,
                                 int mode, void *out_i16, void *stream);
/* A6 as used by DoPalettization (:4126,:4160): double DCT with UseLAB, Round()ed to int32 [n][192].
 * mode TM_PVS_WAVELETS: the double path's Haar branch instead (WaveletGS, :2727-2764, depth 2), Round()ed the same way.
 * (The int16 entry points above reject TM_PVS_WAVELETS, as the reference asserts at :3111.) */
TM_API int tm_stage_features_cluster(const void *tiles, int64_t n, int mode, void *out_i32, void *stream);

/* FrameTilingExtendedPaletteUsage (:1559-1610).
 * ann_kdtree_short_search_multi(k, eps 0) for a batch: the k nearest database rows of every query by true L2, ordered by
 * (distance, index); out_idx i32 [nq][k] (-1 pads a database smaller than k), out_err u32 [nq][k]. */
TM_API int tm_stage_knn_topk(const void *queries_i16, int64_t nq, const void *db_i16, int64_t nt, int k, void *out_idx, void *out_err,
                             void *stream);
/* The re-rank: every unique tile of knn_idx[q][] x every unique palette of those tiles (tile_pal_idx = PalIdx_Initial),
 * distance = CompareEuclideanDCTPtr_asm as written (utils.pas:559-725); first strict minimum in ascending (tile, palette)
 * order.  out_tile / out_pal i32 [nq], out_err u32 [nq].  Blocking (builds and frees the ntiles x npal feature table). */
TM_API int tm_stage_epu_rerank(const void *queries_i16, int64_t nq, const void *knn_idx, int k, const void *pal_px, const void *tile_pal_idx,
                               int64_t ntiles, const void *palettes, int npal, int pal_size, void *out_tile, void *out_pal, void *out_err,
                               void *stream);

/* Motion prediction (PredictMotion :1154-1282 and the redo in Reconstruct :1496-1532).
 * DoDCTs: pvsWeightedDCT features of every 8x8 window of a frame buffer [height][width] u32 0x00BBGGRR
 * -> int16 [(height-7)*(width-7)][192], row-major over window positions. */
TM_API int tm_stage_window_dcts(const void *frame_buffer, int width, int height, void *out_i16, void *stream);
/* DoXY search: cur = features of the frame's tiles in ORIGINAL orientation [tm_h*tm_w][192]; window_dcts of the
 * previous frame buffer (tm_w*8 x tm_h*8); radius = MotionPredictRadius (1..128, decremented inside like :1271).
 * Error = CompareEuclideanDCTPtr_asm as written (utils.pas:559-725, entry xmm7 = 0) + manhattan distance; first strict
 * minimum in raster order.  out_err u32, out_px / out_py int8 (PredictedX / PredictedY). */
TM_API int tm_stage_motion_search(const void *cur_i16, int tm_w, int tm_h, const void *window_dcts, int radius, void *out_err,
                                  void *out_px, void *out_py, void *stream);
/* The two in one, as PredictMotion runs them per frame: the search of cur in frame buffer fb_rgb32 ([tm_h*8][tm_w*8] u32 0x00BBGGRR), whose
 * window features are made straight in the search's matrix layout; the int16 rows (allocated inside) are written only when the frame falls
 * back to the VALU search.  TM_MOTION_PACK_SEPARATE, TM_MOTION_FORCE_FLAG, TM_MOTION_VALU and TM_WINDOW_DCTS_BY_TILE pick its other forms.
 * Blocking. */
TM_API int tm_stage_motion_search_fb(const void *cur_i16, int tm_w, int tm_h, const void *fb_rgb32, int radius, void *out_err,
                                     void *out_px, void *out_py, void *stream);

/* A13+A14 (KNN branch): exact nearest neighbour of every query in the database, both int16 [.][192];
 * what ann_kdtree_short_search(eps=0) answers (:1547).  Ties: lowest database index.
 * out_idx i32 [nq], out_err u32 [nq].  Blocking (needs one 1.5 KB read-back for the digit plan). */
TM_API int tm_stage_knn(const void *queries_i16, int64_t nq, const void *db_i16, int64_t nt,
                        void *out_idx, void *out_err, void *stream);
/* Same with a prepared database (ann_kdtree_create analogue): pack once, search many query batches. */
typedef struct tm_knn_index tm_knn_index;
TM_API tm_knn_index *tm_knn_index_create(const void *db_i16, int64_t nt, void *stream);
TM_API void tm_knn_index_destroy(tm_knn_index *);
TM_API int tm_knn_index_search(tm_knn_index *, const void *queries_i16, int64_t nq, void *out_idx, void *out_err, void *stream);
/* measured device time (ms, HIP events on `stream`) of the distance kernel in the last search, and its MFMA K */
TM_API int tm_knn_index_last_stats(tm_knn_index *, double *kernel_ms, int *k_bytes, int64_t *pairs);
/* diagnostics (tests): entries of the last search's tile lists, and how many of them its consumer took off the lists (fewer where a sorted
 * segment was ended early; equal with TM_KNN_LIST_ORDER=0) */
TM_API int tm_knn_index_last_list_counts(tm_knn_index *, int64_t *listed, int64_t *popped);
/* diagnostics (tests): listed blocks (tile x 32 queries) the last search judged on their first chunk of columns, and how many of them ended
 * there (both 0 with TM_KNN_FIRST_CHUNK=0) */
TM_API int tm_knn_index_last_chunk_counts(tm_knn_index *, int64_t *looked, int64_t *stopped);
/* diagnostics (tests): the survivor queue of the last search's consume kernel -- tiles popped and looked at, those of them none of whose blocks
 * got past its look (never loaded beyond their first chunk), survivor entries pushed to the queue, and entries the full queue turned away
 * (their chains ran in the looking wave), tiles loaded whole (chain tasks run: pushed + ring_full with the look, every tile without) and
 * the consume kernel's blocks that ran to completion; no_survivor, pushed and ring_full are 0 with TM_KNN_FIRST_CHUNK=0 */
TM_API int tm_knn_index_last_survivor_counts(tm_knn_index *, int64_t *tiles, int64_t *no_survivor, int64_t *pushed, int64_t *ring_full, int64_t *whole,
                                             int64_t *completed);
/* diagnostics (tests): the digit plan of the calling thread's last scan -- 32-column chunks that carry a high digit on the database / query
 * side, 0..6 each, and whether it was the k-nearest collection: together they name the instantiation of the scan's kernels that ran -- and
 * how often a scan of this process has been repeated with a larger tile-list arena (TM_KNN_ARENA_ENTRIES sets the first size) */
TM_API int tm_knn_last_plan(int *ht, int *hq, int *topk, int64_t *arena_retries);
/* diagnostics for the tests: the database's row order as the scan of a searched index sees it (host memory, uint32 [nt]: tile t holds rows
 * out[32 t .. 32 t + 31]: the rows the curve sort put there, in ascending index) */
TM_API int tm_knn_index_row_order(tm_knn_index *, void *out_rows_u32, void *stream);
/* ... and the step that orders them, on its own: every run of 32 entries of perm (device memory, uint32 [n]) into ascending order, in place */
TM_API int tm_stage_knn_tile_order(void *perm_u32, int64_t n, void *stream);
/* ... and the key both sides of a search are sorted by, on its own (k_curve_keys' arithmetic: curve_key, tm_knn_kernel.h): n cells of four
 * quantised coordinates (device memory, uint32 [n][4], coordinate d below 2^bits[d]) into keys (device memory, uint32 [n]).  kind 0: the
 * coordinates' bits interleaved (Morton order; the bits sum to 32 at most); kind 1: the Hilbert index on a grid of max(bits) bits per
 * axis, an axis with fewer bits shifted up (every bits[d] 8 at most).  bits: HOST memory, int [4]. */
TM_API int tm_stage_curve_keys(const void *coords_u32, int64_t n, const int *bits, int kind, void *keys_u32, void *stream);

/* Render (:3455-3640) of nframes frames from their tile maps, on device pointers: tile_idx / pal_idx i32 [nframes][tm_h*tm_w],
 * item_flags u8 (bit 0 H mirror, bit 1 V mirror, bit 2 predicted), px / py int8 (PredictedX / PredictedY), pal_px u8 [ntiles][64],
 * palettes i32 [npal][pal_size] 0x00BBGGRR -> out u32 [nframes][tm_h*8][tm_w*8] 0x00RRGGBB, as tm_render_frames draws them. */
TM_API int tm_stage_render(const void *tile_idx, const void *pal_idx, const void *item_flags, const void *px, const void *py, int tm_w, int tm_h,
                           int nframes, const void *pal_px, int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, void *stream);
/* Render's other views (tm_render_view above) from caller-held tables: the pointers of tm_stage_render, plus rgb_px u32 [ntiles][64]
 * 0x00BBGGRR (16-byte aligned; pal_px 4-byte aligned), tile_flags u32 [ntiles] (the tm_tile_hdr.Flags bits) and pal_idx_initial i32 [ntiles].
 * Pages OUTPUT (nframes frames) and TILES (nframes pages from page 0, at most the tiles' page count; the tile-map pointers may be null) ->
 * out u32 [nframes][tm_h*8][tm_w*8]; page INPUT and what tm_probe_render_view_host(view, npal) refuses are TM_E_INVAL.  Queued on `stream`. */
TM_API int tm_stage_render_view(const tm_render_view *view, const void *tile_idx, const void *pal_idx, const void *item_flags, const void *px,
                                const void *py, int tm_w, int tm_h, int nframes, const void *pal_px, const void *rgb_px, const void *tile_flags,
                                const void *pal_idx_initial, int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, void *stream);
/* The sums behind tm_get_frame_quality for two stacks of frames a (source) and b (decoded), u32 0x00RRGGBB [nframes][h][stride_px]
 * (w, h multiples of 4, at least 8): sse_u64 [nframes][3] (R, G, B), ssim_f64 [nframes], both device pointers. */
TM_API int tm_stage_frame_quality(const void *a, const void *b, int nframes, int w, int h, int64_t stride_px, void *sse_u64, void *ssim_f64,
                                  void *stream);

/* A12: Dither (:1873) = PreparePlan (:2268) + DitherTile (:2688) for every tile.  tiles/flags as above,
 * pal_idx i32 [n], palettes i32 [npal][pal_size] -> pal_px u8 [n][64] (canonical orientation). */
TM_API int tm_stage_dither(const void *tiles, const void *flags, const void *pal_idx, int64_t n, const void *palettes,
                           int npal, int pal_size, int use_thomas_knoll, int y2_mixed_colors, void *out_pal_px, void *stream);

/* A8/A16: MakeTilesUnique (:4720) + ReindexTiles (:4626) on n rows of `row_bytes` (256: RGB dwords compared as
 * unsigned dwords; 64: palette indices compared as bytes).  use_in u32[n] or NULL (=1).
 * Outputs: remap i32 [n] (final index of each row's representative, -1 if its use count is 0),
 * order i32 [n] (first *n_unique entries: original index of the representative at each final position),
 * use_out u32 [n].  Blocking. */
TM_API int tm_stage_dedup(const void *rows, int64_t n, int row_bytes, const void *use_in,
                          void *remap, void *order, void *use_out, int64_t *host_n_unique, void *stream);

/* The grouping Reconstruct puts its database rows through (test seam): the distinct rows of n rows of `row_bytes` (a multiple of 16, compared
 * as dwords) in ascending order of their first occurrence.  remap i32 [n] (position of each row's first occurrence in `order`), order i32 [n]
 * (first *n_unique entries: the first occurrences, ascending), use_out u32 [n] (first *n_unique: rows per group).  Blocking. */
TM_API int tm_stage_dedup_by_index(const void *rows, int64_t n, int row_bytes, void *remap, void *order, void *use_out,
                                   int64_t *host_n_unique, void *stream);
/* How often the library has made the host wait for a stream so far in PreparePalettes and the dedup (its small read-backs anywhere, and the
 * stream synchronisations of those stages), over all threads of the process: tests hold a step's number of round trips with it. */
TM_API long long tm_host_waits(void);

/* A9/A10: the build's deterministic k-means (farthest-first init, exact integer sums); pts i32 [n][d],
 * weights u32 [n] or NULL.  assign i32 [n], centroids f64 [k][d] (device).  Returns live centroid count in *host_k. */
TM_API int tm_stage_kmeans(const void *pts_i32, const void *weights, int64_t n, int d, int k, int max_iter,
                           void *assign, void *centroids, int *host_k, int *host_iters, void *stream);
/* The same Lloyd iterations from the caller's own initial centres: host_init_idx[k] = indices of the points to start from (-1: none)
 * instead of the farthest-first picks -- the seam an experiment with another seeding rule (k-means++ and the like) goes through;
 * yakmo's own k-means++ draws cannot be reproduced. */
TM_API int tm_stage_kmeans_seeded(const void *pts_i32, const void *weights, int64_t n, int d, int k, const int64_t *host_init_idx, int max_iter,
                                  void *assign, void *centroids, int *host_k, int *host_iters, void *stream);
/* QuantizeUsingYakmo + DoQuantization (:4434-4564) for every palette at once: pixels of tiles grouped by pal_idx. */
TM_API int tm_stage_quantize_palettes(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter,
                                      void *out_palettes, void *stream);
/* DoPalettization (:4105-4245): cluster features -> PalIdx_Initial ranked by tile count. */
TM_API int tm_stage_palettize(const void *feat_i32, const void *use, int64_t n, int npal, int max_iter, void *out_pal_idx,
                              void *stream);
/* The D^2 seeding of that clustering alone (test seam): the k picked point indices, in pick order, to a host array of k entries (-1 beyond
 * the centres found); *out_kk = the number of centres found.  feat_i32: [n][192]; use: the points' weights, NULL = 1 each. */
TM_API int tm_stage_pp_seeds(const void *feat_i32, const void *use /* may be NULL */, int64_t n, int k,
                             int64_t *out_seeds_host /* k entries, -1 beyond the centres found */, int *out_kk, void *stream);
/* 1 when the calling thread's last k-means (tm_stage_kmeans*, or the one inside tm_stage_palettize / tm_stage_quantize_palettes) ran through a
 * resident launch to its end (k_h_resident, k_kmeans3_persistent), 0 when it took one launch per step -- by shape, by TM_KM_LAUNCHES, or
 * because a barrier of the resident launch gave up and the clustering was repeated (tests tell the two apart with it). */
TM_API int tm_kmeans_last_resident(void);
/* The first look of the calling thread's last tile k-means (D = 192; tm_stage_kmeans*, or the one inside tm_stage_palettize): how many
 * point-scorings (a point against all its centroids, once per plain iteration) were looked at in single precision, and how many of those
 * the look could not decide and handed to the double-precision chain.  Both 0 under TM_KM_FIRST_LOOK=0.  Either pointer may be NULL. */
TM_API void tm_kmeans_last_first_look(int64_t *looked, int64_t *exact);

/* A17: TKModes.ComputeKModes (kmodes.pas:923-1094; unreachable in the reference snapshot, named by the north star): k-modes on rows
 * of cKModesFeatureCount = 80 bytes (kmodes.pas:15; the reference's asm hard-codes 80, :338-342), dissimilarity = sum |a-b| + 2048 per
 * differing byte (:248-259), farthest-first initialisation from a starting point (:694-772), Huang's online mode update (:774-803),
 * empty-cluster repair with the LCG of :88-92 seeded $42381337 (:933), stop on cost non-decrease with three graces (:1040-1049).
 * HOST pointers, like the Pascal arrays: rows [n][80] with values < num_modalities, labels int32 [n] (0-based, as the code returns
 * them), centroids [num_clusters][80].  num_init <= 0: one run from point -num_init; > 0: that many runs from spread starting points
 * (:952-964), the cheapest kept.  max_iter < 0: no limit (aMaxIter = -1).  An upload and a read-back round tm_stage_kmodes_dev. */
TM_API int tm_stage_kmodes(const uint8_t *host_rows, int64_t n, int num_clusters, int num_init, int num_modalities, int max_iter, int32_t *host_labels,
                           uint8_t *host_centroids, uint64_t *host_cost, int *host_iters, void *stream);

/* The same on DEVICE pointers (rows [n][80], labels [n], centroids [num_clusters][80]); cost, the best run's iteration count and the
 * points x iterations gone through (all runs) come back to the host.  Blocking. */
TM_API int tm_stage_kmodes_dev(const uint8_t *dev_rows, int64_t n, int num_clusters, int num_init, int num_modalities, int max_iter, int32_t *dev_labels,
                               uint8_t *dev_centroids, uint64_t *host_cost, int *host_iters, int64_t *host_point_iters, void *stream);

/* A17, the other half: dl3quant (dlquant/quantizer.c:437-455; imported at extern.pas:196, never called, DLL not shipped): Dennis Lee's
 * DL3 quantiser -- histogram at lookup_bpc bits per channel (build_table3, :486-518), greedy merging of the pair of least error
 * (reduce_table3, :583-648; calc_err, :520-541), the entries' rounded means as the palette (set_palette3, :650-664).  DEVICE pointers:
 * npixels x (R, G, B) bytes in, [3][quant_to] planar bytes out (like userpal), *out_colors = colours left (<= quant_to).  Blocking.
 * Parity unpinned (no reference output exists); checked against the oracle's restatement. */
TM_API int tm_stage_dl3quant(const uint8_t *dev_rgb, int64_t npixels, int quant_to, int lookup_bpc, uint8_t *dev_palette, int *out_colors, void *stream);

/* A11: OptimizePalettes (:4309-4432), host arithmetic on HOST memory (P x PaletteSize colours); in place. */
TM_API int tm_optimize_palettes_host(int32_t *palettes, int pal_count, int pal_size, int *sweeps);

/* ======================================================================================= fine seam
 * extern.pas:182-185 (ANN_short.dll), :198-203 (yakmo.dll), :218-223 (BICO.dll).  Host pointers. */
/* ANN.dll (extern.pas:178-180; call sites tilingencoder.pas:4128, 4183-4187): double coordinates, any dimension.  These are the
 * DLL's own export names.  ANN_short.dll exports the SAME names for its int16 build (the `_short` suffix exists on the Pascal
 * side only: `external 'ANN_short.dll' name 'ann_kdtree_create'`, extern.pas:182-185); one shared object cannot export one
 * name twice, so the int16 set is exported as ann_kdtree_short_* and the import unit names those.
 * Exact nearest row (eps is ignored: the reference passes 0), squared distance in *err, ties -> lowest index. */
typedef struct tm_annd tm_annd;
TM_API tm_annd *ann_kdtree_create(double **rows, int n, int dd, int bs, int split);
TM_API void ann_kdtree_destroy(tm_annd *);
TM_API int ann_kdtree_search(tm_annd *, const double *q, double eps, double *err);
TM_API int ann_kdtree_search_batch(tm_annd *, const double *queries, int nq, int32_t *idxs, double *errs);
typedef struct tm_ann tm_ann;
TM_API tm_ann *ann_kdtree_short_create(int16_t **rows, int n, int dd, int bs, int split);
TM_API void ann_kdtree_short_destroy(tm_ann *);
TM_API int ann_kdtree_short_search(tm_ann *, const int16_t *q, uint32_t eps, uint32_t *err);
TM_API void ann_kdtree_short_search_multi(tm_ann *, int32_t *idxs, uint32_t *errs, int cnt, const int16_t *q, uint32_t eps);
TM_API int ann_kdtree_short_search_batch(tm_ann *, const int16_t *queries, int nq, int32_t *idxs, uint32_t *errs);

/* yakmo.dll (extern.pas:198-203).  The clustering is the build's deterministic k-means: yakmo's
 * k-means++ RNG is not recoverable.  Inputs are rounded to int32; 3- or 192-column data only. */
typedef struct tm_yakmo tm_yakmo;
TM_API tm_yakmo *yakmo_create(uint32_t k, uint32_t restart_count, int max_iter, int init_type, int init_seed, int do_normalize, int is_verbose);
TM_API void yakmo_destroy(tm_yakmo *);
TM_API void yakmo_set_num_threads(int num_threads);
TM_API void yakmo_load_train_data(tm_yakmo *, uint32_t row_count, uint32_t col_count, double **dataset);
TM_API void yakmo_train_on_data(tm_yakmo *, int32_t *point_to_cluster);
TM_API void yakmo_get_centroids(tm_yakmo *, double **centroids);

/* BICO.dll (extern.pas:218-223): the "coreset" is the build's weighted k-means with `coresetsize` centres. */
typedef struct tm_bico tm_bico;
TM_API tm_bico *bico_create(int64_t dimension, int64_t npoints, int64_t k, int64_t nrandproj, int64_t coresetsize, int random_seed);
TM_API void bico_destroy(tm_bico *);
TM_API void bico_set_num_threads(int num_threads);
TM_API void bico_set_rebuild_properties(tm_bico *, uint32_t interval, double initial, double grow);
TM_API void bico_insert_line(tm_bico *, const double *line, double weight);
TM_API int64_t bico_get_results(tm_bico *, double *centroids, double *weights);
/* dlquant_dll.dll (extern.pas:196; quantizer.h:20-21): HOST pointers as the import has them -- width x height RGB bytes in, the palette
 * planar into userpal[3][PALETTE_MAX = 65536]; returns 0 on success (1 on failure, message in tm_last_error).  = tm_stage_dl3quant
 * with an upload and a read-back around it. */
TM_API int dl3quant(unsigned char *inbuf, int width, int height, int quant_to, int lookup_bpc, unsigned char userpal[3][65536]);

#ifdef __cplusplus
}
#endif
#endif
