// tm_common.h -- shared host-side helpers of libtilemotion (error plumbing, device buffers, tables).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tilemotion.h"

namespace tmx {

void set_error(const char *fmt, ...);
const char *get_error();

#define TM_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      tmx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);        \
      return (e_ == hipErrorOutOfMemory) ? TM_E_NOMEM : TM_E_HIP;                                      \
    }                                                                                                  \
  } while (0)

#define TM_CHECK(cond, code, ...)        \
  do {                                   \
    if (!(cond)) {                       \
      tmx::set_error(__VA_ARGS__);        \
      return (code);                     \
    }                                    \
  } while (0)

#define TM_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != TM_OK) return rc_; \
  } while (0)

// Fails loudly when no gfx950 device can run the kernels (there is no CPU path).
int require_device();

// The library's environment switches (the table in include/tilemotion.h documents them).  They are sampled at the API boundary -- tm_create,
// tm_run, every tm_stage_* and fine-seam entry (knobs_reload, through require_device) -- into the calling thread's set; nothing inside a step
// calls getenv.
struct Knobs {
  bool knn_debug = false, knn_noprune = false, topk_brute = false, no_query_groups = false, dither_own_keys = false, dither_no_dedup = false,
       dither_literal = false, dedup_plain = false, dedup_sort = false, dedup_degrade_hash = false, dedup_full_order = false, motion_valu = false, pp_debug = false,
       comm_force_dist = false, features_plain = false, km_launches = false, kmodes_binwise = false, kmodes_fast_always = false, pp_sharded = false, window_dcts_by_tile = false, km_resident_fail = false, features_by_tile = false, motion_pack_separate = false, motion_force_flag = false;
  bool knn_first_chunk = true;  // TM_KNN_FIRST_CHUNK=0: the scan runs every listed block's whole chain (A/B runs, tests)
  bool knn_list_order = true;  // TM_KNN_LIST_ORDER=0: the scan's tile lists stay in run order and are consumed to their ends (A/B runs, tests)
  int knn_curve = -1;  // TM_KNN_CURVE=morton|hilbert: the order both sides of every KNN search are sorted in (CURVE_MORTON 0, CURVE_HILBERT 1, tm_knn_kernel.h; A/B runs, tests);
                       // -1, not set: Hilbert, and Morton for the sample index of the k-nearest search's estimate (knn_index_search_topk)
  bool km_first_look = true;  // TM_KM_FIRST_LOOK=0: the plain iterations of the tile k-means score every point with the double-precision chain (A/B runs, tests)
  int topk_estimate = -1;  // TM_TOPK_ESTIMATE: the k-nearest search's first thresholds from a sample of the database: -1 by size, 0 never, 1 whenever possible
  double epu_table_gib = 6.0, comm_timeout_s = 120.0;
  long long knn_arena_entries = 0, dedup_radix_min = 1ll << 20;
  int input_chunk_frames = 0;  // TM_INPUT_CHUNK_FRAMES: frames per chunk of Load's read of a Y4M file or of a lent YUV or RGB clip (0: 16 MB worth; tests: 1, so that small clips take many chunks)
  int recon_chunk_frames = 0;  // TM_RECON_CHUNK_FRAMES: frames per chunk of Reconstruct's query features (0: 8 GiB worth, 2 GiB with the extended palette usage; tests: small, so that a clip takes several chunks)
  bool player_no_worker = false;  // TM_PLAYER_NO_WORKER: the player decodes the next key frame on the calling thread, when the last one has been played
  int player_chunk_frames = 0;    // TM_PLAYER_CHUNK_FRAMES: frames per chunk of the player's record upload (0: 8 MB worth, at most 16)
  int gif_decode = 0;  // TM_GIF_DECODE=host|device: the same for a GIF input and tm_set_gif_decode
  int jpeg_decode = 0; // TM_JPEG_DECODE=host|device: the same for a JPEG input and tm_set_jpeg_decode
  int png_decode = 0;  // TM_PNG_DECODE=host|device: where a PNG input is decoded, whatever tm_set_png_decode said (0: not set; else TM_PNG_DECODE_*)
  int group_fail_shard = -1;  // TM_GROUP_FAIL_SHARD: that shard of a device group fails at the start of its next step (tests)
};
const Knobs &knobs();
void knobs_reload();
void knobs_set(const Knobs &k);  // a device group's worker thread takes the set its caller sampled

// Device memory pool: hipMalloc / hipFree of the pipeline's multi-GB temporaries cost ~16 ms per 720p clip (and hipFree
// synchronises the device), so freed blocks are kept per host thread and handed out again.  A thread drives its encoder on
// one stream, so reuse is stream-ordered; blocks never migrate between threads.  pool_trim() returns everything to the
// driver (called when an encoder is destroyed, and automatically when an allocation fails).
int pool_alloc(void **p, size_t *bytes_inout);
void pool_free(void *p, size_t bytes);
void pool_trim();

// RAII device buffer
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) pool_free(p, bytes);
    p = nullptr;
    bytes = 0;
  }
  int alloc(size_t n) {
    if (n <= bytes && p) return TM_OK;
    release();
    if (n == 0) n = 16;
    size_t got = n;
    const int rc = pool_alloc(&p, &got);
    if (rc != TM_OK) { p = nullptr; return rc; }
    bytes = got;
    return TM_OK;
  }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// rocPRIM's device primitives are called twice with one argument list: with a null temporary they only report its size, with the temporary
// they run.  `call` is (void *tmp, size_t &bytes) -> hipError_t and holds that argument list once; `tmp` grows to the size asked for and stays
// the caller's (later users are ordered behind the primitive on the same stream); `what` names the primitive in the error text.
template <class Call>
inline int with_temp(DevBuf &tmp, const char *what, Call &&call) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e == hipSuccess) {
    const int rc = tmp.alloc(bytes);
    if (rc != TM_OK) return rc;
    e = call(tmp.p, bytes);
  }
  if (e == hipSuccess) return TM_OK;
  set_error("%s failed: %s", what, hipGetErrorString(e));
  return (e == hipErrorOutOfMemory) ? TM_E_NOMEM : TM_E_HIP;
}

// A wait of the host for a stream that is counted (host_waits, exported as tm_host_waits): HostRead::wait, and the plain stream
// synchronisations of PreparePalettes and the dedup (tm_steps, tm_palettize, tm_kmeans*, tm_dedup), so that a test can hold the number of
// round trips of a step.  The count is the process's, over all threads.
hipError_t host_sync(hipStream_t s);
long long host_waits();

// Small read-backs (counts, flags, a handful of sums) through page-locked memory: a device-to-host copy into pageable memory -- a stack
// variable -- takes the runtime's staging path and costs 27 us behind a small kernel where the same copy into pinned memory costs 15
// (tools/micro/readback.hip; a step holds 50-100 of them).  Scoped: the destinations must outlive the object; copies queued and not
// waited for are dropped.  The staging area is the calling thread's (64 KB; larger copies go straight to their destination).
struct HostRead {
  explicit HostRead(hipStream_t s);
  ~HostRead();
  HostRead(const HostRead &) = delete;
  HostRead &operator=(const HostRead &) = delete;
  int get(void *dst, const void *src, size_t bytes);  // queue
  int wait();                                         // synchronise the stream, then fill the destinations
 private:
  struct Item { void *dst; size_t off, bytes; };
  hipStream_t stream;
  Item items[8];
  int n = 0;
};

// sixteen page-locked 32-bit words of the calling thread (nullptr if none are to be had): for flags a host loop polls behind events
// without draining the stream
int *pinned_words();

// Constant tables of the reference (utils.pas:47-109) + LUTs of InitLuts (tilingencoder.pas:1683-1727),
// uploaded once per device.
struct DeviceTables {
  float *dct_lut_f32[2] = {nullptr, nullptr};   // FDCTLut[special][4096]
  double *dct_lut_f64[2] = {nullptr, nullptr};  // FDCTLutDouble
  double *dct_cos_f64[2] = {nullptr, nullptr};  // the LUT's two cosine factors, cos((x + 0.5) u pi / div) as [u][x] (the int16 feature kernel's fast path)
  double *weights = nullptr;                    // cDCTWeights [3][8][8]
  float *srgb_lut = nullptr;                    // inverse sRGB of c/255, as Single
  uint8_t *snake = nullptr;                     // cDCTSnake
  uint8_t *dither_map = nullptr;                // cDitheringMap
};
int get_tables(const DeviceTables **out);

extern const uint8_t kDitheringMap[64];
extern const uint8_t kDCTSnake[64];
extern const double kDCTWeights[3][8][8];

inline bool mode_special(int mode) { return mode == TM_PVS_SPE_DCT || mode == TM_PVS_WEIGHTED_SPE_DCT; }
inline bool mode_weighted(int mode) { return mode == TM_PVS_WEIGHTED_DCT || mode == TM_PVS_WEIGHTED_SPE_DCT; }

// workgroups of 256 for a grid-stride loop over n items: one per 256 items, at most 4096
inline int gridn(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16)); }
// the load and feature kernels' grids: one workgroup per per_block items (what its waves take in one pass of their loop), at most 2048
inline int grid_for(int64_t work_items, int per_block) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((work_items + per_block - 1) / per_block, 256 * 8));
}

}  // namespace tmx
