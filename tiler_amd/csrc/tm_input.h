// tm_input.h -- what the input side's files share (tm_input.hip: Load's choice of a source and the API; tm_input_clip.hip: clips in memory and
// raw files; tm_input_files.hip: coded files; tm_input_probe.hip: what a name turns out to be; tm_yuv_in.hip: planes of Y, U, V into RGB32
// frames), and the two-buffer staging the player shares with them.  tm_encoder.h includes it.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

// ---- what the probe half of Load (tilingencoder.pas:1764-1820) finds out about InputFileName
constexpr int INPUT_YUV_CLIP = 3;  // InputInfo::kind of a YUV clip lent in memory (tm_set_frames_yuv), beside TM_INPUT_Y4M / TM_INPUT_PNGS
constexpr int INPUT_GTM = TM_INPUT_GTM;  // a .gtm stream: Load plays its frames into the device clip (tm_player.hip)
constexpr int INPUT_RGB_CLIP = 5;  // an RGB clip lent in memory (tm_set_frames_rgb)
constexpr int INPUT_PNG_CLIP = 6;  // PNG files lent in memory (tm_set_frames_png)
constexpr int INPUT_GIF_CLIP = 20;  // one GIF file lent in memory (tm_set_frames_gif), beside TM_INPUT_GIF
constexpr int INPUT_JPEG_CLIP = 12;  // JPEG files lent in memory (tm_set_frames_jpeg), beside TM_INPUT_JPEGS
// JFIF's 4:2:2: chroma between the luma pairs.  A layout of chroma_geom for the JPEG reader's planes only: no public TM_CHROMA_* value,
// and check_yuv_clip and the stage seams keep refusing it.
constexpr int CHROMA_422_CENTRED = 5;
struct InputInfo {
  int kind = 0;  // 0: RGB32 frames from memory (pushed or lent); TM_INPUT_Y4M / TM_INPUT_PNGS: from the file; INPUT_YUV_CLIP / INPUT_RGB_CLIP: a lent clip
  std::string name;
  tm_yuv_clip clip{};               // INPUT_YUV_CLIP: the descriptor as it was lent
  tm_rgb_clip rgb_clip{};           // INPUT_RGB_CLIP: the same
  std::vector<const void *> png_files;  // INPUT_PNG_CLIP, INPUT_JPEG_CLIP, INPUT_GIF_CLIP (one file): the files as they were lent
  std::vector<size_t> png_sizes;
  int jpeg_segments = 0;            // JPEG inputs: the restart segments of the first file (what AUTO decides by)
  bool lent = false;                // the clip's memory is still borrowed: no Load has read it yet
  int start = 0, frames = 0, src_w = 0, src_h = 0, dst_w = 0, dst_h = 0, chroma = 0, full_range = 0;
  double fps = 0;
  int64_t frame_bytes = 0;
  std::vector<int64_t> frame_off;   // Y4M: where every whole frame's planes start in the file
  std::vector<int32_t> manual_kf;   // PNGs: frame 0 and the frames a .kf file marks (3380-3384)
  bool decoded = false;             // the device clip holds frames [dec_first, +dec_count) converted with dec_mode
  int dec_first = 0, dec_count = 0, dec_mode = 0;
};
// tm_input_probe.hip (host only)
int probe_input(const std::string &name, int start_frame, int frame_count, double scaling, InputInfo *in);
int format_pattern(const std::string &pat, int64_t i, std::string *out);  // Pascal's Format(pattern, [i])
int read_whole(const std::string &name, std::vector<uint8_t> *out);         // a file's bytes
int scaled_size(int w, int h, double scaling, int *dst_w, int *dst_h);    // Round(W * Scaling) x Round(H * Scaling); refuses an eightfold shrink

// ---- files and staging
struct FdCloser { int fd; ~FdCloser() { if (fd >= 0) close(fd); } };
inline int pread_all(int fd, void *dst, size_t n, int64_t at) {  // exactly n bytes from offset `at`: 0, or -1
  for (size_t got = 0; got < n;) {
    const ssize_t r = pread(fd, (uint8_t *)dst + got, n - got, (off_t)(at + (int64_t)got));
    if (r <= 0) return -1;
    got += (size_t)r;
  }
  return 0;
}
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
// fn(i) for i in [0, n) on up to IN_READERS host threads (the calling one included); the first failure's code and message come back.
// Reading a file that the page cache holds is a copy the memory system bounds, not one core: a single reader brought the 0.41 GB of the
// 720p x 300 clip in at 8 GB/s (50 ms, against 20 ms for the whole Load of the same clip lent as RGB32).
constexpr int IN_READERS = 8;
inline int parallel_for(int n, const std::function<int(int)> &fn) {
  const int nt = std::min(IN_READERS, n);
  if (nt <= 1) {
    for (int i = 0; i < n; i++) TM_TRY(fn(i));
    return TM_OK;
  }
  std::atomic<int> next{0}, rc{TM_OK};
  std::string err;
  std::mutex mu;
  auto work = [&] {
    for (int i = next++; i < n && rc.load() == TM_OK; i = next++) {
      const int r = fn(i);
      if (r != TM_OK) {
        std::lock_guard<std::mutex> lk(mu);
        if (rc.load() == TM_OK) { rc = r; err = get_error(); }  // (the message is the failing thread's: it is handed to the caller's below)
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (std::thread &t : th) t.join();
  if (rc != TM_OK) set_error("%s", err.c_str());
  return rc;
}
struct PinnedBuf {  // page-locked host memory that only grows
  void *p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  int alloc(size_t n) {
    if (p && n <= bytes) return TM_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; bytes = 0;
    TM_HIP(hipHostMalloc(&p, n, hipHostMallocDefault));
    bytes = n;
    return TM_OK;
  }
};
// The order of a two-slot staging ring: chunk after chunk is put into a page-locked host buffer, uploaded into a device buffer on a copy
// stream and worked on on another, slot s = chunk & 1, so that a chunk's transfer runs beside the work on the one before.  The caller
// makes the four calls in this order around its own fill, copy and launches (convert_staged, tm_input_clip.hip; the file decoders of tm_input_files.hip; tm_player::queue_chunks).
struct StagingRing {
  hipEvent_t up[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  bool used[2] = {false, false};  // the slot has had an upload recorded
  StagingRing() = default;
  StagingRing(const StagingRing &) = delete;
  StagingRing &operator=(const StagingRing &) = delete;
  ~StagingRing() { for (hipEvent_t e : {up[0], up[1], done[0], done[1]}) if (e) (void)hipEventDestroy(e); }
  int make() {
    for (hipEvent_t *e : {&up[0], &up[1], &done[0], &done[1]}) TM_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return TM_OK;
  }
  // before the host buffer is filled: wait for the upload that last read it
  int host_free(int s) { if (used[s]) TM_HIP(hipEventSynchronize(up[s])); return TM_OK; }
  // before the upload is queued: the copy stream waits for the work that last read this device buffer
  int device_free(int s, hipStream_t copy) { if (used[s]) TM_HIP(hipStreamWaitEvent(copy, done[s], 0)); return TM_OK; }
  // behind the upload: record it, and the work stream waits for it
  int uploaded(int s, hipStream_t copy, hipStream_t work) {
    TM_HIP(hipEventRecord(up[s], copy));
    TM_HIP(hipStreamWaitEvent(work, up[s], 0));
    used[s] = true;
    return TM_OK;
  }
  // behind the work: record it
  int worked(int s, hipStream_t work) { TM_HIP(hipEventRecord(done[s], work)); return TM_OK; }
};

// ---- tm_yuv_in.hip: planes of Y, U, V into RGB32 frames
// where a layout's chroma samples sit: step and offset (in halves of a luma sample) per axis, plane size
struct ChromaGeom { int sx, sy, ox, oy, cw, ch; };
int chroma_geom(int chroma, int w, int h, ChromaGeom *g);
// how the samples of a clip's planes are stored (tm_yuv_clip): TM_SAMPLES_*, the depth, and whether U and V alternate in the plane `u`
struct SampleFmt {
  int samples = TM_SAMPLES_U8, depth = 8;
  bool pairs = false;
  int bytes() const { return samples == TM_SAMPLES_U8 ? 1 : 2; }
};
// the deep-sample rule (tm_yuv_clip) as the kernels take it: p_d = (word >> rshift) & mask;  p = min(255, (p_d + half) >> nshift), half = 2^(nshift - 1)
struct DeepRule { int rshift, mask, half, nshift; };
inline DeepRule deep_rule_of(const SampleFmt &fmt) {
  if (fmt.bytes() == 1) return DeepRule{0, 0xff, 0, 0};
  const int d = fmt.depth;
  return fmt.samples == TM_SAMPLES_U16_HIGH ? DeepRule{16 - d, 0xffff, 1 << (d - 9), d - 8} : DeepRule{0, (1 << d) - 1, 1 << (d - 9), d - 8};
}
__host__ __device__ __forceinline__ int narrow_word(int word, const DeepRule &d) {
  const int pd = (word >> d.rshift) & d.mask, p = (pd + d.half) >> d.nshift;
  return p < 255 ? p : 255;
}
// the checks of tm_set_frames_yuv and of the stage seam, with no device call; what they find out about the planes
struct ClipPlanes {
  SampleFmt fmt;
  ChromaGeom g{};
  int nplanes = 1;                      // 1 mono, 2 Y + pairs, 3 planar
  int64_t row_bytes[3] = {0, 0, 0};     // of Y, U (or the pairs), V
  int rows[3] = {0, 0, 0};
};
int check_yuv_clip(const tm_yuv_clip *c, ClipPlanes *out);
// the tables of one conversion, made once per (source size, layout, output size) and kept on the device (AxisTaps: tm_internal.h, with the rule's tables)
struct InputTables {
  int src_w = 0, src_h = 0, chroma = -1, dst_w = 0, dst_h = 0, th = 0;  // th: output rows per workgroup
  DevBuf dev;
  AxisTaps lh{}, lv{}, ch{}, cv{};  // luma / chroma, horizontal / vertical
};
int build_input_tables(int src_w, int src_h, int chroma, int dst_w, int dst_h, InputTables *t, hipStream_t stream);
// strides in bytes: row and frame of Y, of U (or the pairs), of V
int launch_yuv_to_rgb32(const InputTables &t, const void *y, const void *u, const void *v, const int64_t strides[6], const SampleFmt &fmt, int nframes, int yuv_mode,
                        void *out, hipStream_t stream);
inline int resolve_yuv_mode(int mode, int full_range) { return mode == TM_YUV_AUTO ? (full_range ? TM_YUV_BT601_FULL : TM_YUV_BT601_LIMITED) : mode; }

// ---- tm_rgb_in.hip: an RGB clip lent in memory (tm_rgb_clip) into RGB32 frames
// The checks of tm_set_frames_rgb and of the stage seam, with no device call, and what they find out.  A clip is "interleaved" when its three
// pointers lie within one step of the lowest and a row holds its last pixel whole: a pixel is then `span` bytes from the lowest pointer on,
// fetched once for the three channels, and the clip stages as one plane of pixel_row_bytes per row.  Otherwise each channel is read sample
// by sample, and each distinct pointer stages as a plane of sample_row_bytes per row.
struct RgbPlan {
  SampleFmt fmt;
  bool interleaved = false;
  const uint8_t *base = nullptr;   // the lowest of the three pointers
  int64_t off[3] = {0, 0, 0};      // interleaved: R, G, B from base, in bytes
  int span = 0;                    // interleaved: off's largest + bytes per sample
  int64_t sample_row_bytes = 0, pixel_row_bytes = 0;  // (width - 1) step + bytes, + off's largest
};
int check_rgb_clip(const tm_rgb_clip *c, RgbPlan *out);
// frames [0, nframes) of the clip as described (device pointers) into out [nframes][dst_h][dst_w]; tables: null at the source's size, else
// prepared for (width, height) -> (dst_w, dst_h), TM_SCALE_LANCZOS3, and uploaded
int launch_rgb_to_rgb32(const tm_rgb_clip &c, const RgbPlan &plan, const ScaleTables *tables, int nframes, int dst_w, int dst_h, void *out, hipStream_t stream);

}  // namespace tmx
