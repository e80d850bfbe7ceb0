// tm_player.hip -- the .gtm player: frames of an existing stream on the device, frame by frame, with no encoder behind it (tm_player_*,
// tm_stage_play_frame; the semantics are DESIGN.md section 16's "What is drawn", the design is section 19).
//
// The sequential form section 16 names: frames are walked in order, and a predicted item is ONE gather from the frame before (which the
// player has just drawn) instead of a chain followed back per pixel.  One plain kernel launch per frame, queued back to back.
//
// Host side, per key frame: the stream is read, decoded and walked into fixed-size records (load_keyframe, tm_player_parse.hip).  A worker
// thread does this for key frame k + 1 while key frame k plays (TM_PLAYER_NO_WORKER: on the calling thread, when k has been played).
// Records go to the device in chunks of frames through two page-locked buffers on a copy stream; a StagingRing (tm_input.h) orders the
// reuse of either, as in convert_staged (tm_input_clip.hip).  The kernel is tm_play_frame.hip's.
//
// Memory, none of it a function of the clip's length beyond the GTMk index (28 bytes per key frame):
//   host    the records of two key frames (playing + decoded ahead): frames_in_kf * tm_w * tm_h * 8 bytes + 64 per intra item;
//           two page-locked chunks of chunk_frames * tm_w * tm_h * 72 bytes (every item intra: the worst case)
//   device  the TileSet (64 bytes per tile), the palettes, two chunks as above, one kept frame (the last one delivered: the next call's
//           "previous frame"), and -- only for host destinations and seeks -- a ring of 2 * chunk_frames frames; with an output size
//           (tm_player_set_output) that ring always, the tables, and for host and YUV destinations a ring of 2 * chunk_frames scaled frames
// chunk_frames = 8 MB worth of worst-case records, at least 1, at most 16 (TM_PLAYER_CHUNK_FRAMES overrides).
//
// Refusals are decided on the host before any device call: tm_player_open touches the device only after the header, the index and the
// first key frame's stream have been accepted (tilemotion.h lists the codes).
#include <unistd.h>

#include <future>
#include <memory>

#include "tm_input.h"
#include "tm_player.h"

namespace tmx {
namespace {

// the calling thread's current device, put back when a player call returns: the player works on its own device and leaves the caller's as it was
struct DeviceScope {
  int before = -1;
  DeviceScope() { if (hipGetDevice(&before) != hipSuccess) before = -1; }
  ~DeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};

// a YUV destination of one read (tm_player_read_yuv): the plan check_yuv_out made of it
struct YuvSink { const tm_yuv_out *dst; YuvOutPlan plan; };

}  // namespace
}  // namespace tmx

using namespace tmx;

struct tm_player {
  std::string path;
  int fd = -1, device = 0;
  GtmIndex ix;
  StreamHead head;
  int per = 0, chunk = 1;
  int64_t fpx = 0;            // pixels of a frame
  int64_t tileset_tiles = 0;
  int pal_count = 0;
  bool no_worker = false, head_held = false;
  // playing
  KfRecords cur, ahead;
  int ahead_index = -1;       // the key frame `ahead` holds or is being decoded into (-1: none)
  std::future<int> ahead_job; // valid: a worker is decoding it
  int pos = 0;                // the frame the next read starts at
  size_t peak_records = 0;
  // device
  bool dev_ready = false;
  hipStream_t play = nullptr, copy = nullptr;
  DevBuf d_tiles, d_pal, d_chunk[2], d_kept, d_ring;
  DevBuf d_yuv;               // host YUV destinations: a ring of two packed chunks of planes
  // an output size (tm_player_set_output; 0, 0: the stream's own): frames are played into the ring and scaled a chunk at a time
  int out_w = 0, out_h = 0, out_filter = TM_SCALE_LANCZOS3;
  ScaleTables scale;
  DevBuf d_scaled;            // host and YUV destinations at an output size: a ring of two scaled chunks
  PinnedBuf h_chunk[2];
  StagingRing staging;
  unsigned chunk_no = 0;
  const uint32_t *prev = nullptr;  // the frame before `pos` (null: black)
  // timings
  double t_open = 0, ms_decode = 0, ms_parse = 0, ms_upload = 0, ms_wait = 0, ms_launch = 0, first_frame_ms = -1;

  ~tm_player() {
    if (ahead_job.valid()) ahead_job.wait();
    if (dev_ready) {
      DeviceScope scope;
      (void)hipSetDevice(device);
      if (play) { (void)hipStreamSynchronize(play); (void)hipStreamDestroy(play); }
      if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
      for (DevBuf *b : {&d_tiles, &d_pal, &d_chunk[0], &d_chunk[1], &d_kept, &d_ring, &d_yuv, &d_scaled, &scale.dev}) b->release();  // (here: the pool files a block under the current device)
    }
    if (fd >= 0) close(fd);
  }

  int kf_of(int frame) const {  // the key frame that holds `frame`
    return (int)(std::upper_bound(ix.kf.begin(), ix.kf.end(), frame, [](int f, const KfEntry &e) { return f < e.frame; }) - ix.kf.begin()) - 1;
  }
  // key frame k from the file into records (any thread, as load_keyframe says); the head is kept from the first key frame 0 on
  int load_kf(int k, KfRecords *out) {
    const int rc = load_keyframe(fd, path.c_str(), ix, k, &head, !head_held, out);
    if (k == 0 && rc == TM_OK) head_held = true;
    return rc;
  }
  void took(const KfRecords &r) { ms_decode += r.decode_ms; ms_parse += r.parse_ms; }
  void decode_ahead(int k) {
    ahead_index = -1;
    if (k >= (int)ix.kf.size()) return;
    ahead_index = k;
    if (!no_worker) ahead_job = std::async(std::launch::async, [this, k] { return load_kf(k, &ahead); });
  }
  void drop_ahead() {
    if (ahead_job.valid()) (void)ahead_job.get();
    ahead_index = -1;
  }
  // make key frame k the current one
  int enter_kf(int k) {
    if (cur.index != k) {
      if (ahead_index == k) {
        int rc;
        if (ahead_job.valid()) { const double t0 = now_ms(); rc = ahead_job.get(); ms_wait += now_ms() - t0; }
        else rc = load_kf(k, &ahead);
        if (rc != TM_OK) { set_error("%s", ahead.err.c_str()); ahead_index = -1; return rc; }
        peak_records = std::max(peak_records, cur.bytes() + ahead.bytes());  // (both are held at this moment)
        std::swap(cur, ahead);
      } else {
        drop_ahead();
        const int rc = load_kf(k, &cur);
        if (rc != TM_OK) { cur.index = -1; return rc; }
        peak_records = std::max(peak_records, cur.bytes());
      }
      took(cur);
    }
    if (ahead_index != k + 1) { drop_ahead(); decode_ahead(k + 1); }
    return TM_OK;
  }

  int init_device() {
    TM_TRY(require_device());
    DeviceScope scope;
    int n = 0;
    TM_HIP(hipGetDeviceCount(&n));
    TM_CHECK(device >= 0 && device < n, TM_E_INVAL, "device %d of %d", device, n);
    TM_HIP(hipSetDevice(device));
    TM_HIP(hipStreamCreateWithFlags(&play, hipStreamNonBlocking));
    TM_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    dev_ready = true;
    TM_TRY(staging.make());
    TM_TRY(d_tiles.alloc(head.tileset.size()));
    if (!head.tileset.empty()) TM_HIP(hipMemcpy(d_tiles.p, head.tileset.data(), head.tileset.size(), hipMemcpyHostToDevice));
    TM_TRY(d_pal.alloc(head.palettes.size() * 4));
    if (!head.palettes.empty()) TM_HIP(hipMemcpy(d_pal.p, head.palettes.data(), head.palettes.size() * 4, hipMemcpyHostToDevice));
    tileset_tiles = head.tileset_tiles(); pal_count = head.pal_count();
    std::vector<uint8_t>().swap(head.tileset);  // (the device holds them now)
    std::vector<int32_t>().swap(head.palettes);
    const size_t cb = (size_t)chunk * per * (sizeof(PlayRec) + 64);
    for (int i = 0; i < 2; i++) { TM_TRY(d_chunk[i].alloc(cb)); TM_TRY(h_chunk[i].alloc(cb)); }
    TM_TRY(d_kept.alloc((size_t)fpx * 4));
    return TM_OK;
  }

  // the next `count` frames into dev_out, or through the ring into host_out, or (both null) nowhere: a seek's catching up; with `yuv` the
  // frames are played into the ring and each is converted behind its launch, into the caller's device planes or a packed ring of planes
  // A key frame that cannot be read ends the call at the frame before it: those frames are delivered and counted in *got, the last of them
  // is kept, and the next call stands at the damaged key frame again.  After a device error nothing is known about the frames in flight:
  // the player forgets its place in the key frame and its previous frame, so that no later launch reads a pointer left over from this call.
  int play_frames(int count, uint32_t *dev_out, uint32_t *host_out, int *got, const YuvSink *yuv = nullptr) {
    DeviceScope scope;
    TM_HIP(hipSetDevice(device));
    int n_done = 0;
    bool between_chunks = true;  // false: queue_chunks stopped inside a chunk (a device call failed)
    const int rc = queue_chunks(count, dev_out, host_out, &n_done, &between_chunks, yuv);
    hipError_t e = hipSuccess;
    if (n_done > 0 && between_chunks) {  // the last frame stays with the player: the caller's buffer, or the ring, may be overwritten before the next call
      e = hipMemcpyAsync(d_kept.p, prev, (size_t)fpx * 4, hipMemcpyDeviceToDevice, play);
      if (e == hipSuccess) prev = d_kept.as<uint32_t>();
    }
    const hipError_t es = hipStreamSynchronize(play);  // also after a failure: what was queued still writes the caller's memory
    if (e == hipSuccess) e = es;
    if (e != hipSuccess || !between_chunks) { prev = nullptr; cur.index = -1; n_done = 0; }
    if (got) *got = n_done;
    TM_TRY(rc);
    TM_HIP(e);
    return TM_OK;
  }
  int queue_chunks(int count, uint32_t *dev_out, uint32_t *host_out, int *n_done_out, bool *between_chunks, const YuvSink *yuv) {
    const bool scaled = out_w > 0 && (dev_out || host_out || yuv);  // (a seek's catching up scales nothing)
    const int64_t opx = (int64_t)out_w * out_h;
    const bool ring = dev_out == nullptr || scaled;
    if (ring && count > 0) TM_TRY(d_ring.alloc((size_t)2 * chunk * fpx * 4));
    if (scaled && !dev_out && count > 0) TM_TRY(d_scaled.alloc((size_t)2 * chunk * opx * 4));
    const bool yuv_host = yuv && yuv->dst->memory == TM_MEM_HOST;
    const size_t yuv_chunk = yuv_host ? (size_t)yuv->plan.frame_bytes() * chunk : 0;
    if (yuv_host && count > 0) TM_TRY(d_yuv.alloc(2 * yuv_chunk));
    int &n_done = *n_done_out;
    while (n_done < count && pos < ix.frames) {
      if (cur.index < 0 || pos < cur.first || pos >= cur.first + cur.nframes) {
        TM_TRY(enter_kf(kf_of(pos)));
      }
      const int in_kf = pos - cur.first;
      const int n = std::min(std::min(chunk, count - n_done), cur.nframes - in_kf);
      const int b = (int)(chunk_no++ & 1);
      *between_chunks = false;
      double t0 = now_ms();
      const int64_t i0 = cur.intra_first[(size_t)in_kf], i1 = cur.intra_first[(size_t)(in_kf + n)];
      const size_t rb = (size_t)n * per * sizeof(PlayRec), ib = (size_t)(i1 - i0) * 64;
      TM_TRY(staging.host_free(b));
      memcpy(h_chunk[b].p, cur.recs.data() + (size_t)in_kf * per, rb);
      if (ib) memcpy((uint8_t *)h_chunk[b].p + rb, cur.intra.data() + (size_t)i0 * 64, ib);
      TM_TRY(staging.device_free(b, copy));
      TM_HIP(hipMemcpyAsync(d_chunk[b].p, h_chunk[b].p, rb + ib, hipMemcpyHostToDevice, copy));
      TM_TRY(staging.uploaded(b, copy, play));
      ms_upload += now_ms() - t0;
      t0 = now_ms();
      for (int i = 0; i < n; i++) {
        uint32_t *dst = ring ? d_ring.as<uint32_t>() + ((int64_t)b * chunk + i) * fpx : dev_out + (int64_t)(n_done + i) * fpx;
        const int64_t f0 = cur.intra_first[(size_t)(in_kf + i)], f1 = cur.intra_first[(size_t)(in_kf + i + 1)];
        TM_TRY(launch_play_frame(d_chunk[b].as<uint8_t>() + (size_t)i * per * sizeof(PlayRec), d_chunk[b].as<uint8_t>() + rb + (size_t)(f0 - i0) * 64, f1 - f0, d_tiles.p,
                                 tileset_tiles, d_pal.p, pal_count, head.pal_size, prev, dst, head.tm_w, head.tm_h, play));
        prev = dst;
        if (yuv && !scaled) {
          const YuvDst to = yuv_host ? yuv_dst_packed(yuv->plan, d_yuv.as<uint8_t>() + yuv_chunk * b, chunk, i) : yuv_dst_of(*yuv->dst, n_done + i);
          TM_TRY(launch_rgb32_to_yuv(yuv->plan, dst, head.tm_w * 8, 1, to, play));
        }
      }
      TM_TRY(staging.worked(b, play));
      if (scaled) {  // the chunk's frames in one launch, behind them: into the caller's device buffer, or into the scaled ring
        uint32_t *to = dev_out ? dev_out + (int64_t)n_done * opx : d_scaled.as<uint32_t>() + (int64_t)b * chunk * opx;
        TM_TRY(launch_scale_rgb32(scale, d_ring.as<uint32_t>() + (int64_t)b * chunk * fpx, head.tm_w * 8, fpx, n, to, out_w, opx, play));
        if (yuv) TM_TRY(launch_rgb32_to_yuv(yuv->plan, to, out_w, n, yuv_host ? yuv_dst_packed(yuv->plan, d_yuv.as<uint8_t>() + yuv_chunk * b, chunk, 0) : yuv_dst_of(*yuv->dst, n_done), play));
        if (host_out) TM_HIP(hipMemcpyAsync(host_out + (int64_t)n_done * opx, to, (size_t)n * opx * 4, hipMemcpyDeviceToHost, play));
      }
      if (yuv_host) TM_TRY(yuv_copy_out(yuv->plan, d_yuv.as<uint8_t>() + yuv_chunk * b, chunk, *yuv->dst, n_done, n, play));
      if (host_out && !scaled) TM_HIP(hipMemcpyAsync(host_out + (int64_t)n_done * fpx, d_ring.as<uint32_t>() + (int64_t)b * chunk * fpx, (size_t)n * fpx * 4, hipMemcpyDeviceToHost, play));
      ms_launch += now_ms() - t0;
      if (first_frame_ms < 0 && (dev_out || host_out || yuv)) {  // (once in a player's life: the wait is part of what is measured)
        TM_HIP(hipStreamSynchronize(play));
        first_frame_ms = now_ms() - t_open;
      }
      n_done += n; pos += n;
      *between_chunks = true;
    }
    return TM_OK;
  }

  // tm_player_set_output: the tables are made and uploaded before the setting changes, so that a refusal leaves it as it was
  int set_output(int width, int height, int filter) {
    if (width == 0 && height == 0) { out_w = out_h = 0; out_filter = TM_SCALE_LANCZOS3; return TM_OK; }
    ScaleTables next;
    TM_TRY(next.prepare(head.tm_w * 8, head.tm_h * 8, width, height, filter));
    DeviceScope scope;
    TM_HIP(hipSetDevice(device));
    const int rc = next.upload(play);
    if (rc == TM_OK) { std::swap(scale, next); out_w = width; out_h = height; out_filter = filter; }
    next.dev.release();  // (here: the pool files a block under the current device)
    return rc;
  }

  int seek(int frame) {
    TM_CHECK(frame >= 0 && frame <= ix.frames, TM_E_INVAL, "seek to frame %d of %d", frame, ix.frames);
    if (frame == ix.frames) { pos = frame; return TM_OK; }
    const bool forward = cur.index >= 0 && pos >= cur.first && pos <= cur.first + cur.nframes && frame >= pos && frame < cur.first + cur.nframes;
    if (!forward) {
      TM_TRY(enter_kf(kf_of(frame)));
      pos = cur.first;
      prev = nullptr;
    }
    if (frame > pos) TM_TRY(play_frames(frame - pos, nullptr, nullptr, nullptr));
    return TM_OK;
  }
};

extern "C" {

int tm_player_open(const char *path, int device, tm_player **out) {
  TM_CHECK(path && out, TM_E_INVAL, "null argument");
  *out = nullptr;
  knobs_reload();
  std::unique_ptr<tm_player> p(new tm_player());
  p->t_open = now_ms();
  p->path = path; p->device = device;
  p->no_worker = knobs().player_no_worker;
  TM_TRY(open_stream_head(path, &p->fd, &p->ix, &p->head, &p->cur));
  p->head_held = true;
  p->took(p->cur);
  p->peak_records = p->cur.bytes();
  p->per = p->head.tm_w * p->head.tm_h;
  p->fpx = (int64_t)p->per * 64;
  const size_t worst = (size_t)p->per * (sizeof(PlayRec) + 64);
  p->chunk = knobs().player_chunk_frames > 0 ? std::min(knobs().player_chunk_frames, 16) : (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)8 << 20) / worst));
  TM_TRY(p->init_device());  // (every refusal above was decided without a device call)
  TM_TRY(p->enter_kf(0));    // starts the worker on key frame 1
  *out = p.release();
  return TM_OK;
}

void tm_player_close(tm_player *p) { delete p; }

int tm_player_info(tm_player *p, tm_gtm_info *info) {
  TM_CHECK(p && info, TM_E_INVAL, "null argument");
  fill_info(p->ix, p->head, p->tileset_tiles, p->pal_count, info);
  info->host_bytes = (int64_t)(p->h_chunk[0].bytes + p->h_chunk[1].bytes + p->peak_records + p->ix.kf.size() * sizeof(KfEntry));
  info->device_bytes = (int64_t)(p->d_tiles.bytes + p->d_pal.bytes + p->d_chunk[0].bytes + p->d_chunk[1].bytes + p->d_kept.bytes + p->d_ring.bytes + p->d_yuv.bytes +
                                   p->d_scaled.bytes + p->scale.dev.bytes);
  return TM_OK;
}

int tm_player_keyframes(tm_player *p, int32_t *start_frames) {
  TM_CHECK(p && start_frames, TM_E_INVAL, "null argument");
  for (size_t k = 0; k < p->ix.kf.size(); k++) start_frames[k] = p->ix.kf[k].frame;
  return TM_OK;
}

int tm_player_settings_text(tm_player *p, char *buf, size_t cap, size_t *n) {
  TM_CHECK(p && n, TM_E_INVAL, "null argument");
  *n = p->head.settings.size();
  if (!buf) return TM_OK;
  TM_CHECK(cap >= *n, TM_E_INVAL, "settings text: %zu bytes needed, %zu given", *n, cap);
  memcpy(buf, p->head.settings.data(), *n);
  return TM_OK;
}

int tm_player_read(tm_player *p, int count, void *out, int out_on_device, int *got) {
  TM_CHECK(p && got && (out || count == 0), TM_E_INVAL, "null argument");
  *got = 0;
  TM_CHECK(count >= 0, TM_E_INVAL, "read of %d frames", count);
  TM_CHECK(((uintptr_t)out & 15) == 0 || !out_on_device, TM_E_INVAL, "the device destination must be 16-byte aligned");
  if (count == 0) return TM_OK;
  return out_on_device ? p->play_frames(count, (uint32_t *)out, nullptr, got) : p->play_frames(count, nullptr, (uint32_t *)out, got);
}

int tm_player_read_yuv(tm_player *p, int count, const tm_yuv_out *dst, int mode, int *got) {
  TM_CHECK(p && got, TM_E_INVAL, "null argument");
  *got = 0;
  TM_CHECK(count >= 0, TM_E_INVAL, "read of %d frames", count);
  YuvSink sink{dst, YuvOutPlan()};
  TM_TRY(check_yuv_out(dst, p->out_w > 0 ? p->out_w : p->head.tm_w * 8, p->out_w > 0 ? p->out_h : p->head.tm_h * 8, mode, &sink.plan));
  const int deliver = std::min(count, p->ix.frames - p->pos);  // (as tm_player_read: what is left of the stream is what a call delivers)
  TM_CHECK(deliver <= dst->frames, TM_E_INVAL, "yuv out: %d frames to deliver, room for %d", deliver, dst->frames);
  if (dst->memory == TM_MEM_DEVICE) {
    DeviceScope scope;
    TM_TRY(yuv_out_is_device(*dst, p->device));
  }
  if (count == 0) return TM_OK;
  return p->play_frames(count, nullptr, nullptr, got, &sink);
}

int tm_player_set_output(tm_player *p, int width, int height, int filter) {
  TM_CHECK(p, TM_E_INVAL, "null argument");
  return p->set_output(width, height, filter);
}

int tm_player_get_output(tm_player *p, int *width, int *height, int *filter) {
  TM_CHECK(p, TM_E_INVAL, "null argument");
  if (width) *width = p->out_w;
  if (height) *height = p->out_h;
  if (filter) *filter = p->out_filter;
  return TM_OK;
}

int tm_player_seek(tm_player *p, int frame) {
  TM_CHECK(p, TM_E_INVAL, "null argument");
  return p->seek(frame);
}

int tm_player_tell(tm_player *p) { return p ? p->pos : TM_E_INVAL; }

int tm_player_timings(tm_player *p, double ms[5], double *first_frame_ms) {
  TM_CHECK(p, TM_E_INVAL, "null argument");
  if (ms) { ms[0] = p->ms_decode; ms[1] = p->ms_parse; ms[2] = p->ms_upload; ms[3] = p->ms_wait; ms[4] = p->ms_launch; }
  if (first_frame_ms) *first_frame_ms = p->first_frame_ms;
  return TM_OK;
}


}  // extern "C"
