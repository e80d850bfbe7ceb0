// tm_player.hip -- the .gtm player: frames of an existing stream on the device, frame by frame, with no encoder behind it (tm_player_*,
// tm_stage_play_frame; the semantics are DESIGN.md section 16's "What is drawn", the design is section 19).
//
// The sequential form section 16 names: frames are walked in order, and a predicted item is ONE gather from the frame before (which the
// player has just drawn) instead of a chain followed back per pixel.  One plain kernel launch per frame, queued back to back.
//
// Host side, per key frame: the compressed stream is read from the file at its GTMk offset, decoded (lz_decompress), and walked
// (walk_gtm_keyframe, tm_gtm_walk.h: the grammar tm_reload_gtm reads by) into fixed-size records -- 8 bytes per tile-map item, and the
// 64 index bytes of every intra item, which travel with the frame that draws them, so no table of intra slots exists.  A worker thread does
// this for key frame k + 1 while key frame k plays (TM_PLAYER_NO_WORKER: on the calling thread, when k has been played).  Records go to the
// device in chunks of frames through two page-locked buffers on a copy stream; events order the reuse of either (the scheme of
// convert_staged, tm_input.hip).
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
#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <future>
#include <memory>

#include "tm_common.h"
#include "tm_device.h"
#include "tm_gtm_walk.h"
#include "tm_internal.h"

namespace tmx {
namespace {

// ---- the record of one tile-map item (tilemotion.h, tm_player_parse_host, describes it for callers)
struct PlayRec {
  uint32_t a;      // tile index | intra: index among the frame's intra tiles | predicted: (uint8) x | (uint8) y << 8
  uint16_t pal;
  uint8_t flags;   // bit 0 H mirror, bit 1 V mirror, bit 2 predicted, bit 3 intra
  uint8_t zero;
};
static_assert(sizeof(PlayRec) == 8, "record layout");
constexpr uint8_t REC_PRED = 4, REC_INTRA = 8;

// ---- the kernel: one frame.  A workgroup of 256 owns 16 consecutive items; an item is 64 pixels = 16 lanes x one 16-byte store.  Lanes are
// laid out row-major over the 16 items' common picture rows (8 rows x 32 lanes), so that the 32 lanes of a row store 512 contiguous bytes
// where the items lie in one tile row.  No LDS: a drawn lane reads 4 index bytes (one word) and 4 palette entries (the palettes stay in
// L2), a predicted lane gathers 4 pixels of the previous frame, each clamped on its own.
__global__ __launch_bounds__(256) void k_play_frame(const uint2 *__restrict__ recs, const uint8_t *__restrict__ intra, int64_t nintra,
                                                    const uint8_t *__restrict__ tiles, int64_t ntiles, const int32_t *__restrict__ palettes, int npal,
                                                    int pal_size, const uint32_t *prev, uint32_t *out, int tm_w, int tm_h) {
  const int t = threadIdx.x, row = t >> 5, half = t & 1;
  const int i = blockIdx.x * 16 + ((t & 31) >> 1);
  if (i >= tm_w * tm_h) return;
  const uint2 r = recs[i];
  const uint32_t a = r.x, pal = r.y & 0xffffu, fl = (r.y >> 16) & 0xffu;
  const int iy = i / tm_w, ix = i - iy * tm_w;
  const int W = tm_w * 8, H = tm_h * 8;
  const int y = iy * 8 + row, x = ix * 8 + half * 4;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (fl & REC_PRED) {
    if (prev) {  // (before frame 0 the picture is 0)
      const int ox = (int8_t)(a & 0xff), oy = (int8_t)((a >> 8) & 0xff);
      const uint32_t *src = prev + (int64_t)min(max(y + oy, 0), H - 1) * W;
      const int sx = x + ox;
      v.x = src[min(max(sx, 0), W - 1)];
      v.y = src[min(max(sx + 1, 0), W - 1)];
      v.z = src[min(max(sx + 2, 0), W - 1)];
      v.w = src[min(max(sx + 3, 0), W - 1)];
    }
  } else {
    const uint8_t *px = nullptr;
    if (fl & REC_INTRA) { if ((int64_t)a < nintra) px = intra + (int64_t)a * 64; }
    else if ((int64_t)a < ntiles) px = tiles + (int64_t)a * 64;
    if (px != nullptr && (int)pal < npal) {
      const int ty = (fl & 2) ? 7 - row : row, tx = (fl & 1) ? 4 - half * 4 : half * 4;  // DrawTile, tilingencoder.pas:3457-3503
      uint32_t w = *reinterpret_cast<const uint32_t *>(px + ty * 8 + tx);
      if (fl & 1) w = __builtin_bswap32(w);
      const int32_t *p = palettes + (int64_t)pal * pal_size;
      const int c0 = w & 0xff, c1 = (w >> 8) & 0xff, c2 = (w >> 16) & 0xff, c3 = w >> 24;
      v.x = c0 < pal_size ? swap_rb((uint32_t)p[c0]) : 0u;
      v.y = c1 < pal_size ? swap_rb((uint32_t)p[c1]) : 0u;
      v.z = c2 < pal_size ? swap_rb((uint32_t)p[c2]) : 0u;
      v.w = c3 < pal_size ? swap_rb((uint32_t)p[c3]) : 0u;
    }
  }
  *reinterpret_cast<uint4 *>(out + (int64_t)y * W + x) = v;
}

int launch_play_frame(const void *recs, const void *intra, int64_t nintra, const void *tiles, int64_t ntiles, const void *palettes, int npal, int pal_size,
                      const void *prev, void *out, int tm_w, int tm_h, hipStream_t stream) {
  const int per = tm_w * tm_h;
  hipLaunchKernelGGL(k_play_frame, dim3((unsigned)((per + 15) / 16)), dim3(256), 0, stream, (const uint2 *)recs, (const uint8_t *)intra, nintra,
                     (const uint8_t *)tiles, ntiles, (const int32_t *)palettes, npal, pal_size, (const uint32_t *)prev, (uint32_t *)out, tm_w, tm_h);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- header and index ------------------------------------------------------------------------------------------------------------------
struct KfEntry { int32_t frame; uint32_t raw, comp, ms; int64_t offset; };
static_assert(sizeof(KfEntry) == 24, "the index in memory: 24 bytes per key frame (tm_player_info's host_bytes counts it)");
struct GtmIndex {
  int32_t width = 0, height = 0, frames = 0, version = 0;
  uint32_t avg = 0, kf_max = 0;
  std::vector<KfEntry> kf;
};
uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int pread_all(int fd, void *dst, size_t n, int64_t at) {
  for (size_t got = 0; got < n;) {
    const ssize_t r = pread(fd, (uint8_t *)dst + got, n - got, (off_t)(at + (int64_t)got));
    if (r <= 0) return -1;
    got += (size_t)r;
  }
  return 0;
}

// GTMv (40 bytes) + GTMk x key frames (28 each), tilingencoder.pas:30-51; every stream must lie inside the file
int read_index(int fd, const char *path, GtmIndex *ix) {
  const int64_t fsize = lseek(fd, 0, SEEK_END);
  uint8_t h[40];
  TM_CHECK(fsize >= 4 && pread_all(fd, h, 4, 0) == 0, TM_E_IO, "%s: too short to be a .gtm file", path);
  if (memcmp(h, "GTMv", 4) != 0) {
    set_error("%s has no GTMv header: a headerless stream has no index, so no seek and no frame count (tm_reload_gtm reads those)", path);
    return TM_E_UNSUPPORTED;
  }
  TM_CHECK(fsize >= 40 && pread_all(fd, h, 40, 0) == 0, TM_E_IO, "%s: truncated GTMv header", path);
  const uint32_t riff = rd32(h + 4), whole = rd32(h + 8), nkf = rd32(h + 24), frames = rd32(h + 28);
  ix->version = (int32_t)rd32(h + 12); ix->width = (int32_t)rd32(h + 16); ix->height = (int32_t)rd32(h + 20);
  ix->avg = rd32(h + 32); ix->kf_max = rd32(h + 36);
  TM_CHECK(riff == 32 && nkf >= 1 && nkf <= (1u << 24) && (uint64_t)whole == 40 + 28 * (uint64_t)nkf && (int64_t)whole <= fsize, TM_E_IO,
           "%s: damaged GTMv header (%u key frames, header of %u bytes, file of %lld)", path, nkf, whole, (long long)fsize);
  TM_CHECK(frames >= nkf && frames <= 0x7fffffffu && ix->width > 0 && ix->height > 0 && ix->width <= 65536 * 8 && ix->height <= 65536 * 8, TM_E_IO,
           "%s: damaged GTMv header (%u frames in %u key frames, %d x %d)", path, frames, nkf, ix->width, ix->height);
  ix->frames = (int32_t)frames;
  std::vector<uint8_t> raw((size_t)nkf * 28);
  TM_CHECK(pread_all(fd, raw.data(), raw.size(), 40) == 0, TM_E_IO, "%s: truncated GTMk index", path);
  ix->kf.resize(nkf);
  int64_t off = whole;
  for (uint32_t k = 0; k < nkf; k++) {
    const uint8_t *e = raw.data() + (size_t)k * 28;
    KfEntry &d = ix->kf[k];
    d.frame = (int32_t)rd32(e + 12); d.raw = rd32(e + 16); d.comp = rd32(e + 20); d.ms = rd32(e + 24); d.offset = off;
    TM_CHECK(memcmp(e, "GTMk", 4) == 0 && rd32(e + 4) == 20 && rd32(e + 8) == k, TM_E_IO, "%s: damaged GTMk entry %u", path, k);
    TM_CHECK(k == 0 ? d.frame == 0 : (d.frame > ix->kf[k - 1].frame && (uint32_t)d.frame < frames), TM_E_IO, "%s: GTMk entry %u starts at frame %d", path, k, d.frame);
    TM_CHECK(d.comp >= 18 && off + (int64_t)d.comp <= fsize, TM_E_IO, "%s: key frame %u (%u bytes at %lld) runs past the file's %lld bytes", path, k, d.comp,
             (long long)off, (long long)fsize);
    off += d.comp;
  }
  return TM_OK;
}

// ---- the command stream into records ---------------------------------------------------------------------------------------------------
constexpr int64_t MAX_ITEMS = (int64_t)1 << 24;  // items of a frame the player takes: a gigapixel picture, 128 MB of records a frame; beyond it a SetDimensions is damage
struct StreamHead {  // what the first key frame says about the whole stream
  int want_w = 0, want_h = 0;  // the GTMv header's picture size, which SetDimensions must match (0: no header at hand, tm_player_parse_host)
  bool have_dims = false;
  int tm_w = 0, tm_h = 0, pal_size = 0;
  uint32_t frame_ns = 0;
  int64_t tile_count = 0;
  std::string settings;
  std::vector<uint8_t> tileset;    // [tileset_tiles][64]: tiles drawn by index
  std::vector<int32_t> palettes;   // [pal_count][pal_size] 0x00BBGGRR
  int64_t tileset_tiles() const { return (int64_t)(tileset.size() / 64); }
  int pal_count() const { return pal_size > 0 ? (int)(palettes.size() / (size_t)pal_size) : 0; }
};
struct KfRecords {
  int index = -1, first = 0, nframes = 0;
  std::vector<PlayRec> recs;           // [nframes][tm_w * tm_h]
  std::vector<uint8_t> intra;          // the frames' intra tiles, 64 bytes each, in item order
  std::vector<int64_t> intra_first;    // [nframes + 1]
  double decode_ms = 0, parse_ms = 0;
  std::string err;
  size_t bytes() const { return recs.size() * sizeof(PlayRec) + intra.size() + intra_first.size() * sizeof(int64_t); }
};
struct RecordSink {
  StreamHead *head;
  bool takes_head;  // the first key frame: SetDimensions, TileSet, LoadPalette and the settings text are taken; later ones must not bring any
  bool keeps_head;  // ... and kept (false: the first key frame read again after a seek -- the player holds them already)
  int max_frames;   // the frames the index gives this key frame: more is a damaged stream, not a reason to grow
  KfRecords *kf;
  int tm_pos = 0;
  bool frame_open = false;

  int per() const { return head->tm_w * head->tm_h; }
  int place(PlayRec r, const char *what) {
    TM_CHECK(head->have_dims && tm_pos < per(), TM_E_IO, "%s past the tile map", what);
    if (!frame_open) {
      TM_CHECK(kf->nframes < max_frames, TM_E_IO, "more frames in the key frame than the %d its index entry gives it", max_frames);
      kf->recs.resize(kf->recs.size() + (size_t)per());
      if (kf->intra_first.empty()) kf->intra_first.push_back(0);
      frame_open = true;
    }
    kf->recs[kf->recs.size() - (size_t)per() + tm_pos] = r;
    tm_pos++;
    return TM_OK;
  }
  int settings(uint32_t kind, const uint8_t *text, size_t n) {
    if (!(takes_head && keeps_head && kind == 0)) return TM_OK;
    head->settings.assign((const char *)text, n);
    if (head->pal_size == 0) head->pal_size = settings_palette_size(text, n);  // (until a TileSet says it: a stream of intra and predicted items has none)
    return TM_OK;
  }
  int dimensions(int tm_w, int tm_h, uint32_t ns, uint32_t tc) {
    if (head->have_dims) {
      TM_CHECK(tm_w == head->tm_w && tm_h == head->tm_h && (int64_t)tc == head->tile_count, TM_E_IO, "SetDimensions changes the stream's %d x %d, %lld tiles",
               head->tm_w, head->tm_h, (long long)head->tile_count);
      return TM_OK;
    }
    TM_CHECK(takes_head, TM_E_IO, "SetDimensions outside the first key frame");
    TM_CHECK(head->want_w == 0 || ((int64_t)tm_w * 8 == head->want_w && (int64_t)tm_h * 8 == head->want_h), TM_E_IO,
             "SetDimensions' %d x %d tiles are not the GTMv header's %d x %d pixels", tm_w, tm_h, head->want_w, head->want_h);
    TM_CHECK((int64_t)tm_w * tm_h <= MAX_ITEMS, TM_E_IO, "SetDimensions' %d x %d tiles: more than %lld items a frame", tm_w, tm_h, (long long)MAX_ITEMS);
    head->tm_w = tm_w; head->tm_h = tm_h; head->frame_ns = ns; head->tile_count = tc; head->have_dims = true;
    return TM_OK;
  }
  int pal_size() const { return head->pal_size; }
  int tile_set(int pal_size, uint32_t a, uint32_t b, const uint8_t *px) {
    if (!takes_head) { set_error("a TileSet outside the first key frame is not played (tm_reload_gtm reads such streams)"); return TM_E_UNSUPPORTED; }
    if (!keeps_head) return TM_OK;
    TM_CHECK(head->have_dims && (int64_t)b < head->tile_count, TM_E_IO, "tile set [%u, %u] beyond the declared tile count %lld", a, b, (long long)head->tile_count);
    if ((int64_t)a > head->tileset_tiles()) { set_error("a TileSet that leaves a gap (starts at %u after %lld tiles) is not played", a, (long long)head->tileset_tiles()); return TM_E_UNSUPPORTED; }
    if (head->tileset.size() < ((size_t)b + 1) * 64) head->tileset.resize(((size_t)b + 1) * 64);
    memcpy(&head->tileset[(size_t)a * 64], px, ((size_t)b - a + 1) * 64);
    head->pal_size = pal_size;
    return TM_OK;
  }
  int load_palette(uint32_t pi, const uint8_t *c) {
    if (!takes_head) { set_error("a LoadPalette outside the first key frame is not played (tm_reload_gtm reads such streams)"); return TM_E_UNSUPPORTED; }
    if (!keeps_head) return TM_OK;
    const size_t ps = (size_t)head->pal_size;
    if ((size_t)pi > (size_t)head->pal_count()) { set_error("a LoadPalette that leaves a gap (palette %u after %d) is not played", pi, head->pal_count()); return TM_E_UNSUPPORTED; }
    if (head->palettes.size() < ((size_t)pi + 1) * ps) head->palettes.resize(((size_t)pi + 1) * ps, 0);
    for (size_t k = 0; k < ps; k++, c += 4) head->palettes[(size_t)pi * ps + k] = (int32_t)(rd32(c) & 0xffffffu);  // alpha stripped (4951)
    return TM_OK;
  }
  int frame_end(bool) {
    TM_CHECK(head->have_dims && tm_pos == per(), TM_E_IO, "incomplete tile map at FrameEnd (%d of %d items)", tm_pos, head->have_dims ? per() : 0);
    tm_pos = 0;
    frame_open = false;
    kf->nframes++;
    kf->intra_first.push_back((int64_t)(kf->intra.size() / 64));
    return TM_OK;
  }
  int skip(uint32_t count) {
    for (uint32_t k = 0; k < count; k++) TM_TRY(place(PlayRec{0, 0, REC_PRED, 0}, "SkipBlock"));
    return TM_OK;
  }
  int predicted(int ox, int oy) { return place(PlayRec{(uint32_t)(uint8_t)ox | ((uint32_t)(uint8_t)oy << 8), 0, REC_PRED, 0}, "a predicted item"); }
  int drawn(uint32_t tile, uint32_t pal, uint32_t mirror) { return place(PlayRec{tile, (uint16_t)pal, (uint8_t)mirror, 0}, "a tile-map item"); }
  int intra(uint32_t pal, uint32_t mirror, const uint8_t *px) {
    const int64_t in_frame = (int64_t)(kf->intra.size() / 64) - (kf->intra_first.empty() ? 0 : kf->intra_first.back());
    TM_TRY(place(PlayRec{(uint32_t)in_frame, (uint16_t)pal, (uint8_t)(mirror | REC_INTRA), 0}, "an intra item"));
    kf->intra.insert(kf->intra.end(), px, px + 64);
    return TM_OK;
  }
};

int parse_keyframe(const uint8_t *raw, size_t n, const char *name, StreamHead *head, bool takes_head, bool keeps_head, int max_frames, KfRecords *kf) {
  kf->recs.clear(); kf->intra.clear(); kf->intra_first.clear();
  kf->nframes = 0;
  RecordSink sink{head, takes_head, keeps_head, max_frames, kf};
  TM_TRY(walk_gtm_keyframe(raw, n, name, sink));
  if (kf->intra_first.empty()) kf->intra_first.push_back(0);
  return TM_OK;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the calling thread's current device, put back when a player call returns: the player works on its own device and leaves the caller's as it was
struct DeviceScope {
  int before = -1;
  DeviceScope() { if (hipGetDevice(&before) != hipSuccess) before = -1; }
  ~DeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};

// a YUV destination of one read (tm_player_read_yuv): the plan check_yuv_out made of it
struct YuvSink { const tm_yuv_out *dst; YuvOutPlan plan; };

struct Events2 {
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~Events2() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  int make() { for (hipEvent_t &e : ev) TM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return TM_OK; }
};

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
  Events2 up, done;
  bool used[2] = {false, false};
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

  int kf_frames(int k) const { return (k + 1 < (int)ix.kf.size() ? ix.kf[(size_t)k + 1].frame : ix.frames) - ix.kf[(size_t)k].frame; }

  // key frame k from the file into records (any thread: reads only the index and, for k > 0, the head's dimensions)
  int load_kf(int k, KfRecords *out) {
    const KfEntry &e = ix.kf[(size_t)k];
    std::vector<uint8_t> comp(e.comp), raw;
    int rc = TM_OK;
    auto fail = [&](int code) { out->err = get_error(); return code; };
    if (pread_all(fd, comp.data(), comp.size(), e.offset) != 0) { set_error("%s: cannot read key frame %d", path.c_str(), k); return fail(TM_E_IO); }
    double t0 = now_ms();
    size_t used_bytes = 0;
    rc = lz_decompress(comp.data(), comp.size(), raw, &used_bytes, (size_t)e.raw + 1);  // (one more than the index says: enough to see that it is wrong)
    if (rc != TM_OK) { set_error("%s: key frame %d: %s", path.c_str(), k, std::string(get_error()).c_str()); return fail(TM_E_IO); }
    out->decode_ms = now_ms() - t0;
    if (raw.size() != e.raw) { set_error("%s: key frame %d decodes to %zu bytes, its GTMk entry says %u", path.c_str(), k, raw.size(), e.raw); return fail(TM_E_IO); }
    t0 = now_ms();
    rc = parse_keyframe(raw.data(), raw.size(), path.c_str(), &head, k == 0, !head_held, kf_frames(k), out);
    if (k == 0 && rc == TM_OK) head_held = true;
    out->parse_ms = now_ms() - t0;
    if (rc != TM_OK) return fail(rc);
    if (out->nframes != kf_frames(k)) { set_error("%s: key frame %d holds %d frames, the index says %d", path.c_str(), k, out->nframes, kf_frames(k)); return fail(TM_E_IO); }
    out->index = k; out->first = e.frame;
    return TM_OK;
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
    TM_TRY(up.make()); TM_TRY(done.make());
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
        const int k = (int)(std::upper_bound(ix.kf.begin(), ix.kf.end(), pos, [](int f, const KfEntry &e) { return f < e.frame; }) - ix.kf.begin()) - 1;
        TM_TRY(enter_kf(k));
      }
      const int in_kf = pos - cur.first;
      const int n = std::min(std::min(chunk, count - n_done), cur.nframes - in_kf);
      const int b = (int)(chunk_no++ & 1);
      *between_chunks = false;
      double t0 = now_ms();
      const int64_t i0 = cur.intra_first[(size_t)in_kf], i1 = cur.intra_first[(size_t)(in_kf + n)];
      const size_t rb = (size_t)n * per * sizeof(PlayRec), ib = (size_t)(i1 - i0) * 64;
      if (used[b]) TM_HIP(hipEventSynchronize(up.ev[b]));  // the upload that last read this host buffer
      memcpy(h_chunk[b].p, cur.recs.data() + (size_t)in_kf * per, rb);
      if (ib) memcpy((uint8_t *)h_chunk[b].p + rb, cur.intra.data() + (size_t)i0 * 64, ib);
      if (used[b]) TM_HIP(hipStreamWaitEvent(copy, done.ev[b], 0));  // the frames that last read this device buffer
      TM_HIP(hipMemcpyAsync(d_chunk[b].p, h_chunk[b].p, rb + ib, hipMemcpyHostToDevice, copy));
      TM_HIP(hipEventRecord(up.ev[b], copy));
      TM_HIP(hipStreamWaitEvent(play, up.ev[b], 0));
      used[b] = true;
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
      TM_HIP(hipEventRecord(done.ev[b], play));
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
      const int k = (int)(std::upper_bound(ix.kf.begin(), ix.kf.end(), frame, [](int f, const KfEntry &e) { return f < e.frame; }) - ix.kf.begin()) - 1;
      TM_TRY(enter_kf(k));
      pos = cur.first;
      prev = nullptr;
    }
    if (frame > pos) TM_TRY(play_frames(frame - pos, nullptr, nullptr, nullptr));
    return TM_OK;
  }
};

namespace {
int fill_info(const GtmIndex &ix, const StreamHead &h, int64_t tileset_tiles, int pal_count, tm_gtm_info *o) {
  memset(o, 0, sizeof(*o));
  o->width = ix.width; o->height = ix.height; o->frames = ix.frames; o->keyframes = (int32_t)ix.kf.size();
  o->encoder_version = ix.version; o->avg_bytes_per_s = ix.avg; o->kf_max_bytes_per_s = ix.kf_max;
  o->tm_w = h.tm_w; o->tm_h = h.tm_h; o->tile_count = (int32_t)h.tile_count; o->tileset_tiles = (int32_t)tileset_tiles;
  o->pal_size = h.pal_size; o->pal_count = pal_count;
  o->fps = h.frame_ns ? 1000.0 * 1000 * 1000 / h.frame_ns : 0.0;
  return TM_OK;
}
}  // namespace

namespace tmx {
int probe_gtm(const char *path, int *width, int *height, double *fps, int *frames) {
  tm_player p;  // (no device call: the index and the first key frame's stream, as tm_player_open reads them)
  p.path = path;
  p.fd = open(path, O_RDONLY);
  TM_CHECK(p.fd >= 0, TM_E_IO, "cannot open %s", path);
  TM_TRY(read_index(p.fd, path, &p.ix));
  p.head.want_w = p.ix.width; p.head.want_h = p.ix.height;
  const int rc = p.load_kf(0, &p.cur);
  if (rc != TM_OK) { set_error("%s", p.cur.err.c_str()); return rc; }
  TM_CHECK(p.head.have_dims, TM_E_IO, "%s: the first key frame has no SetDimensions", path);
  *width = p.head.tm_w * 8; *height = p.head.tm_h * 8; *frames = p.ix.frames;
  *fps = 1000.0 * 1000 * 1000 / p.head.frame_ns;
  return TM_OK;
}
}  // namespace tmx

extern "C" {

int tm_player_open(const char *path, int device, tm_player **out) {
  TM_CHECK(path && out, TM_E_INVAL, "null argument");
  *out = nullptr;
  knobs_reload();
  std::unique_ptr<tm_player> p(new tm_player());
  p->t_open = now_ms();
  p->path = path; p->device = device;
  p->no_worker = knobs().player_no_worker;
  p->fd = open(path, O_RDONLY);
  TM_CHECK(p->fd >= 0, TM_E_IO, "cannot open %s", path);
  TM_TRY(read_index(p->fd, path, &p->ix));
  p->head.want_w = p->ix.width; p->head.want_h = p->ix.height;
  {
    const int rc = p->load_kf(0, &p->cur);
    if (rc != TM_OK) { set_error("%s", p->cur.err.c_str()); return rc; }
    p->took(p->cur);
    p->peak_records = p->cur.bytes();
  }
  TM_CHECK(p->head.have_dims, TM_E_IO, "%s: the first key frame has no SetDimensions", path);
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

int tm_player_probe_host(const char *path, tm_gtm_info *info, int32_t *kf, int cap_kf, int *nkf) {
  TM_CHECK(path, TM_E_INVAL, "null argument");
  const int fd = open(path, O_RDONLY);
  TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", path);
  struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
  GtmIndex ix;
  TM_TRY(read_index(fd, path, &ix));
  if (info) fill_info(ix, StreamHead(), 0, 0, info);
  if (nkf) *nkf = (int)ix.kf.size();
  if (kf)
    for (int k = 0; k < std::min(cap_kf, (int)ix.kf.size()); k++) {
      kf[4 * k] = ix.kf[(size_t)k].frame; kf[4 * k + 1] = (int32_t)ix.kf[(size_t)k].raw; kf[4 * k + 2] = (int32_t)ix.kf[(size_t)k].comp; kf[4 * k + 3] = (int32_t)ix.kf[(size_t)k].ms;
    }
  return TM_OK;
}

int tm_player_parse_host(const uint8_t *raw, size_t n, int tm_w, int tm_h, int64_t tile_count, uint64_t *records, int cap_frames, uint8_t *intra, int64_t cap_intra,
                         int64_t *intra_first, int *frames, int64_t *nintra) {
  TM_CHECK((raw || n == 0) && frames && nintra, TM_E_INVAL, "null argument");
  TM_CHECK(tm_w >= 0 && tm_h >= 0 && tm_w <= 65535 && tm_h <= 65535 && tile_count >= 0, TM_E_INVAL, "bad dimensions %d x %d", tm_w, tm_h);
  TM_CHECK(!records || (tm_w > 0 && tm_h > 0), TM_E_INVAL, "records are sized by tm_w and tm_h: pass them");
  TM_CHECK((int64_t)tm_w * tm_h <= MAX_ITEMS, TM_E_INVAL, "%d x %d tiles: more than %lld items a frame", tm_w, tm_h, (long long)MAX_ITEMS);
  StreamHead head;
  if (tm_w > 0 && tm_h > 0) { head.tm_w = tm_w; head.tm_h = tm_h; head.tile_count = tile_count; head.frame_ns = 1; head.have_dims = true; }
  KfRecords kf;
  TM_TRY(parse_keyframe(raw, n, "key frame", &head, true, true, 0x7fffffff, &kf));
  *frames = kf.nframes;
  *nintra = (int64_t)(kf.intra.size() / 64);
  TM_CHECK((!records && !intra && !intra_first) || (kf.nframes <= cap_frames && *nintra <= cap_intra), TM_E_INVAL, "%d frames and %lld intra tiles: capacities %d and %lld",
           kf.nframes, (long long)*nintra, cap_frames, (long long)cap_intra);
  if (records) memcpy(records, kf.recs.data(), (size_t)kf.nframes * head.tm_w * head.tm_h * sizeof(PlayRec));
  if (intra) memcpy(intra, kf.intra.data(), (size_t)*nintra * 64);
  if (intra_first) memcpy(intra_first, kf.intra_first.data(), ((size_t)kf.nframes + 1) * sizeof(int64_t));
  return TM_OK;
}

int tm_stage_play_frame(const void *records, const void *intra, int64_t nintra, const void *tiles, const void *palettes, const void *prev, void *out, int tm_w, int tm_h,
                        int pal_size, int64_t ntiles, int npal, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(records && out && tm_w > 0 && tm_h > 0 && tm_w <= 65535 && tm_h <= 65535 && pal_size >= 0 && ntiles >= 0 && npal >= 0 && nintra >= 0 && (intra || nintra == 0) &&
               (tiles || ntiles == 0) && (palettes || npal == 0), TM_E_INVAL, "play_frame: bad arguments");
  TM_CHECK((((uintptr_t)out | (uintptr_t)records) & 15) == 0 && (((uintptr_t)intra | (uintptr_t)tiles | (uintptr_t)palettes | (uintptr_t)prev) & 3) == 0, TM_E_INVAL,
           "play_frame: out and records must be 16-byte aligned, the other arrays 4-byte aligned");
  return launch_play_frame(records, intra, nintra, tiles, ntiles, palettes, npal, pal_size, prev, out, tm_w, tm_h, (hipStream_t)stream);
}

}  // extern "C"
