// tm_gif_in.hip -- the GIF reader.  The rule is tm_gif.h's; the host twins (tm_gif_lzw_streams_host,
// tm_gif_decode_host) run the same text on one lane, and the tests' Python restatement and Pillow are the independent checks.
//
//   host      parse_gif walks the container with every refusal and leaves a descriptor per image: rectangle, graphic control, the colours
//             that apply, where the sub-block chain lies in the file.  The sub-blocks are not joined.
//   lzw       k_gif_lzw, one wave (one workgroup) per image, every image of a chunk in one launch.  The decode state is the same in every
//             lane.  In LDS: the table, 4096 x (32-bit position, 16-bit length), and a stage of 1 KiB of payload gathered through the
//             sub-block chain (25 KB: six workgroups to a compute unit's 160 KB).  A string is copied by the whole wave out of the image's
//             own earlier output in memory, in 4-byte stores where the destination is whole words.  The copy's source may be anything the
//             image has written since the last clear, so it cannot all live in LDS; what makes the read of another lane's store correct is
//             `drained`: output below it was stored before a __syncthreads() (a release and an acquire fence at workgroup scope, which
//             waits for the wave's stores), and a copy whose source reaches at or above it makes that barrier first.  Nothing depends on
//             how long a store takes.
//   compose   k_gif_compose, pixel-parallel and frame-serial, one launch per chunk: a lane owns four neighbouring canvas pixels with their
//             canvas and saved-canvas values in registers, walks the chunk's frames and writes one 16-byte store per delivered frame.
//             Between chunks the two canvases lie in two device buffers.
//
// Every loop is bounded by a stream's span, its npix or the screen; plain launches, nothing waits on another workgroup.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "tm_common.h"
#include "tm_internal.h"
#include "tm_gif.h"

namespace tmx {
namespace gif {
namespace {

constexpr uint32_t kStage = 1024;  // payload bytes staged in LDS

// ---- the host IO: one lane
struct HostIO {
  const uint8_t *src;
  uint32_t src_bytes;
  uint8_t *dst;
  Chain chain;
  uint32_t run_at = 0, run_n = 0;
  uint32_t pos_[kTableSize];
  uint16_t len_[kTableSize];
  bool next_byte(uint32_t *b) {
    if (run_n == 0 && !chain_next_run(chain, src_bytes, [this](uint32_t p) { return (uint32_t)src[p]; }, 0xffffffffu, &run_at, &run_n)) return false;
    *b = src[run_at];
    run_at++; run_n--;
    return true;
  }
  void entry_set(uint32_t i, uint32_t pos, uint32_t len) { pos_[i] = pos; len_[i] = (uint16_t)len; }
  void entry_get(uint32_t i, uint32_t *pos, uint32_t *len) const { *pos = pos_[i]; *len = len_[i]; }
  void put(uint32_t out, uint32_t v) { dst[out] = (uint8_t)v; }
  void copy(uint32_t out, uint32_t s, uint32_t len, uint32_t period) {
    for (uint32_t k = 0; k < len; k++) dst[out + k] = dst[s + (k < period ? k : k - period)];
  }
  void finish(uint32_t) {}
};

// ---- the device IO: one wave
struct WaveLds {
  uint32_t pos[kTableSize];
  uint16_t len[kTableSize];
  uint8_t stage[kStage];
};

struct WaveIO {
  WaveLds &m;
  const uint8_t *src;
  uint32_t src_bytes;
  uint8_t *dst;  // (read back by other lanes: never __restrict__)
  uint32_t lane_;
  Chain chain;
  uint32_t sn = 0, sp = 0;  // payload bytes in the stage, and how many of them have been handed out
  uint32_t drained = 0;     // output bytes [0, drained) were stored before the last barrier: every lane may read them
  __device__ WaveIO(WaveLds &m_, const uint8_t *src_, uint32_t src_bytes_, uint8_t *dst_) : m(m_), src(src_), src_bytes(src_bytes_), dst(dst_), lane_(threadIdx.x) {}
  // the next payload bytes into LDS, gathered through the sub-block chain (the same walk in every lane)
  __device__ bool restage() {
    __syncthreads();
    sn = 0; sp = 0;
    const uint8_t *s = src;
    uint32_t at, n;
    while (sn < kStage && chain_next_run(chain, src_bytes, [s](uint32_t p) { return (uint32_t)s[p]; }, kStage - sn, &at, &n)) {
      for (uint32_t k = lane_; k < n; k += 64) m.stage[sn + k] = src[at + k];  // at + n <= src_bytes (chain_next_run)
      sn += n;
    }
    __syncthreads();
    return sn > 0;
  }
  __device__ bool next_byte(uint32_t *b) {
    if (sp >= sn && !restage()) return false;
    *b = m.stage[sp++];
    return true;
  }
  __device__ void entry_set(uint32_t i, uint32_t pos, uint32_t len) { m.pos[i] = pos; m.len[i] = (uint16_t)len; }  // (every lane writes the same values)
  __device__ void entry_get(uint32_t i, uint32_t *pos, uint32_t *len) const { *pos = m.pos[i]; *len = m.len[i]; }
  __device__ void put(uint32_t out, uint32_t v) { if (lane_ == 0) dst[out] = (uint8_t)v; }
  __device__ void copy(uint32_t out, uint32_t s, uint32_t len, uint32_t period) {
    if (s + (len < period ? len : period) > drained) {  // the source holds bytes stored since the last barrier
      __syncthreads();
      drained = out;
    }
    // word j of the run covers its bytes [4 j - skew, 4 j - skew + 4): a whole word is one store, the run's ragged ends go byte by byte
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(dst + out) & 3u);
    const uint32_t words = (skew + len + 3) / 4;
    for (uint32_t j = lane_; j < words; j += 64) {
      const int32_t k0 = (int32_t)(4 * j) - (int32_t)skew;
      if (k0 >= 0 && (uint32_t)k0 + 4 <= len) {
        uint32_t v = 0;
        for (uint32_t t = 0; t < 4; t++) {
          const uint32_t k = (uint32_t)k0 + t;
          v |= (uint32_t)dst[s + (k < period ? k : k - period)] << (8 * t);
        }
        *reinterpret_cast<uint32_t *>(dst + out + k0) = v;
      } else {
        for (int32_t t = 0; t < 4; t++) {
          const int32_t k = k0 + t;
          if (k >= 0 && (uint32_t)k < len) dst[out + (uint32_t)k] = dst[s + ((uint32_t)k < period ? (uint32_t)k : (uint32_t)k - period)];
        }
      }
    }
  }
  __device__ void finish(uint32_t) {}
};

TM_GIF_HD inline bool stream_fits(const tm_gif_stream &st, uint64_t blob_bytes, uint64_t dst_bytes) {
  return st.src_off <= blob_bytes && st.src_bytes <= blob_bytes - st.src_off && st.dst_off <= dst_bytes && st.npix <= dst_bytes - st.dst_off && st.min_code_size >= 2 &&
         st.min_code_size <= 8;
}

// One wave per image.  A stream whose span or destination does not lie inside what the launch was given is refused untouched.
__global__ __launch_bounds__(64) void k_gif_lzw(const uint8_t *__restrict__ blob, uint64_t blob_bytes, const tm_gif_stream *__restrict__ streams, uint8_t *dst,
                                                uint64_t dst_bytes, tm_gif_status *__restrict__ status) {
  __shared__ __align__(16) WaveLds lds;
  const tm_gif_stream st = streams[blockIdx.x];
  tm_gif_status res{kBadDesc, 0, 0};
  if (stream_fits(st, blob_bytes, dst_bytes)) {
    WaveIO io(lds, blob + st.src_off, st.src_bytes, dst + st.dst_off);
    lzw_stream(io, st.min_code_size, st.npix, &res);
  }
  if (threadIdx.x == 0) status[blockIdx.x] = res;
}

// Four neighbouring pixels of the canvas (in row-major order over the screen) per lane, the chunk's frames one after another.
// descs: has_prev + nframes descriptors, the first being the frame before the chunk when has_prev.  failed_in / failed_out: whether an
// image before this chunk / up to its end was refused (nothing is delivered from the first refused image on).
__global__ __launch_bounds__(256) void k_gif_compose(const FrameDesc *__restrict__ descs, int nframes, int has_prev, const uint32_t *__restrict__ colours,
                                                     const uint8_t *__restrict__ idx, const tm_gif_status *__restrict__ lzw, int W, int H, uint32_t bg,
                                                     uint32_t *__restrict__ out, int64_t frame_px, uint32_t *__restrict__ canvas_buf, uint32_t *__restrict__ saved_buf,
                                                     int fresh, const int32_t *__restrict__ failed_in, int32_t *__restrict__ failed_out) {
  const bool first_lane = blockIdx.x == 0 && threadIdx.x == 0;
  if (*failed_in) {
    if (first_lane) *failed_out = 1;
    return;
  }
  const int64_t total = (int64_t)W * H, q0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (q0 >= total) return;
  const int nq = total - q0 < 4 ? (int)(total - q0) : 4;
  const bool wide = nq == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (frame_px & 3) == 0;
  int x[4], y[4];
  uint32_t canvas[4], saved[4];
  for (int k = 0; k < 4; k++) {
    const int64_t q = q0 + (k < nq ? k : 0);
    y[k] = (int)(q / W); x[k] = (int)(q - (int64_t)y[k] * W);
    canvas[k] = fresh ? bg : canvas_buf[q];
    saved[k] = fresh ? bg : saved_buf[q];
  }
  for (int f = 0; f < nframes; f++) {
    const FrameDesc cur = descs[has_prev + f];
    if (lzw[cur.stream].code != kOk) {  // (the same in every lane)
      if (first_lane) *failed_out = 1;
      break;
    }
    if (has_prev || f > 0) {
      const FrameDesc prev = descs[has_prev + f - 1];
      for (int k = 0; k < 4; k++) canvas[k] = dispose_pixel(canvas[k], saved[k], prev, x[k], y[k], bg);
    }
    for (int k = 0; k < 4; k++) {
      saved[k] = canvas[k];
      if (in_rect(cur, x[k], y[k])) canvas[k] = draw_pixel(canvas[k], cur, idx[index_at(cur, x[k], y[k])], colours);
    }
    if (cur.slot >= 0) {
      uint32_t *to = out + cur.slot * frame_px + q0;
      if (wide) *reinterpret_cast<uint4 *>(to) = make_uint4(canvas[0], canvas[1], canvas[2], canvas[3]);
      else
        for (int k = 0; k < nq; k++) to[k] = canvas[k];
    }
  }
  for (int k = 0; k < nq; k++) { canvas_buf[q0 + k] = canvas[k]; saved_buf[q0 + k] = saved[k]; }
}

void lzw_one_host(const uint8_t *src, uint32_t src_bytes, uint32_t min_code, uint8_t *dst, uint32_t npix, tm_gif_status *st) {
  HostIO io{src, src_bytes, dst};
  lzw_stream(io, min_code, npix, st);
}

int check_streams(const char *who, const uint8_t *blob, size_t blob_bytes, const tm_gif_stream *streams, int nstreams, const void *dst, size_t dst_bytes, const tm_gif_status *status) {
  TM_CHECK((blob || !blob_bytes) && (streams || !nstreams) && (dst || !dst_bytes) && (status || !nstreams) && nstreams >= 0, TM_E_INVAL, "%s: null argument", who);
  TM_CHECK(blob_bytes < ((size_t)1 << 32), TM_E_UNSUPPORTED, "%s: a blob of %zu bytes (below 4 GiB)", who, blob_bytes);
  for (int s = 0; s < nstreams; s++) {
    const tm_gif_stream &st = streams[s];
    TM_CHECK(st.min_code_size >= 2 && st.min_code_size <= 8, TM_E_INVAL, "%s: stream %d has a minimum code size of %u (2..8)", who, s, st.min_code_size);
    TM_CHECK(st.src_off <= blob_bytes && st.src_bytes <= blob_bytes - st.src_off, TM_E_INVAL, "%s: stream %d's data lies outside the blob", who, s);
    TM_CHECK(st.dst_off <= dst_bytes && st.npix <= dst_bytes - st.dst_off, TM_E_INVAL, "%s: stream %d's destination lies outside the %zu bytes given", who, s, dst_bytes);
  }
  return TM_OK;
}

uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// fn(i) for i in [0, n) on up to `threads` host threads, the calling one included
template <class F>
void each_on_threads(int n, int threads, F fn) {
  const int nt = std::max(1, std::min(threads, n));
  std::atomic<int> next{0};
  auto work = [&]() { for (int i = next++; i < n; i = next++) fn(i); };
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; t++) pool.emplace_back(work);
  work();
  for (std::thread &t : pool) t.join();
}

// the chunks of images [0, n): chunk_frames each, or as many as 1 GiB of stored indices holds
std::vector<int> chunk_ends(const GifInfo &info, int n, int chunk_frames) {
  std::vector<int> ends;
  uint64_t held = 0;
  int in_chunk = 0;
  for (int i = 0; i < n; i++) {
    const uint64_t px = ((uint64_t)info.images[(size_t)i].w * (uint64_t)info.images[(size_t)i].h + 15) & ~(uint64_t)15;
    const bool full = chunk_frames > 0 ? in_chunk >= chunk_frames : (in_chunk > 0 && held + px > ((uint64_t)1 << 30));
    if (full) { ends.push_back(i); held = 0; in_chunk = 0; }
    held += px; in_chunk++;
  }
  if (n > 0) ends.push_back(n);
  return ends;
}

FrameDesc desc_of(const Image &im, int32_t stream, uint64_t idx_off, int64_t slot) {
  return FrameDesc{im.left, im.top, im.w, im.h, im.disposal, im.transparent, im.interlaced, (int32_t)im.table_n, im.table_off, stream, idx_off, slot};
}

int check_decode(const char *who, const void *file, size_t size, int first, int count, int background, const void *out, int64_t frame_px, const int32_t *status,
                 GifInfo *info) {
  TM_CHECK(file && (out || !count) && status && first >= 0 && count >= 0, TM_E_INVAL, "%s: null argument or a negative frame range", who);
  TM_CHECK(background >= -1 && background <= 0xffffff, TM_E_INVAL, "%s: background %d (-1 or 0x00RRGGBB)", who, background);
  TM_TRY(parse_gif((const uint8_t *)file, size, "the file", info));
  TM_CHECK((int64_t)first + count <= (int64_t)info->images.size(), TM_E_INVAL, "%s: frames [%d, %d) of %zu", who, first, first + count, info->images.size());
  TM_CHECK(frame_px >= (int64_t)info->w * info->h, TM_E_INVAL, "%s: frames %lld pixels apart, the screen has %lld", who, (long long)frame_px, (long long)info->w * info->h);
  return TM_OK;
}

}  // namespace

// ---- the container walk
int parse_gif(const uint8_t *file, size_t n, const char *name, GifInfo *info) {
  *info = GifInfo();
  TM_CHECK(n >= 6 && (!memcmp(file, "GIF87a", 6) || !memcmp(file, "GIF89a", 6)), TM_E_UNSUPPORTED, "%s is not a GIF file", name);
  TM_CHECK(n < ((size_t)1 << 32), TM_E_UNSUPPORTED, "%s: a file of %zu bytes (below 4 GiB)", name, n);
  info->version = file[4] == '7' ? 87 : 89;
  TM_CHECK(n >= 13, TM_E_IO, "%s: the logical screen descriptor runs past the end of the file", name);
  info->w = (int32_t)le16(file + 6); info->h = (int32_t)le16(file + 8);
  TM_CHECK(info->w > 0 && info->h > 0, TM_E_IO, "%s: a screen of %dx%d", name, info->w, info->h);
  info->bg_index = file[11];
  size_t pos = 13;
  if (file[10] & 0x80) {
    info->global_n = 2 << (file[10] & 7);
    TM_CHECK(pos + 3 * (size_t)info->global_n <= n, TM_E_IO, "%s: the global colour table runs past the end of the file", name);
    for (int i = 0; i < info->global_n; i++, pos += 3) info->colours.push_back((uint32_t)file[pos] << 16 | (uint32_t)file[pos + 1] << 8 | file[pos + 2]);
  }
  info->bg = info->bg_index < info->global_n ? info->colours[(size_t)info->bg_index] : 0u;
  int delay = 0, disposal = 0, transparent = -1;  // of the graphic control extension that applies to the next image
  // skips sub-blocks from pos on, terminator included
  auto skip_blocks = [&](const char *what) -> int {
    for (;;) {
      TM_CHECK(pos < n, TM_E_IO, "%s: %s runs past the end of the file", name, what);
      const size_t len = file[pos];
      pos++;
      if (!len) return (int)TM_OK;
      TM_CHECK(len <= n - pos, TM_E_IO, "%s: a sub-block of %s runs past the end of the file", name, what);
      pos += len;
    }
  };
  for (;;) {
    if (pos >= n) {  // no trailer: accepted behind a whole image
      TM_CHECK(!info->images.empty(), TM_E_IO, "%s: the file ends before its first image", name);
      break;
    }
    const uint8_t b = file[pos];
    if (b == 0x3b) break;
    if (b == 0x21) {
      TM_CHECK(pos + 2 <= n, TM_E_IO, "%s: an extension runs past the end of the file", name);
      const uint8_t label = file[pos + 1];
      pos += 2;
      if (label == 0xf9) {
        if (pos < n && file[pos] >= 4 && (size_t)file[pos] <= n - pos - 1) {
          const uint8_t *g = file + pos + 1;
          disposal = (g[0] >> 2) & 7;
          delay = (int)le16(g + 1);
          transparent = (g[0] & 1) ? (int)g[3] : -1;
        }
        TM_TRY(skip_blocks("a graphic control extension"));
      } else if (label == 0xff) {
        if (pos + 1 + 11 + 1 + 3 <= n && file[pos] == 11 && (!memcmp(file + pos + 1, "NETSCAPE2.0", 11) || !memcmp(file + pos + 1, "ANIMEXTS1.0", 11)) && file[pos + 12] >= 3 &&
            file[pos + 13] == 1)
          info->loop = (int32_t)le16(file + pos + 14);
        TM_TRY(skip_blocks("an application extension"));
      } else
        TM_TRY(skip_blocks(label == 0xfe ? "a comment extension" : label == 0x01 ? "a plain text extension" : "an extension"));
      continue;
    }
    TM_CHECK(b == 0x2c, TM_E_IO, "%s: unknown block introducer 0x%02x at offset %zu", name, b, pos);
    TM_CHECK(pos + 10 <= n, TM_E_IO, "%s: an image descriptor runs past the end of the file", name);
    Image im{};
    im.left = (int32_t)le16(file + pos + 1); im.top = (int32_t)le16(file + pos + 3); im.w = (int32_t)le16(file + pos + 5); im.h = (int32_t)le16(file + pos + 7);
    const uint8_t packed = file[pos + 9];
    pos += 10;
    const int image = (int)info->images.size();
    TM_CHECK(im.w > 0 && im.h > 0, TM_E_IO, "%s: image %d is %dx%d", name, image, im.w, im.h);
    im.interlaced = (packed & 0x40) ? 1 : 0;
    im.local = (packed & 0x80) ? 1 : 0;
    if (im.local) {
      im.table_n = 2u << (packed & 7);
      TM_CHECK(pos + 3 * (size_t)im.table_n <= n, TM_E_IO, "%s: image %d's colour table runs past the end of the file", name, image);
      im.table_off = (uint32_t)info->colours.size();
      for (uint32_t i = 0; i < im.table_n; i++, pos += 3) info->colours.push_back((uint32_t)file[pos] << 16 | (uint32_t)file[pos + 1] << 8 | file[pos + 2]);
    } else {
      TM_CHECK(info->global_n > 0, TM_E_IO, "%s: image %d has no colour table and the file has no global one", name, image);
      im.table_off = 0; im.table_n = (uint32_t)info->global_n;
    }
    TM_CHECK(pos < n, TM_E_IO, "%s: image %d's data runs past the end of the file", name, image);
    im.min_code = file[pos];
    pos++;
    TM_CHECK(im.min_code >= 2 && im.min_code <= 8, TM_E_IO, "%s: image %d has a minimum code size of %d (2..8)", name, image, im.min_code);
    im.data_off = pos;
    TM_TRY(skip_blocks("the image data"));
    im.data_bytes = pos - im.data_off;
    im.delay = delay; im.disposal = disposal; im.transparent = transparent;
    delay = 0; disposal = 0; transparent = -1;
    info->images.push_back(im);
  }
  TM_CHECK(!info->images.empty(), TM_E_IO, "%s: no image before the trailer", name);
  TM_CHECK(info->images.size() < ((size_t)1 << 31), TM_E_UNSUPPORTED, "%s: too many images", name);
  int64_t sum = 0;
  const int d0 = info->images[0].delay < 2 ? 10 : info->images[0].delay;
  for (const Image &im : info->images) {
    const int d = im.delay < 2 ? 10 : im.delay;  // (0 and 1 count as 10, as browsers have it)
    sum += d;
    if (d != d0) info->uniform_delay = 0;
  }
  info->fps = 100.0 * (double)info->images.size() / (double)sum;
  return TM_OK;
}

int gif_status_error(int status, const char *name, int image) {
  if (status == kOk) return TM_OK;
  if (status == kTruncated) set_error("%s: image %d: the LZW data ends before the picture is whole", name, image);
  else if (status == kBadCode) set_error("%s: image %d: an LZW code that the table does not hold", name, image);
  else set_error("%s: image %d: refused (code %d)", name, image, status);
  return TM_E_IO;
}

int gif_decode_host(const uint8_t *file, size_t size, const GifInfo &info, int first, int count, uint32_t bg, uint32_t *out, int64_t frame_px, int32_t *status, int threads) {
  (void)size;
  const int n = first + count, W = info.w, H = info.h;
  const std::vector<int> ends = chunk_ends(info, n, 64);
  std::vector<uint32_t> canvas((size_t)W * H, bg), saved((size_t)W * H, bg);
  std::vector<uint8_t> idx;
  std::vector<uint64_t> at;
  std::vector<tm_gif_status> st;
  bool failed = false;
  int c0 = 0;
  for (int c1 : ends) {
    const int nf = c1 - c0;
    at.assign((size_t)nf, 0);
    uint64_t bytes = 0;
    for (int i = 0; i < nf; i++) { at[(size_t)i] = bytes; bytes += (uint64_t)info.images[(size_t)(c0 + i)].w * (uint64_t)info.images[(size_t)(c0 + i)].h; }
    idx.resize((size_t)bytes);
    st.assign((size_t)nf, tm_gif_status{0, 0, 0});
    each_on_threads(nf, threads, [&](int i) {
      const Image &im = info.images[(size_t)(c0 + i)];
      lzw_one_host(file + im.data_off, (uint32_t)im.data_bytes, (uint32_t)im.min_code, idx.data() + at[(size_t)i], (uint32_t)im.w * (uint32_t)im.h, &st[(size_t)i]);
    });
    for (int i = 0; i < nf; i++) {
      const int f = c0 + i;
      status[f] = st[(size_t)i].code;
      if (status[f] != kOk) failed = true;
      if (failed) continue;  // nothing is delivered from the first refused image on
      const FrameDesc cur = desc_of(info.images[(size_t)f], i, at[(size_t)i], f >= first ? f - first : -1);
      if (f > 0) {
        const FrameDesc prev = desc_of(info.images[(size_t)(f - 1)], -1, 0, -1);
        if (prev.disposal == 2 || prev.disposal == 3)
          for (int y = std::max(prev.top, 0); y < std::min(prev.top + prev.h, H); y++)
            for (int x = std::max(prev.left, 0); x < std::min(prev.left + prev.w, W); x++) {
              const size_t q = (size_t)y * W + x;
              canvas[q] = dispose_pixel(canvas[q], saved[q], prev, x, y, bg);
            }
      }
      if (cur.disposal == 3) saved = canvas;  // (`saved` is read only where this frame is disposed of with 3)
      for (int y = std::max(cur.top, 0); y < std::min(cur.top + cur.h, H); y++)
        for (int x = std::max(cur.left, 0); x < std::min(cur.left + cur.w, W); x++) {
          const size_t q = (size_t)y * W + x;
          canvas[q] = draw_pixel(canvas[q], cur, idx[(size_t)index_at(cur, x, y)], info.colours.data());
        }
      if (cur.slot >= 0) memcpy(out + cur.slot * frame_px, canvas.data(), canvas.size() * 4);
    }
    c0 = c1;
  }
  return TM_OK;
}

int gif_decode_device(const uint8_t *file, size_t size, const GifInfo &info, int first, int count, uint32_t bg, uint32_t *dev_out, int64_t frame_px, int32_t *status,
                      int chunk_frames, void *hip_stream, int64_t *bytes_uploaded) {
  hipStream_t hs = (hipStream_t)hip_stream;
  const int n = first + count, W = info.w, H = info.h;
  if (!n) return TM_OK;
  const std::vector<int> ends = chunk_ends(info, n, chunk_frames);
  const size_t nchunks = ends.size();
  size_t max_idx = 16, max_desc = 16;
  {
    int c0 = 0;
    for (int c1 : ends) {
      uint64_t bytes = 0;
      for (int i = c0; i < c1; i++) bytes += ((uint64_t)info.images[(size_t)i].w * (uint64_t)info.images[(size_t)i].h + 15) & ~(uint64_t)15;
      max_idx = std::max<size_t>(max_idx, (size_t)bytes);
      max_desc = std::max<size_t>(max_desc, (size_t)(c1 - c0) * sizeof(tm_gif_stream) + (size_t)(c1 - c0 + 1) * sizeof(FrameDesc));
      c0 = c1;
    }
  }
  const size_t colours = std::max<size_t>(info.colours.size(), 1);
  DevBuf d_file, d_colours, d_desc, d_idx, d_canvas, d_saved, d_flags, d_status;
  TM_TRY(d_file.alloc(size)); TM_TRY(d_colours.alloc(colours * 4)); TM_TRY(d_idx.alloc(max_idx));
  TM_TRY(d_canvas.alloc((size_t)W * H * 4)); TM_TRY(d_saved.alloc((size_t)W * H * 4)); TM_TRY(d_flags.alloc((nchunks + 1) * 4));
  TM_TRY(d_status.alloc((size_t)n * sizeof(tm_gif_status)));
  TM_HIP(hipMemcpyAsync(d_file.p, file, size, hipMemcpyHostToDevice, hs));
  if (!info.colours.empty()) TM_HIP(hipMemcpyAsync(d_colours.p, info.colours.data(), info.colours.size() * 4, hipMemcpyHostToDevice, hs));
  TM_HIP(hipMemsetAsync(d_flags.p, 0, (nchunks + 1) * 4, hs));
  if (bytes_uploaded) *bytes_uploaded += (int64_t)size + (int64_t)info.colours.size() * 4;
  std::vector<std::vector<uint8_t>> blobs(nchunks);  // (alive until the stream has been waited for)
  std::vector<DevBuf> d_descs(nchunks);
  int c0 = 0;
  for (size_t c = 0; c < nchunks; c++) {
    const int c1 = ends[c], nf = c1 - c0, has_prev = c0 > 0 ? 1 : 0;
    std::vector<uint8_t> &blob = blobs[c];
    blob.resize((size_t)nf * sizeof(tm_gif_stream) + (size_t)(nf + has_prev) * sizeof(FrameDesc));
    tm_gif_stream *streams = reinterpret_cast<tm_gif_stream *>(blob.data());
    FrameDesc *descs = reinterpret_cast<FrameDesc *>(blob.data() + (size_t)nf * sizeof(tm_gif_stream));
    if (has_prev) descs[0] = desc_of(info.images[(size_t)(c0 - 1)], -1, 0, -1);
    uint64_t at = 0;
    for (int i = 0; i < nf; i++) {
      const Image &im = info.images[(size_t)(c0 + i)];
      const uint32_t npix = (uint32_t)im.w * (uint32_t)im.h;
      streams[i] = tm_gif_stream{im.data_off, at, (uint32_t)im.data_bytes, npix, (uint32_t)im.min_code, 0};
      descs[has_prev + i] = desc_of(im, i, at, c0 + i >= first ? c0 + i - first : -1);
      at += ((uint64_t)npix + 15) & ~(uint64_t)15;
    }
    TM_TRY(d_descs[c].alloc(blob.size()));
    TM_HIP(hipMemcpyAsync(d_descs[c].p, blob.data(), blob.size(), hipMemcpyHostToDevice, hs));
    if (bytes_uploaded) *bytes_uploaded += (int64_t)blob.size();
    const tm_gif_stream *dv_streams = d_descs[c].as<tm_gif_stream>();
    const FrameDesc *dv_descs = reinterpret_cast<const FrameDesc *>(d_descs[c].as<uint8_t>() + (size_t)nf * sizeof(tm_gif_stream));
    tm_gif_status *dv_status = d_status.as<tm_gif_status>() + c0;
    hipLaunchKernelGGL(k_gif_lzw, dim3((unsigned)nf), dim3(64), 0, hs, d_file.as<uint8_t>(), (uint64_t)size, dv_streams, d_idx.as<uint8_t>(), (uint64_t)at, dv_status);
    const int64_t quads = ((int64_t)W * H + 3) / 4;
    hipLaunchKernelGGL(k_gif_compose, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, hs, dv_descs, nf, has_prev, d_colours.as<uint32_t>(), d_idx.as<uint8_t>(), dv_status, W,
                       H, bg, dev_out, frame_px, d_canvas.as<uint32_t>(), d_saved.as<uint32_t>(), c0 == 0 ? 1 : 0, d_flags.as<int32_t>() + c, d_flags.as<int32_t>() + c + 1);
    TM_HIP(hipGetLastError());
    c0 = c1;
  }
  std::vector<tm_gif_status> st((size_t)n);
  TM_HIP(hipMemcpyAsync(st.data(), d_status.p, (size_t)n * sizeof(tm_gif_status), hipMemcpyDeviceToHost, hs));
  TM_HIP(hipStreamSynchronize(hs));
  for (int i = 0; i < n; i++) status[i] = st[(size_t)i].code;
  return TM_OK;
}

}  // namespace gif
}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_gif_host(const void *file, size_t size, tm_gif_info *out) {
  TM_CHECK(file && out, TM_E_INVAL, "tm_probe_gif_host: null argument");
  gif::GifInfo info;
  TM_TRY(gif::parse_gif((const uint8_t *)file, size, "the file", &info));
  *out = tm_gif_info{info.w, info.h, (int32_t)info.images.size(), info.uniform_delay, info.loop, info.global_n, info.bg_index, info.version, info.bg, 0, info.fps};
  return TM_OK;
}

int tm_gif_frames_host(const void *file, size_t size, tm_gif_frame *out, int cap, int *nframes) {
  TM_CHECK(file && (out || cap <= 0) && nframes, TM_E_INVAL, "tm_gif_frames_host: null argument");
  gif::GifInfo info;
  TM_TRY(gif::parse_gif((const uint8_t *)file, size, "the file", &info));
  *nframes = (int)info.images.size();
  for (int i = 0; i < *nframes && i < cap; i++) {
    const gif::Image &im = info.images[(size_t)i];
    out[i] = tm_gif_frame{im.left, im.top, im.w, im.h, im.delay, im.disposal, im.transparent, im.interlaced, (int32_t)im.table_n, im.local, im.min_code, 0, im.data_off, im.data_bytes};
  }
  return TM_OK;
}

int tm_gif_lzw_streams_host(const uint8_t *blob, size_t blob_bytes, const tm_gif_stream *streams, int nstreams, uint8_t *dst, size_t dst_bytes, tm_gif_status *status) {
  TM_TRY(gif::check_streams("tm_gif_lzw_streams_host", blob, blob_bytes, streams, nstreams, dst, dst_bytes, status));
  for (int s = 0; s < nstreams; s++)
    gif::lzw_one_host(blob + streams[s].src_off, streams[s].src_bytes, streams[s].min_code_size, dst + streams[s].dst_off, streams[s].npix, &status[s]);
  return TM_OK;
}

int tm_stage_gif_lzw(const uint8_t *blob, size_t blob_bytes, const tm_gif_stream *streams, int nstreams, uint8_t *dev_dst, size_t dst_bytes, tm_gif_status *status, void *stream) {
  TM_TRY(gif::check_streams("tm_stage_gif_lzw", blob, blob_bytes, streams, nstreams, dev_dst, dst_bytes, status));
  knobs_reload();
  TM_TRY(require_device());
  if (!nstreams) return TM_OK;
  hipStream_t hs = (hipStream_t)stream;
  DevBuf d_blob, d_streams, d_status;
  TM_TRY(d_blob.alloc(blob_bytes)); TM_TRY(d_streams.alloc((size_t)nstreams * sizeof(tm_gif_stream))); TM_TRY(d_status.alloc((size_t)nstreams * sizeof(tm_gif_status)));
  if (blob_bytes) TM_HIP(hipMemcpyAsync(d_blob.p, blob, blob_bytes, hipMemcpyHostToDevice, hs));
  TM_HIP(hipMemcpyAsync(d_streams.p, streams, (size_t)nstreams * sizeof(tm_gif_stream), hipMemcpyHostToDevice, hs));
  hipLaunchKernelGGL(gif::k_gif_lzw, dim3((unsigned)nstreams), dim3(64), 0, hs, d_blob.as<uint8_t>(), (uint64_t)blob_bytes, d_streams.as<tm_gif_stream>(), dev_dst,
                     (uint64_t)dst_bytes, d_status.as<tm_gif_status>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipMemcpyAsync(status, d_status.p, (size_t)nstreams * sizeof(tm_gif_status), hipMemcpyDeviceToHost, hs));
  TM_HIP(hipStreamSynchronize(hs));
  return TM_OK;
}

int tm_gif_decode_host(const void *file, size_t size, int first, int count, int background, uint32_t *out, int64_t frame_px, int32_t *status) {
  gif::GifInfo info;
  TM_TRY(gif::check_decode("tm_gif_decode_host", file, size, first, count, background, out, frame_px, status, &info));
  return gif::gif_decode_host((const uint8_t *)file, size, info, first, count, gif::gif_background(info, background), out, frame_px, status, 1);
}

int tm_stage_gif_decode(const void *file, size_t size, int first, int count, int background, uint32_t *dev_out, int64_t frame_px, int32_t *status, void *stream) {
  gif::GifInfo info;
  TM_TRY(gif::check_decode("tm_stage_gif_decode", file, size, first, count, background, dev_out, frame_px, status, &info));
  knobs_reload();
  TM_TRY(require_device());
  return gif::gif_decode_device((const uint8_t *)file, size, info, first, count, gif::gif_background(info, background), dev_out, frame_px, status, knobs().input_chunk_frames,
                                stream, nullptr);
}

}  // extern "C"
