// tm_input.hip -- Load's input: where the clip comes from when it is not pushed in as RGB32 -- a Y4M file, a YUV clip lent in memory
// (tm_set_frames_yuv), a numbered PNG sequence, a .gtm stream -- and the API around it (tm_open_input, tm_set_frames_yuv, tm_get_video,
// tm_set_input_yuv).  What a name turns out to be: tm_input_probe.hip; planes of Y, U, V into RGB32: tm_yuv_in.hip; shared: tm_input.h.
//
// The reference opens "any file" through FFmpeg (extern.pas:780-781, 837-840), which does not exist here (DESIGN.md sections 9 and 17):
// Y4M is the uncompressed container every FFmpeg build writes.
#include <fcntl.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "tm_encoder.h"
#include "tm_inflate.h"
#include "tm_gif.h"
#include "tm_jpeg.h"

// fn(i) for i in [0, n) on up to IN_READERS host threads (the calling one included); the first failure's code and message come back.
// Reading a file that the page cache holds is a copy the memory system bounds, not one core: a single reader brought the 0.41 GB of the
// 720p x 300 clip in at 8 GB/s (50 ms, against 20 ms for the whole Load of the same clip lent as RGB32).
constexpr int IN_READERS = 8;
static int parallel_for(int n, const std::function<int(int)> &fn) {
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

// Frames [a, b) through the encoder's two staging buffers, `fb` staged bytes per frame: a chunk of frames is brought into a device buffer on
// the copy stream and converted on the main stream, so that a chunk's transfer runs beside the conversion of the one before.  fill_host(f0,
// nf, dst) puts the chunk into page-locked memory, from where it is uploaded in one copy (a file, pageable memory); without it copy_in(f0,
// nf, dst, stream) queues the copies into the device buffer itself (page-locked memory, another device).  convert(base, f0, nf) launches.
struct StagedSource {
  size_t fb = 0;
  std::function<int(int, int, uint8_t *)> fill_host;
  std::function<int(int, int, uint8_t *, hipStream_t)> copy_in;
  std::function<int(const uint8_t *, int, int)> convert;
};
static int convert_staged(tm_encoder *e, int a, int b, const StagedSource &src) {
  const size_t fb = src.fb;
  const size_t per_chunk = knobs().input_chunk_frames > 0 ? (size_t)knobs().input_chunk_frames : ((size_t)16 << 20) / fb;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)(b - a), per_chunk));
  PinnedBuf *host = e->input_pinned;  // (kept between Loads: page-locking 32 MB costs more than reading them)
  DevBuf dev[2];
  StagingRing ring;
  TM_TRY(ring.make());
  for (int i = 0; i < 2; i++) {
    if (src.fill_host) TM_TRY(host[i].alloc(fb * chunk));
    TM_TRY(dev[i].alloc(fb * chunk));
  }
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  int c = 0;
  for (int f0 = a; f0 < b; f0 += chunk, c++) {
    const int nf = std::min(chunk, b - f0), s = c & 1;
    if (src.fill_host) {
      TM_TRY(ring.host_free(s));
      TM_TRY(src.fill_host(f0, nf, (uint8_t *)host[s].p));
    }
    TM_TRY(ring.device_free(s, e->copy_stream));
    if (src.fill_host) TM_HIP(hipMemcpyAsync(dev[s].p, host[s].p, fb * nf, hipMemcpyHostToDevice, e->copy_stream));
    else TM_TRY(src.copy_in(f0, nf, dev[s].as<uint8_t>(), e->copy_stream));
    TM_TRY(ring.uploaded(s, e->copy_stream, e->stream));
    TM_TRY(src.convert(dev[s].as<uint8_t>(), f0, nf));
    TM_TRY(ring.worked(s, e->stream));
  }
  TM_HIP(hipStreamSynchronize(e->stream));  // the staging buffers go back to the pool and to the host
  return TM_OK;
}

// frames [a, b) of the Y4M clip into the encoder's device clip: the chunks are read into the page-locked buffers by several threads
static int decode_y4m(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  InputTables &tables = e->input_tables;
  TM_TRY(build_input_tables(in.src_w, in.src_h, in.chroma, e->width, e->height, &tables, e->stream));
  const int fd = open(in.name.c_str(), O_RDONLY);
  TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", in.name.c_str());
  FdCloser closer{fd};
  ChromaGeom g;
  TM_TRY(chroma_geom(in.chroma, in.src_w, in.src_h, &g));
  const size_t fb = (size_t)in.frame_bytes, out_fb = (size_t)e->width * e->height * 4;
  const int64_t y_plane = (int64_t)in.src_w * in.src_h, c_plane = (int64_t)g.cw * g.ch;
  const int64_t strides[6] = {in.src_w, (int64_t)fb, g.cw, (int64_t)fb, g.cw, (int64_t)fb};
  const int mode = resolve_yuv_mode(e->input_yuv, in.full_range);
  StagedSource src;
  src.fb = fb;
  src.fill_host = [&](int f0, int nf, uint8_t *host) -> int {
    return parallel_for(nf, [&](int i) -> int {
      TM_CHECK(pread_all(fd, host + fb * i, fb, in.frame_off[(size_t)(in.start + f0 + i)]) == 0, TM_E_IO, "%s: cannot read frame %d", in.name.c_str(), in.start + f0 + i);
      return (int)TM_OK;
    });
  };
  src.convert = [&](const uint8_t *base, int f0, int nf) -> int {
    return launch_yuv_to_rgb32(tables, base, base + y_plane, base + y_plane + c_plane, strides, SampleFmt(), nf, mode, e->frames_owned.as<uint8_t>() + out_fb * f0, e->stream);
  };
  return convert_staged(e, a, b, src);
}

// rows x row_bytes of nf frames from a plane with strides into a packed one, as few copies as the strides allow
static int copy_plane_async(uint8_t *dst, const uint8_t *src, int64_t row_stride, int64_t frame_stride, int64_t row_bytes, int rows, int nf, hipStream_t stream) {
  if (row_stride == row_bytes && frame_stride == row_bytes * rows) {
    TM_HIP(hipMemcpyAsync(dst, src, (size_t)(row_bytes * rows) * nf, hipMemcpyDefault, stream));
  } else if (frame_stride == row_stride * rows) {
    TM_HIP(hipMemcpy2DAsync(dst, (size_t)row_bytes, src, (size_t)row_stride, (size_t)row_bytes, (size_t)rows * nf, hipMemcpyDefault, stream));
  } else {
    for (int f = 0; f < nf; f++)
      TM_HIP(hipMemcpy2DAsync(dst + row_bytes * rows * f, (size_t)row_bytes, src + frame_stride * f, (size_t)row_stride, (size_t)row_bytes, (size_t)rows, hipMemcpyDefault, stream));
  }
  return TM_OK;
}

static bool is_page_locked(const void *p) {
  hipPointerAttribute_t at;
  const bool yes = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // (pageable memory is an error to some runtimes and "unregistered" to others)
  return yes;
}

// frames [a, b) of the lent clip into the encoder's device clip
static int convert_yuv_clip(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  const tm_yuv_clip &c = in.clip;
  ClipPlanes pl;
  TM_TRY(check_yuv_clip(&c, &pl));
  InputTables &tables = e->input_tables;
  TM_TRY(build_input_tables(c.width, c.height, c.chroma, e->width, e->height, &tables, e->stream));
  const int mode = resolve_yuv_mode(e->input_yuv, c.full_range);
  const size_t out_fb = (size_t)e->width * e->height * 4;
  const uint8_t *ptr[3] = {(const uint8_t *)c.y, (const uint8_t *)c.u, (const uint8_t *)c.v};
  const int64_t row[3] = {c.y_row, c.u_row, c.v_row}, frame[3] = {c.y_frame, c.u_frame, c.v_frame};
  bool in_place = false;
  if (c.memory == TM_MEM_DEVICE) {
    hipPointerAttribute_t at;
    TM_CHECK(hipPointerGetAttributes(&at, c.y) == hipSuccess && at.type == hipMemoryTypeDevice, TM_E_INVAL, "yuv clip: the y plane is not device memory");
    in_place = at.device == e->device;
  }
  if (in_place) {  // the planes are converted where they are
    constexpr int IN_LAUNCH_FRAMES = 4096;
    const int64_t strides[6] = {row[0], frame[0], row[1], frame[1], row[2], frame[2]};
    for (int f0 = a; f0 < b; f0 += IN_LAUNCH_FRAMES) {
      const int nf = std::min(IN_LAUNCH_FRAMES, b - f0);
      TM_TRY(launch_yuv_to_rgb32(tables, ptr[0] + frame[0] * f0, ptr[1] ? ptr[1] + frame[1] * f0 : nullptr, ptr[2] ? ptr[2] + frame[2] * f0 : nullptr, strides, pl.fmt, nf,
                                 mode, e->frames_owned.as<uint8_t>() + out_fb * f0, e->stream));
    }
    TM_HIP(hipStreamSynchronize(e->stream));  // the planes are the caller's again when Load returns
    return TM_OK;
  }
  // Staged: a chunk holds nf packed frames of Y, then of U (or of the pairs), then of V
  int64_t plane_bytes[3], fb = 0;
  for (int i = 0; i < pl.nplanes; i++) { plane_bytes[i] = pl.row_bytes[i] * pl.rows[i]; fb += plane_bytes[i]; }
  bool pinned = c.memory == TM_MEM_DEVICE;  // (another device of the group: copied by the runtime as page-locked memory is)
  if (!pinned) {
    pinned = true;
    for (int i = 0; i < pl.nplanes; i++) pinned = pinned && is_page_locked(ptr[i]);
  }
  StagedSource src;
  src.fb = (size_t)fb;
  if (pinned)
    src.copy_in = [&](int f0, int nf, uint8_t *dst, hipStream_t stream) -> int {
      for (int i = 0; i < pl.nplanes; i++) {
        TM_TRY(copy_plane_async(dst, ptr[i] + frame[i] * f0, row[i], frame[i], pl.row_bytes[i], pl.rows[i], nf, stream));
        dst += plane_bytes[i] * nf;
      }
      return (int)TM_OK;
    };
  else
    src.fill_host = [&](int f0, int nf, uint8_t *host) -> int {
      return parallel_for(nf, [&](int f) -> int {
        uint8_t *base = host;
        for (int i = 0; i < pl.nplanes; i++) {
          uint8_t *dst = base + plane_bytes[i] * f;
          const uint8_t *from = ptr[i] + frame[i] * (f0 + f);
          if (row[i] == pl.row_bytes[i]) memcpy(dst, from, (size_t)plane_bytes[i]);
          else
            for (int r = 0; r < pl.rows[i]; r++) memcpy(dst + pl.row_bytes[i] * r, from + row[i] * r, (size_t)pl.row_bytes[i]);
          base += plane_bytes[i] * nf;
        }
        return (int)TM_OK;
      });
    };
  src.convert = [&](const uint8_t *base, int f0, int nf) -> int {
    const uint8_t *u = base + plane_bytes[0] * nf, *v = pl.nplanes == 3 ? u + plane_bytes[1] * nf : nullptr;
    const int64_t strides[6] = {pl.row_bytes[0], plane_bytes[0], pl.row_bytes[1], plane_bytes[1], pl.row_bytes[2], plane_bytes[2]};
    return launch_yuv_to_rgb32(tables, base, u, v, strides, pl.fmt, nf, mode, e->frames_owned.as<uint8_t>() + out_fb * f0, e->stream);
  };
  return convert_staged(e, a, b, src);
}

// frames [a, b) of the lent RGB clip into the encoder's device clip (convert_yuv_clip's twin)
static int convert_rgb_clip(tm_encoder *e, int a, int b) {
  const tm_rgb_clip &c = e->input.rgb_clip;
  RgbPlan pl;
  TM_TRY(check_rgb_clip(&c, &pl));
  const ScaleTables *tables = nullptr;
  if (e->width != c.width || e->height != c.height) {
    TM_TRY(e->rgb_in_tables.prepare(c.width, c.height, e->width, e->height, TM_SCALE_LANCZOS3));
    TM_TRY(e->rgb_in_tables.upload(e->stream));
    tables = &e->rgb_in_tables;
  }
  uint8_t *const out = e->frames_owned.as<uint8_t>();
  const size_t out_fb = (size_t)e->width * e->height * 4;
  const uint8_t *const ptr[3] = {(const uint8_t *)c.r, (const uint8_t *)c.g, (const uint8_t *)c.b};
  // the planes a chunk is staged as: the pixels from the lowest pointer on, or every distinct channel pointer; which plane a channel reads
  int nplanes = 0, plane_of[3] = {0, 0, 0};
  const uint8_t *plane[3] = {nullptr, nullptr, nullptr};
  if (pl.interleaved) { plane[nplanes++] = pl.base; }
  else
    for (int i = 0; i < 3; i++) {
      int j = 0;
      while (j < nplanes && plane[j] != ptr[i]) j++;
      if (j == nplanes) plane[nplanes++] = ptr[i];
      plane_of[i] = j;
    }
  bool in_place = false;
  if (c.memory == TM_MEM_DEVICE) {
    for (int i = 0; i < nplanes; i++) {
      hipPointerAttribute_t at;
      TM_CHECK(hipPointerGetAttributes(&at, plane[i]) == hipSuccess && at.type == hipMemoryTypeDevice, TM_E_INVAL, "rgb clip: a channel pointer is not device memory");
      if (i == 0) in_place = at.device == e->device;
    }
  }
  if (in_place) {  // the clip is converted where it is
    tm_rgb_clip part = c;
    part.r = ptr[0] + c.frame * a; part.g = ptr[1] + c.frame * a; part.b = ptr[2] + c.frame * a;
    RgbPlan pp = pl;
    pp.base = pl.base + c.frame * a;
    TM_TRY(launch_rgb_to_rgb32(part, pp, tables, b - a, e->width, e->height, out + out_fb * a, e->stream));
    TM_HIP(hipStreamSynchronize(e->stream));  // the clip is the caller's again when Load returns
    return TM_OK;
  }
  // Staged: a chunk holds nf frames of the first plane, then of the second, then of the third; steps and offsets stay as they are.
  // Rows that are all but dense (alpha or padding bytes, at most 1/16 of the row) keep their stride: a frame -- a whole chunk, where the
  // frames follow one another -- then travels as one linear copy from its first described byte to its last, and no byte behind that is
  // read.  (As a 2-D copy of 5119 of every 5120 bytes the 720p x 300 BGRA clip took 2.2 s to stage instead of 21 ms.)  Other rows are packed.
  const int64_t row_bytes = pl.interleaved ? pl.pixel_row_bytes : pl.sample_row_bytes;
  const bool keep_rows = (c.row - row_bytes) * 16 <= c.row, keep_frames = keep_rows && c.frame == c.row * c.height;
  const int64_t srow = keep_rows ? c.row : row_bytes, plane_bytes = srow * c.height, frame_bytes = srow * (c.height - 1) + row_bytes;  // frame_bytes: first to last described byte
  bool pinned = c.memory == TM_MEM_DEVICE;  // (another device of the group: copied by the runtime as page-locked memory is)
  if (!pinned) {
    pinned = true;
    for (int i = 0; i < nplanes; i++) pinned = pinned && is_page_locked(plane[i]);
  }
  StagedSource src;
  src.fb = (size_t)(plane_bytes * nplanes);
  if (pinned)
    src.copy_in = [&](int f0, int nf, uint8_t *dst, hipStream_t stream) -> int {
      for (int i = 0; i < nplanes; i++) {
        uint8_t *to = dst + plane_bytes * nf * i;
        const uint8_t *from = plane[i] + c.frame * f0;
        if (keep_frames) TM_HIP(hipMemcpyAsync(to, from, (size_t)(plane_bytes * (nf - 1) + frame_bytes), hipMemcpyDefault, stream));
        else if (keep_rows)
          for (int f = 0; f < nf; f++) TM_HIP(hipMemcpyAsync(to + plane_bytes * f, from + c.frame * f, (size_t)frame_bytes, hipMemcpyDefault, stream));
        else TM_TRY(copy_plane_async(to, from, c.row, c.frame, row_bytes, c.height, nf, stream));
      }
      return (int)TM_OK;
    };
  else
    src.fill_host = [&](int f0, int nf, uint8_t *host) -> int {
      return parallel_for(nf, [&](int f) -> int {
        for (int i = 0; i < nplanes; i++) {
          uint8_t *dst = host + plane_bytes * nf * i + plane_bytes * f;
          const uint8_t *from = plane[i] + c.frame * (f0 + f);
          if (keep_rows) memcpy(dst, from, (size_t)frame_bytes);
          else
            for (int r = 0; r < c.height; r++) memcpy(dst + row_bytes * r, from + c.row * r, (size_t)row_bytes);
        }
        return (int)TM_OK;
      });
    };
  src.convert = [&](const uint8_t *base, int f0, int nf) -> int {
    tm_rgb_clip part = c;
    RgbPlan pp = pl;
    const uint8_t *ch[3];
    for (int i = 0; i < 3; i++) ch[i] = pl.interleaved ? base + pl.off[i] : base + plane_bytes * nf * plane_of[i];
    part.r = ch[0]; part.g = ch[1]; part.b = ch[2];
    part.row = srow; part.frame = plane_bytes; part.frames = nf; part.memory = TM_MEM_DEVICE;
    pp.base = base;
    return launch_rgb_to_rgb32(part, pp, tables, nf, e->width, e->height, out + out_fb * f0, e->stream);
  };
  return convert_staged(e, a, b, src);
}

namespace tmx { int decode_png(const uint8_t *file, size_t n, const char *name, uint32_t *out, int64_t cap_px, int *w_out, int *h_out); }  // tm_png.hip

static bool png_kind(int kind) { return kind == TM_INPUT_PNGS || kind == INPUT_PNG_CLIP; }
// where a PNG input is decoded: TM_PNG_DECODE, else what tm_set_png_decode said.  AUTO is the device (0.33 s against
// 0.93 s for the 720p x 300 clip), and the host for pictures whose rows the kernels' 32-bit positions cannot hold
static int png_decode_where(const tm_encoder *e) {
  const int w = knobs().png_decode ? knobs().png_decode : e->png_decode;
  if (w != TM_PNG_DECODE_AUTO) return w;
  return ((uint64_t)e->width * 4 + 1) * (uint64_t)e->height < ((uint64_t)1 << 32) ? TM_PNG_DECODE_DEVICE : TM_PNG_DECODE_HOST;
}
static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// the PNG sequence, or the lent PNG files, decoded on the host into a clip the encoder keeps until Load's chunked host-clip upload has taken it
static int decode_pngs(tm_encoder *e) {
  InputInfo &in = e->input;
  const size_t px = (size_t)e->width * e->height;
  e->input_clip.resize(px * e->nframes);
  std::atomic<int64_t> file_bytes{0};
  const int rc = parallel_for(e->nframes, [&](int i) -> int {  // (frames are files of their own: inflate is the time, and it is one core's per file)
    int w = 0, h = 0;
    if (in.kind == INPUT_PNG_CLIP) {
      char name[32];
      snprintf(name, sizeof(name), "frame %d", i);
      const uint8_t *file = (const uint8_t *)in.png_files[(size_t)i];
      const size_t n = in.png_sizes[(size_t)i];
      TM_TRY(decode_png(file, n, name, nullptr, 0, &w, &h));
      TM_CHECK(w == e->width && h == e->height, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", name, w, h, e->width, e->height);
      file_bytes += (int64_t)n;
      return decode_png(file, n, name, e->input_clip.data() + px * i, (int64_t)px, &w, &h);
    }
    std::string path;
    TM_TRY(format_pattern(in.name, (int64_t)in.start + i, &path));
    TM_TRY(read_png(path.c_str(), nullptr, 0, &w, &h));
    TM_CHECK(w == e->width && h == e->height, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", path.c_str(), w, h, e->width, e->height);
    struct stat sb;
    if (stat(path.c_str(), &sb) == 0) file_bytes += (int64_t)sb.st_size;
    return read_png(path.c_str(), e->input_clip.data() + px * i, (int64_t)px, &w, &h);
  });
  e->input_stats.file_bytes = file_bytes.load();
  return rc;
}

// Frames [a, b) of the PNG sequence, or of the lent files, decoded on the device into the encoder's clip.  A chunk of
// files is read into a page-locked buffer (the reader threads; each walks its file's chunks and checks what decode_png checks before the
// stream), the descriptor of the chunk is written behind the files, and both go up in one copy on the copy stream; k_inflate and
// k_png_unfilter run on the main stream while the next chunk is read.  What only decoding finds comes back as a status per frame.
static int decode_pngs_device(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  tm_input_stats &stats = e->input_stats;
  const bool lent = in.kind == INPUT_PNG_CLIP;
  const int n = b - a, w = e->width, h = e->height;
  std::vector<std::string> names((size_t)n);
  std::vector<size_t> sizes((size_t)n);
  for (int i = 0; i < n; i++) {
    if (lent) {
      names[(size_t)i] = "frame " + std::to_string(a + i);
      sizes[(size_t)i] = in.png_sizes[(size_t)(a + i)];
    } else {
      TM_TRY(format_pattern(in.name, (int64_t)in.start + a + i, &names[(size_t)i]));
      struct stat sb;
      TM_CHECK(stat(names[(size_t)i].c_str(), &sb) == 0, TM_E_IO, "cannot open %s", names[(size_t)i].c_str());
      sizes[(size_t)i] = (size_t)sb.st_size;
    }
    stats.file_bytes += (int64_t)sizes[(size_t)i];
  }
  // A stream is one wave's work from end to end, so a chunk should hold as many frames as the device has room for waves (four to a compute
  // unit): as many as 2 GiB of inflated rows and 512 MiB of files allow.  The 720p x 300 clip is one chunk; in chunks of 32 frames its
  // Load took 2.8 s, one launch of 32 waves after the other.
  const size_t raw_frame = (((size_t)w * 4 + 1) * (size_t)h + 15) & ~(size_t)15, out_fb = (size_t)w * h * 4;
  size_t largest = 16;
  for (size_t sz : sizes) largest = std::max(largest, (sz + 15) & ~(size_t)15);
  const size_t by_room = std::max<size_t>(1, std::min(((size_t)2 << 30) / raw_frame, ((size_t)512 << 20) / largest));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, knobs().input_chunk_frames > 0 ? (size_t)knobs().input_chunk_frames : by_room));
  size_t cap = 0;  // a chunk's files, each on 16 bytes, and the most its descriptor can take (a span per 12 bytes of file at the worst)
  for (int f0 = 0; f0 < n; f0 += chunk) {
    size_t files = 0;
    const int nf = std::min(chunk, n - f0);
    for (int i = 0; i < nf; i++) files += (sizes[(size_t)(f0 + i)] + 15) & ~(size_t)15;
    cap = std::max(cap, files + (size_t)nf * (sizeof(inf::Stream) + sizeof(inf::Picture) + 768) + (files / 12 + (size_t)nf) * sizeof(inf::Span) + 64);
  }
  TM_CHECK(cap < ((size_t)1 << 32), TM_E_UNSUPPORTED, "a chunk of %d PNG files takes %zu bytes (below 4 GiB: lower TM_INPUT_CHUNK_FRAMES)", chunk, cap);
  PinnedBuf *host = e->input_pinned;
  DevBuf dev[2], raw, inflated, status;
  StagingRing ring;
  TM_TRY(ring.make());
  for (int i = 0; i < (n > chunk ? 2 : 1); i++) { TM_TRY(host[i].alloc(cap)); TM_TRY(dev[i].alloc(cap)); }
  TM_TRY(raw.alloc(raw_frame * chunk)); TM_TRY(inflated.alloc((size_t)n * sizeof(tm_inflate_status))); TM_TRY(status.alloc((size_t)n * 4));
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  inf::PngBatch batch[2];
  std::vector<inf::PngInfo> infos((size_t)chunk);
  std::vector<size_t> at((size_t)chunk);
  int c = 0;
  for (int f0 = 0; f0 < n; f0 += chunk, c++) {
    const int nf = std::min(chunk, n - f0), s = c & 1;
    TM_TRY(ring.host_free(s));
    const auto t0 = std::chrono::steady_clock::now();
    size_t files = 0;
    for (int i = 0; i < nf; i++) { at[(size_t)i] = files; files += (sizes[(size_t)(f0 + i)] + 15) & ~(size_t)15; }
    uint8_t *hb = (uint8_t *)host[s].p;
    TM_TRY(parallel_for(nf, [&](int i) -> int {
      const std::string &name = names[(size_t)(f0 + i)];
      const size_t sz = sizes[(size_t)(f0 + i)];
      uint8_t *to = hb + at[(size_t)i];
      if (lent) memcpy(to, in.png_files[(size_t)(a + f0 + i)], sz);
      else {
        const int fd = open(name.c_str(), O_RDONLY);
        TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", name.c_str());
        FdCloser closer{fd};
        TM_CHECK(pread_all(fd, to, sz, 0) == 0, TM_E_IO, "cannot read %s", name.c_str());
      }
      TM_TRY(inf::parse_png(to, sz, name.c_str(), &infos[(size_t)i]));
      return inf::png_check_decodable(infos[(size_t)i], name.c_str(), w, h);
    }));
    batch[s].clear();
    for (int i = 0; i < nf; i++) batch[s].add(infos[(size_t)i], at[(size_t)i]);
    TM_CHECK(files + batch[s].desc_bytes() <= cap, TM_E_INVAL, "a PNG file changed while it was being read");
    const size_t used = files + batch[s].write_desc(hb + files);
    stats.ms_read += ms_since(t0);
    stats.bytes_uploaded += (int64_t)used;
    TM_TRY(ring.device_free(s, e->copy_stream));
    TM_HIP(hipMemcpyAsync(dev[s].p, hb, used, hipMemcpyHostToDevice, e->copy_stream));
    TM_TRY(ring.uploaded(s, e->copy_stream, e->stream));
    TM_TRY(inf::png_batch_launch(batch[s], dev[s].as<uint8_t>(), used, files, raw.as<uint8_t>(), inflated.as<tm_inflate_status>() + f0, w, h,
                                 reinterpret_cast<uint32_t *>(e->frames_owned.as<uint8_t>() + out_fb * (size_t)(a + f0)), (int64_t)w * h, status.as<int32_t>() + f0, e->stream));
    TM_TRY(ring.worked(s, e->stream));
  }
  std::vector<int32_t> st((size_t)n);
  TM_HIP(hipMemcpyAsync(st.data(), status.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));  // the staging buffers go back to the pool and to the host
  for (int i = 0; i < n; i++) TM_TRY(inf::png_status_error(st[(size_t)i], names[(size_t)i].c_str()));
  return TM_OK;
}

static bool jpeg_kind(int kind) { return kind == TM_INPUT_JPEGS || kind == INPUT_JPEG_CLIP; }
// where a JPEG input is decoded: TM_JPEG_DECODE, else what tm_set_jpeg_decode said.  AUTO goes by the first file:
// a file's segments are the lanes it keeps busy.  The 720p x 300 clip on the device against the host's reader threads: 227 ms against
// 138 ms with one segment a file, 150 against 142 with two, 96 against 142 with four, 26 against 139 with 45.  Three were not measured
// and stay with the host.
constexpr int JPEG_AUTO_DEVICE_SEGMENTS = 4;
static int jpeg_decode_where(const tm_encoder *e) {
  const int w = knobs().jpeg_decode ? knobs().jpeg_decode : e->jpeg_decode;
  if (w != TM_PNG_DECODE_AUTO) return w;
  return e->input.jpeg_segments >= JPEG_AUTO_DEVICE_SEGMENTS ? TM_PNG_DECODE_DEVICE : TM_PNG_DECODE_HOST;
}

// Frames [a, b) of the JPEG sequence, or of the lent files, into the encoder's clip.  The reader threads bring a
// chunk's files into memory and walk them.  DEVICE: the files lie in the page-locked buffer, the chunk's descriptor is written behind
// them, both go up in one copy on the copy stream and k_jpeg_decode writes the chunk's planes.  HOST: the reader threads decode with the
// host form into the page-locked buffer and the planes go up.  Either way the planes -- MCU-padded, with the true size and a row stride
// handed on -- are converted by k_yuv_to_rgb32 on the main stream while the next chunk is read.
static int decode_jpegs(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  tm_input_stats &stats = e->input_stats;
  const bool lent = in.kind == INPUT_JPEG_CLIP, on_device = jpeg_decode_where(e) == TM_PNG_DECODE_DEVICE;
  const int n = b - a, w = e->width, h = e->height, layout = in.chroma;
  std::vector<std::string> names((size_t)n);
  std::vector<size_t> sizes((size_t)n);
  for (int i = 0; i < n; i++) {
    if (lent) {
      names[(size_t)i] = "frame " + std::to_string(a + i);
      sizes[(size_t)i] = in.png_sizes[(size_t)(a + i)];
    } else {
      TM_TRY(format_pattern(in.name, (int64_t)in.start + a + i, &names[(size_t)i]));
      struct stat sb;
      TM_CHECK(stat(names[(size_t)i].c_str(), &sb) == 0, TM_E_IO, "cannot open %s", names[(size_t)i].c_str());
      sizes[(size_t)i] = (size_t)sb.st_size;
    }
    stats.file_bytes += (int64_t)sizes[(size_t)i];
  }
  InputTables &tables = e->input_tables;
  TM_TRY(build_input_tables(w, h, layout, w, h, &tables, e->stream));
  const int mode = resolve_yuv_mode(e->input_yuv, in.full_range);
  // the planes of a frame, whole MCUs: an MCU is 8 hs x 8 vs luma samples (8 x 8 for a single component)
  const bool mono = layout == TM_CHROMA_MONO;
  const uint32_t hs = (mono || layout == TM_CHROMA_444) ? 1 : 2, vs = layout == TM_CHROMA_420JPEG ? 2 : 1;
  const uint32_t ypw = ((uint32_t)w + 8 * hs - 1) / (8 * hs) * (8 * hs), yph = ((uint32_t)h + 8 * vs - 1) / (8 * vs) * (8 * vs);
  const uint32_t cpw = mono ? 0 : ypw / hs, cph = mono ? 0 : yph / vs;
  const size_t yb = (size_t)ypw * yph, cb = (size_t)cpw * cph, fb = yb + 2 * cb, out_fb = (size_t)w * h * 4;
  const size_t mcus = (size_t)(ypw / (8 * hs)) * (yph / (8 * vs));
  // A file without restart markers is one lane's work from end to end, so a chunk should hold as many frames as the device has room for
  // (the PNG path's rule): as many as 1 GiB of planes and 512 MiB of files allow.
  size_t largest = 16;
  for (size_t sz : sizes) largest = std::max(largest, (sz + 15) & ~(size_t)15);
  const size_t by_room = std::max<size_t>(1, std::min(((size_t)1 << 30) / fb, ((size_t)512 << 20) / largest));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, knobs().input_chunk_frames > 0 ? (size_t)knobs().input_chunk_frames : by_room));
  size_t cap = fb * (size_t)chunk;  // HOST: a chunk's planes.  DEVICE: its files, each on 16 bytes, and the most its descriptor can take (a segment per MCU)
  if (on_device) {
    cap = 0;
    for (int f0 = 0; f0 < n; f0 += chunk) {
      size_t files = 0;
      const int nf = std::min(chunk, n - f0);
      for (int i = 0; i < nf; i++) files += (sizes[(size_t)(f0 + i)] + 15) & ~(size_t)15;
      cap = std::max(cap, files + (size_t)nf * (sizeof(jpg::Frame) + sizeof(jpg::TableSet) + mcus * sizeof(jpg::Seg)) + 64);
    }
    TM_CHECK(cap < ((size_t)1 << 32), TM_E_UNSUPPORTED, "a chunk of %d JPEG files takes %zu bytes (below 4 GiB: lower TM_INPUT_CHUNK_FRAMES)", chunk, cap);
  }
  PinnedBuf *host = e->input_pinned;
  DevBuf dev[2], planes, status;
  StagingRing ring;
  TM_TRY(ring.make());
  for (int i = 0; i < (n > chunk ? 2 : 1); i++) { TM_TRY(host[i].alloc(cap)); TM_TRY(dev[i].alloc(cap)); }
  if (on_device) { TM_TRY(planes.alloc(fb * (size_t)chunk)); TM_TRY(status.alloc((size_t)n * 4)); }
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  jpg::JpegBatch batch[2];
  std::vector<jpg::JpegInfo> infos((size_t)chunk);
  std::vector<size_t> at((size_t)chunk);
  auto layout_of = [&](int i) {  // frame i of a chunk: its offset in the Y planes, in the U planes, in the V planes
    jpg::PlaneLayout pl;
    pl.off[0] = yb * (size_t)i; pl.stride[0] = ypw; pl.w[0] = ypw; pl.h[0] = yph;
    for (int c = 1; c < (mono ? 1 : 3); c++) { pl.off[c] = cb * (size_t)i; pl.stride[c] = cpw; pl.w[c] = cpw; pl.h[c] = cph; }
    return pl;
  };
  auto check_like_first = [&](const jpg::JpegInfo &info, const std::string &name) -> int {
    TM_CHECK(info.w == w && info.h == h, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", name.c_str(), info.w, info.h, w, h);
    TM_CHECK(info.layout() == layout, TM_E_INVAL, "%s has %d component(s) sampled %dx%d, which is not the sampling of the sequence's first frame", name.c_str(), info.ncomp,
             info.hs, info.vs);
    return (int)TM_OK;
  };
  int c = 0;
  for (int f0 = 0; f0 < n; f0 += chunk, c++) {
    const int nf = std::min(chunk, n - f0), s = c & 1;
    TM_TRY(ring.host_free(s));
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *hb = (uint8_t *)host[s].p;
    size_t used = 0, files = 0;
    if (on_device) {
      for (int i = 0; i < nf; i++) { at[(size_t)i] = files; files += (sizes[(size_t)(f0 + i)] + 15) & ~(size_t)15; }
      TM_TRY(parallel_for(nf, [&](int i) -> int {
        const std::string &name = names[(size_t)(f0 + i)];
        const size_t sz = sizes[(size_t)(f0 + i)];
        uint8_t *to = hb + at[(size_t)i];
        if (lent) memcpy(to, in.png_files[(size_t)(a + f0 + i)], sz);
        else {
          const int fd = open(name.c_str(), O_RDONLY);
          TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", name.c_str());
          FdCloser closer{fd};
          TM_CHECK(pread_all(fd, to, sz, 0) == 0, TM_E_IO, "cannot read %s", name.c_str());
        }
        TM_TRY(jpg::parse_jpeg(to, sz, name.c_str(), &infos[(size_t)i]));
        return check_like_first(infos[(size_t)i], name);
      }));
      batch[s].clear();
      for (int i = 0; i < nf; i++) batch[s].add(infos[(size_t)i], at[(size_t)i], layout_of(i));
      TM_CHECK(files + batch[s].desc_bytes() <= cap, TM_E_INVAL, "a JPEG file changed while it was being read");
      used = files + batch[s].write_desc(hb + files);
    } else {
      uint8_t *const pl3[3] = {hb, hb + yb * (size_t)nf, hb + (yb + cb) * (size_t)nf};
      TM_TRY(parallel_for(nf, [&](int i) -> int {
        const std::string &name = names[(size_t)(f0 + i)];
        const size_t sz = sizes[(size_t)(f0 + i)];
        std::vector<uint8_t> mine;
        const uint8_t *file = lent ? (const uint8_t *)in.png_files[(size_t)(a + f0 + i)] : nullptr;
        if (!lent) {
          mine.resize(sz);
          const int fd = open(name.c_str(), O_RDONLY);
          TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", name.c_str());
          FdCloser closer{fd};
          TM_CHECK(pread_all(fd, mine.data(), sz, 0) == 0, TM_E_IO, "cannot read %s", name.c_str());
          file = mine.data();
        }
        jpg::JpegInfo info;
        TM_TRY(jpg::parse_jpeg(file, sz, name.c_str(), &info));
        TM_TRY(check_like_first(info, name));
        return jpg::jpeg_status_error(jpg::jpeg_decode_one_host(info, file, sz, layout_of(i), pl3), name.c_str());
      }));
      used = fb * (size_t)nf;
    }
    stats.ms_read += ms_since(t0);
    stats.bytes_uploaded += (int64_t)used;
    TM_TRY(ring.device_free(s, e->copy_stream));
    TM_HIP(hipMemcpyAsync(dev[s].p, hb, used, hipMemcpyHostToDevice, e->copy_stream));
    TM_TRY(ring.uploaded(s, e->copy_stream, e->stream));
    uint8_t *py = on_device ? planes.as<uint8_t>() : dev[s].as<uint8_t>();
    uint8_t *pu = mono ? nullptr : py + yb * (size_t)nf, *pv = mono ? nullptr : pu + cb * (size_t)nf;
    if (on_device) {
      const uint64_t plane_bytes[3] = {yb * (uint64_t)nf, cb * (uint64_t)nf, cb * (uint64_t)nf};
      TM_TRY(jpg::jpeg_batch_launch(batch[s], dev[s].as<uint8_t>(), used, files, py, pu, pv, plane_bytes, status.as<int32_t>() + f0, e->stream));
    }
    const int64_t strides[6] = {(int64_t)ypw, (int64_t)yb, (int64_t)cpw, (int64_t)cb, (int64_t)cpw, (int64_t)cb};
    TM_TRY(launch_yuv_to_rgb32(tables, py, pu, pv, strides, SampleFmt(), nf, mode, e->frames_owned.as<uint8_t>() + out_fb * (size_t)(a + f0), e->stream));
    TM_TRY(ring.worked(s, e->stream));
  }
  std::vector<int32_t> st((size_t)n, 0);
  if (on_device) TM_HIP(hipMemcpyAsync(st.data(), status.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));  // the staging buffers go back to the pool and to the host
  for (int i = 0; i < n; i++) TM_TRY(jpg::jpeg_status_error(st[(size_t)i], names[(size_t)i].c_str()));
  return TM_OK;
}

static bool gif_kind(int kind) { return kind == TM_INPUT_GIF || kind == INPUT_GIF_CLIP; }
// where a GIF input is decoded: TM_GIF_DECODE, else what tm_set_gif_decode said.  AUTO is the device: two clips of
// 480 x 270 x 120 written by Pillow, OpenInput + Load from a memory-backed directory, median of 7 (range): the bench clip in 256 colours
// 24.4 ms (24.3 - 25.0) on the device against 32.8 ms (31.7 - 35.6) on the host's reader threads, a flat 16-colour one 2.19 ms (2.16 - 2.24)
// against 24.5 ms (24.3 - 24.7); the ranges do not meet on either.
static int gif_decode_where(const tm_encoder *e) {
  const int w = knobs().gif_decode ? knobs().gif_decode : e->gif_decode;
  return w != TM_PNG_DECODE_AUTO ? w : (int)TM_PNG_DECODE_DEVICE;
}

// Frames [a, b) of the GIF file, or of the lent one, into the encoder's clip.  A frame is what the frames before it
// left with its own rectangle drawn over it, so images 0 .. StartFrame + b - 1 are decoded and composited and [StartFrame + a, StartFrame +
// b) are delivered.  DEVICE: the file goes up once, then a descriptor, k_gif_lzw and k_gif_compose per chunk of images.  HOST: the reader
// threads run the LZW image by image, the frames are composited on this thread and uploaded.
static int decode_gif(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  tm_input_stats &stats = e->input_stats;
  const bool lent = in.kind == INPUT_GIF_CLIP, on_device = gif_decode_where(e) == TM_PNG_DECODE_DEVICE;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> mine;
  const uint8_t *file = lent ? (const uint8_t *)in.png_files[0] : nullptr;
  size_t size = lent ? in.png_sizes[0] : 0;
  const std::string name = lent ? std::string("the lent GIF") : in.name;
  if (!lent) {
    TM_TRY(read_whole(in.name, &mine));
    file = mine.data(); size = mine.size();
  }
  stats.file_bytes += (int64_t)size;
  gif::GifInfo info;
  TM_TRY(gif::parse_gif(file, size, name.c_str(), &info));
  TM_CHECK(info.w == e->width && info.h == e->height && (int64_t)in.start + b <= (int64_t)info.images.size(), TM_E_INVAL, "%s changed since it was opened", name.c_str());
  const int first = in.start + a, count = b - a;
  const int64_t frame_px = (int64_t)e->width * e->height;
  const uint32_t bg = gif::gif_background(info, e->gif_background);
  uint32_t *dev_out = e->frames_owned.as<uint32_t>() + frame_px * a;
  std::vector<int32_t> status((size_t)(first + count), 0);
  if (on_device) {
    stats.ms_read += ms_since(t0);
    TM_TRY(gif::gif_decode_device(file, size, info, first, count, bg, dev_out, frame_px, status.data(), knobs().input_chunk_frames, e->stream, &stats.bytes_uploaded));
  } else {
    std::vector<uint32_t> clip((size_t)frame_px * (size_t)count);
    TM_TRY(gif::gif_decode_host(file, size, info, first, count, bg, clip.data(), frame_px, status.data(), IN_READERS));
    stats.ms_read += ms_since(t0);
    stats.bytes_uploaded += (int64_t)clip.size() * 4;
    TM_HIP(hipMemcpyAsync(dev_out, clip.data(), clip.size() * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP(hipStreamSynchronize(e->stream));
  }
  for (int i = 0; i < first + count; i++) TM_TRY(gif::gif_status_error(status[(size_t)i], name.c_str(), i));
  return TM_OK;
}

// frames [a, b) of the .gtm stream, played straight into the encoder's device clip (the player writes frame i where frame i + 1 reads it)
static int play_gtm(tm_encoder *e, int a, int b) {
  const InputInfo &in = e->input;
  tm_player *p = nullptr;
  TM_TRY(tm_player_open(in.name.c_str(), e->device, &p));
  struct Closer { tm_player *p; ~Closer() { tm_player_close(p); } } closer{p};
  TM_TRY(tm_player_seek(p, in.start + a));
  int got = 0;
  TM_TRY(tm_player_read(p, b - a, e->frames_owned.as<uint8_t>() + (size_t)e->width * e->height * 4 * a, 1, &got));
  TM_CHECK(got == b - a, TM_E_IO, "%s: %d of %d frames played", in.name.c_str(), got, b - a);
  return TM_OK;
}

// Load's first lines when the frames come from a file or from lent YUV planes: leaves the clip where tm_set_frames_device / tm_set_frames_host would have put it
int load_from_input(tm_encoder *e) {
  InputInfo &in = e->input;
  const bool pngs = png_kind(in.kind);
  const auto t0 = std::chrono::steady_clock::now();
  if (pngs && png_decode_where(e) == TM_PNG_DECODE_HOST) {
    if (in.decoded && e->frames != nullptr) return TM_OK;  // a second Run(esLoad): the device copy of the last one
    TM_CHECK(in.kind != INPUT_PNG_CLIP || in.lent, TM_E_INVAL, "the PNG files were given back when the last Load returned: lend them again (tm_set_frames_png)");
    e->input_stats = tm_input_stats{};
    e->has_input_stats = false;
    TM_TRY(decode_pngs(e));
    e->frames = nullptr;
    e->frames_host = e->input_clip.data();
    e->hclip_cur = -1;
    in.decoded = true;
    in.lent = false;
    e->input_stats.frames = e->nframes; e->input_stats.bytes_uploaded = (int64_t)e->input_clip.size() * 4;
    e->input_stats.where = TM_PNG_DECODE_HOST; e->input_stats.kind = in.kind;
    e->input_stats.ms_read = e->input_stats.ms_wall = ms_since(t0);
    e->has_input_stats = true;
    return TM_OK;
  }
  int64_t a = 0, b = e->nframes;
  if (e->dist() && e->s.MotionPredictRadius <= 0) {  // a shard decodes what its Load reads: its frames and the one before them
    share_of(e->nframes, e->co.rank, e->co.world, &a, &b);
    a = std::max<int64_t>(a - 1, 0);
  }
  const int mode = resolve_yuv_mode(e->input_yuv, in.full_range);
  const bool rgb_clip = in.kind == INPUT_RGB_CLIP;  // (no YUV rule takes part in its conversion: dec_mode is not compared)
  if (in.decoded && e->frames == e->frames_owned.p && e->frames_owned.p && in.dec_first <= a && b <= in.dec_first + in.dec_count && (rgb_clip || in.dec_mode == mode))
    return TM_OK;
  const bool lent_clip = in.kind == INPUT_YUV_CLIP || rgb_clip;
  const bool jpegs = jpeg_kind(in.kind), gifs = gif_kind(in.kind);
  TM_CHECK(in.kind != INPUT_GIF_CLIP || in.lent, TM_E_INVAL, "the GIF file was given back when the last Load returned: lend it again (tm_set_frames_gif) for more frames");
  TM_CHECK(in.kind != INPUT_JPEG_CLIP || in.lent, TM_E_INVAL,
           "the JPEG files were given back when the last Load returned: lend them again (tm_set_frames_jpeg) to convert them with another InputYUV or for more frames");
  TM_CHECK(in.kind != INPUT_PNG_CLIP || in.lent, TM_E_INVAL, "the PNG files were given back when the last Load returned: lend them again (tm_set_frames_png) for more frames");
  TM_CHECK(!rgb_clip || in.lent, TM_E_INVAL, "the RGB clip was given back when the last Load returned: lend the clip again (tm_set_frames_rgb) for more frames");
  TM_CHECK(!lent_clip || in.lent, TM_E_INVAL,
           "the YUV planes were given back when the last Load returned: lend the clip again (tm_set_frames_yuv) to convert it with another InputYUV or for more frames");
  TM_HIP(hipStreamSynchronize(e->stream));  // the destination may have been handed out by the pool a moment ago
  TM_TRY(e->frames_owned.alloc((size_t)e->width * e->height * 4 * e->nframes));
  e->frames = e->frames_owned.p;
  e->frames_host = nullptr;
  e->hclip_cur = -1;
  in.decoded = false;
  if (pngs || jpegs || gifs) {
    e->input_stats = tm_input_stats{};
    e->has_input_stats = false;
    int rc = TM_OK;
    if (b > a) rc = pngs ? decode_pngs_device(e, (int)a, (int)b) : gifs ? decode_gif(e, (int)a, (int)b) : decode_jpegs(e, (int)a, (int)b);
    if (rc != TM_OK) {  // as a failed host decode leaves it: no clip, and the next Load decodes again
      (void)hipStreamSynchronize(e->stream);
      e->frames = nullptr;
      return rc;
    }
    e->input_stats.frames = b - a; e->input_stats.where = pngs ? (int)TM_PNG_DECODE_DEVICE : gifs ? gif_decode_where(e) : jpeg_decode_where(e); e->input_stats.kind = in.kind;
    e->input_stats.ms_wall = ms_since(t0);
    e->input_stats.ms_device = std::max(0.0, e->input_stats.ms_wall - e->input_stats.ms_read);
    e->has_input_stats = true;
  } else if (b > a) TM_TRY(rgb_clip ? convert_rgb_clip(e, (int)a, (int)b) : lent_clip ? convert_yuv_clip(e, (int)a, (int)b) : in.kind == INPUT_GTM ? play_gtm(e, (int)a, (int)b) : decode_y4m(e, (int)a, (int)b));
  in.lent = false;  // (a lent clip is borrowed until this Load has returned: from here on the encoder reads its own RGB32 clip)
  in.decoded = true; in.dec_first = (int)a; in.dec_count = (int)(b - a); in.dec_mode = mode;
  return TM_OK;
}

extern "C" {

int tm_open_input(tm_encoder *e) {  // the probe half of Load, tilingencoder.pas:1764-1820
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (e->grp) return group_each(e, [](tm_encoder *s) { return tm_open_input(s); });
  InputInfo in;
  TM_TRY(probe_input(e->s.InputFileName, e->s.StartFrame, e->s.FrameCount, e->s.Scaling, &in));
  TM_TRY(tm_set_video(e, in.dst_w, in.dst_h, in.fps, in.frames));
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_set_frames_yuv(tm_encoder *e, const tm_yuv_clip *clip) {  // what tm_open_input does for a file, for planes in memory
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_TRY(check_yuv_clip(clip, nullptr));
  int dw = 0, dh = 0;
  TM_TRY(scaled_size(clip->width, clip->height, e->s.Scaling, &dw, &dh));
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_yuv(s, clip); });  // every shard converts what its Load reads
  TM_TRY(tm_set_video(e, dw, dh, clip->fps, clip->frames));
  InputInfo in;
  in.kind = INPUT_YUV_CLIP;
  in.clip = *clip;
  in.lent = true;
  in.frames = clip->frames; in.src_w = clip->width; in.src_h = clip->height; in.dst_w = dw; in.dst_h = dh;
  in.chroma = clip->chroma; in.full_range = clip->full_range ? 1 : 0; in.fps = clip->fps;
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_set_frames_rgb(tm_encoder *e, const tm_rgb_clip *clip) {  // tm_set_frames_yuv's twin
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_TRY(check_rgb_clip(clip, nullptr));
  int dw = 0, dh = 0;
  TM_TRY(scaled_size(clip->width, clip->height, e->s.Scaling, &dw, &dh));
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_rgb(s, clip); });  // every shard converts what its Load reads
  TM_TRY(tm_set_video(e, dw, dh, clip->fps, clip->frames));
  InputInfo in;
  in.kind = INPUT_RGB_CLIP;
  in.rgb_clip = *clip;
  in.lent = true;
  in.frames = clip->frames; in.src_w = clip->width; in.src_h = clip->height; in.dst_w = dw; in.dst_h = dh;
  in.chroma = TM_CHROMA_444; in.fps = clip->fps;
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_probe_png_clip_host(const void *const *files, const size_t *sizes, int nframes, double fps, int *width, int *height) {
  TM_CHECK(files && sizes && nframes >= 1 && fps > 0, TM_E_INVAL, "png clip: a null list, no frames or fps <= 0");
  for (int i = 0; i < nframes; i++) TM_CHECK(files[i] && sizes[i], TM_E_INVAL, "png clip: frame %d is null or empty", i);
  inf::PngInfo info;
  TM_TRY(inf::parse_png((const uint8_t *)files[0], sizes[0], "frame 0", &info));
  if (width) *width = info.w;
  if (height) *height = info.h;
  return TM_OK;
}

int tm_set_frames_png(tm_encoder *e, const void *const *files, const size_t *sizes, int nframes, double fps) {  // tm_set_frames_rgb's twin for files
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  int w = 0, h = 0;
  TM_TRY(tm_probe_png_clip_host(files, sizes, nframes, fps, &w, &h));
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_png(s, files, sizes, nframes, fps); });  // every shard decodes what its Load reads
  TM_TRY(tm_set_video(e, w, h, fps, nframes));
  InputInfo in;
  in.kind = INPUT_PNG_CLIP;
  in.png_files.assign(files, files + nframes);
  in.png_sizes.assign(sizes, sizes + nframes);
  in.lent = true;
  in.frames = nframes; in.src_w = in.dst_w = w; in.src_h = in.dst_h = h;
  in.chroma = TM_CHROMA_444; in.fps = fps;
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_probe_jpeg_clip_host(const void *const *files, const size_t *sizes, int nframes, double fps, int *width, int *height) {
  TM_CHECK(files && sizes && nframes >= 1 && fps > 0, TM_E_INVAL, "jpeg clip: a null list, no frames or fps <= 0");
  for (int i = 0; i < nframes; i++) TM_CHECK(files[i] && sizes[i], TM_E_INVAL, "jpeg clip: frame %d is null or empty", i);
  jpg::JpegInfo info;
  TM_TRY(jpg::parse_jpeg((const uint8_t *)files[0], sizes[0], "frame 0", &info));
  if (width) *width = info.w;
  if (height) *height = info.h;
  return TM_OK;
}

int tm_set_frames_jpeg(tm_encoder *e, const void *const *files, const size_t *sizes, int nframes, double fps) {  // tm_set_frames_png's twin
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  int w = 0, h = 0;
  TM_TRY(tm_probe_jpeg_clip_host(files, sizes, nframes, fps, &w, &h));
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_jpeg(s, files, sizes, nframes, fps); });  // every shard decodes what its Load reads
  jpg::JpegInfo info;
  TM_TRY(jpg::parse_jpeg((const uint8_t *)files[0], sizes[0], "frame 0", &info));
  TM_TRY(tm_set_video(e, w, h, fps, nframes));
  InputInfo in;
  in.kind = INPUT_JPEG_CLIP;
  in.png_files.assign(files, files + nframes);
  in.png_sizes.assign(sizes, sizes + nframes);
  in.lent = true;
  in.frames = nframes; in.src_w = in.dst_w = w; in.src_h = in.dst_h = h;
  in.chroma = info.layout(); in.full_range = 1; in.fps = fps;  // (JFIF: full-range BT.601)
  in.jpeg_segments = (int)info.nsegs;
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_probe_gif_clip_host(const void *file, size_t size, double fps, int *width, int *height, int *frames, double *out_fps) {
  TM_CHECK(file && size, TM_E_INVAL, "gif clip: the file is null or empty");
  gif::GifInfo info;
  TM_TRY(gif::parse_gif((const uint8_t *)file, size, "the lent GIF", &info));
  if (width) *width = info.w;
  if (height) *height = info.h;
  if (frames) *frames = (int)info.images.size();
  if (out_fps) *out_fps = fps > 0 ? fps : info.fps;
  return TM_OK;
}

int tm_set_frames_gif(tm_encoder *e, const void *file, size_t size, double fps) {  // tm_set_frames_png's twin for one file of many frames
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  int w = 0, h = 0, n = 0;
  double rate = 0;
  TM_TRY(tm_probe_gif_clip_host(file, size, fps, &w, &h, &n, &rate));
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_gif(s, file, size, fps); });  // every shard decodes from image 0 to the last frame its Load reads
  TM_TRY(tm_set_video(e, w, h, rate, n));
  InputInfo in;
  in.kind = INPUT_GIF_CLIP;
  in.png_files.assign(1, file);
  in.png_sizes.assign(1, size);
  in.lent = true;
  in.frames = n; in.src_w = in.dst_w = w; in.src_h = in.dst_h = h;
  in.chroma = TM_CHROMA_444; in.fps = rate;
  e->input = std::move(in);
  e->input_clip.clear();
  return TM_OK;
}

int tm_set_gif_decode(tm_encoder *e, int where) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(where >= TM_PNG_DECODE_AUTO && where <= TM_PNG_DECODE_DEVICE, TM_E_INVAL, "bad GIF decode place %d", where);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_gif_decode(s, where); });
  e->gif_decode = where;
  return TM_OK;
}

int tm_get_gif_decode(tm_encoder *e, int *where) {
  TM_CHECK(e && where, TM_E_INVAL, "null argument");
  *where = e->gif_decode;
  return TM_OK;
}

int tm_set_gif_background(tm_encoder *e, int background) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(background >= -1 && background <= 0xffffff, TM_E_INVAL, "bad GIF background %d (-1 or 0x00RRGGBB)", background);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_gif_background(s, background); });
  e->gif_background = background;
  return TM_OK;
}

int tm_get_gif_background(tm_encoder *e, int *background) {
  TM_CHECK(e && background, TM_E_INVAL, "null argument");
  *background = e->gif_background;
  return TM_OK;
}

int tm_set_jpeg_decode(tm_encoder *e, int where) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(where >= TM_PNG_DECODE_AUTO && where <= TM_PNG_DECODE_DEVICE, TM_E_INVAL, "bad JPEG decode place %d", where);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_jpeg_decode(s, where); });
  e->jpeg_decode = where;
  return TM_OK;
}

int tm_get_jpeg_decode(tm_encoder *e, int *where) {
  TM_CHECK(e && where, TM_E_INVAL, "null argument");
  *where = e->jpeg_decode;
  return TM_OK;
}

int tm_set_png_decode(tm_encoder *e, int where) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(where >= TM_PNG_DECODE_AUTO && where <= TM_PNG_DECODE_DEVICE, TM_E_INVAL, "bad PNG decode place %d", where);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_png_decode(s, where); });
  e->png_decode = where;
  return TM_OK;
}

int tm_get_png_decode(tm_encoder *e, int *where) {
  TM_CHECK(e && where, TM_E_INVAL, "null argument");
  *where = e->png_decode;
  return TM_OK;
}

int tm_get_input_stats(tm_encoder *e, tm_input_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_input_stats, TM_E_INVAL, "no Load has read a PNG, JPEG or GIF input yet");
  *out = e->input_stats;
  return TM_OK;
}

int tm_get_video(tm_encoder *e, int *width, int *height, double *fps, int *frames) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (width) *width = e->width;
  if (height) *height = e->height;
  if (fps) *fps = e->fps;
  if (frames) *frames = e->nframes;
  return TM_OK;
}

int tm_set_input_yuv(tm_encoder *e, int mode) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(mode >= TM_YUV_AUTO && mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "bad YUV mode %d", mode);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_input_yuv(s, mode); });
  e->input_yuv = mode;
  return TM_OK;
}


}  // extern "C"
