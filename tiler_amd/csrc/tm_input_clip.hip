// tm_input_clip.hip -- Load's sources that need no decoder: a Y4M file, a YUV or an RGB clip lent in memory (converted where it is, or staged
// through the encoder's two page-locked buffers: convert_staged), a .gtm stream played into the clip.  Coded files: tm_input_files.hip;
// the choice among them and the API: tm_input.hip; the kernels: tm_yuv_in.hip, tm_rgb_in.hip, tm_play_frame.hip; shared: tm_input.h.
//
// The reference opens "any file" through FFmpeg (extern.pas:780-781, 837-840), which does not exist here (DESIGN.md sections 9 and 17):
// Y4M is the uncompressed container every FFmpeg build writes.
#include <fcntl.h>

#include "tm_encoder.h"

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
int decode_y4m(tm_encoder *e, int a, int b) {
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
int convert_yuv_clip(tm_encoder *e, int a, int b) {
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
int convert_rgb_clip(tm_encoder *e, int a, int b) {
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

// frames [a, b) of the .gtm stream, played straight into the encoder's device clip (the player writes frame i where frame i + 1 reads it)
int play_gtm(tm_encoder *e, int a, int b) {
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
