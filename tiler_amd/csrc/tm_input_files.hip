// tm_input_files.hip -- Load's sources that are coded files, numbered on disk or lent in memory: a PNG sequence (host: decode_pngs; device:
// decode_pngs_device), a JPEG sequence (decode_jpegs), an animated GIF (decode_gif), and where each kind is decoded.  The two sequence
// decoders bring their files up a chunk at a time by the same steps, stated once (SequenceFiles).  The parsers and kernels: tm_png_in.hip,
// tm_jpeg_in.hip, tm_gif_in.hip, tm_png.hip; clips that need no decoder: tm_input_clip.hip; the choice and the API: tm_input.hip.
#include <fcntl.h>
#include <sys/stat.h>

#include "tm_encoder.h"
#include "tm_inflate.h"
#include "tm_gif.h"
#include "tm_jpeg.h"

namespace tmx { int decode_png(const uint8_t *file, size_t n, const char *name, uint32_t *out, int64_t cap_px, int *w_out, int *h_out); }  // tm_png.hip

// where a PNG input is decoded: TM_PNG_DECODE, else what tm_set_png_decode said.  AUTO is the device (0.33 s against
// 0.93 s for the 720p x 300 clip), and the host for pictures whose rows the kernels' 32-bit positions cannot hold
int png_decode_where(const tm_encoder *e) {
  const int w = knobs().png_decode ? knobs().png_decode : e->png_decode;
  if (w != TM_PNG_DECODE_AUTO) return w;
  return ((uint64_t)e->width * 4 + 1) * (uint64_t)e->height < ((uint64_t)1 << 32) ? TM_PNG_DECODE_DEVICE : TM_PNG_DECODE_HOST;
}
// where a JPEG input is decoded: TM_JPEG_DECODE, else what tm_set_jpeg_decode said.  AUTO goes by the first file:
// a file's segments are the lanes it keeps busy.  The 720p x 300 clip on the device against the host's reader threads: 227 ms against
// 138 ms with one segment a file, 150 against 142 with two, 96 against 142 with four, 26 against 139 with 45.  Three were not measured
// and stay with the host.
constexpr int JPEG_AUTO_DEVICE_SEGMENTS = 4;
int jpeg_decode_where(const tm_encoder *e) {
  const int w = knobs().jpeg_decode ? knobs().jpeg_decode : e->jpeg_decode;
  if (w != TM_PNG_DECODE_AUTO) return w;
  return e->input.jpeg_segments >= JPEG_AUTO_DEVICE_SEGMENTS ? TM_PNG_DECODE_DEVICE : TM_PNG_DECODE_HOST;
}

// where a GIF input is decoded: TM_GIF_DECODE, else what tm_set_gif_decode said.  AUTO is the device: two clips of
// 480 x 270 x 120 written by Pillow, OpenInput + Load from a memory-backed directory, median of 7 (range): the bench clip in 256 colours
// 24.4 ms (24.3 - 25.0) on the device against 32.8 ms (31.7 - 35.6) on the host's reader threads, a flat 16-colour one 2.19 ms (2.16 - 2.24)
// against 24.5 ms (24.3 - 24.7); the ranges do not meet on either.
int gif_decode_where(const tm_encoder *e) {
  const int w = knobs().gif_decode ? knobs().gif_decode : e->gif_decode;
  return w != TM_PNG_DECODE_AUTO ? w : (int)TM_PNG_DECODE_DEVICE;
}

// the PNG sequence, or the lent PNG files, decoded on the host into a clip the encoder keeps until Load's chunked host-clip upload has taken it
int decode_pngs(tm_encoder *e) {
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

// ---- What the PNG and the JPEG sequence share: files [a, a + n) of the numbered sequence or of the lent list, brought up a chunk at a time.
// A chunk's files lie in a staging slot one behind the other, each on a 16-byte boundary, the chunk's descriptor behind them.  The steps in
// the order their callers take them: list, plan, capacity, slots; per chunk place, read (on the reader threads), unchanged; at last statuses.
namespace {
constexpr size_t FILE_ROOM = (size_t)512 << 20;  // the files of a chunk: so many bytes of the largest
size_t on16(size_t n) { return (n + 15) & ~(size_t)15; }

struct SequenceFiles {
  const char *what;  // "PNG" / "JPEG", in the messages
  const InputInfo &in;
  bool lent;
  int a = 0, n = 0, chunk = 0;
  size_t cap = 0;  // bytes of a staging slot
  std::vector<std::string> names;
  std::vector<size_t> sizes, at;  // at[i]: where file i of the chunk last placed lies in its slot

  int list(int first, int last, tm_input_stats *stats) {  // names and sizes; every file exists
    a = first; n = last - first;
    names = std::vector<std::string>((size_t)n); sizes = std::vector<size_t>((size_t)n);
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
      stats->file_bytes += (int64_t)sizes[(size_t)i];
    }
    return TM_OK;
  }
  // the frames of a chunk: all n, or TM_INPUT_CHUNK_FRAMES, or as many as have room: frame_room bytes of decoded frames, file_room of files
  void plan(size_t frame_room, size_t frame_bytes, size_t file_room) {
    size_t largest = 16;
    for (size_t sz : sizes) largest = std::max(largest, on16(sz));
    const size_t by_room = std::max<size_t>(1, std::min(frame_room / frame_bytes, file_room / largest));
    chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, knobs().input_chunk_frames > 0 ? (size_t)knobs().input_chunk_frames : by_room));
    at.resize((size_t)chunk);
  }
  size_t place(int f0, int nf) {  // the chunk's files one behind the other: their bytes in all
    size_t bytes = 0;
    for (int i = 0; i < nf; i++) { at[(size_t)i] = bytes; bytes += on16(sizes[(size_t)(f0 + i)]); }
    return bytes;
  }
  // a slot holds the largest chunk's files and the most its descriptor can take, desc_bound(bytes of files, files); below 4 GiB
  template <class Bound> int capacity(Bound desc_bound) {
    cap = 0;
    for (int f0 = 0; f0 < n; f0 += chunk) {
      const int nf = std::min(chunk, n - f0);
      const size_t bytes = place(f0, nf);
      cap = std::max(cap, bytes + desc_bound(bytes, (size_t)nf) + 64);
    }
    TM_CHECK(cap < ((size_t)1 << 32), TM_E_UNSUPPORTED, "a chunk of %d %s files takes %zu bytes (below 4 GiB: lower TM_INPUT_CHUNK_FRAMES)", chunk, what, cap);
    return TM_OK;
  }
  int slots(PinnedBuf *host, DevBuf *dev) const {  // two of `cap` bytes, or one when there is one chunk
    for (int i = 0; i < (n > chunk ? 2 : 1); i++) { TM_TRY(host[i].alloc(cap)); TM_TRY(dev[i].alloc(cap)); }
    return TM_OK;
  }
  const char *name(int f0, int i) const { return names[(size_t)(f0 + i)].c_str(); }
  size_t size(int f0, int i) const { return sizes[(size_t)(f0 + i)]; }
  const uint8_t *lent_file(int f0, int i) const { return (const uint8_t *)in.png_files[(size_t)(a + f0 + i)]; }
  int read(int f0, int i, uint8_t *to) const {  // file i of the chunk at f0, whole
    if (lent) { memcpy(to, lent_file(f0, i), size(f0, i)); return TM_OK; }
    const int fd = open(name(f0, i), O_RDONLY);
    TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", name(f0, i));
    FdCloser closer{fd};
    TM_CHECK(pread_all(fd, to, size(f0, i), 0) == 0, TM_E_IO, "cannot read %s", name(f0, i));
    return TM_OK;
  }
  int unchanged(size_t bytes, size_t desc_bytes) const {  // (the descriptor is made of what was read, the slot of what was listed)
    TM_CHECK(bytes + desc_bytes <= cap, TM_E_INVAL, "a %s file changed while it was being read", what);
    return TM_OK;
  }
  // what only decoding finds: a status per frame, read back behind the last chunk's work (no buffer: none was refused there); the first
  // refusal comes back by its file's name
  int statuses(tm_encoder *e, const DevBuf &status, int (*error_of)(int, const char *)) const {
    std::vector<int32_t> st((size_t)n, 0);
    if (status.p) TM_HIP(hipMemcpyAsync(st.data(), status.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    TM_HIP(hipStreamSynchronize(e->stream));  // the staging buffers go back to the pool and to the host
    for (int i = 0; i < n; i++) TM_TRY(error_of(st[(size_t)i], names[(size_t)i].c_str()));
    return TM_OK;
  }
};
}  // namespace

// Frames [a, b) of the PNG sequence, or of the lent files, decoded on the device into the encoder's clip.  A chunk of
// files is read into a page-locked buffer (the reader threads; each walks its file's chunks and checks what decode_png checks before the
// stream), the descriptor of the chunk is written behind the files, and both go up in one copy on the copy stream; k_inflate and
// k_png_unfilter run on the main stream while the next chunk is read.  What only decoding finds comes back as a status per frame.
int decode_pngs_device(tm_encoder *e, int a, int b) {
  tm_input_stats &stats = e->input_stats;
  const int n = b - a, w = e->width, h = e->height;
  SequenceFiles files{"PNG", e->input, e->input.kind == INPUT_PNG_CLIP};
  TM_TRY(files.list(a, b, &stats));
  // A stream is one wave's work from end to end, so a chunk should hold as many frames as the device has room for waves (four to a compute
  // unit): as many as 2 GiB of inflated rows and 512 MiB of files allow.  The 720p x 300 clip is one chunk; in chunks of 32 frames its
  // Load took 2.8 s, one launch of 32 waves after the other.
  const size_t raw_frame = on16(((size_t)w * 4 + 1) * (size_t)h), out_fb = (size_t)w * h * 4;
  files.plan((size_t)2 << 30, raw_frame, FILE_ROOM);
  const int chunk = files.chunk;
  TM_TRY(files.capacity([](size_t bytes, size_t nf) {  // (a span per 12 bytes of file at the worst)
    return nf * (sizeof(inf::Stream) + sizeof(inf::Picture) + 768) + (bytes / 12 + nf) * sizeof(inf::Span);
  }));
  PinnedBuf *host = e->input_pinned;
  DevBuf dev[2], raw, inflated, status;
  StagingRing ring;
  TM_TRY(ring.make());
  TM_TRY(files.slots(host, dev));
  TM_TRY(raw.alloc(raw_frame * chunk)); TM_TRY(inflated.alloc((size_t)n * sizeof(tm_inflate_status))); TM_TRY(status.alloc((size_t)n * 4));
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  inf::PngBatch batch[2];
  std::vector<inf::PngInfo> infos((size_t)chunk);
  int c = 0;
  for (int f0 = 0; f0 < n; f0 += chunk, c++) {
    const int nf = std::min(chunk, n - f0), s = c & 1;
    TM_TRY(ring.host_free(s));
    const auto t0 = std::chrono::steady_clock::now();
    const size_t bytes = files.place(f0, nf);
    uint8_t *hb = (uint8_t *)host[s].p;
    TM_TRY(parallel_for(nf, [&](int i) -> int {
      uint8_t *to = hb + files.at[(size_t)i];
      TM_TRY(files.read(f0, i, to));
      TM_TRY(inf::parse_png(to, files.size(f0, i), files.name(f0, i), &infos[(size_t)i]));
      return inf::png_check_decodable(infos[(size_t)i], files.name(f0, i), w, h);
    }));
    batch[s].clear();
    for (int i = 0; i < nf; i++) batch[s].add(infos[(size_t)i], files.at[(size_t)i]);
    TM_TRY(files.unchanged(bytes, batch[s].desc_bytes()));
    const size_t used = bytes + batch[s].write_desc(hb + bytes);
    stats.ms_read += ms_since(t0);
    stats.bytes_uploaded += (int64_t)used;
    TM_TRY(ring.device_free(s, e->copy_stream));
    TM_HIP(hipMemcpyAsync(dev[s].p, hb, used, hipMemcpyHostToDevice, e->copy_stream));
    TM_TRY(ring.uploaded(s, e->copy_stream, e->stream));
    TM_TRY(inf::png_batch_launch(batch[s], dev[s].as<uint8_t>(), used, bytes, raw.as<uint8_t>(), inflated.as<tm_inflate_status>() + f0, w, h,
                                 reinterpret_cast<uint32_t *>(e->frames_owned.as<uint8_t>() + out_fb * (size_t)(a + f0)), (int64_t)w * h, status.as<int32_t>() + f0, e->stream));
    TM_TRY(ring.worked(s, e->stream));
  }
  return files.statuses(e, status, inf::png_status_error);
}

// Frames [a, b) of the JPEG sequence, or of the lent files, into the encoder's clip.  The reader threads bring a
// chunk's files into memory and walk them.  DEVICE: the files lie in the page-locked buffer, the chunk's descriptor is written behind
// them, both go up in one copy on the copy stream and k_jpeg_decode writes the chunk's planes.  HOST: the reader threads decode with the
// host form into the page-locked buffer and the planes go up.  Either way the planes -- MCU-padded, with the true size and a row stride
// handed on -- are converted by k_yuv_to_rgb32 on the main stream while the next chunk is read.
int decode_jpegs(tm_encoder *e, int a, int b) {
  InputInfo &in = e->input;
  tm_input_stats &stats = e->input_stats;
  const bool lent = in.kind == INPUT_JPEG_CLIP, on_device = jpeg_decode_where(e) == TM_PNG_DECODE_DEVICE;
  const int n = b - a, w = e->width, h = e->height, layout = in.chroma;
  SequenceFiles files{"JPEG", in, lent};
  TM_TRY(files.list(a, b, &stats));
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
  files.plan((size_t)1 << 30, fb, FILE_ROOM);
  const int chunk = files.chunk;
  // a slot holds, HOST: a chunk's planes.  DEVICE: its files and the most its descriptor can take (a segment per MCU)
  if (on_device) TM_TRY(files.capacity([&](size_t, size_t nf) { return nf * (sizeof(jpg::Frame) + sizeof(jpg::TableSet) + mcus * sizeof(jpg::Seg)); }));
  else files.cap = fb * (size_t)chunk;
  PinnedBuf *host = e->input_pinned;
  DevBuf dev[2], planes, status;
  StagingRing ring;
  TM_TRY(ring.make());
  TM_TRY(files.slots(host, dev));
  if (on_device) { TM_TRY(planes.alloc(fb * (size_t)chunk)); TM_TRY(status.alloc((size_t)n * 4)); }
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  jpg::JpegBatch batch[2];
  std::vector<jpg::JpegInfo> infos((size_t)chunk);
  auto layout_of = [&](int i) {  // frame i of a chunk: its offset in the Y planes, in the U planes, in the V planes
    jpg::PlaneLayout pl;
    pl.off[0] = yb * (size_t)i; pl.stride[0] = ypw; pl.w[0] = ypw; pl.h[0] = yph;
    for (int c = 1; c < (mono ? 1 : 3); c++) { pl.off[c] = cb * (size_t)i; pl.stride[c] = cpw; pl.w[c] = cpw; pl.h[c] = cph; }
    return pl;
  };
  auto check_like_first = [&](const jpg::JpegInfo &info, const char *name) -> int {
    TM_CHECK(info.w == w && info.h == h, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", name, info.w, info.h, w, h);
    TM_CHECK(info.layout() == layout, TM_E_INVAL, "%s has %d component(s) sampled %dx%d, which is not the sampling of the sequence's first frame", name, info.ncomp,
             info.hs, info.vs);
    return (int)TM_OK;
  };
  int c = 0;
  for (int f0 = 0; f0 < n; f0 += chunk, c++) {
    const int nf = std::min(chunk, n - f0), s = c & 1;
    TM_TRY(ring.host_free(s));
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t *hb = (uint8_t *)host[s].p;
    size_t used = 0, bytes = 0;
    if (on_device) {
      bytes = files.place(f0, nf);
      TM_TRY(parallel_for(nf, [&](int i) -> int {
        uint8_t *to = hb + files.at[(size_t)i];
        TM_TRY(files.read(f0, i, to));
        TM_TRY(jpg::parse_jpeg(to, files.size(f0, i), files.name(f0, i), &infos[(size_t)i]));
        return check_like_first(infos[(size_t)i], files.name(f0, i));
      }));
      batch[s].clear();
      for (int i = 0; i < nf; i++) batch[s].add(infos[(size_t)i], files.at[(size_t)i], layout_of(i));
      TM_TRY(files.unchanged(bytes, batch[s].desc_bytes()));
      used = bytes + batch[s].write_desc(hb + bytes);
    } else {
      uint8_t *const pl3[3] = {hb, hb + yb * (size_t)nf, hb + (yb + cb) * (size_t)nf};
      TM_TRY(parallel_for(nf, [&](int i) -> int {
        const size_t sz = files.size(f0, i);
        std::vector<uint8_t> mine;  // (a lent file is decoded where it is)
        if (!lent) {
          mine.resize(sz);
          TM_TRY(files.read(f0, i, mine.data()));
        }
        const uint8_t *file = lent ? files.lent_file(f0, i) : mine.data();
        jpg::JpegInfo info;
        TM_TRY(jpg::parse_jpeg(file, sz, files.name(f0, i), &info));
        TM_TRY(check_like_first(info, files.name(f0, i)));
        return jpg::jpeg_status_error(jpg::jpeg_decode_one_host(info, file, sz, layout_of(i), pl3), files.name(f0, i));
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
      TM_TRY(jpg::jpeg_batch_launch(batch[s], dev[s].as<uint8_t>(), used, bytes, py, pu, pv, plane_bytes, status.as<int32_t>() + f0, e->stream));
    }
    const int64_t strides[6] = {(int64_t)ypw, (int64_t)yb, (int64_t)cpw, (int64_t)cb, (int64_t)cpw, (int64_t)cb};
    TM_TRY(launch_yuv_to_rgb32(tables, py, pu, pv, strides, SampleFmt(), nf, mode, e->frames_owned.as<uint8_t>() + out_fb * (size_t)(a + f0), e->stream));
    TM_TRY(ring.worked(s, e->stream));
  }
  return files.statuses(e, status, jpg::jpeg_status_error);
}

// Frames [a, b) of the GIF file, or of the lent one, into the encoder's clip.  A frame is what the frames before it
// left with its own rectangle drawn over it, so images 0 .. StartFrame + b - 1 are decoded and composited and [StartFrame + a, StartFrame +
// b) are delivered.  DEVICE: the file goes up once, then a descriptor, k_gif_lzw and k_gif_compose per chunk of images.  HOST: the reader
// threads run the LZW image by image, the frames are composited on this thread and uploaded.
int decode_gif(tm_encoder *e, int a, int b) {
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
