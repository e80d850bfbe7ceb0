// tm_export.hip -- the frames leaving the encoder as files: GenerateY4M / GeneratePNGs / GenerateJPEGs / GenerateMJPEG / GenerateGIF / GenerateWebP
// with their options and stats.  The frames are the device render's (RenderSource and the chunk rule: tm_encoder.h; the entry points that
// hand them to a caller: tm_render_api.hip); the coders are tm_deflate.hip / tm_png_out.hip, tm_jpeg_out.hip, tm_gif_out.hip, tm_webp_out.hip.
#include <chrono>
#include <cmath>
#include <fstream>

#include "tm_deflate.h"
#include "tm_encoder.h"
#include "tm_gif_out.h"
#include "tm_webp_out.h"
#include "tm_jpeg_out.h"

// ---- GenerateY4M / GeneratePNGs (tilingencoder.pas:2126-2199, 2075-2124): the frames as Render (3455-3640) draws them with the
// constructor's defaults (FRenderPredicted, FRenderMirrored, FRenderOutputDithered on, no gamma: 5505-5507) -- the device render's
// pictures, brought to the host a chunk of frames at a time.  An export refuses exactly what the device render of the whole clip refuses
// (init, before any file is opened: a refused call leaves no file behind).  In a device group it reads shard 0, the front encoder.
namespace {
struct ExportFrames {
  tm_encoder *e;
  bool input;
  bool y4m = false;  // the frames come to the host as GenerateY4M's planes (Y, U, V of a frame in a row: 3 bytes a pixel), not as RGB32
  bool keep = false; // the frames stay on the device as RGB32 (the coders on the device take them there): dev holds frames [first, first + count)
  RenderSource src{};
  int sw = 0, sh = 0, chunk = 0, first = 0, count = 0;
  DevBuf dev;
  std::vector<uint32_t> host;  // frames [first, first + count), 0x00RRGGBB
  DevBuf dev_yuv;
  std::vector<uint8_t> host_yuv;
  tm_yuv_out planes{};
  YuvOutPlan plan;
  int init() {
    TM_HIP(hipSetDevice(e->device));
    src.input = input;
    TM_TRY(src.prepare(e, 0, e->nframes));
    sw = e->tm_w * 8; sh = e->tm_h * 8;
    const size_t fbytes = (size_t)sw * sh * 4;
    chunk = render_chunk_frames(e->nframes, fbytes);
    TM_TRY(dev.alloc(fbytes * chunk));
    if (keep) return TM_OK;
    if (!y4m) { host.resize((size_t)sw * sh * chunk); return TM_OK; }
    const int64_t plane = (int64_t)sw * sh;
    TM_TRY(dev_yuv.alloc((size_t)plane * 3 * chunk));
    host_yuv.resize((size_t)plane * 3 * chunk);
    planes.y = dev_yuv.p; planes.u = dev_yuv.as<uint8_t>() + plane; planes.v = dev_yuv.as<uint8_t>() + 2 * plane;
    planes.y_row = planes.u_row = planes.v_row = sw;
    planes.y_frame = planes.u_frame = planes.v_frame = 3 * plane;
    planes.width = sw; planes.height = sh; planes.frames = chunk; planes.fps = 1.0;
    planes.chroma = TM_CHROMA_444; planes.samples = TM_SAMPLES_U8; planes.depth = 8; planes.memory = TM_MEM_DEVICE;
    return check_yuv_out(&planes, sw, sh, TM_YUV_TILER, &plan);
  }
  bool fresh(int f) const { return f >= first + count; }  // frame f starts a chunk that has not been drawn yet
  int frame(int f, const uint32_t **px) {  // frames are asked for in order
    if (fresh(f)) {
      first = f;
      count = std::min(chunk, e->nframes - f);
      TM_TRY(src.draw(first, count, dev.p, e->stream));
      if (y4m) {
        TM_TRY(launch_rgb32_to_yuv(plan, dev.p, sw, count, yuv_dst_of(planes, 0), e->stream));
        TM_HIP(hipMemcpyAsync(host_yuv.data(), dev_yuv.p, (size_t)count * sw * sh * 3, hipMemcpyDeviceToHost, e->stream));
      } else if (!keep) {
        TM_HIP(hipMemcpyAsync(host.data(), dev.p, (size_t)count * sw * sh * 4, hipMemcpyDeviceToHost, e->stream));
      }
      TM_HIP(hipStreamSynchronize(e->stream));
    }
    if (px) *px = keep ? nullptr : host.data() + (size_t)(f - first) * sw * sh;  // (keep: the frames are in dev, none on the host)
    return TM_OK;
  }
  int frame_y4m(int f, const uint8_t **yuv) {
    TM_TRY(frame(f, nullptr));
    *yuv = host_yuv.data() + (size_t)(f - first) * sw * sh * 3;
    return TM_OK;
  }
};

// An export's time-keeping, for any of the four stats structs: the wall clock runs from the construction, start() opens the first lap,
// coded() closes one of render, coding and read-back, wrote() one of writing `files` files of `bytes` bytes in all
struct ExportClock {
  using clock = std::chrono::steady_clock;
  clock::time_point wall0 = clock::now(), mark = wall0;
  double ms_device = 0, ms_write = 0;
  int64_t frames = 0, file_bytes = 0;
  static double ms(clock::time_point from, clock::time_point to) { return std::chrono::duration<double, std::milli>(to - from).count(); }
  double lap() {
    const clock::time_point now = clock::now();
    const double d = ms(mark, now);
    mark = now;
    return d;
  }
  void start() { mark = clock::now(); }
  void coded() { ms_device += lap(); }
  void wrote(int64_t files, int64_t bytes) { ms_write += lap(); frames += files; file_bytes += bytes; }
  template <class Stats> void fill(Stats *st) const {  // (a one-file export's frames and bytes are its encoder's count: it adds none)
    st->frames += frames; st->file_bytes += file_bytes;
    st->ms_device = ms_device; st->ms_write = ms_write; st->ms_wall = ms(wall0, clock::now());
  }
};

// a finished file (a PNG: pf24bit, 2086; its bytes are made by png_stored of tm_deflate.hip or on the device by tm_png_out.hip) to its place
int write_file(const std::string &path, const std::vector<uint8_t> &bytes) {
  std::ofstream f(path, std::ios::binary);
  TM_CHECK(f.good(), TM_E_IO, "cannot write %s", path.c_str());
  f.write((const char *)bytes.data(), (std::streamsize)bytes.size());
  TM_CHECK(f.good(), TM_E_IO, "write to %s failed", path.c_str());
  return TM_OK;
}
std::string strip_ext(const std::string &p) {  // ChangeFileExt(name, '')
  const size_t dot = p.find_last_of('.'), sep = p.find_last_of("/\\");
  return (dot != std::string::npos && (sep == std::string::npos || dot > sep)) ? p.substr(0, dot) : p;
}
std::string frame_file(const std::string &base, int f, const char *ext) {  // base_0007.png
  char name[32];
  snprintf(name, sizeof(name), "_%04d.%s", f, ext);
  return base + name;
}

// Every frame of the clip as a file of its own, coded on the device: encode(files) codes the chunk `r` has just drawn into one file per
// frame, sink(f, bytes) takes frame f's.  (Both are called directly: this loop runs per frame.)
template <class Encode, class Sink>
int export_frame_files(ExportFrames &r, ExportClock &clk, Encode &&encode, Sink &&sink) {
  std::vector<std::vector<uint8_t>> files;
  clk.start();
  for (int fr = 0; fr < r.e->nframes; fr++) {
    const bool fresh = r.fresh(fr);
    TM_TRY(r.frame(fr, nullptr));
    if (fresh) TM_TRY(encode(files));
    clk.coded();
    const std::vector<uint8_t> &bytes = files[(size_t)(fr - r.first)];
    TM_TRY(sink(fr, bytes));
    clk.wrote(1, (int64_t)bytes.size());
  }
  return TM_OK;
}

// Every frame of the clip into one file, coded on the device by an encoder of begin / chunk / end that takes at most `most` frames a call.
// The file is opened once every chunk has been coded: a refused frame leaves none.
template <class Encoder, class Options>
int export_one_file(ExportFrames &r, ExportClock &clk, Encoder &encoder, const Options &opt, int most, const char *path) {
  tm_encoder *e = r.e;
  const int64_t px = (int64_t)r.sw * r.sh;
  std::vector<uint8_t> file;
  TM_TRY(encoder.begin(r.sw, r.sh, e->fps, opt, e->stream, file));
  clk.start();
  for (int fr = 0; fr < e->nframes; fr += r.count) {
    TM_TRY(r.frame(fr, nullptr));
    for (int f0 = 0; f0 < r.count; f0 += most) TM_TRY(encoder.chunk(r.dev.as<uint32_t>() + px * f0, r.sw, px, std::min(most, r.count - f0), file));
  }
  TM_TRY(encoder.end(file));
  clk.coded();
  TM_TRY(write_file(path, file));
  clk.wrote(0, 0);
  return TM_OK;
}
}  // namespace

static int generate_y4m(tm_encoder *e, const char *path, bool input) {  // GenerateY4M, tilingencoder.pas:2126-2199
  TM_CHECK(path && *path, TM_E_INVAL, "GenerateY4M: no file name");
  ExportFrames r{e, input, true};
  TM_TRY(r.init());
  std::ofstream f(path, std::ios::binary);
  TM_CHECK(f.good(), TM_E_IO, "cannot write %s", path);
  char hdr[128];
  snprintf(hdr, sizeof(hdr), "YUV4MPEG2 W%d H%d F%lld:1000000 Ip C444\n", r.sw, r.sh, (long long)std::nearbyint(e->fps * 1000000.0));  // 2146
  f << hdr;
  // RGBToYUV (utils.pas:478-490), rounded and clamped, runs on the device (TM_YUV_TILER, tm_yuv_out.hip): the planes arrive as the file holds them
  const size_t plane = (size_t)r.sw * r.sh;
  for (int fr = 0; fr < e->nframes; fr++) {
    const uint8_t *yuv = nullptr;
    TM_TRY(r.frame_y4m(fr, &yuv));
    f << "FRAME \n";  // (with the space, 2161)
    f.write((const char *)yuv, (std::streamsize)(plane * 3));
    if ((fr & 15) == 15) progress(e, TM_STEP_SAVE, fr, e->nframes);
  }
  TM_CHECK(f.good(), TM_E_IO, "write to %s failed", path);
  return TM_OK;
}

static int generate_pngs(tm_encoder *e, bool input) {  // GeneratePNGs, tilingencoder.pas:2075-2124
  TM_CHECK(!e->s.OutputFileName.empty(), TM_E_INVAL, "GeneratePNGs: OutputFileName is not set");
  ExportClock clk;
  const tm_png_options opt = e->png_options;
  // AUTO: the Output page is palettised, which the coder takes best unfiltered; the Input page is a photograph
  const int filter = opt.filter == TM_PNG_FILTER_AUTO ? (input ? TM_PNG_FILTER_ADAPTIVE : TM_PNG_FILTER_NONE) : opt.filter;
  e->has_export_stats = false;
  ExportFrames r{e, input};
  r.keep = opt.level != 0;
  TM_TRY(r.init());
  const std::string base = strip_ext(e->s.OutputFileName);
  {
    std::ofstream pf(base + ".txt");  // the palettes, one colour per line: IntToHex($ff000000 or PaletteRGB, 8) (2101-2104)
    TM_CHECK(pf.good(), TM_E_IO, "cannot write %s.txt", base.c_str());
    char line[16];
    for (int32_t c : e->palettes_host) { snprintf(line, sizeof(line), "%08X", 0xff000000u | (uint32_t)c); pf << line << "\n"; }
  }
  tm_export_stats st{};
  st.level = opt.level; st.filter = opt.level ? filter : opt.filter;
  if (opt.level) {  // level 1: the chunk stays on the device, is coded there (tm_png_out.hip), and only the files' bytes come back
    dfl::PngDeviceEncoder encoder;  // (its device buffers serve every chunk)
    TM_TRY(export_frame_files(
        r, clk,
        [&](std::vector<std::vector<uint8_t>> &files) -> int {
          return encoder.encode(r.dev.as<uint32_t>(), r.sw, (int64_t)r.sw * r.sh, r.count, r.sw, r.sh, filter, e->stream, files);
        },
        [&](int fr, const std::vector<uint8_t> &bytes) -> int { return write_file(frame_file(base, fr, "png"), bytes); }));
  } else {  // level 0: a chunk of frames comes to the host and each is written in stored blocks
    std::vector<uint8_t> file;
    clk.start();
    for (int fr = 0; fr < e->nframes; fr++) {
      const uint32_t *px = nullptr;
      TM_TRY(r.frame(fr, &px));
      clk.coded();
      dfl::png_stored(px, r.sw, r.sw, r.sh, file);
      TM_TRY(write_file(frame_file(base, fr, "png"), file));
      clk.wrote(1, (int64_t)file.size());
    }
  }
  clk.fill(&st);
  e->export_stats = st;
  e->has_export_stats = true;
  return TM_OK;
}

// GenerateJPEGs / GenerateMJPEG: the frames GeneratePNGs writes, kept on the device a chunk at a time and coded there
// (tm_jpeg_out.hip); only the files' bytes come back.  path: the one file they go to behind one another, or null: a file per frame next
// to OutputFileName.
static int generate_jpegs(tm_encoder *e, const char *path, bool input) {
  const char *who = path ? "GenerateMJPEG" : "GenerateJPEGs";
  TM_CHECK(!path || *path, TM_E_INVAL, "GenerateMJPEG: no file name");
  TM_CHECK(path || !e->s.OutputFileName.empty(), TM_E_INVAL, "GenerateJPEGs: OutputFileName is not set");
  ExportClock clk;
  const tm_jpeg_options opt = e->jpeg_options;
  e->has_jpeg_export_stats = false;
  ExportFrames r{e, input};
  r.keep = true;
  TM_TRY(r.init());
  TM_TRY(jpo::jpeg_out_check(who, r.dev.p, r.sw, (int64_t)r.sw * r.sh, e->nframes, r.sw, r.sh, &opt));
  const std::string base = strip_ext(e->s.OutputFileName);
  std::ofstream all;
  if (path) {
    all.open(path, std::ios::binary);
    TM_CHECK(all.good(), TM_E_IO, "cannot write %s", path);
  }
  tm_jpeg_export_stats st{};
  st.quality = opt.quality; st.sampling = opt.sampling; st.restart_rows = opt.restart_rows;
  jpo::JpegDeviceEncoder encoder;  // (its device buffers serve every chunk)
  auto encode = [&](std::vector<std::vector<uint8_t>> &files) -> int {
    return encoder.encode(r.dev.as<uint32_t>(), r.sw, (int64_t)r.sw * r.sh, r.count, r.sw, r.sh, opt, e->stream, files);
  };
  if (path)
    TM_TRY(export_frame_files(r, clk, encode, [&](int, const std::vector<uint8_t> &bytes) -> int {
      all.write((const char *)bytes.data(), (std::streamsize)bytes.size());
      TM_CHECK(all.good(), TM_E_IO, "write to %s failed", path);
      return TM_OK;
    }));
  else
    TM_TRY(export_frame_files(r, clk, encode, [&](int fr, const std::vector<uint8_t> &bytes) -> int { return write_file(frame_file(base, fr, "jpg"), bytes); }));
  clk.fill(&st);
  e->jpeg_export_stats = st;
  e->has_jpeg_export_stats = true;
  return TM_OK;
}

// GenerateGIF: the frames GeneratePNGs writes as one animated GIF, kept on the device a chunk at a time and coded
// there (tm_gif_out.hip); only the file's bytes come back.
static int generate_gif(tm_encoder *e, const char *path, bool input) {
  TM_CHECK(path && *path, TM_E_INVAL, "GenerateGIF: no file name");
  ExportClock clk;
  const tm_gif_options opt = e->gif_options;
  e->has_gif_export_stats = false;
  ExportFrames r{e, input};
  r.keep = true;
  TM_TRY(r.init());
  int delay;
  TM_TRY(gfo::gif_out_check("GenerateGIF", r.dev.p, r.sw, (int64_t)r.sw * r.sh, e->nframes, r.sw, r.sh, e->fps, &opt, &delay));
  gfo::GifDeviceEncoder encoder;  // (its device buffers serve every chunk)
  TM_TRY(export_one_file(r, clk, encoder, opt, r.chunk, path));
  tm_gif_export_stats st = encoder.stats;
  clk.fill(&st);
  e->gif_export_stats = st;
  e->has_gif_export_stats = true;
  return TM_OK;
}

// GenerateWebP: the frames GeneratePNGs writes as one animated lossless WebP, kept on the device a chunk at a time and
// coded there (tm_webp_out.hip), wpo::kMaxChunk frames a call; only the file's bytes come back.
static int generate_webp(tm_encoder *e, const char *path, bool input) {
  TM_CHECK(path && *path, TM_E_INVAL, "GenerateWebP: no file name");
  ExportClock clk;
  const tm_webp_options opt = e->webp_options;
  e->has_webp_export_stats = false;
  ExportFrames r{e, input};
  r.keep = true;
  TM_TRY(r.init());
  int duration;
  TM_TRY(wpo::webp_out_check("GenerateWebP", r.dev.p, r.sw, (int64_t)r.sw * r.sh, e->nframes, r.sw, r.sh, e->fps, &opt, &duration));
  wpo::WebpDeviceEncoder encoder;  // (its device buffers serve every chunk)
  TM_TRY(export_one_file(r, clk, encoder, opt, wpo::kMaxChunk, path));
  tm_webp_export_stats st = encoder.stats;
  clk.fill(&st);
  e->webp_export_stats = st;
  e->has_webp_export_stats = true;
  return TM_OK;
}

// the getters of the options and stats: *out = the encoder's field; stats only once an export has left them (`has`, else the refusal `none`)
template <class T> static int get_field(tm_encoder *e, T *out, T tm_encoder::*field, bool tm_encoder::*has = nullptr, const char *none = nullptr) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(!has || e->*has, TM_E_INVAL, "%s", none);
  *out = e->*field;
  return TM_OK;
}

extern "C" {

int tm_generate_y4m(tm_encoder *e, const char *path, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  return generate_y4m(e, path, input != 0);
}

int tm_generate_pngs(tm_encoder *e, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  return generate_pngs(e, input != 0);
}

int tm_set_png_options(tm_encoder *e, const tm_png_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  TM_CHECK(opt->level == 0 || opt->level == 1, TM_E_INVAL, "png options: unknown level %d (0 or 1)", opt->level);
  TM_CHECK(opt->filter >= TM_PNG_FILTER_AUTO && opt->filter <= TM_PNG_FILTER_SMALLER, TM_E_INVAL, "png options: unknown filter %d", opt->filter);
  e->png_options = *opt;
  return TM_OK;
}
int tm_get_png_options(tm_encoder *e, tm_png_options *opt) { return get_field(e, opt, &tm_encoder::png_options); }
int tm_get_export_stats(tm_encoder *e, tm_export_stats *out) { return get_field(e, out, &tm_encoder::export_stats, &tm_encoder::has_export_stats, "export stats: this encoder has not written PNGs"); }

int tm_generate_jpegs(tm_encoder *e, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  return generate_jpegs(e, nullptr, input != 0);
}

int tm_generate_mjpeg(tm_encoder *e, const char *path, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(path, TM_E_INVAL, "GenerateMJPEG: no file name");
  return generate_jpegs(e, path, input != 0);
}

int tm_set_jpeg_options(tm_encoder *e, const tm_jpeg_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  TM_TRY(jpo::jpeg_options_check("jpeg options", opt));
  e->jpeg_options = *opt;
  return TM_OK;
}
int tm_get_jpeg_options(tm_encoder *e, tm_jpeg_options *opt) { return get_field(e, opt, &tm_encoder::jpeg_options); }
int tm_get_jpeg_export_stats(tm_encoder *e, tm_jpeg_export_stats *out) { return get_field(e, out, &tm_encoder::jpeg_export_stats, &tm_encoder::has_jpeg_export_stats, "jpeg export stats: this encoder has not written JPEGs"); }

int tm_generate_gif(tm_encoder *e, const char *path, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(path, TM_E_INVAL, "GenerateGIF: no file name");
  return generate_gif(e, path, input != 0);
}

int tm_set_gif_options(tm_encoder *e, const tm_gif_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  TM_TRY(gfo::gif_options_check("gif options", opt));
  e->gif_options = *opt;
  return TM_OK;
}
int tm_get_gif_options(tm_encoder *e, tm_gif_options *opt) { return get_field(e, opt, &tm_encoder::gif_options); }
int tm_get_gif_export_stats(tm_encoder *e, tm_gif_export_stats *out) { return get_field(e, out, &tm_encoder::gif_export_stats, &tm_encoder::has_gif_export_stats, "gif export stats: this encoder has not written a GIF"); }

int tm_generate_webp(tm_encoder *e, const char *path, int input) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(path, TM_E_INVAL, "GenerateWebP: no file name");
  return generate_webp(e, path, input != 0);
}

int tm_set_webp_options(tm_encoder *e, const tm_webp_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  TM_TRY(wpo::webp_options_check("webp options", opt));
  e->webp_options = *opt;
  return TM_OK;
}
int tm_get_webp_options(tm_encoder *e, tm_webp_options *opt) { return get_field(e, opt, &tm_encoder::webp_options); }
int tm_get_webp_export_stats(tm_encoder *e, tm_webp_export_stats *out) { return get_field(e, out, &tm_encoder::webp_export_stats, &tm_encoder::has_webp_export_stats, "webp export stats: this encoder has not written a WebP"); }

}  // extern "C"
