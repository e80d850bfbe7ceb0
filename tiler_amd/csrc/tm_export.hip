// tm_export.hip -- what leaves the encoder as files or pictures: Save (.gtm), ReloadGTM, GenerateY4M / GeneratePNGs / GenerateJPEGs, and the device
// render entry points tm_render_frames / tm_get_frame_quality (kernels in tm_render.hip).
#include <chrono>
#include <cmath>
#include <fstream>

#include "tm_deflate.h"
#include "tm_encoder.h"
#include "tm_gif_out.h"
#include "tm_webp_out.h"
#include "tm_gtm.h"
#include "tm_jpeg_out.h"

int save_to(tm_encoder *e, const char *path) {  // Save, tilingencoder.pas:2040-2058 -> SaveStream, 5177
  TM_TRY(need(e, TM_STEP_REINDEX, "Reindex"));
  TM_CHECK(path && *path, TM_E_INVAL, "Save: no output file name");
  TM_TRY(load_tail(e));
  TM_HIP(hipSetDevice(e->device));
  GtmInput in;
  in.tm_w = e->tm_w; in.tm_h = e->tm_h; in.nframes = e->nframes; in.fps = e->fps;
  in.kf_start = e->kf_start;
  std::vector<uint8_t> pal_px((size_t)e->t * 64);
  in.use.resize((size_t)e->t);
  if (e->t) {
    TM_HIP(hipMemcpy(pal_px.data(), e->gpal_px.p, pal_px.size(), hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(in.use.data(), e->guse.p, (size_t)e->t * 4, hipMemcpyDeviceToHost));
  }
  in.pal_px = pal_px.data();
  in.palettes = e->palettes_host.data();
  in.pal_count = e->s.PaletteCount; in.pal_size = e->s.PaletteSize;
  std::vector<tm_tilemap_item> tmi((size_t)e->q);
  TM_TRY(tm_get_tilemaps(e, 0, e->nframes, tmi.data()));
  in.tilemap = tmi.data();
  in.settings = settings_text(e->s);
  // the key frames' streams are coded side by side, their match lists found on this encoder's device unless TM_SAVE_FINDER says otherwise
  in.has_device = true; in.stream = e->stream; in.stats = &e->save_stats;
  e->has_save_stats = false;
  TM_TRY(write_gtm(path, in));
  e->has_save_stats = true;
  return TM_OK;
}

// ---- the decoded frames on the device (tm_render.hip): what tm_render_frames, tm_get_frame_quality and the exports draw
int render_range_ok(tm_encoder *e, int first, int count) {
  TM_CHECK(e->nframes > 0 && first >= 0 && count >= 0 && (int64_t)first + count <= e->nframes, TM_E_INVAL, "frame range [%d,+%d) outside 0..%d",
           first, count, e->nframes);
  return TM_OK;
}
int render_output_map(tm_encoder *e, RenderMap *m) {
  TM_CHECK(e->has_pal_px && (e->steps_done & (1 << TM_STEP_RECONSTRUCT)) && e->tm_tile.p && e->tm_pal.p && e->fflags.p && e->palettes_dev.p, TM_E_INVAL,
           "output frames: Reconstruct (or ReloadGTM) has not been run");
  const bool pm = e->has_pm && e->tm_pred.p && e->tm_px.p && e->tm_py.p;
  // (the palettes as made: a PaletteCount set since then does not reach past them)
  const int npal = (int)std::min<int64_t>(e->s.PaletteCount, (int64_t)e->palettes_host.size() / std::max(1, e->s.PaletteSize));
  *m = RenderMap{e->tm_tile.as<int32_t>(), e->tm_pal.as<int32_t>(), e->fflags.as<uint8_t>(), pm ? e->tm_pred.as<uint8_t>() : nullptr, 0xff,
                 pm ? e->tm_px.as<int8_t>() : nullptr, pm ? e->tm_py.as<int8_t>() : nullptr, e->gpal_px.as<uint8_t>(), e->t,
                 e->palettes_dev.as<int32_t>(), npal, e->s.PaletteSize, e->tm_w, e->tm_h};
  return TM_OK;
}
int render_input_src(tm_encoder *e, int first, int count, RenderInput *in) {
  TM_CHECK(e->src_tiles && (e->steps_done & (1 << TM_STEP_LOAD)) && e->ftiles.p && e->fflags.p, TM_E_INVAL,
           "source frames: the frame tiles are not in memory (run Load; ReloadGTM does not bring them)");
  TM_CHECK(!e->load_sharded || (first >= e->load_first && first + count <= e->load_first + e->load_count), TM_E_INVAL,
           "source frames: this process's Load kept frames [%d,+%d) only, not [%d,+%d)", e->load_first, e->load_count, first, count);
  *in = RenderInput{e->ftiles.as<uint32_t>(), e->fflags.as<uint8_t>(), e->tm_w, e->tm_h};
  return TM_OK;
}

// ---- GenerateY4M / GeneratePNGs (tilingencoder.pas:2126-2199, 2075-2124): the frames as Render (3455-3640) draws them with the
// constructor's defaults (FRenderPredicted, FRenderMirrored, FRenderOutputDithered on, no gamma: 5505-5507) -- the device render's
// pictures, brought to the host a chunk of frames at a time.  An export refuses exactly what the device render of the whole clip refuses
// (init, before any file is opened: a refused call leaves no file behind).  In a device group it reads shard 0, the front encoder.
namespace {
struct ExportFrames {
  tm_encoder *e;
  bool input;
  bool y4m = false;  // the frames come to the host as GenerateY4M's planes (Y, U, V of a frame in a row: 3 bytes a pixel), not as RGB32
  bool keep = false; // the frames stay on the device as RGB32 (GeneratePNGs at level 1 codes them there): dev holds frames [first, first + count)
  RenderMap m{};
  RenderInput in{};
  int sw = 0, sh = 0, chunk = 0, first = 0, count = 0;
  DevBuf dev;
  std::vector<uint32_t> host;  // frames [first, first + count), 0x00RRGGBB
  DevBuf dev_yuv;
  std::vector<uint8_t> host_yuv;
  tm_yuv_out planes{};
  YuvOutPlan plan;
  int init() {
    TM_HIP(hipSetDevice(e->device));
    if (input) TM_TRY(render_input_src(e, 0, e->nframes, &in));
    else TM_TRY(render_output_map(e, &m));
    sw = e->tm_w * 8; sh = e->tm_h * 8;
    const size_t fbytes = (size_t)sw * sh * 4;
    chunk = (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)256 << 20) / fbytes));  // 32 frames or 256 MB, whichever is less
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
  int frame(int f, const uint32_t **px) {  // frames are asked for in order
    if (f >= first + count) {
      first = f;
      count = std::min(chunk, e->nframes - f);
      TM_TRY(input ? launch_render_input(in, first, count, dev.p, e->stream) : launch_render_output(m, first, count, dev.p, e->stream));
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

// a finished PNG (pf24bit, 2086; its bytes are made by png_stored of tm_deflate.hip or on the device by tm_png_out.hip) to its file
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
  const auto wall0 = std::chrono::steady_clock::now();
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
  // level 0: a chunk of frames comes to the host and each is written in stored blocks.  Level 1: the chunk stays on the device, is coded
  // there (tm_png_out.hip), and only the files' bytes come back
  tm_export_stats st{};
  st.level = opt.level; st.filter = opt.level ? filter : opt.filter;
  std::vector<uint8_t> file;
  std::vector<std::vector<uint8_t>> files;
  dfl::PngDeviceEncoder encoder;  // (its device buffers serve every chunk)
  for (int fr = 0; fr < e->nframes; fr++) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool fresh = fr >= r.first + r.count;
    const uint32_t *px = nullptr;
    TM_TRY(r.frame(fr, &px));
    if (fresh && opt.level) TM_TRY(encoder.encode(r.dev.as<uint32_t>(), r.sw, (int64_t)r.sw * r.sh, r.count, r.sw, r.sh, filter, e->stream, files));
    const auto t1 = std::chrono::steady_clock::now();
    if (!opt.level) dfl::png_stored(px, r.sw, r.sw, r.sh, file);
    const std::vector<uint8_t> &bytes = opt.level ? files[(size_t)(fr - r.first)] : file;
    char name[32];
    snprintf(name, sizeof(name), "_%04d.png", fr);
    TM_TRY(write_file(base + name, bytes));
    const auto t2 = std::chrono::steady_clock::now();
    st.frames++; st.file_bytes += (int64_t)bytes.size();
    st.ms_device += std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_write += std::chrono::duration<double, std::milli>(t2 - t1).count();
  }
  st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
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
  const auto wall0 = std::chrono::steady_clock::now();
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
  std::vector<std::vector<uint8_t>> files;
  jpo::JpegDeviceEncoder encoder;  // (its device buffers serve every chunk)
  for (int fr = 0; fr < e->nframes; fr++) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool fresh = fr >= r.first + r.count;
    TM_TRY(r.frame(fr, nullptr));
    if (fresh) TM_TRY(encoder.encode(r.dev.as<uint32_t>(), r.sw, (int64_t)r.sw * r.sh, r.count, r.sw, r.sh, opt, e->stream, files));
    const auto t1 = std::chrono::steady_clock::now();
    const std::vector<uint8_t> &bytes = files[(size_t)(fr - r.first)];
    if (path) {
      all.write((const char *)bytes.data(), (std::streamsize)bytes.size());
      TM_CHECK(all.good(), TM_E_IO, "write to %s failed", path);
    } else {
      char name[32];
      snprintf(name, sizeof(name), "_%04d.jpg", fr);
      TM_TRY(write_file(base + name, bytes));
    }
    const auto t2 = std::chrono::steady_clock::now();
    st.frames++; st.file_bytes += (int64_t)bytes.size();
    st.ms_device += std::chrono::duration<double, std::milli>(t1 - t0).count();
    st.ms_write += std::chrono::duration<double, std::milli>(t2 - t1).count();
  }
  st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  e->jpeg_export_stats = st;
  e->has_jpeg_export_stats = true;
  return TM_OK;
}

// GenerateGIF: the frames GeneratePNGs writes as one animated GIF, kept on the device a chunk at a time and coded
// there (tm_gif_out.hip); only the file's bytes come back.  The file is opened once every chunk has been coded: a refused frame leaves none.
static int generate_gif(tm_encoder *e, const char *path, bool input) {
  TM_CHECK(path && *path, TM_E_INVAL, "GenerateGIF: no file name");
  const auto wall0 = std::chrono::steady_clock::now();
  const tm_gif_options opt = e->gif_options;
  e->has_gif_export_stats = false;
  ExportFrames r{e, input};
  r.keep = true;
  TM_TRY(r.init());
  int delay;
  TM_TRY(gfo::gif_out_check("GenerateGIF", r.dev.p, r.sw, (int64_t)r.sw * r.sh, e->nframes, r.sw, r.sh, e->fps, &opt, &delay));
  std::vector<uint8_t> file;
  gfo::GifDeviceEncoder encoder;  // (its device buffers serve every chunk)
  TM_TRY(encoder.begin(r.sw, r.sh, e->fps, opt, e->stream, file));
  const auto t0 = std::chrono::steady_clock::now();
  for (int fr = 0; fr < e->nframes; fr += r.count) {
    TM_TRY(r.frame(fr, nullptr));
    TM_TRY(encoder.chunk(r.dev.as<uint32_t>(), r.sw, (int64_t)r.sw * r.sh, r.count, file));
  }
  TM_TRY(encoder.end(file));
  const auto t1 = std::chrono::steady_clock::now();
  TM_TRY(write_file(path, file));
  tm_gif_export_stats st = encoder.stats;
  st.ms_device = std::chrono::duration<double, std::milli>(t1 - t0).count();
  st.ms_write = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  e->gif_export_stats = st;
  e->has_gif_export_stats = true;
  return TM_OK;
}

// GenerateWebP: the frames GeneratePNGs writes as one animated lossless WebP, kept on the device a chunk at a time and
// coded there (tm_webp_out.hip); only the file's bytes come back.  The file is opened once every chunk has been coded.
static int generate_webp(tm_encoder *e, const char *path, bool input) {
  TM_CHECK(path && *path, TM_E_INVAL, "GenerateWebP: no file name");
  const auto wall0 = std::chrono::steady_clock::now();
  const tm_webp_options opt = e->webp_options;
  e->has_webp_export_stats = false;
  ExportFrames r{e, input};
  r.keep = true;
  TM_TRY(r.init());
  int duration;
  TM_TRY(wpo::webp_out_check("GenerateWebP", r.dev.p, r.sw, (int64_t)r.sw * r.sh, e->nframes, r.sw, r.sh, e->fps, &opt, &duration));
  std::vector<uint8_t> file;
  wpo::WebpDeviceEncoder encoder;  // (its device buffers serve every chunk)
  TM_TRY(encoder.begin(r.sw, r.sh, e->fps, opt, e->stream, file));
  const auto t0 = std::chrono::steady_clock::now();
  for (int fr = 0; fr < e->nframes; fr += r.count) {
    TM_TRY(r.frame(fr, nullptr));
    for (int f0 = 0; f0 < r.count; f0 += wpo::kMaxChunk)
      TM_TRY(encoder.chunk(r.dev.as<uint32_t>() + (int64_t)f0 * r.sw * r.sh, r.sw, (int64_t)r.sw * r.sh, std::min((int)wpo::kMaxChunk, r.count - f0), file));
  }
  TM_TRY(encoder.end(file));
  const auto t1 = std::chrono::steady_clock::now();
  TM_TRY(write_file(path, file));
  tm_webp_export_stats st = encoder.stats;
  st.ms_device = std::chrono::duration<double, std::milli>(t1 - t0).count();
  st.ms_write = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  e->webp_export_stats = st;
  e->has_webp_export_stats = true;
  return TM_OK;
}

extern "C" {

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

int tm_get_webp_options(tm_encoder *e, tm_webp_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  *opt = e->webp_options;
  return TM_OK;
}

int tm_get_webp_export_stats(tm_encoder *e, tm_webp_export_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_webp_export_stats, TM_E_INVAL, "webp export stats: this encoder has not written a WebP");
  *out = e->webp_export_stats;
  return TM_OK;
}

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

int tm_get_gif_options(tm_encoder *e, tm_gif_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  *opt = e->gif_options;
  return TM_OK;
}

int tm_get_gif_export_stats(tm_encoder *e, tm_gif_export_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_gif_export_stats, TM_E_INVAL, "gif export stats: this encoder has not written a GIF");
  *out = e->gif_export_stats;
  return TM_OK;
}

int tm_reload_gtm(tm_encoder *e, const char *path) {  // ReloadGTM, tilingencoder.pas:2059 -> LoadStream, 4880-5175
  TM_CHECK(e && path, TM_E_INVAL, "null argument");
  TM_CHECK(e->nframes > 0 && e->width > 0, TM_E_INVAL, "tm_set_video has not been called");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_reload_gtm(s, path); });
  GtmLoaded g;
  TM_TRY(read_gtm(path, &g));
  // "Mismatch between GTM and loaded video!" (5021-5032)
  TM_CHECK(g.header_frames < 0 || (g.header_frames == e->nframes && g.header_w == e->tm_w * 8 && g.header_h == e->tm_h * 8), TM_E_INVAL,
           "mismatch between GTM (%d frames, %dx%d) and loaded video (%d frames, %dx%d)", g.header_frames, g.header_w, g.header_h, e->nframes,
           e->tm_w * 8, e->tm_h * 8);
  TM_CHECK(g.nframes == e->nframes && g.tm_w == e->tm_w && g.tm_h == e->tm_h, TM_E_INVAL, "GTM stream does not match the loaded video");
  TM_HIP(hipSetDevice(e->device));
  const int64_t q = (int64_t)e->nframes * e->tm_size(), T = (int64_t)g.use.size();
  e->q = q; e->t = T; e->fps = g.fps;
  e->s.PaletteSize = g.pal_size; e->s.PaletteCount = std::max(1, g.pal_count);
  TM_TRY(load_tail(e));  // (not after these lines: a pending tail would put Load's key frames over the stream's)
  e->kf_start = g.kf_start;
  e->correl.assign((size_t)e->nframes, 0.0f);
  e->palettes_host.assign(g.palettes.begin(), g.palettes.end());
  e->palettes_host.resize((size_t)e->s.PaletteCount * e->s.PaletteSize, 0);
  TM_TRY(e->palettes_dev.alloc(e->palettes_host.size() * 4));
  TM_HIP(hipMemcpy(e->palettes_dev.p, e->palettes_host.data(), e->palettes_host.size() * 4, hipMemcpyHostToDevice));
  e->pair_keys_n = 0;
  TM_TRY(e->gtiles.alloc((size_t)std::max<int64_t>(T, 1) * 256)); TM_TRY(e->gpal_px.alloc((size_t)std::max<int64_t>(T, 1) * 64));
  TM_TRY(e->gflags.alloc((size_t)std::max<int64_t>(T, 1))); TM_TRY(e->guse.alloc((size_t)std::max<int64_t>(T, 1) * 4));
  TM_TRY(e->gpal_idx.alloc((size_t)std::max<int64_t>(T, 1) * 4));
  TM_HIP(hipMemset(e->gtiles.p, 0, (size_t)std::max<int64_t>(T, 1) * 256));  // the stream carries no RGB pixels (HasRGBPixels = False, 4937)
  TM_HIP(hipMemset(e->gflags.p, 0, (size_t)std::max<int64_t>(T, 1)));
  TM_HIP(hipMemset(e->gpal_idx.p, 0xff, (size_t)std::max<int64_t>(T, 1) * 4));
  if (T) {
    TM_HIP(hipMemcpy(e->gpal_px.p, g.pal_px.data(), (size_t)T * 64, hipMemcpyHostToDevice));
    TM_HIP(hipMemcpy(e->guse.p, g.use.data(), (size_t)T * 4, hipMemcpyHostToDevice));
  }
  std::vector<int32_t> ti((size_t)q), pi((size_t)q);
  std::vector<uint32_t> er((size_t)q, 0xffffffffu);
  std::vector<int8_t> px((size_t)q), py((size_t)q);
  std::vector<uint8_t> pr((size_t)q);
  e->h_fflags.assign((size_t)q, 0);
  for (int64_t i = 0; i < q; i++) {
    const tm_tilemap_item &it = g.tilemap[(size_t)i];
    ti[(size_t)i] = it.TileIdx; pi[(size_t)i] = it.PalIdx; px[(size_t)i] = it.PredictedX; py[(size_t)i] = it.PredictedY;
    pr[(size_t)i] = (it.Flags & 4) ? 1 : 0;
    e->h_fflags[(size_t)i] = (uint8_t)(it.Flags & 3);
  }
  TM_TRY(e->tm_tile.alloc((size_t)q * 4)); TM_TRY(e->tm_pal.alloc((size_t)q * 4)); TM_TRY(e->tm_err.alloc((size_t)q * 4));
  TM_TRY(e->tm_px.alloc((size_t)q)); TM_TRY(e->tm_py.alloc((size_t)q)); TM_TRY(e->tm_pred.alloc((size_t)q)); TM_TRY(e->pm_err.alloc((size_t)q * 4));
  TM_TRY(e->fflags.alloc((size_t)q));
  TM_HIP(hipMemcpy(e->tm_tile.p, ti.data(), (size_t)q * 4, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->tm_pal.p, pi.data(), (size_t)q * 4, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->tm_err.p, er.data(), (size_t)q * 4, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->pm_err.p, er.data(), (size_t)q * 4, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->tm_px.p, px.data(), (size_t)q, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->tm_py.p, py.data(), (size_t)q, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->tm_pred.p, pr.data(), (size_t)q, hipMemcpyHostToDevice));
  TM_HIP(hipMemcpy(e->fflags.p, e->h_fflags.data(), (size_t)q, hipMemcpyHostToDevice));
  e->has_pm = true;
  e->has_pal_px = true;
  e->reconstructed = false;  // PSNR is not in the stream
  e->src_tiles = false;      // (the mirror flags are the stream's now; the source frames need a Load)
  e->gtiles_have_rgb = false;
  e->drop_prefetch();
  // every step's product the stream holds is in place: Save, Reindex and the read-back views work.  Steps that compute from the frame
  // tiles or from RGB pixels check for them (need_frame_tiles / need_global_rgb) and ask for Load / Reduce when they are missing.
  e->steps_done = 0xff;
  return TM_OK;
}

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

int tm_get_png_options(tm_encoder *e, tm_png_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  *opt = e->png_options;
  return TM_OK;
}

int tm_get_export_stats(tm_encoder *e, tm_export_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_export_stats, TM_E_INVAL, "export stats: this encoder has not written PNGs");
  *out = e->export_stats;
  return TM_OK;
}

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

int tm_get_jpeg_options(tm_encoder *e, tm_jpeg_options *opt) {
  TM_CHECK(e && opt, TM_E_INVAL, "null argument");
  *opt = e->jpeg_options;
  return TM_OK;
}

int tm_get_jpeg_export_stats(tm_encoder *e, tm_jpeg_export_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_jpeg_export_stats, TM_E_INVAL, "jpeg export stats: this encoder has not written JPEGs");
  *out = e->jpeg_export_stats;
  return TM_OK;
}

int tm_save_gtm(tm_encoder *e, const char *path) {
  TM_CHECK(e && path, TM_E_INVAL, "null argument");
  return save_to(e, path);
}

int tm_render_frames(tm_encoder *e, int first_frame, int frame_count, int input, void *out, int out_on_device) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  if (e->grp && input && e->load_sharded && frame_count > 0) {
    // the source frames of a sharded Load: every shard draws the piece of the range it loaded
    const std::vector<Piece> pc = group_pieces(e, first_frame, frame_count);
    const size_t fb = (size_t)e->tm_w * 8 * e->tm_h * 8 * 4;
    const int home = e->device;
    return group_each(e, [&](tm_encoder *s) -> int {
      const Piece p = pc[(size_t)s->co.rank];
      if (p.count == 0) return TM_OK;
      uint8_t *dst = (uint8_t *)out + fb * (size_t)(p.first - first_frame);
      if (!out_on_device || s->device == home) return tm_render_frames(s, p.first, p.count, 1, dst, out_on_device);
      DevBuf tmp;  // another device: drawn here, then copied to the caller's device
      TM_TRY(tmp.alloc(fb * p.count));
      TM_TRY(tm_render_frames(s, p.first, p.count, 1, tmp.p, 1));
      TM_HIP(hipMemcpyPeer(dst, home, tmp.p, s->device, fb * p.count));
      return TM_OK;
    });
  }
  TM_HIP(hipSetDevice(e->device));
  RenderMap m{};
  RenderInput in{};
  if (input) TM_TRY(render_input_src(e, first_frame, frame_count, &in));
  else TM_TRY(render_output_map(e, &m));
  if (frame_count == 0) return TM_OK;
  const size_t bytes = (size_t)frame_count * e->tm_w * 8 * e->tm_h * 8 * 4;
  DevBuf tmp;
  void *dst = out;
  if (!out_on_device) {
    TM_TRY(tmp.alloc(bytes));
    dst = tmp.p;
  }
  TM_TRY(input ? launch_render_input(in, first_frame, frame_count, dst, e->stream) : launch_render_output(m, first_frame, frame_count, dst, e->stream));
  if (!out_on_device) TM_HIP(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, e->stream));  // page-locked destination: one DMA
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

int tm_render_frames_yuv(tm_encoder *e, int first_frame, int frame_count, int input, const tm_yuv_out *dst, int mode) {
  TM_CHECK(e, TM_E_INVAL, "null argument");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  YuvOutPlan plan;
  TM_TRY(check_yuv_out(dst, e->tm_w * 8, e->tm_h * 8, mode, &plan));
  TM_CHECK(frame_count <= dst->frames, TM_E_INVAL, "yuv out: %d frames asked for, room for %d", frame_count, dst->frames);
  TM_HIP(hipSetDevice(e->device));
  RenderMap m{};
  RenderInput in{};
  if (input) TM_TRY(render_input_src(e, first_frame, frame_count, &in));
  else TM_TRY(render_output_map(e, &m));
  const bool to_device = dst->memory == TM_MEM_DEVICE;
  if (to_device) TM_TRY(yuv_out_is_device(*dst, e->device));
  if (frame_count == 0) return TM_OK;
  // a chunk of frames is drawn as RGB32 and converted behind the render; host planes go through a packed chunk, one copy per plane
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  const size_t fbytes = (size_t)sw * sh * 4;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(frame_count, 32), ((size_t)256 << 20) / fbytes));
  DevBuf rgb, packed;
  TM_TRY(rgb.alloc(fbytes * chunk));
  if (!to_device) TM_TRY(packed.alloc((size_t)plan.frame_bytes() * chunk));
  for (int f0 = 0; f0 < frame_count; f0 += chunk) {
    const int nf = std::min(chunk, frame_count - f0);
    TM_TRY(input ? launch_render_input(in, first_frame + f0, nf, rgb.p, e->stream) : launch_render_output(m, first_frame + f0, nf, rgb.p, e->stream));
    TM_TRY(launch_rgb32_to_yuv(plan, rgb.p, sw, nf, to_device ? yuv_dst_of(*dst, f0) : yuv_dst_packed(plan, packed.as<uint8_t>(), chunk, 0), e->stream));
    if (!to_device) TM_TRY(yuv_copy_out(plan, packed.as<uint8_t>(), chunk, *dst, f0, nf, e->stream));
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

// ---- the same frames at a caller's size (tm_scale.hip): drawn natively a chunk at a time -- at most 32 frames or
// 256 MB, of either size -- scaled behind the render on the encoder's stream, then delivered or converted
static int scaled_chunk_frames(int frame_count, size_t native_bytes, size_t scaled_bytes) {
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(frame_count, 32), ((size_t)256 << 20) / std::max(native_bytes, scaled_bytes)));
}

int tm_render_frames_scaled(tm_encoder *e, int first_frame, int frame_count, int input, int out_w, int out_h, int filter, void *out, int out_on_device) {
  TM_CHECK(e && (out || frame_count == 0), TM_E_INVAL, "null argument");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  ScaleTables tables;
  TM_TRY(tables.prepare(sw, sh, out_w, out_h, filter));
  const bool gathered = e->grp && input && e->load_sharded;  // tm_render_frames asks every shard for its piece (and makes the checks there)
  RenderMap m{};
  RenderInput in{};
  if (!gathered) TM_TRY(input ? render_input_src(e, first_frame, frame_count, &in) : render_output_map(e, &m));
  if (frame_count == 0) return TM_OK;
  TM_HIP(hipSetDevice(e->device));
  const int64_t spx = (int64_t)sw * sh, opx = (int64_t)out_w * out_h;
  const int chunk = scaled_chunk_frames(frame_count, (size_t)spx * 4, (size_t)opx * 4);
  DevBuf native, scaled;
  TM_TRY(native.alloc((size_t)spx * 4 * chunk));
  if (!out_on_device) TM_TRY(scaled.alloc((size_t)opx * 4 * chunk));
  TM_TRY(tables.upload(e->stream));
  for (int f0 = 0; f0 < frame_count; f0 += chunk) {
    const int nf = std::min(chunk, frame_count - f0);
    TM_TRY(tm_render_frames(e, first_frame + f0, nf, input, native.p, 1));  // (blocking: the chunk before has left `native` and `scaled`)
    TM_HIP(hipSetDevice(e->device));
    uint32_t *to = out_on_device ? (uint32_t *)out + opx * f0 : scaled.as<uint32_t>();
    TM_TRY(launch_scale_rgb32(tables, native.p, sw, spx, nf, to, out_w, opx, e->stream));
    if (!out_on_device) TM_HIP(hipMemcpyAsync((uint32_t *)out + opx * f0, to, (size_t)opx * 4 * nf, hipMemcpyDeviceToHost, e->stream));
    TM_HIP(hipStreamSynchronize(e->stream));
  }
  return TM_OK;
}

int tm_render_frames_yuv_scaled(tm_encoder *e, int first_frame, int frame_count, int input, const tm_yuv_out *dst, int mode, int filter) {
  TM_CHECK(e, TM_E_INVAL, "null argument");
  TM_CHECK(dst, TM_E_INVAL, "yuv out: null descriptor");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  const int sw = e->tm_w * 8, sh = e->tm_h * 8, ow = dst->width, oh = dst->height;
  ScaleTables tables;
  TM_TRY(tables.prepare(sw, sh, ow, oh, filter));
  YuvOutPlan plan;
  TM_TRY(check_yuv_out(dst, ow, oh, mode, &plan));
  TM_CHECK(frame_count <= dst->frames, TM_E_INVAL, "yuv out: %d frames asked for, room for %d", frame_count, dst->frames);
  RenderMap m{};
  RenderInput in{};
  TM_TRY(input ? render_input_src(e, first_frame, frame_count, &in) : render_output_map(e, &m));  // (shard 0 of a group, as tm_render_frames_yuv reads)
  TM_HIP(hipSetDevice(e->device));
  const bool to_device = dst->memory == TM_MEM_DEVICE;
  if (to_device) TM_TRY(yuv_out_is_device(*dst, e->device));
  if (frame_count == 0) return TM_OK;
  const int64_t spx = (int64_t)sw * sh, opx = (int64_t)ow * oh;
  const int chunk = scaled_chunk_frames(frame_count, (size_t)spx * 4, (size_t)opx * 4);
  DevBuf native, scaled, packed;
  TM_TRY(native.alloc((size_t)spx * 4 * chunk));
  TM_TRY(scaled.alloc((size_t)opx * 4 * chunk));
  if (!to_device) TM_TRY(packed.alloc((size_t)plan.frame_bytes() * chunk));
  TM_TRY(tables.upload(e->stream));
  for (int f0 = 0; f0 < frame_count; f0 += chunk) {
    const int nf = std::min(chunk, frame_count - f0);
    TM_TRY(input ? launch_render_input(in, first_frame + f0, nf, native.p, e->stream) : launch_render_output(m, first_frame + f0, nf, native.p, e->stream));
    TM_TRY(launch_scale_rgb32(tables, native.p, sw, spx, nf, scaled.p, ow, opx, e->stream));
    TM_TRY(launch_rgb32_to_yuv(plan, scaled.p, ow, nf, to_device ? yuv_dst_of(*dst, f0) : yuv_dst_packed(plan, packed.as<uint8_t>(), chunk, 0), e->stream));
    if (!to_device) TM_TRY(yuv_copy_out(plan, packed.as<uint8_t>(), chunk, *dst, f0, nf, e->stream));
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

int tm_get_frame_quality(tm_encoder *e, int first_frame, int frame_count, uint64_t *sse, double *psnr, double *ssim_y, double *clip_psnr,
                         double *clip_ssim_y) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  TM_CHECK(frame_count > 0, TM_E_INVAL, "frame quality: no frames");
  std::vector<uint64_t> h_sse((size_t)frame_count * 3);
  std::vector<double> h_ssim((size_t)frame_count);
  if (e->grp && e->load_sharded) {
    // a sharded Load: every shard measures the piece of the range it loaded, the frames' sums are combined below in frame order
    const std::vector<Piece> pc = group_pieces(e, first_frame, frame_count);
    TM_TRY(group_each(e, [&](tm_encoder *s) {
      const Piece p = pc[(size_t)s->co.rank];
      if (p.count == 0) return (int)TM_OK;
      const size_t off = (size_t)(p.first - first_frame);
      return tm_get_frame_quality(s, p.first, p.count, h_sse.data() + off * 3, nullptr, h_ssim.data() + off, nullptr, nullptr);
    }));
  } else {
  TM_HIP(hipSetDevice(e->device));
  RenderMap m{};
  RenderInput in{};
  TM_TRY(render_output_map(e, &m));
  TM_TRY(render_input_src(e, first_frame, frame_count, &in));
  DevBuf d_sse, d_ssim;
  TM_TRY(d_sse.alloc((size_t)frame_count * 3 * 8));
  TM_TRY(d_ssim.alloc((size_t)frame_count * 8));
  TM_TRY(launch_quality_render(in, m, first_frame, frame_count, d_sse.p, d_ssim.p, e->stream));
  TM_HIP(hipMemcpyAsync(h_sse.data(), d_sse.p, h_sse.size() * 8, hipMemcpyDeviceToHost, e->stream));
  TM_HIP(hipMemcpyAsync(h_ssim.data(), d_ssim.p, h_ssim.size() * 8, hipMemcpyDeviceToHost, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));
  }
  // PSNR = 10 log10(3 W H 255^2 / SSE) over the three channels; the clip's from the summed SSE, its SSIM the mean of the frames'
  const double peak = 3.0 * (e->tm_w * 8) * (e->tm_h * 8) * 255.0 * 255.0;
  auto to_psnr = [](double top, uint64_t err) { return err ? 10.0 * std::log10(top / (double)err) : HUGE_VAL; };
  uint64_t total = 0;
  double ssum = 0.0;
  for (int f = 0; f < frame_count; f++) {
    const uint64_t fe = h_sse[(size_t)f * 3] + h_sse[(size_t)f * 3 + 1] + h_sse[(size_t)f * 3 + 2];
    total += fe;
    ssum += h_ssim[(size_t)f];
    if (psnr) psnr[f] = to_psnr(peak, fe);
  }
  if (sse) memcpy(sse, h_sse.data(), h_sse.size() * 8);
  if (ssim_y) memcpy(ssim_y, h_ssim.data(), h_ssim.size() * 8);
  if (clip_psnr) *clip_psnr = to_psnr(peak * frame_count, total);
  if (clip_ssim_y) *clip_ssim_y = ssum / frame_count;
  return TM_OK;
}

}  // extern "C"
