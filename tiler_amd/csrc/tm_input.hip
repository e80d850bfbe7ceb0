// tm_input.hip -- Load's input: where the clip comes from when it is not pushed in as RGB32 -- the choice among the sources (load_from_input)
// and the API around them (tm_open_input, tm_set_frames_yuv / _rgb / _png / _jpeg / _gif, the decode places, tm_get_video, tm_set_input_yuv).
// The sources: tm_input_clip.hip (a Y4M file, clips lent in memory, a .gtm stream) and tm_input_files.hip (PNG and JPEG sequences, a GIF).
// What a name turns out to be: tm_input_probe.hip; shared: tm_input.h.
#include "tm_encoder.h"
#include "tm_inflate.h"
#include "tm_gif.h"
#include "tm_jpeg.h"

static bool png_kind(int kind) { return kind == TM_INPUT_PNGS || kind == INPUT_PNG_CLIP; }
static bool jpeg_kind(int kind) { return kind == TM_INPUT_JPEGS || kind == INPUT_JPEG_CLIP; }
static bool gif_kind(int kind) { return kind == TM_INPUT_GIF || kind == INPUT_GIF_CLIP; }

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

// what tm_set_frames_png / _jpeg / _gif describe: `nfiles` coded files lent in memory that hold `frames` frames of w x h (RGB unless the caller says otherwise)
static InputInfo lent_files(int kind, const void *const *files, const size_t *sizes, int nfiles, int frames, int w, int h, double fps) {
  InputInfo in;
  in.kind = kind;
  in.png_files.assign(files, files + nfiles);
  in.png_sizes.assign(sizes, sizes + nfiles);
  in.lent = true;
  in.frames = frames; in.src_w = in.dst_w = w; in.src_h = in.dst_h = h;
  in.chroma = TM_CHROMA_444; in.fps = fps;
  return in;
}
// tm_set_png_decode / _jpeg_decode / _gif_decode: `where` into the encoder's field `place`, in every shard of a group; bad_place is the refusal's text
static int set_decode_place(tm_encoder *e, int where, int tm_encoder::*place, const char *bad_place) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(where >= TM_PNG_DECODE_AUTO && where <= TM_PNG_DECODE_DEVICE, TM_E_INVAL, bad_place, where);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return set_decode_place(s, where, place, bad_place); });
  e->*place = where;
  return TM_OK;
}
static int get_decode_place(tm_encoder *e, int *where, int tm_encoder::*place) {
  TM_CHECK(e && where, TM_E_INVAL, "null argument");
  *where = e->*place;
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
  e->input = lent_files(INPUT_PNG_CLIP, files, sizes, nframes, nframes, w, h, fps);
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
  InputInfo in = lent_files(INPUT_JPEG_CLIP, files, sizes, nframes, nframes, w, h, fps);
  in.chroma = info.layout(); in.full_range = 1;  // (JFIF: full-range BT.601)
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
  e->input = lent_files(INPUT_GIF_CLIP, &file, &size, 1, n, w, h, rate);
  e->input_clip.clear();
  return TM_OK;
}

int tm_set_gif_decode(tm_encoder *e, int where) { return set_decode_place(e, where, &tm_encoder::gif_decode, "bad GIF decode place %d"); }
int tm_get_gif_decode(tm_encoder *e, int *where) { return get_decode_place(e, where, &tm_encoder::gif_decode); }

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

int tm_set_jpeg_decode(tm_encoder *e, int where) { return set_decode_place(e, where, &tm_encoder::jpeg_decode, "bad JPEG decode place %d"); }
int tm_get_jpeg_decode(tm_encoder *e, int *where) { return get_decode_place(e, where, &tm_encoder::jpeg_decode); }

int tm_set_png_decode(tm_encoder *e, int where) { return set_decode_place(e, where, &tm_encoder::png_decode, "bad PNG decode place %d"); }
int tm_get_png_decode(tm_encoder *e, int *where) { return get_decode_place(e, where, &tm_encoder::png_decode); }

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
