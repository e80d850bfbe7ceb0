// tm_input_probe.hip -- the probe half of Load (tilingencoder.pas:1764-1820), host code only: what InputFileName turns out to be -- a .gtm
// stream, a Y4M file, or the pattern of a numbered PNG sequence -- with its sizes, rate and frame range, and the size Scaling makes of it.
#include <sys/stat.h>

#include <cmath>

#include "tm_gtm.h"
#include "tm_input.h"
#include "tm_gif.h"
#include "tm_jpeg.h"

namespace tmx {

// ---- probing (host) --------------------------------------------------------------------------------------------
static bool file_exists(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

static int pas_round_dim(double v) {  // Round(W * Scaling), at least 1 (extern.pas:780-781)
  return (int)std::max<long long>(1, llrint(v));
}
// the size a file or a lent clip is scaled to
int scaled_size(int w, int h, double scaling, int *dst_w, int *dst_h) {
  *dst_w = pas_round_dim(w * scaling);
  *dst_h = pas_round_dim(h * scaling);
  TM_CHECK((double)w / *dst_w <= 8.0 && (double)h / *dst_h <= 8.0, TM_E_UNSUPPORTED, "Scaling %g shrinks %dx%d by more than 8 (more than %d taps)", scaling, w, h,
           TM_RESAMPLE_MAX_TAPS);
  return TM_OK;
}
// the frames Load takes of a file that holds `total` (1778-1782): FrameCount of them from StartFrame on, or all that follow it
static int frame_range(const std::string &name, int64_t total, const char *what, int start_frame, int frame_count, int *frames) {
  const int64_t cnt = frame_count > 0 ? frame_count : total - start_frame;
  TM_CHECK(cnt > 0 && start_frame + cnt <= total, TM_E_INVAL, "%s holds %lld %s: frames [%d,+%lld) are not all there", name.c_str(), (long long)total, what, start_frame,
           (long long)cnt);
  *frames = (int)cnt;
  return TM_OK;
}

// Pascal's Format(pattern, [i]) for a pattern with exactly one integer specifier, %d or %.Nd; %% is a literal
int format_pattern(const std::string &pat, int64_t i, std::string *out) {
  out->clear();
  int specs = 0;
  for (size_t p = 0; p < pat.size(); p++) {
    if (pat[p] != '%') { *out += pat[p]; continue; }
    if (p + 1 < pat.size() && pat[p + 1] == '%') { *out += '%'; p++; continue; }
    size_t q = p + 1;
    int prec = 0;
    if (q < pat.size() && pat[q] == '.') {
      q++;
      TM_CHECK(q < pat.size() && isdigit((unsigned char)pat[q]), TM_E_INVAL, "input pattern '%s': digits expected after '%%.'", pat.c_str());
      while (q < pat.size() && isdigit((unsigned char)pat[q])) prec = std::min(prec * 10 + (pat[q++] - '0'), 64);
    }
    TM_CHECK(q < pat.size() && (pat[q] == 'd' || pat[q] == 'D'), TM_E_INVAL, "input pattern '%s': only %%d and %%.Nd are understood", pat.c_str());
    char buf[96];
    snprintf(buf, sizeof(buf), "%.*lld", prec, (long long)i);
    *out += buf;
    specs++;
    p = q;
  }
  TM_CHECK(specs == 1, TM_E_INVAL, "'%s' is neither an existing file nor a pattern with one %%d or %%.Nd", pat.c_str());
  return TM_OK;
}

static std::string change_ext(const std::string &p, const char *ext) {  // ChangeFileExt
  const size_t dot = p.find_last_of('.'), sep = p.find_last_of("/\\");
  return ((dot != std::string::npos && (sep == std::string::npos || dot > sep)) ? p.substr(0, dot) : p) + ext;
}

static int parse_y4m(const std::string &name, InputInfo *in) {
  FILE *f = fopen(name.c_str(), "rb");
  TM_CHECK(f, TM_E_IO, "cannot open %s", name.c_str());
  struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
  char line[1024];
  const size_t got = fread(line, 1, sizeof(line) - 1, f);
  line[got] = 0;
  TM_CHECK(got >= 10 && !memcmp(line, "YUV4MPEG2 ", 10), TM_E_UNSUPPORTED,
           "%s is not a Y4M file and there is no decoder in this build; convert with `ffmpeg -i ... -f yuv4mpegpipe`", name.c_str());
  const char *nl = (const char *)memchr(line, '\n', got);
  TM_CHECK(nl, TM_E_INVAL, "%s: the Y4M header has no end", name.c_str());
  int w = 0, h = 0, chroma = TM_CHROMA_420JPEG, full = 0;
  long long num = 0, den = -1;
  for (const char *p = line + 10; p < nl;) {
    while (p < nl && *p == ' ') p++;
    const char *q = p;
    while (q < nl && *q != ' ') q++;
    if (q == p) break;
    const std::string tag(p, q);
    const char *val = tag.c_str() + 1;
    switch (tag[0]) {
      case 'W': w = atoi(val); break;
      case 'H': h = atoi(val); break;
      case 'F': TM_CHECK(sscanf(val, "%lld:%lld", &num, &den) == 2, TM_E_INVAL, "%s: bad frame rate tag '%s'", name.c_str(), tag.c_str()); break;
      case 'I': TM_CHECK(!strcmp(val, "p") || !strcmp(val, "?"), TM_E_UNSUPPORTED, "%s: interlaced video (tag '%s') is not read", name.c_str(), tag.c_str()); break;
      case 'C':
        if (!strcmp(val, "444")) chroma = TM_CHROMA_444;
        else if (!strcmp(val, "422")) chroma = TM_CHROMA_422;
        else if (!strcmp(val, "420jpeg")) chroma = TM_CHROMA_420JPEG;
        else if (!strcmp(val, "420mpeg2")) chroma = TM_CHROMA_420MPEG2;
        else if (!strcmp(val, "mono")) chroma = TM_CHROMA_MONO;
        else { set_error("%s: pixel layout '%s' is not read (8-bit C444, C422, C420jpeg, C420mpeg2, Cmono only)", name.c_str(), tag.c_str()); return TM_E_UNSUPPORTED; }
        break;
      case 'X':
        if (tag == "XCOLORRANGE=FULL") full = 1;
        else if (tag == "XCOLORRANGE=LIMITED") full = 0;
        break;
      default: break;  // (A: the pixel aspect, and whatever else a writer adds)
    }
    p = q;
  }
  TM_CHECK(w > 0 && h > 0 && w <= 65536 && h <= 65536, TM_E_INVAL, "%s: bad size %dx%d", name.c_str(), w, h);
  TM_CHECK(den != -1, TM_E_INVAL, "%s: no frame rate tag", name.c_str());
  TM_CHECK(den > 0 && num > 0, TM_E_INVAL, "%s: frame rate %lld:%lld", name.c_str(), num, den);
  ChromaGeom g;
  TM_TRY(chroma_geom(chroma, w, h, &g));
  in->kind = TM_INPUT_Y4M;
  in->src_w = w; in->src_h = h; in->chroma = chroma; in->full_range = full;
  in->fps = (double)num / (double)den;
  in->frame_bytes = (int64_t)w * h + 2 * (int64_t)g.cw * g.ch;
  // the frames: 'FRAME' + parameters + '\n' + the planes; a last frame that is cut short does not count
  fseek(f, 0, SEEK_END);
  const int64_t fsize = ftell(f);
  int64_t pos = (nl - line) + 1;
  in->frame_off.clear();
  while (pos < fsize) {
    char fh[256];
    fseek(f, (long)pos, SEEK_SET);
    const size_t n = fread(fh, 1, sizeof(fh), f);
    if (n < 6) break;
    TM_CHECK(!memcmp(fh, "FRAME", 5), TM_E_INVAL, "%s: no FRAME header at offset %lld", name.c_str(), (long long)pos);
    const char *e = (const char *)memchr(fh, '\n', n);
    TM_CHECK(e || n < sizeof(fh), TM_E_INVAL, "%s: the FRAME header at offset %lld has no end", name.c_str(), (long long)pos);
    if (!e) break;
    const int64_t data = pos + (e - fh) + 1;
    if (data + in->frame_bytes > fsize) break;
    in->frame_off.push_back(data);
    pos = data + in->frame_bytes;
  }
  return TM_OK;
}

static bool has_gtm_magic(const std::string &name) {
  FILE *f = fopen(name.c_str(), "rb");
  if (!f) return false;
  uint8_t m[4] = {0, 0, 0, 0};
  const size_t n = fread(m, 1, 4, f);
  fclose(f);
  return n == 4 && gtm_has_magic(m, GTM_HEADER_MAGIC);
}

static bool starts_with_soi(const std::string &name) {
  FILE *f = fopen(name.c_str(), "rb");
  if (!f) return false;
  uint8_t m[2] = {0, 0};
  const size_t n = fread(m, 1, 2, f);
  fclose(f);
  return n == 2 && m[0] == 0xff && m[1] == 0xd8;
}
static bool starts_with_gif(const std::string &name) {
  FILE *f = fopen(name.c_str(), "rb");
  if (!f) return false;
  char m[6] = {0};
  const size_t n = fread(m, 1, 6, f);
  fclose(f);
  return n == 6 && (!memcmp(m, "GIF87a", 6) || !memcmp(m, "GIF89a", 6));
}
int read_whole(const std::string &name, std::vector<uint8_t> *out) {
  FILE *f = fopen(name.c_str(), "rb");
  TM_CHECK(f, TM_E_IO, "cannot open %s", name.c_str());
  struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize(n > 0 ? (size_t)n : 0);
  TM_CHECK(fread(out->data(), 1, out->size(), f) == out->size(), TM_E_IO, "cannot read %s", name.c_str());
  return TM_OK;
}

// what tm_open_input finds out, without a device: the kind of input, its sizes, rate, frame range
int probe_input(const std::string &name, int start_frame, int frame_count, double scaling, InputInfo *in) {
  *in = InputInfo();
  TM_CHECK(!name.empty(), TM_E_INVAL, "InputFileName is empty");
  TM_CHECK(start_frame >= 0, TM_E_INVAL, "StartFrame %d", start_frame);
  in->name = name;
  in->start = start_frame;
  if (file_exists(name) && has_gtm_magic(name)) {  // a .gtm stream: its frames are played into the clip (play_gtm, tm_input_clip.hip)
    TM_CHECK(scaling == 1.0, TM_E_UNSUPPORTED, "%s: Scaling %g with a .gtm input (the resampler takes YUV planes; only Scaling = 1 is read)", name.c_str(), scaling);
    int total = 0;
    TM_TRY(probe_gtm(name.c_str(), &in->src_w, &in->src_h, &in->fps, &total));
    in->kind = INPUT_GTM;
    in->chroma = TM_CHROMA_444;
    TM_TRY(frame_range(name, total, "frames", start_frame, frame_count, &in->frames));
    in->dst_w = in->src_w; in->dst_h = in->src_h;
    return TM_OK;
  }
  if (file_exists(name) && starts_with_gif(name)) {  // an animated GIF: its frames are decoded and composited into the clip (decode_gif, tm_input_files.hip)
    TM_CHECK(scaling == 1.0, TM_E_UNSUPPORTED, "%s: Scaling %g with a GIF input (only Scaling = 1 is read)", name.c_str(), scaling);
    std::vector<uint8_t> file;
    TM_TRY(read_whole(name, &file));
    gif::GifInfo info;
    TM_TRY(gif::parse_gif(file.data(), file.size(), name.c_str(), &info));
    in->kind = TM_INPUT_GIF;
    in->chroma = TM_CHROMA_444;
    in->src_w = in->dst_w = info.w; in->src_h = in->dst_h = info.h; in->fps = info.fps;
    return frame_range(name, (int64_t)info.images.size(), "frames", start_frame, frame_count, &in->frames);
  }
  if (file_exists(name)) {
    TM_TRY(parse_y4m(name, in));
    TM_TRY(frame_range(name, (int64_t)in->frame_off.size(), "whole frames", start_frame, frame_count, &in->frames));
    return scaled_size(in->src_w, in->src_h, scaling, &in->dst_w, &in->dst_h);
  }
  // a numbered PNG sequence (LoadInputVideo, 3340-3353): Format(name, [i + StartFrame])
  std::string path;
  TM_TRY(format_pattern(name, start_frame, &path));
  in->kind = TM_INPUT_PNGS;
  in->fps = 24.0;  // 1791
  in->chroma = TM_CHROMA_444;
  int cnt = frame_count;
  if (cnt <= 0) {  // count the files up to the first gap (1797-1806)
    cnt = 0;
    for (;; cnt++) {
      TM_TRY(format_pattern(name, (int64_t)start_frame + cnt, &path));
      if (!file_exists(path)) break;
    }
  }
  TM_TRY(format_pattern(name, start_frame, &path));
  TM_CHECK(cnt > 0 && file_exists(path), TM_E_IO, "input: %s does not exist", path.c_str());
  in->frames = cnt;
  if (starts_with_soi(path)) {  // a JPEG sequence: the size and the sampling are the first file's
    std::vector<uint8_t> file;
    TM_TRY(read_whole(path, &file));
    jpg::JpegInfo info;
    TM_TRY(jpg::parse_jpeg(file.data(), file.size(), path.c_str(), &info));
    in->kind = TM_INPUT_JPEGS;
    in->src_w = info.w; in->src_h = info.h; in->chroma = info.layout(); in->full_range = 1;  // (JFIF: full-range BT.601)
    in->jpeg_segments = (int)info.nsegs;
  } else
    TM_TRY(read_png(path.c_str(), nullptr, 0, &in->src_w, &in->src_h));  // the size comes from the first file (1813-1814)
  in->dst_w = in->src_w; in->dst_h = in->src_h;                         // Scaling plays no part on this path (3347-3348)
  // manual key frames (FindKeyFrames(AManualMode), 3380-3384): frame i where Format(ChangeFileExt(name, '.kf'), [i + StartFrame]) exists
  const std::string kf = change_ext(name, ".kf");
  in->manual_kf.clear();
  for (int i = 0; i < cnt; i++) {
    TM_TRY(format_pattern(kf, (int64_t)start_frame + i, &path));
    if (i == 0 || file_exists(path)) in->manual_kf.push_back(i);
  }
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" int tm_probe_input_host(const char *name, int start_frame, int frame_count, double scaling, int *kind, int *width, int *height, int *dst_width, int *dst_height,
                        double *fps, int *frames, int *chroma) {
  TM_CHECK(name, TM_E_INVAL, "null argument");
  InputInfo in;
  TM_TRY(probe_input(name, start_frame, frame_count, scaling, &in));
  if (kind) *kind = in.kind;
  if (width) *width = in.src_w;
  if (height) *height = in.src_h;
  if (dst_width) *dst_width = in.dst_w;
  if (dst_height) *dst_height = in.dst_h;
  if (fps) *fps = in.fps;
  if (frames) *frames = in.frames;
  if (chroma) *chroma = in.chroma == CHROMA_422_CENTRED ? (int)TM_CHROMA_422 : in.chroma;
  return TM_OK;
}
