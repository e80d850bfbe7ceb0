// tm_input.hip -- Load's input: the probe half of Load (tilingencoder.pas:1764-1820) for Y4M files and numbered PNG sequences, YUV clips lent
// in memory (tm_set_frames_yuv), and the kernel that turns planes of Y, U, V into the RGB32 frames Load reads (its Lanczos-3 tables: tm_resample.hip).
//
// The reference opens "any file" through FFmpeg and scales with libswscale's Lanczos (extern.pas:780-781, 837-840).  Neither exists here
// (DESIGN.md sections 9 and 17): Y4M is the uncompressed container every FFmpeg build writes, and the resampler is a stated integer rule of
// this build -- separable, horizontal pass first, coefficients in 1/16384 from tables made on the host in double:
//   r = n / m;  f = max(1, r / s);  u_j = ((j + 0.5) r - 0.5 - o) / s;  taps ceil(u_j - 3f) .. floor(u_j + 3f) inside the plane
//   c_k = RoundHalfEven(16384 w_k / sum w), the remainder to the tap of largest w;  h = (sum c p + 64) >> 7;  v = clamp((sum c h + 2^20) >> 21)
// for a plane whose samples sit at luma positions s k + o (s = 2 for subsampled chroma, o = 0.5 where it is centred).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <thread>

#include "tm_encoder.h"

namespace tmx {

// where a layout's chroma samples sit: step and offset (in halves of a luma sample) per axis, plane size
struct ChromaGeom { int sx, sy, ox, oy, cw, ch; };
static int chroma_geom(int chroma, int w, int h, ChromaGeom *g) {
  switch (chroma) {
    case TM_CHROMA_444: *g = {1, 1, 0, 0, w, h}; break;
    case TM_CHROMA_422: *g = {2, 1, 0, 0, (w + 1) / 2, h}; break;
    case TM_CHROMA_420JPEG: *g = {2, 2, 1, 1, (w + 1) / 2, (h + 1) / 2}; break;
    case TM_CHROMA_420MPEG2: *g = {2, 2, 0, 1, (w + 1) / 2, (h + 1) / 2}; break;
    case TM_CHROMA_MONO: *g = {1, 1, 0, 0, 0, 0}; break;
    default: set_error("bad chroma layout %d", chroma); return TM_E_INVAL;
  }
  return TM_OK;
}

// ---- the kernel ------------------------------------------------------------------------------------------------
// A workgroup owns IN_TW x th output pixels of one frame.  Per plane: the horizontal pass of the source rows its vertical taps reach goes
// into LDS as int32 (the rule keeps 7 extra bits between the passes), then every lane runs the vertical pass for four neighbouring pixels of
// one row out of LDS; the three results stay in registers for the colour conversion and leave as one 16-byte store.  No plane goes to HBM
// between the passes.  The host picks th so that the rows a tile reaches fit IN_HROWS (in_tile_rows).
//
// The samples are read in one place, the horizontal pass, and how is a compile-time property of the kernel: BYTES per sample (1, or 2 for
// little-endian words) and CSTEP, the distance in samples between a chroma plane's neighbours (2 where U and V alternate in one plane: NV12,
// P010; V's plane then starts one sample behind U's).  Words become bytes right there (DeepRule), so everything behind the fetch is the 8-bit rule.
constexpr int IN_TW = 64, IN_HROWS = 96;
static_assert(RESAMPLE_TH_MAX * 16 == 256, "a workgroup's 256 lanes: 16 per output row of the tile");
struct PlaneSrc { const uint8_t *p; int64_t row, frame; };  // strides in bytes
struct DeepRule { int rshift, mask, half, nshift; };  // p_d = (word >> rshift) & mask;  p = min(255, (p_d + half) >> nshift), half = 2^(nshift - 1)

template <int BYTES>
__device__ __forceinline__ int fetch_sample(const uint8_t *at, const DeepRule &d) {
  if constexpr (BYTES == 1) return (int)*at;
  else {
    const int pd = ((int)*reinterpret_cast<const uint16_t *>(at) >> d.rshift) & d.mask;
    return min(255, (pd + d.half) >> d.nshift);
  }
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__device__ __forceinline__ uint32_t yuv_to_rgb32(int Y, int U, int V, int mode) {
  const int D = U - 128, E = V - 128;
  int R, G, B;
  if (mode == TM_YUV_BT601_FULL) {  // libjpeg's constants, 16 fractional bits
    R = (65536 * Y + 91881 * E + 32768) >> 16;
    G = (65536 * Y - 22554 * D - 46802 * E + 32768) >> 16;
    B = (65536 * Y + 116130 * D + 32768) >> 16;
  } else if (mode == TM_YUV_BT709_FULL) {  // round(k 2^16) of the matrix of Kr = 0.2126, Kb = 0.0722
    R = (65536 * Y + 103206 * E + 32768) >> 16;
    G = (65536 * Y - 12276 * D - 30679 * E + 32768) >> 16;
    B = (65536 * Y + 121609 * D + 32768) >> 16;
  } else if (mode == TM_YUV_BT709_LIMITED) {  // the same matrix, luma scaled by 255/219 and chroma by 255/224, 8 fractional bits
    const int C = Y - 16;
    R = (298 * C + 459 * E + 128) >> 8;
    G = (298 * C - 55 * D - 136 * E + 128) >> 8;
    B = (298 * C + 541 * D + 128) >> 8;
  } else if (mode == TM_YUV_TILER) {  // YUVToRGB, utils.pas:492-509: Single operands, every right-hand side in double, narrowed once
    const double y = (double)(float)Y, u = (double)(float)D, v = (double)(float)E;
    const float r = __double2float_rn(__dadd_rn(y, __dmul_rn(v, 1.13983)));
    const float g = __double2float_rn(__dsub_rn(__dsub_rn(y, __dmul_rn(u, 0.39465)), __dmul_rn(v, 0.58060)));
    const float b = __double2float_rn(__dadd_rn(y, __dmul_rn(u, 2.03211)));
    R = __float2int_rn(r); G = __float2int_rn(g); B = __float2int_rn(b);  // Round: half to even
  } else {  // BT.601, limited range
    const int C = Y - 16;
    R = (298 * C + 409 * E + 128) >> 8;
    G = (298 * C - 100 * D - 208 * E + 128) >> 8;
    B = (298 * C + 516 * D + 128) >> 8;
  }
  return (uint32_t)clamp255(R) << 16 | (uint32_t)clamp255(G) << 8 | (uint32_t)clamp255(B);
}

template <int BYTES, int CSTEP>
__global__ __launch_bounds__(256) void k_yuv_to_rgb32(PlaneSrc sy, PlaneSrc su, PlaneSrc sv, DeepRule deep, AxisTaps lh, AxisTaps lv, AxisTaps ch, AxisTaps cv, int dst_w,
                                                      int dst_h, int th, int mode, int vec_ok, uint32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) int32_t hbuf[IN_HROWS * IN_TW];
  const int x0 = blockIdx.x * IN_TW, y0 = blockIdx.y * th, frame = blockIdx.z;
  const int y_last = min(y0 + th, dst_h) - 1;
  const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
  const int hx = threadIdx.x & (IN_TW - 1), hr0 = threadIdx.x / IN_TW;  // the horizontal pass: one column, rows hr0, hr0 + 4, ...
  const bool mine = ty < th && y0 + ty <= y_last;
  // every table entry the three planes will need, asked for at once: the passes below then wait for one load, not for a chain of them
  const int oxc = min(x0 + hx, dst_w - 1), oyc = min(y0 + ty, dst_h - 1);
  const int hfirst[2] = {lh.first[oxc], ch.first[oxc]}, hcount[2] = {lh.count[oxc], ch.count[oxc]};
  const int vfirst[2] = {lv.first[oyc], cv.first[oyc]}, vcount[2] = {lv.count[oyc], cv.count[oyc]};
  const int2 span[2] = {lv.span[blockIdx.y], cv.span[blockIdx.y]};  // the source rows the tile's samples reach: first row, number of rows
  int val[3][4];
#pragma unroll
  for (int p = 0; p < 3; p++) {
    const PlaneSrc src = p == 0 ? sy : p == 1 ? su : sv;
    if (src.p == nullptr) {  // Cmono: U = V = 128
#pragma unroll
      for (int j = 0; j < 4; j++) val[p][j] = 128;
      continue;
    }
    const AxisTaps ah = p == 0 ? lh : ch, av = p == 0 ? lv : cv;
    const int c01 = p == 0 ? 0 : 1, r0 = span[c01].x, rows = span[c01].y;
    const int eb = (p == 0 ? 1 : CSTEP) * BYTES;  // bytes from one of the plane's samples to the next (the loop over p is unrolled: a constant)
    __syncthreads();  // the plane before has been read
    if (x0 + hx < dst_w) {
      const int ox = x0 + hx, k0 = hfirst[c01], cnt = hcount[c01];
      const uint8_t *col = src.p + (int64_t)frame * src.frame + (int64_t)k0 * eb;
      // four rows at a time, so that a coefficient is loaded once for four products
      constexpr int RS = 256 / IN_TW;
      for (int rb = hr0; rb < rows; rb += 4 * RS) {
        const uint8_t *row = col + (int64_t)(r0 + rb) * src.row;
        int acc[4] = {0, 0, 0, 0};
        for (int k = 0; k < cnt; k++) {
          const int c = ah.coef[(int64_t)k * dst_w + ox];
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (rb + i * RS < rows) acc[i] += c * fetch_sample<BYTES>(row + (int64_t)i * RS * src.row + k * eb, deep);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (rb + i * RS < rows) hbuf[(rb + i * RS) * IN_TW + hx] = (acc[i] + 64) >> 7;  // (arithmetic shift, no clamp)
      }
    }
    __syncthreads();
    if (mine) {
      const int oy = y0 + ty, k0 = vfirst[c01] - r0, cnt = vcount[c01];
      int acc[4] = {0, 0, 0, 0};
      for (int k = 0; k < cnt; k++) {
        const int c = av.coef[(int64_t)k * dst_h + oy];
        const int4 h = *reinterpret_cast<const int4 *>(&hbuf[(k0 + k) * IN_TW + tx]);
        acc[0] += c * h.x; acc[1] += c * h.y; acc[2] += c * h.z; acc[3] += c * h.w;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) val[p][j] = clamp255((acc[j] + (1 << 20)) >> 21);
    }
  }
  if (!mine || x0 + tx >= dst_w) return;
  uint32_t px[4];
#pragma unroll
  for (int j = 0; j < 4; j++) px[j] = yuv_to_rgb32(val[0][j], val[1][j], val[2][j], mode);
  uint32_t *o = out + ((int64_t)frame * dst_h + (y0 + ty)) * dst_w + x0 + tx;
  if (vec_ok && x0 + tx + 3 < dst_w) *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);
  else
    for (int j = 0; j < 4 && x0 + tx + j < dst_w; j++) o[j] = px[j];
}

// ---- the tables of one conversion (InputTables, tm_internal.h), made once per (source size, layout, output size) and kept on the device.
// The rule's tables, their trimming, the tile spans and the device layout are tm_resample.hip's; here: which axes a layout has.
static int build_input_tables(int src_w, int src_h, int chroma, int dst_w, int dst_h, InputTables *t, hipStream_t stream) {
  if (t->dev.p && t->src_w == src_w && t->src_h == src_h && t->chroma == chroma && t->dst_w == dst_w && t->dst_h == dst_h) return TM_OK;
  ChromaGeom g;
  TM_TRY(chroma_geom(chroma, src_w, src_h, &g));
  const bool has_c = chroma != TM_CHROMA_MONO;
  const int na = has_c ? 4 : 2;
  // axis tables: 0 luma horizontal, 1 luma vertical, 2 chroma horizontal, 3 chroma vertical
  AxisTable ax[4];
  for (int a = 0; a < na; a++) {
    const bool horiz = (a & 1) == 0, c = a >= 2;
    TM_TRY(ax[a].make(horiz ? src_w : src_h, horiz ? dst_w : dst_h, c ? (horiz ? g.cw : g.ch) : (horiz ? src_w : src_h), c ? (horiz ? g.sx : g.sy) : 1,
                      c ? (horiz ? g.ox : g.oy) : 0));
  }
  for (int a = 0; a < na; a += 2) TM_TRY(check_resample_sums(ax[a], ax[a + 1], src_w, src_h, dst_w, dst_h));
  for (int a = 0; a < na; a++) ax[a].trim();
  const AxisTable *const vert[2] = {&ax[1], &ax[3]};
  const int th = resample_tile_rows(vert, has_c ? 2 : 1, IN_HROWS);
  TM_CHECK(th > 0, TM_E_UNSUPPORTED, "resample: %d -> %d rows reach too many source rows per tile", src_h, dst_h);
  const AxisTable *const all[4] = {&ax[0], &ax[1], &ax[2], &ax[3]};
  AxisTaps dev[4];
  TM_TRY(upload_axis_tables(all, na, th, IN_HROWS, &t->dev, dev, stream));
  t->lh = dev[0]; t->lv = dev[1];
  t->ch = dev[has_c ? 2 : 0]; t->cv = dev[has_c ? 3 : 1];  // Cmono: the chroma tables are never read
  t->src_w = src_w; t->src_h = src_h; t->chroma = chroma; t->dst_w = dst_w; t->dst_h = dst_h; t->th = th;
  return TM_OK;
}

// how the samples of a clip's planes are stored (tm_yuv_clip): TM_SAMPLES_*, the depth, and whether U and V alternate in the plane `u`
struct SampleFmt {
  int samples = TM_SAMPLES_U8, depth = 8;
  bool pairs = false;
  int bytes() const { return samples == TM_SAMPLES_U8 ? 1 : 2; }
};

static int launch_yuv_to_rgb32(const InputTables &t, const void *y, const void *u, const void *v, const int64_t strides[6], const SampleFmt &fmt, int nframes,
                               int yuv_mode, void *out, hipStream_t stream) {
  if (nframes == 0) return TM_OK;
  const bool has_c = t.chroma != TM_CHROMA_MONO, pairs = has_c && fmt.pairs;
  const PlaneSrc sy{(const uint8_t *)y, strides[0], strides[1]}, su{has_c ? (const uint8_t *)u : nullptr, strides[2], strides[3]},
      sv{has_c ? (pairs ? (const uint8_t *)u + fmt.bytes() : (const uint8_t *)v) : nullptr, strides[pairs ? 2 : 4], strides[pairs ? 3 : 5]};
  DeepRule deep{0, 0xff, 0, 0};
  if (fmt.bytes() == 2) {
    const int d = fmt.depth;
    deep = fmt.samples == TM_SAMPLES_U16_HIGH ? DeepRule{16 - d, 0xffff, 1 << (d - 9), d - 8} : DeepRule{0, (1 << d) - 1, 1 << (d - 9), d - 8};
  }
  const int vec_ok = (t.dst_w % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((t.dst_w + IN_TW - 1) / IN_TW), (unsigned)((t.dst_h + t.th - 1) / t.th), (unsigned)nframes);
  TM_CHECK(grid.y <= 65535 && grid.z <= 65535, TM_E_UNSUPPORTED, "yuv_to_rgb32: %d rows x %d frames in one launch", t.dst_h, nframes);
  auto kernel = fmt.bytes() == 1 ? (pairs ? k_yuv_to_rgb32<1, 2> : k_yuv_to_rgb32<1, 1>) : (pairs ? k_yuv_to_rgb32<2, 2> : k_yuv_to_rgb32<2, 1>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, sy, su, sv, deep, t.lh, t.lv, t.ch, t.cv, t.dst_w, t.dst_h, t.th, yuv_mode, vec_ok, (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- probing (host) --------------------------------------------------------------------------------------------
static bool file_exists(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

static int pas_round_dim(double v) {  // Round(W * Scaling), at least 1 (extern.pas:780-781)
  return (int)std::max<long long>(1, llrint(v));
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
  char m[4] = {0, 0, 0, 0};
  const size_t n = fread(m, 1, 4, f);
  fclose(f);
  return n == 4 && memcmp(m, "GTMv", 4) == 0;
}

// what tm_open_input finds out, without a device: the kind of input, its sizes, rate, frame range
int probe_input(const std::string &name, int start_frame, int frame_count, double scaling, InputInfo *in) {
  *in = InputInfo();
  TM_CHECK(!name.empty(), TM_E_INVAL, "InputFileName is empty");
  TM_CHECK(start_frame >= 0, TM_E_INVAL, "StartFrame %d", start_frame);
  in->name = name;
  in->start = start_frame;
  if (file_exists(name) && has_gtm_magic(name)) {  // a .gtm stream: its frames are played into the clip (tm_player.hip)
    TM_CHECK(scaling == 1.0, TM_E_UNSUPPORTED, "%s: Scaling %g with a .gtm input (the resampler takes YUV planes; only Scaling = 1 is read)", name.c_str(), scaling);
    int total = 0;
    TM_TRY(probe_gtm(name.c_str(), &in->src_w, &in->src_h, &in->fps, &total));
    in->kind = INPUT_GTM;
    in->chroma = TM_CHROMA_444;
    const int64_t cnt = frame_count > 0 ? frame_count : (int64_t)total - start_frame;  // 1778-1782
    TM_CHECK(cnt > 0 && start_frame + cnt <= total, TM_E_INVAL, "%s holds %d frames: frames [%d,+%lld) are not all there", name.c_str(), total, start_frame, (long long)cnt);
    in->frames = (int)cnt;
    in->dst_w = in->src_w; in->dst_h = in->src_h;
    return TM_OK;
  }
  if (file_exists(name)) {
    TM_TRY(parse_y4m(name, in));
    const int64_t total = (int64_t)in->frame_off.size();
    const int64_t cnt = frame_count > 0 ? frame_count : total - start_frame;  // 1778-1782
    TM_CHECK(cnt > 0 && start_frame + cnt <= total, TM_E_INVAL, "%s holds %lld whole frames: frames [%d,+%lld) are not all there", name.c_str(), (long long)total,
             start_frame, (long long)cnt);
    in->frames = (int)cnt;
    in->dst_w = pas_round_dim(in->src_w * scaling);
    in->dst_h = pas_round_dim(in->src_h * scaling);
    TM_CHECK((double)in->src_w / in->dst_w <= 8.0 && (double)in->src_h / in->dst_h <= 8.0, TM_E_UNSUPPORTED,
             "Scaling %g shrinks %dx%d by more than 8 (more than %d taps)", scaling, in->src_w, in->src_h, TM_RESAMPLE_MAX_TAPS);
    return TM_OK;
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

// ---- Load from the file ------------------------------------------------------------------------------------------
namespace {
struct Events {
  std::vector<hipEvent_t> ev;
  ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  int make(int n) {
    for (int i = 0; i < n; i++) { hipEvent_t e; TM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ev.push_back(e); }
    return TM_OK;
  }
};
}  // namespace

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

static int resolve_yuv_mode(int mode, int full_range) { return mode == TM_YUV_AUTO ? (full_range ? TM_YUV_BT601_FULL : TM_YUV_BT601_LIMITED) : mode; }

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
  Events up, done;
  TM_TRY(up.make(2)); TM_TRY(done.make(2));
  for (int i = 0; i < 2; i++) {
    if (src.fill_host) TM_TRY(host[i].alloc(fb * chunk));
    TM_TRY(dev[i].alloc(fb * chunk));
  }
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  int c = 0;
  for (int f0 = a; f0 < b; f0 += chunk, c++) {
    const int nf = std::min(chunk, b - f0), s = c & 1;
    if (src.fill_host) {
      if (c >= 2) TM_HIP(hipEventSynchronize(up.ev[s]));  // the upload that last read this host buffer
      TM_TRY(src.fill_host(f0, nf, (uint8_t *)host[s].p));
    }
    if (c >= 2) TM_HIP(hipStreamWaitEvent(e->copy_stream, done.ev[s], 0));  // the conversion that last read this device buffer
    if (src.fill_host) TM_HIP(hipMemcpyAsync(dev[s].p, host[s].p, fb * nf, hipMemcpyHostToDevice, e->copy_stream));
    else TM_TRY(src.copy_in(f0, nf, dev[s].as<uint8_t>(), e->copy_stream));
    TM_HIP(hipEventRecord(up.ev[s], e->copy_stream));
    TM_HIP(hipStreamWaitEvent(e->stream, up.ev[s], 0));
    TM_TRY(src.convert(dev[s].as<uint8_t>(), f0, nf));
    TM_HIP(hipEventRecord(done.ev[s], e->stream));
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
  struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
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
      uint8_t *dst = host + fb * i;
      const int64_t at = in.frame_off[(size_t)(in.start + f0 + i)];
      for (size_t got = 0; got < fb;) {
        const ssize_t n = pread(fd, dst + got, fb - got, (off_t)(at + (int64_t)got));
        TM_CHECK(n > 0, TM_E_IO, "%s: cannot read frame %d", in.name.c_str(), in.start + f0 + i);
        got += (size_t)n;
      }
      return (int)TM_OK;
    });
  };
  src.convert = [&](const uint8_t *base, int f0, int nf) -> int {
    return launch_yuv_to_rgb32(tables, base, base + y_plane, base + y_plane + c_plane, strides, SampleFmt(), nf, mode, e->frames_owned.as<uint8_t>() + out_fb * f0, e->stream);
  };
  return convert_staged(e, a, b, src);
}

// ---- a YUV clip lent in memory (tm_set_frames_yuv) ---------------------------------------------------------------------------------------
// the checks of tm_set_frames_yuv and of the stage seam, with no device call; what they find out about the planes
struct ClipPlanes {
  SampleFmt fmt;
  ChromaGeom g{};
  int nplanes = 1;                      // 1 mono, 2 Y + pairs, 3 planar
  int64_t row_bytes[3] = {0, 0, 0};     // of Y, U (or the pairs), V
  int rows[3] = {0, 0, 0};
};
static int check_yuv_clip(const tm_yuv_clip *c, ClipPlanes *out) {
  TM_CHECK(c, TM_E_INVAL, "yuv clip: null descriptor");
  TM_CHECK(c->chroma >= TM_CHROMA_444 && c->chroma <= TM_CHROMA_MONO, TM_E_INVAL, "yuv clip: unknown chroma layout %d", c->chroma);
  TM_CHECK(c->samples >= TM_SAMPLES_U8 && c->samples <= TM_SAMPLES_U16_HIGH, TM_E_INVAL, "yuv clip: unknown sample format %d", c->samples);
  TM_CHECK(c->memory == TM_MEM_HOST || c->memory == TM_MEM_DEVICE, TM_E_INVAL, "yuv clip: unknown memory kind %d", c->memory);
  TM_CHECK(c->y, TM_E_INVAL, "yuv clip: null y plane");
  const bool has_c = c->chroma != TM_CHROMA_MONO;
  TM_CHECK(!(c->v && !c->u), TM_E_INVAL, "yuv clip: a v plane without a u plane");
  TM_CHECK(!has_c || c->u, TM_E_INVAL, "yuv clip: layout %d has chroma, but u is null", c->chroma);
  TM_CHECK(c->width >= 1 && c->width <= 65536 && c->height >= 1 && c->height <= 65536, TM_E_INVAL, "yuv clip: bad size %dx%d", c->width, c->height);
  TM_CHECK(c->frames >= 1, TM_E_INVAL, "yuv clip: %d frames", c->frames);
  TM_CHECK(c->fps > 0, TM_E_INVAL, "yuv clip: frame rate %g", c->fps);
  if (c->samples == TM_SAMPLES_U8) TM_CHECK(c->depth == 8, TM_E_INVAL, "yuv clip: depth %d with 8-bit samples", c->depth);
  else TM_CHECK(c->depth >= 9 && c->depth <= 16, TM_E_INVAL, "yuv clip: depth %d with 16-bit samples (9 .. 16)", c->depth);
  ClipPlanes p;
  p.fmt.samples = c->samples; p.fmt.depth = c->depth; p.fmt.pairs = has_c && !c->v;
  TM_TRY(chroma_geom(c->chroma, c->width, c->height, &p.g));
  const int B = p.fmt.bytes();
  p.nplanes = !has_c ? 1 : p.fmt.pairs ? 2 : 3;
  p.row_bytes[0] = (int64_t)c->width * B; p.rows[0] = c->height;
  p.row_bytes[1] = (int64_t)p.g.cw * B * (p.fmt.pairs ? 2 : 1); p.rows[1] = p.g.ch;
  p.row_bytes[2] = (int64_t)p.g.cw * B; p.rows[2] = p.g.ch;
  const void *ptr[3] = {c->y, c->u, c->v};
  const int64_t row[3] = {c->y_row, c->u_row, c->v_row}, frame[3] = {c->y_frame, c->u_frame, c->v_frame};
  static const char *const names[3] = {"y", "u", "v"};
  for (int i = 0; i < p.nplanes; i++) {
    TM_CHECK(row[i] >= p.row_bytes[i], TM_E_INVAL, "yuv clip: the %s row stride %lld is shorter than a row of %lld bytes", names[i], (long long)row[i], (long long)p.row_bytes[i]);
    TM_CHECK(frame[i] >= 0, TM_E_INVAL, "yuv clip: negative %s frame stride %lld", names[i], (long long)frame[i]);
    TM_CHECK(B == 1 || (((uintptr_t)ptr[i] | (uint64_t)row[i] | (uint64_t)frame[i]) & 1) == 0, TM_E_INVAL, "yuv clip: an odd %s pointer or stride with 16-bit samples", names[i]);
  }
  if (out) *out = p;
  return TM_OK;
}
static int yuv_clip_dst(const tm_yuv_clip *c, double scaling, int *dw, int *dh) {  // as probe_input describes a file
  *dw = pas_round_dim(c->width * scaling);
  *dh = pas_round_dim(c->height * scaling);
  TM_CHECK((double)c->width / *dw <= 8.0 && (double)c->height / *dh <= 8.0, TM_E_UNSUPPORTED, "Scaling %g shrinks %dx%d by more than 8 (more than %d taps)", scaling,
           c->width, c->height, TM_RESAMPLE_MAX_TAPS);
  return TM_OK;
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

// the PNG sequence, decoded on the host into a clip the encoder keeps until Load's chunked host-clip upload has taken it
static int decode_pngs(tm_encoder *e) {
  InputInfo &in = e->input;
  const size_t px = (size_t)e->width * e->height;
  e->input_clip.resize(px * e->nframes);
  return parallel_for(e->nframes, [&](int i) -> int {  // (frames are files of their own: inflate is the time, and it is one core's per file)
    std::string path;
    TM_TRY(format_pattern(in.name, (int64_t)in.start + i, &path));
    int w = 0, h = 0;
    TM_TRY(read_png(path.c_str(), nullptr, 0, &w, &h));
    TM_CHECK(w == e->width && h == e->height, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", path.c_str(), w, h, e->width, e->height);
    return read_png(path.c_str(), e->input_clip.data() + px * i, (int64_t)px, &w, &h);
  });
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
  if (in.kind == TM_INPUT_PNGS) {
    if (in.decoded && e->frames != nullptr) return TM_OK;  // a second Run(esLoad): the device copy of the last one
    TM_TRY(decode_pngs(e));
    e->frames = nullptr;
    e->frames_host = e->input_clip.data();
    e->hclip_cur = -1;
    in.decoded = true;
    return TM_OK;
  }
  int64_t a = 0, b = e->nframes;
  if (e->dist() && e->s.MotionPredictRadius <= 0) {  // a shard decodes what its Load reads: its frames and the one before them
    share_of(e->nframes, e->co.rank, e->co.world, &a, &b);
    a = std::max<int64_t>(a - 1, 0);
  }
  const int mode = resolve_yuv_mode(e->input_yuv, in.full_range);
  if (in.decoded && e->frames == e->frames_owned.p && e->frames_owned.p && in.dec_first <= a && b <= in.dec_first + in.dec_count && in.dec_mode == mode) return TM_OK;
  const bool lent_clip = in.kind == INPUT_YUV_CLIP;
  TM_CHECK(!lent_clip || in.lent, TM_E_INVAL,
           "the YUV planes were given back when the last Load returned: lend the clip again (tm_set_frames_yuv) to convert it with another InputYUV or for more frames");
  TM_HIP(hipStreamSynchronize(e->stream));  // the destination may have been handed out by the pool a moment ago
  TM_TRY(e->frames_owned.alloc((size_t)e->width * e->height * 4 * e->nframes));
  e->frames = e->frames_owned.p;
  e->frames_host = nullptr;
  e->hclip_cur = -1;
  in.decoded = false;
  if (b > a) TM_TRY(lent_clip ? convert_yuv_clip(e, (int)a, (int)b) : in.kind == INPUT_GTM ? play_gtm(e, (int)a, (int)b) : decode_y4m(e, (int)a, (int)b));
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
  TM_TRY(yuv_clip_dst(clip, e->s.Scaling, &dw, &dh));
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

int tm_probe_yuv_clip_host(const tm_yuv_clip *clip, double scaling, int *dst_width, int *dst_height) {
  TM_TRY(check_yuv_clip(clip, nullptr));
  int dw = 0, dh = 0;
  TM_TRY(yuv_clip_dst(clip, scaling, &dw, &dh));
  if (dst_width) *dst_width = dw;
  if (dst_height) *dst_height = dh;
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

int tm_probe_input_host(const char *name, int start_frame, int frame_count, double scaling, int *kind, int *width, int *height, int *dst_width, int *dst_height,
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
  if (chroma) *chroma = in.chroma;
  return TM_OK;
}

int tm_resample_taps_host(int n, int m, int np, int s, int o_halves, int32_t *first, int32_t *count, int32_t *coef) {
  TM_CHECK(first && count && coef, TM_E_INVAL, "null argument");
  return resample_taps(n, m, np, s, o_halves, first, count, coef, nullptr);
}

int tm_stage_yuv_to_rgb32(const void *y, const void *u, const void *v, const int64_t strides[6], int nframes, int src_w, int src_h, int chroma, int dst_w, int dst_h,
                          int yuv_mode, void *out_rgb32, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  ChromaGeom g;
  TM_TRY(chroma_geom(chroma, src_w, src_h, &g));
  const bool has_c = chroma != TM_CHROMA_MONO;
  TM_CHECK(y && out_rgb32 && strides && (!has_c || (u && v)) && nframes >= 0 && src_w > 0 && src_h > 0 && dst_w > 0 && dst_h > 0, TM_E_INVAL, "yuv_to_rgb32: bad arguments");
  TM_CHECK(yuv_mode >= TM_YUV_AUTO && yuv_mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "bad YUV mode %d", yuv_mode);
  TM_CHECK(strides[0] >= src_w && strides[1] >= 0 && (!has_c || (strides[2] >= g.cw && strides[4] >= g.cw && strides[3] >= 0 && strides[5] >= 0)), TM_E_INVAL,
           "yuv_to_rgb32: a row stride is shorter than its plane's rows");
  InputTables tables;
  TM_TRY(build_input_tables(src_w, src_h, chroma, dst_w, dst_h, &tables, (hipStream_t)stream));
  // (without a header to say otherwise a clip is limited range, as FFmpeg assumes)
  TM_TRY(launch_yuv_to_rgb32(tables, y, u, v, strides, SampleFmt(), nframes, resolve_yuv_mode(yuv_mode, 0), out_rgb32, (hipStream_t)stream));
  TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the tables are freed on return
  return TM_OK;
}

int tm_stage_yuv_to_rgb32_fmt(const void *y, const void *u, const void *v, const int64_t strides[6], int nframes, int src_w, int src_h, int chroma, int samples, int depth,
                              int dst_w, int dst_h, int yuv_mode, void *out_rgb32, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(out_rgb32 && strides && nframes >= 0 && dst_w > 0 && dst_h > 0, TM_E_INVAL, "yuv_to_rgb32: bad arguments");
  TM_CHECK(yuv_mode >= TM_YUV_AUTO && yuv_mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "bad YUV mode %d", yuv_mode);
  tm_yuv_clip c{};  // the planes as a clip: the checks are tm_set_frames_yuv's
  c.y = y; c.u = u; c.v = v;
  c.y_row = strides[0]; c.y_frame = strides[1]; c.u_row = strides[2]; c.u_frame = strides[3]; c.v_row = strides[4]; c.v_frame = strides[5];
  c.width = src_w; c.height = src_h; c.frames = std::max(nframes, 1); c.fps = 1.0;
  c.chroma = chroma; c.samples = samples; c.depth = depth; c.memory = TM_MEM_DEVICE;
  ClipPlanes pl;
  TM_TRY(check_yuv_clip(&c, &pl));
  InputTables tables;
  TM_TRY(build_input_tables(src_w, src_h, chroma, dst_w, dst_h, &tables, (hipStream_t)stream));
  TM_TRY(launch_yuv_to_rgb32(tables, y, u, v, strides, pl.fmt, nframes, resolve_yuv_mode(yuv_mode, 0), out_rgb32, (hipStream_t)stream));
  TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the tables are freed on return
  return TM_OK;
}

}  // extern "C"
