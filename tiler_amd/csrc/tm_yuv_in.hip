// tm_yuv_in.hip -- planes of Y, U, V into the RGB32 frames Load reads, scaled on the way (the mirror image of
// tm_yuv_out.hip): the checks of a lent clip (tm_yuv_clip), the tables of one conversion, k_yuv_to_rgb32 and its stage seams.
//
// The reference opens "any file" through FFmpeg and scales with libswscale's Lanczos (extern.pas:780-781, 837-840).  Neither exists here
// (DESIGN.md sections 9 and 17): the resampler is a stated integer rule of this build -- separable, horizontal pass first, coefficients in
// 1/16384 from tables made on the host in double (tm_resample.hip, where the rule is written out).
#include "tm_input.h"

namespace tmx {

int chroma_geom(int chroma, int w, int h, ChromaGeom *g) {
  switch (chroma) {
    case TM_CHROMA_444: *g = {1, 1, 0, 0, w, h}; break;
    case TM_CHROMA_422: *g = {2, 1, 0, 0, (w + 1) / 2, h}; break;
    case TM_CHROMA_420JPEG: *g = {2, 2, 1, 1, (w + 1) / 2, (h + 1) / 2}; break;
    case TM_CHROMA_420MPEG2: *g = {2, 2, 0, 1, (w + 1) / 2, (h + 1) / 2}; break;
    case TM_CHROMA_MONO: *g = {1, 1, 0, 0, 0, 0}; break;
    case CHROMA_422_CENTRED: *g = {2, 1, 1, 0, (w + 1) / 2, h}; break;
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

template <int BYTES>
__device__ __forceinline__ int fetch_sample(const uint8_t *at, const DeepRule &d) {
  if constexpr (BYTES == 1) return (int)*at;
  else return narrow_word((int)*reinterpret_cast<const uint16_t *>(at), d);
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

// ---- the tables of one conversion (InputTables, tm_input.h), made once per (source size, layout, output size) and kept on the device.
// The rule's tables, their trimming, the tile spans and the device layout are tm_resample.hip's; here: which axes a layout has.
int build_input_tables(int src_w, int src_h, int chroma, int dst_w, int dst_h, InputTables *t, hipStream_t stream) {
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

int launch_yuv_to_rgb32(const InputTables &t, const void *y, const void *u, const void *v, const int64_t strides[6], const SampleFmt &fmt, int nframes, int yuv_mode,
                        void *out, hipStream_t stream) {
  if (nframes == 0) return TM_OK;
  const bool has_c = t.chroma != TM_CHROMA_MONO, pairs = has_c && fmt.pairs;
  const PlaneSrc sy{(const uint8_t *)y, strides[0], strides[1]}, su{has_c ? (const uint8_t *)u : nullptr, strides[2], strides[3]},
      sv{has_c ? (pairs ? (const uint8_t *)u + fmt.bytes() : (const uint8_t *)v) : nullptr, strides[pairs ? 2 : 4], strides[pairs ? 3 : 5]};
  const DeepRule deep = deep_rule_of(fmt);
  const int vec_ok = (t.dst_w % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)((t.dst_w + IN_TW - 1) / IN_TW), (unsigned)((t.dst_h + t.th - 1) / t.th), (unsigned)nframes);
  TM_CHECK(grid.y <= 65535 && grid.z <= 65535, TM_E_UNSUPPORTED, "yuv_to_rgb32: %d rows x %d frames in one launch", t.dst_h, nframes);
  auto kernel = fmt.bytes() == 1 ? (pairs ? k_yuv_to_rgb32<1, 2> : k_yuv_to_rgb32<1, 1>) : (pairs ? k_yuv_to_rgb32<2, 2> : k_yuv_to_rgb32<2, 1>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, sy, su, sv, deep, t.lh, t.lv, t.ch, t.cv, t.dst_w, t.dst_h, t.th, yuv_mode, vec_ok, (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- a YUV clip lent in memory (tm_set_frames_yuv): its checks, and the stage seam's, with no device call
int check_yuv_clip(const tm_yuv_clip *c, ClipPlanes *out) {
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

// what both stage seams do once their arguments are accepted: the tables of this one conversion, the launch, and the wait for it
static int stage_convert(const void *y, const void *u, const void *v, const int64_t strides[6], const SampleFmt &fmt, int nframes, int src_w, int src_h, int chroma,
                         int dst_w, int dst_h, int yuv_mode, void *out_rgb32, hipStream_t stream) {
  InputTables tables;
  TM_TRY(build_input_tables(src_w, src_h, chroma, dst_w, dst_h, &tables, stream));
  // (without a header to say otherwise a clip is limited range, as FFmpeg assumes)
  TM_TRY(launch_yuv_to_rgb32(tables, y, u, v, strides, fmt, nframes, resolve_yuv_mode(yuv_mode, 0), out_rgb32, stream));
  TM_HIP(hipStreamSynchronize(stream));  // the tables are freed on return
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_yuv_clip_host(const tm_yuv_clip *clip, double scaling, int *dst_width, int *dst_height) {
  TM_TRY(check_yuv_clip(clip, nullptr));
  int dw = 0, dh = 0;
  TM_TRY(scaled_size(clip->width, clip->height, scaling, &dw, &dh));
  if (dst_width) *dst_width = dw;
  if (dst_height) *dst_height = dh;
  return TM_OK;
}

int tm_stage_yuv_to_rgb32(const void *y, const void *u, const void *v, const int64_t strides[6], int nframes, int src_w, int src_h, int chroma, int dst_w, int dst_h,
                          int yuv_mode, void *out_rgb32, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  ChromaGeom g;
  TM_CHECK(chroma >= TM_CHROMA_444 && chroma <= TM_CHROMA_MONO, TM_E_INVAL, "bad chroma layout %d", chroma);
  TM_TRY(chroma_geom(chroma, src_w, src_h, &g));
  const bool has_c = chroma != TM_CHROMA_MONO;
  TM_CHECK(y && out_rgb32 && strides && (!has_c || (u && v)) && nframes >= 0 && src_w > 0 && src_h > 0 && dst_w > 0 && dst_h > 0, TM_E_INVAL, "yuv_to_rgb32: bad arguments");
  TM_CHECK(yuv_mode >= TM_YUV_AUTO && yuv_mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "bad YUV mode %d", yuv_mode);
  TM_CHECK(strides[0] >= src_w && strides[1] >= 0 && (!has_c || (strides[2] >= g.cw && strides[4] >= g.cw && strides[3] >= 0 && strides[5] >= 0)), TM_E_INVAL,
           "yuv_to_rgb32: a row stride is shorter than its plane's rows");
  return stage_convert(y, u, v, strides, SampleFmt(), nframes, src_w, src_h, chroma, dst_w, dst_h, yuv_mode, out_rgb32, (hipStream_t)stream);
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
  return stage_convert(y, u, v, strides, pl.fmt, nframes, src_w, src_h, chroma, dst_w, dst_h, yuv_mode, out_rgb32, (hipStream_t)stream);
}

}  // extern "C"
