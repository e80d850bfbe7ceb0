// tm_yuv_out.hip -- decoded frames leave as YUV: the forward colour rules, the checks of a destination (tm_yuv_out), and the kernel that
// turns RGB32 frames into planes of Y, U, V on the device (the mirror image of tm_yuv_in.hip's k_yuv_to_rgb32).
//
// One sample, one rounding.  A sample at depth d is ((c . S + half) >> s) + off, clamped to 0 .. 2^d - 1: c the row of the 16-bit matrix, S the
// weighted sum of R, G, B over the sample's footprint (weights totalling 2^lw), s = 16 - (d - 8) + lw, half = 1 << (s - 1).  Footprints: the
// pixel (luma, 4:4:4); the 2 x 2 block (420jpeg); columns 2k - 1, 2k, 2k + 1 with weights 1, 2, 1 (422), on rows 2j and 2j + 1 (420mpeg2).
// Coordinates outside the picture repeat the edge pixel.
#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

// ---- the colour rules -------------------------------------------------------------------------------------------------------------------
// round(k 65536) of the matrix that follows from Kr, Kb (limited: luma x 219/255, chroma x 224/255); the G column absorbs the rounding, so
// that the Y row sums to round(ys 65536) and the U and V rows to 0: grey stays grey at every level.  Rows Y, U, V; columns R, G, B.
static const int32_t kForward[4][3][3] = {
    {{16829, 33039, 6416}, {-9714, -19070, 28784}, {28784, -24103, -4681}},   // BT601_LIMITED
    {{19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}},  // BT601_FULL
    {{11966, 40254, 4064}, {-6596, -22188, 28784}, {28784, -26145, -2639}},   // BT709_LIMITED
    {{13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}},   // BT709_FULL
};
static int matrix_of(int mode) {
  switch (mode) {
    case TM_YUV_BT601_LIMITED: return 0;
    case TM_YUV_BT601_FULL: return 1;
    case TM_YUV_BT709_LIMITED: return 2;
    case TM_YUV_BT709_FULL: return 3;
    default: return -1;
  }
}
static bool mode_is_full(int mode) { return mode == TM_YUV_BT601_FULL || mode == TM_YUV_BT709_FULL; }

struct YuvRule {  // what the kernel and the host seam convert by
  int32_t c[3][3];
  int depth, yoff, coff;
  int hshift;  // U16_HIGH: the stored word is the sample << (16 - depth)
  int tiler;   // TM_YUV_TILER: RGBToYUV's arithmetic instead of the matrix
};
static YuvRule make_rule(int mode, int samples, int depth) {
  YuvRule r{};
  r.depth = depth;
  r.hshift = samples == TM_SAMPLES_U16_HIGH ? 16 - depth : 0;
  r.tiler = mode == TM_YUV_TILER;
  const int m = matrix_of(mode);
  if (m >= 0) memcpy(r.c, kForward[m], sizeof(r.c));
  r.yoff = mode_is_full(mode) || r.tiler ? 0 : 16 << (depth - 8);
  r.coff = 128 << (depth - 8);
  return r;
}

__host__ __device__ __forceinline__ int yuv_sample(const int32_t c[3], int sr, int sg, int sb, int lw, int depth, int off) {
  const int s = 16 - (depth - 8) + lw;
  const int v = ((c[0] * sr + c[1] * sg + c[2] * sb + (1 << (s - 1))) >> s) + off;  // (arithmetic shift: floor)
  const int top = (1 << depth) - 1;
  return v < 0 ? 0 : v > top ? top : v;
}

// RGBToYUV (utils.pas:478-490) as GenerateY4M rounds it: the decimal constants are doubles, every right-hand side narrows to Single once,
// + 128 in Single, round half to even, clamp.  Plain double arithmetic: the build compiles host and device code with contraction off.
__host__ __device__ __forceinline__ int tiler_round(float v) {
  const double q = __builtin_rint((double)v);
  return q < 0.0 ? 0 : q > 255.0 ? 255 : (int)q;
}
__host__ __device__ __forceinline__ void tiler_yuv(int rr, int gg, int bb, int *y, int *u, int *v) {
  const float yy = (float)(rr * (299.0 / 1000) + gg * (587.0 / 1000) + bb * (114.0 / 1000));
  const float uu = (float)(((double)bb - (double)yy) * 0.492), vv = (float)(((double)rr - (double)yy) * 0.877);
  *y = tiler_round(yy + 0.0f);
  *u = tiler_round(uu + 128.0f);
  *v = tiler_round(vv + 128.0f);
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------------
// A lane owns YO_PX = 16 neighbouring pixels of one row -- of two rows where the layout's chroma spans two (420jpeg, 420mpeg2) -- so every
// RGB pixel is loaded once, as four 16-byte loads per row, and every sample a lane stores comes from pixels it holds.  The one exception is
// the left neighbour of the 1-2-1 footprint (column 16 g - 1): it comes from the lane before by a cross-lane move (__shfl_up: one
// ds_bpermute_b32 per row in the ISA -- the LDS crossbar, no LDS memory); only the first lane of a wave loads it, 4 bytes that its neighbour
// wave has just brought into the cache.  Lanes are numbered row-major over (row unit, group of 16 columns), so waves stay full whatever the
// width.  No LDS memory is used.
//   Stores: a lane's 16 luma samples are 16 bytes (32 as words), its chroma 8 to 64; each run leaves as 16-byte stores where its address is
// 16-byte aligned, as 8- or 4-byte stores where only that holds, sample by sample otherwise and at the picture's right edge.
//   BYTES per sample (1, or 2 for little-endian words) and CSTEP (2: U and V alternate in one plane, NV12 / P010) are compile-time, as in
// k_yuv_to_rgb32; so is TWO, the rows a lane holds, so that the one-row layouts (444, 422, mono) carry half the registers.
constexpr int YO_PX = 16;
struct PlaneDst { uint8_t *p; int64_t row, frame; };  // strides in bytes
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int BYTES, int N>
__device__ __forceinline__ void store_run(uint8_t *dst, const int (&v)[N], int n) {
  constexpr int NB = N * BYTES, NW = NB / 4;
  if (n >= N) {
    uint32_t w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) {
      if constexpr (BYTES == 1) w[i] = (uint32_t)v[4 * i] | (uint32_t)v[4 * i + 1] << 8 | (uint32_t)v[4 * i + 2] << 16 | (uint32_t)v[4 * i + 3] << 24;
      else w[i] = (uint32_t)v[2 * i] | (uint32_t)v[2 * i + 1] << 16;
    }
    const uintptr_t a = (uintptr_t)dst;
    if constexpr (NB % 16 == 0) {
      if ((a & 15) == 0) {
#pragma unroll
        for (int i = 0; i < NW / 4; i++) reinterpret_cast<uint4 *>(dst)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
        return;
      }
    }
    if ((a & 7) == 0) {
#pragma unroll
      for (int i = 0; i < NW / 2; i++) reinterpret_cast<uint2 *>(dst)[i] = make_uint2(w[2 * i], w[2 * i + 1]);
      return;
    }
    if ((a & 3) == 0) {
#pragma unroll
      for (int i = 0; i < NW; i++) reinterpret_cast<uint32_t *>(dst)[i] = w[i];
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++)
    if (i < n) {
      if constexpr (BYTES == 1) dst[i] = (uint8_t)v[i];
      else reinterpret_cast<uint16_t *>(dst)[i] = (uint16_t)v[i];
    }
}

// NC chroma samples of a lane from their footprints' sums: planar into pu and pv, or as (U, V) pairs into pu
template <int BYTES, int CSTEP, int NC>
__device__ __forceinline__ void put_chroma(const int (&sr)[NC], const int (&sg)[NC], const int (&sb)[NC], int lw, const YuvRule &rule, uint8_t *pu, uint8_t *pv, int n) {
  int U[NC], V[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    U[k] = yuv_sample(rule.c[1], sr[k], sg[k], sb[k], lw, rule.depth, rule.coff) << rule.hshift;
    V[k] = yuv_sample(rule.c[2], sr[k], sg[k], sb[k], lw, rule.depth, rule.coff) << rule.hshift;
  }
  if constexpr (CSTEP == 2) {
    int uv[2 * NC];
#pragma unroll
    for (int k = 0; k < NC; k++) { uv[2 * k] = U[k]; uv[2 * k + 1] = V[k]; }
    store_run<BYTES, 2 * NC>(pu, uv, 2 * n);
  } else {
    store_run<BYTES, NC>(pu, U, n);
    store_run<BYTES, NC>(pv, V, n);
  }
}

__device__ __forceinline__ int ch_r(uint32_t c) { return (int)((c >> 16) & 0xff); }
__device__ __forceinline__ int ch_g(uint32_t c) { return (int)((c >> 8) & 0xff); }
__device__ __forceinline__ int ch_b(uint32_t c) { return (int)(c & 0xff); }

template <int BYTES, int CSTEP, bool TWO>
__global__ __launch_bounds__(256) void k_rgb32_to_yuv(const uint32_t *__restrict__ rgb, int64_t stride_px, int w, int h, PlaneDst dy, PlaneDst du, PlaneDst dv, YuvRule rule,
                                                      int chroma, int ngx, int nru) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < (int64_t)ngx * nru;
  const int ru = live ? (int)(idx / ngx) : 0, gx = live ? (int)(idx - (int64_t)ru * ngx) : 0;  // (a lane past the end reads group 0: the moves below need every lane)
  const int64_t frame = blockIdx.y;
  constexpr bool two = TWO;  // 420jpeg, 420mpeg2: the lane owns rows 2 ru and 2 ru + 1
  constexpr int ROWS = TWO ? 2 : 1;
  const bool wide = chroma == TM_CHROMA_422 || chroma == TM_CHROMA_420MPEG2;    // the 1-2-1 footprint
  const int x0 = gx * YO_PX, y0 = two ? ru * 2 : ru;
  const uint32_t *src = rgb + frame * h * stride_px;
  uint32_t px[ROWS][YO_PX], left[ROWS] = {};
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const uint32_t *row = src + (int64_t)min(y0 + r, h - 1) * stride_px;
    if (x0 + YO_PX <= w && ((uintptr_t)(row + x0) & 15) == 0) {
#pragma unroll
      for (int i = 0; i < YO_PX / 4; i++) {
        u32x4 q = reinterpret_cast<const u32x4 *>(row + x0)[i];
        asm volatile("" : "+v"(q));  // (keeps the four words one value: without it the compiler folds this path into the clamped one below, word by word)
        px[r][4 * i] = q.x; px[r][4 * i + 1] = q.y; px[r][4 * i + 2] = q.z; px[r][4 * i + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < YO_PX; i++) px[r][i] = row[min(x0 + i, w - 1)];
    }
    if (wide) {
      const uint32_t before = __shfl_up(px[r][YO_PX - 1], 1);  // (the lane before holds group gx - 1 of the same rows whenever gx > 0)
      left[r] = gx == 0 ? px[r][0] : (threadIdx.x & 63) == 0 ? row[x0 - 1] : before;
    }
  }
  if (!live) return;
  const int ny = min(YO_PX, w - x0);
  uint8_t *ybase = dy.p + frame * dy.frame + (int64_t)x0 * BYTES;

  if constexpr (BYTES == 1) {
    if (rule.tiler) {  // 8-bit 4:4:4 or mono (check_yuv_out)
      int Y[YO_PX], U[YO_PX], V[YO_PX];
#pragma unroll
      for (int i = 0; i < YO_PX; i++) tiler_yuv(ch_r(px[0][i]), ch_g(px[0][i]), ch_b(px[0][i]), &Y[i], &U[i], &V[i]);
      store_run<1, YO_PX>(ybase + (int64_t)y0 * dy.row, Y, ny);
      if (chroma == TM_CHROMA_444) {
        uint8_t *pu = du.p + frame * du.frame + (int64_t)y0 * du.row + (int64_t)x0 * CSTEP;
        if constexpr (CSTEP == 2) {
          int uv[2 * YO_PX];
#pragma unroll
          for (int i = 0; i < YO_PX; i++) { uv[2 * i] = U[i]; uv[2 * i + 1] = V[i]; }
          store_run<1, 2 * YO_PX>(pu, uv, 2 * ny);
        } else {
          store_run<1, YO_PX>(pu, U, ny);
          store_run<1, YO_PX>(dv.p + frame * dv.frame + (int64_t)y0 * dv.row + x0, V, ny);
        }
      }
      return;
    }
  }

#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    if (y0 + r >= h) continue;
    int Y[YO_PX];
#pragma unroll
    for (int i = 0; i < YO_PX; i++) Y[i] = yuv_sample(rule.c[0], ch_r(px[r][i]), ch_g(px[r][i]), ch_b(px[r][i]), 0, rule.depth, rule.yoff) << rule.hshift;
    store_run<BYTES, YO_PX>(ybase + (int64_t)(y0 + r) * dy.row, Y, ny);
  }
  if (chroma == TM_CHROMA_MONO) return;

  if (chroma == TM_CHROMA_444) {
    int sr[YO_PX], sg[YO_PX], sb[YO_PX];
#pragma unroll
    for (int i = 0; i < YO_PX; i++) { sr[i] = ch_r(px[0][i]); sg[i] = ch_g(px[0][i]); sb[i] = ch_b(px[0][i]); }
    const int64_t at = (int64_t)x0 * CSTEP * BYTES;
    put_chroma<BYTES, CSTEP, YO_PX>(sr, sg, sb, 0, rule, du.p + frame * du.frame + (int64_t)y0 * du.row + at, dv.p + frame * dv.frame + (int64_t)y0 * dv.row + at, ny);
    return;
  }
  constexpr int NC = YO_PX / 2;
  int sr[NC], sg[NC], sb[NC];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    sr[k] = sg[k] = sb[k] = 0;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const uint32_t a = px[r][2 * k], b = px[r][2 * k + 1];
      if (wide) {  // columns 2k - 1, 2k, 2k + 1: weights 1, 2, 1
        const uint32_t l = k == 0 ? left[r] : px[r][(2 * k - 1) & (YO_PX - 1)];
        sr[k] += ch_r(l) + 2 * ch_r(a) + ch_r(b); sg[k] += ch_g(l) + 2 * ch_g(a) + ch_g(b); sb[k] += ch_b(l) + 2 * ch_b(a) + ch_b(b);
      } else if (two) {  // the 2 x 2 block
        sr[k] += ch_r(a) + ch_r(b); sg[k] += ch_g(a) + ch_g(b); sb[k] += ch_b(a) + ch_b(b);
      }
    }
  }
  const int lw = chroma == TM_CHROMA_420MPEG2 ? 3 : 2;
  const int cw = (w + 1) / 2, cx0 = gx * NC, cy = two ? ru : y0;
  const int64_t at = (int64_t)cx0 * CSTEP * BYTES;
  put_chroma<BYTES, CSTEP, NC>(sr, sg, sb, lw, rule, du.p + frame * du.frame + (int64_t)cy * du.row + at, dv.p + frame * dv.frame + (int64_t)cy * dv.row + at, min(NC, cw - cx0));
}

// ---- the destination's checks (no device call) --------------------------------------------------------------------------------------------
int check_yuv_out(const tm_yuv_out *d, int width, int height, int mode, YuvOutPlan *out) {
  TM_CHECK(d, TM_E_INVAL, "yuv out: null descriptor");
  TM_CHECK(d->chroma >= TM_CHROMA_444 && d->chroma <= TM_CHROMA_MONO, TM_E_INVAL, "yuv out: unknown chroma layout %d", d->chroma);
  TM_CHECK(d->samples >= TM_SAMPLES_U8 && d->samples <= TM_SAMPLES_U16_HIGH, TM_E_INVAL, "yuv out: unknown sample format %d", d->samples);
  TM_CHECK(d->memory == TM_MEM_HOST || d->memory == TM_MEM_DEVICE, TM_E_INVAL, "yuv out: unknown memory kind %d", d->memory);
  TM_CHECK(mode >= TM_YUV_AUTO && mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "yuv out: bad YUV mode %d", mode);
  TM_CHECK(d->y, TM_E_INVAL, "yuv out: null y plane");
  const bool has_c = d->chroma != TM_CHROMA_MONO;
  TM_CHECK(!(d->v && !d->u), TM_E_INVAL, "yuv out: a v plane without a u plane");
  TM_CHECK(!has_c || d->u, TM_E_INVAL, "yuv out: layout %d has chroma, but u is null", d->chroma);
  TM_CHECK(width >= 1 && height >= 1 && d->width == width && d->height == height, TM_E_INVAL, "yuv out: the destination is %dx%d, the frames are %dx%d", d->width,
           d->height, width, height);
  TM_CHECK(d->frames >= 1, TM_E_INVAL, "yuv out: room for %d frames", d->frames);
  if (d->samples == TM_SAMPLES_U8) TM_CHECK(d->depth == 8, TM_E_INVAL, "yuv out: depth %d with 8-bit samples", d->depth);
  else TM_CHECK(d->depth >= 9 && d->depth <= 16, TM_E_INVAL, "yuv out: depth %d with 16-bit samples (9 .. 16)", d->depth);
  YuvOutPlan p;
  p.mode = mode == TM_YUV_AUTO ? (d->full_range ? TM_YUV_BT601_FULL : TM_YUV_BT601_LIMITED) : mode;
  if (p.mode == TM_YUV_TILER)
    TM_CHECK(d->samples == TM_SAMPLES_U8 && (d->chroma == TM_CHROMA_444 || d->chroma == TM_CHROMA_MONO), TM_E_INVAL,
             "yuv out: TM_YUV_TILER is defined for 8-bit 4:4:4 and mono only");
  if (mode_is_full(p.mode) && d->samples != TM_SAMPLES_U8) {
    set_error("yuv out: a full-range rule with %d-bit samples is not delivered (its scale (2^d - 1) / 255 is not a shift)", d->depth);
    return TM_E_UNSUPPORTED;
  }
  p.w = width; p.h = height; p.chroma = d->chroma; p.samples = d->samples; p.depth = d->depth;
  p.bytes = d->samples == TM_SAMPLES_U8 ? 1 : 2;
  p.pairs = has_c && !d->v;
  const bool half_w = d->chroma != TM_CHROMA_444, half_h = d->chroma == TM_CHROMA_420JPEG || d->chroma == TM_CHROMA_420MPEG2;
  p.cw = !has_c ? 0 : half_w ? (width + 1) / 2 : width;
  p.ch = !has_c ? 0 : half_h ? (height + 1) / 2 : height;
  p.nplanes = !has_c ? 1 : p.pairs ? 2 : 3;
  p.row_bytes[0] = (int64_t)width * p.bytes; p.rows[0] = height;
  p.row_bytes[1] = (int64_t)p.cw * p.bytes * (p.pairs ? 2 : 1); p.rows[1] = p.ch;
  p.row_bytes[2] = (int64_t)p.cw * p.bytes; p.rows[2] = p.ch;
  const void *ptr[3] = {d->y, d->u, d->v};
  const int64_t row[3] = {d->y_row, d->u_row, d->v_row}, frame[3] = {d->y_frame, d->u_frame, d->v_frame};
  static const char *const names[3] = {"y", "u", "v"};
  for (int i = 0; i < p.nplanes; i++) {
    TM_CHECK(row[i] >= p.row_bytes[i], TM_E_INVAL, "yuv out: the %s row stride %lld is shorter than a row of %lld bytes", names[i], (long long)row[i], (long long)p.row_bytes[i]);
    TM_CHECK(frame[i] >= 0, TM_E_INVAL, "yuv out: negative %s frame stride %lld", names[i], (long long)frame[i]);
    TM_CHECK(p.bytes == 1 || (((uintptr_t)ptr[i] | (uint64_t)row[i] | (uint64_t)frame[i]) & 1) == 0, TM_E_INVAL, "yuv out: an odd %s pointer or stride with 16-bit samples", names[i]);
  }
  if (out) *out = p;
  return TM_OK;
}

YuvDst yuv_dst_of(const tm_yuv_out &d, int64_t frame0) {
  YuvDst o{};
  uint8_t *ptr[3] = {(uint8_t *)d.y, (uint8_t *)d.u, (uint8_t *)d.v};
  const int64_t row[3] = {d.y_row, d.u_row, d.v_row}, frame[3] = {d.y_frame, d.u_frame, d.v_frame};
  for (int i = 0; i < 3; i++) { o.p[i] = ptr[i] ? ptr[i] + frame[i] * frame0 : nullptr; o.row[i] = row[i]; o.frame[i] = frame[i]; }
  return o;
}

YuvDst yuv_dst_packed(const YuvOutPlan &p, uint8_t *base, int cap, int frame0) {
  YuvDst o{};
  for (int i = 0; i < p.nplanes; i++) {
    o.p[i] = base + p.plane_bytes(i) * frame0; o.row[i] = p.row_bytes[i]; o.frame[i] = p.plane_bytes(i);
    base += p.plane_bytes(i) * cap;
  }
  return o;
}

int yuv_out_is_device(const tm_yuv_out &d, int device) {
  const void *ptr[3] = {d.y, d.u, d.v};
  for (const void *q : ptr) {
    if (!q) continue;
    hipPointerAttribute_t at;
    const bool ok = hipPointerGetAttributes(&at, q) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device;
    (void)hipGetLastError();
    TM_CHECK(ok, TM_E_INVAL, "yuv out: a plane is not memory of device %d", device);
  }
  return TM_OK;
}

int launch_rgb32_to_yuv(const YuvOutPlan &p, const void *rgb, int64_t stride_px, int nframes, const YuvDst &d, hipStream_t stream) {
  if (nframes <= 0) return TM_OK;
  const bool has_c = p.chroma != TM_CHROMA_MONO, two = p.chroma == TM_CHROMA_420JPEG || p.chroma == TM_CHROMA_420MPEG2;
  const int ngx = (p.w + YO_PX - 1) / YO_PX, nru = two ? (p.h + 1) / 2 : p.h;
  const int64_t lanes = (int64_t)ngx * nru;
  const PlaneDst dy{d.p[0], d.row[0], d.frame[0]}, du{has_c ? d.p[1] : nullptr, d.row[1], d.frame[1]},
      dv{has_c ? (p.pairs ? d.p[1] + p.bytes : d.p[2]) : nullptr, d.row[p.pairs ? 1 : 2], d.frame[p.pairs ? 1 : 2]};
  const YuvRule rule = make_rule(p.mode, p.samples, p.depth);
  auto kernel = two ? (p.bytes == 1 ? (p.pairs ? k_rgb32_to_yuv<1, 2, true> : k_rgb32_to_yuv<1, 1, true>) : (p.pairs ? k_rgb32_to_yuv<2, 2, true> : k_rgb32_to_yuv<2, 1, true>))
                    : (p.bytes == 1 ? (p.pairs ? k_rgb32_to_yuv<1, 2, false> : k_rgb32_to_yuv<1, 1, false>) : (p.pairs ? k_rgb32_to_yuv<2, 2, false> : k_rgb32_to_yuv<2, 1, false>));
  constexpr int LAUNCH_FRAMES = 32768;  // (grid.y)
  for (int f0 = 0; f0 < nframes; f0 += LAUNCH_FRAMES) {
    const int nf = std::min(LAUNCH_FRAMES, nframes - f0);
    auto at = [&](PlaneDst q) { if (q.p) q.p += q.frame * f0; return q; };
    hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)nf), dim3(256), 0, stream, (const uint32_t *)rgb + (int64_t)f0 * p.h * stride_px, stride_px,
                       p.w, p.h, at(dy), at(du), at(dv), rule, p.chroma, ngx, nru);
  }
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// nf frames of a packed chunk (yuv_dst_packed) into the caller's planes from frame0 on: one copy per plane where the strides allow it
int yuv_copy_out(const YuvOutPlan &p, const uint8_t *packed, int cap, const tm_yuv_out &d, int64_t frame0, int nf, hipStream_t stream) {
  const YuvDst o = yuv_dst_of(d, frame0);
  for (int i = 0; i < p.nplanes; i++) {
    const int64_t rb = p.row_bytes[i], pb = p.plane_bytes(i);
    if (pb == 0) continue;
    if (o.row[i] == rb && (o.frame[i] == pb || nf == 1)) {
      TM_HIP(hipMemcpyAsync(o.p[i], packed, (size_t)pb * nf, hipMemcpyDeviceToHost, stream));
    } else if (o.frame[i] == o.row[i] * p.rows[i]) {
      TM_HIP(hipMemcpy2DAsync(o.p[i], (size_t)o.row[i], packed, (size_t)rb, (size_t)rb, (size_t)p.rows[i] * nf, hipMemcpyDeviceToHost, stream));
    } else {
      for (int f = 0; f < nf; f++) {
        if (o.row[i] == rb) TM_HIP(hipMemcpyAsync(o.p[i] + o.frame[i] * f, packed + pb * f, (size_t)pb, hipMemcpyDeviceToHost, stream));
        else TM_HIP(hipMemcpy2DAsync(o.p[i] + o.frame[i] * f, (size_t)o.row[i], packed + pb * f, (size_t)rb, (size_t)rb, (size_t)p.rows[i], hipMemcpyDeviceToHost, stream));
      }
    }
    packed += pb * cap;
  }
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_yuv_out_host(const tm_yuv_out *dst, int width, int height, int mode) { return check_yuv_out(dst, width, height, mode, nullptr); }

int tm_yuv_out_matrix_host(int mode, int32_t m[9]) {
  const int k = matrix_of(mode);
  TM_CHECK(m && k >= 0, TM_E_INVAL, "yuv out: mode %d has no integer matrix", mode);
  memcpy(m, kForward[k], sizeof(kForward[k]));
  return TM_OK;
}

int tm_rgb32_to_yuv_host(const uint32_t *rgb, int64_t n, int mode, int depth, uint16_t *y, uint16_t *u, uint16_t *v) {
  TM_CHECK((rgb || n == 0) && n >= 0, TM_E_INVAL, "rgb32_to_yuv: bad arguments");
  TM_CHECK(mode >= TM_YUV_AUTO && mode <= TM_YUV_BT709_FULL, TM_E_INVAL, "yuv out: bad YUV mode %d", mode);
  TM_CHECK(depth >= 8 && depth <= 16, TM_E_INVAL, "yuv out: depth %d (8 .. 16)", depth);
  if (mode == TM_YUV_AUTO) mode = TM_YUV_BT601_LIMITED;  // (no destination says otherwise)
  TM_CHECK(mode != TM_YUV_TILER || depth == 8, TM_E_INVAL, "yuv out: TM_YUV_TILER is defined for 8-bit samples only");
  if (mode_is_full(mode) && depth != 8) {
    set_error("yuv out: a full-range rule with %d-bit samples is not delivered (its scale (2^d - 1) / 255 is not a shift)", depth);
    return TM_E_UNSUPPORTED;
  }
  const YuvRule r = make_rule(mode, depth == 8 ? TM_SAMPLES_U8 : TM_SAMPLES_U16_LOW, depth);
  for (int64_t i = 0; i < n; i++) {
    const uint32_t c = rgb[i];
    const int rr = (c >> 16) & 0xff, gg = (c >> 8) & 0xff, bb = c & 0xff;
    int Y, U, V;
    if (r.tiler) tiler_yuv(rr, gg, bb, &Y, &U, &V);
    else {
      Y = yuv_sample(r.c[0], rr, gg, bb, 0, depth, r.yoff);
      U = yuv_sample(r.c[1], rr, gg, bb, 0, depth, r.coff);
      V = yuv_sample(r.c[2], rr, gg, bb, 0, depth, r.coff);
    }
    if (y) y[i] = (uint16_t)Y;
    if (u) u[i] = (uint16_t)U;
    if (v) v[i] = (uint16_t)V;
  }
  return TM_OK;
}

int tm_stage_rgb32_to_yuv_fmt(const void *rgb32, int64_t stride_px, int nframes, int w, int h, void *y, void *u, void *v, const int64_t *strides, int chroma, int samples,
                              int depth, int mode, void *stream) {
  TM_CHECK(rgb32 && strides && nframes >= 0 && w >= 1 && h >= 1 && stride_px >= w && ((uintptr_t)rgb32 & 3) == 0, TM_E_INVAL, "rgb32_to_yuv: bad arguments");
  tm_yuv_out d{};  // the planes as a destination: the checks are tm_player_read_yuv's
  d.y = y; d.u = u; d.v = v;
  d.y_row = strides[0]; d.y_frame = strides[1]; d.u_row = strides[2]; d.u_frame = strides[3]; d.v_row = strides[4]; d.v_frame = strides[5];
  d.width = w; d.height = h; d.frames = std::max(nframes, 1); d.fps = 1.0;
  d.chroma = chroma; d.samples = samples; d.depth = depth; d.memory = TM_MEM_DEVICE;
  YuvOutPlan plan;
  TM_TRY(check_yuv_out(&d, w, h, mode, &plan));  // (AUTO: limited, there is no header)
  knobs_reload();
  TM_TRY(require_device());
  return launch_rgb32_to_yuv(plan, rgb32, stride_px, nframes, yuv_dst_of(d, 0), (hipStream_t)stream);
}

}  // extern "C"
