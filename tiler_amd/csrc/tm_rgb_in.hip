// tm_rgb_in.hip -- an RGB clip lent in memory (tm_rgb_clip: packed, planar, 8- or 16-bit, host or device) into the RGB32 frames Load reads,
// scaled on the way (tm_yuv_in.hip's twin for RGB sources): the checks of a lent clip, the two kernels, the host twin
// and the stage seam.  No arithmetic of its own: a sample becomes a byte by tm_yuv_clip's deep rule (DeepRule, tm_input.h), a pixel is
// R << 16 | G << 8 | B, and a clip at another size is tm_scale.hip's Lanczos rule on those pixels, with its tables (ScaleTables).
#include "tm_input.h"

namespace tmx {

// ---- the fetch ---------------------------------------------------------------------------------------------------------------------------
// What a kernel is told about the clip: the three channel pointers and the shared strides, in bytes.  How a pixel is read is a compile-time
// property of the kernel: BYTES per sample, and PIX.
//   PIX (interleaved layouts whose pixel spans at most 4 bytes, or 6 bytes of words): the pixel's `span` bytes from the lowest pointer are
// fetched for the three channels at once, as the aligned 4-byte granule that holds its first byte and the granule that holds its last
// byte (the same one again when the pixel does not run on into the next).  Both hold a described sample byte of this pixel, and an aligned
// granule cannot cross a page: no load touches memory that the clip's own samples do not share a granule with.  (A 4-byte load at an RGB24
// pixel's own address would run a byte past the clip's last pixel.)  span - 1 + (address & 3) < 8 for these spans, so the second granule
// is the first one itself or its neighbour, and the two make one 64-bit word the channels are shifted out of.
//   !PIX (planar clips, odd descriptors): every sample is loaded on its own, at its own address and width.
struct RgbSrc {
  const uint8_t *c[3];      // R, G, B of pixel (0, 0) of the first frame of the launch
  const uint8_t *base;      // PIX: the lowest of the three
  int64_t step, row, frame;
  int shift[3];             // PIX: 8 x (c[i] - base)
  int span;                 // PIX: bytes from base to the end of the pixel's last sample
};

template <int BYTES, bool PIX>
__device__ __forceinline__ void fetch_rgb(const RgbSrc &s, int64_t at, const DeepRule &d, int &R, int &G, int &B) {
  int v[3];
  if constexpr (PIX) {
    const uintptr_t a = (uintptr_t)(s.base + at), lo_a = a & ~(uintptr_t)3, hi_a = (a + (uintptr_t)(s.span - 1)) & ~(uintptr_t)3;
    const uint32_t lo = *reinterpret_cast<const uint32_t *>(lo_a), hi = *reinterpret_cast<const uint32_t *>(hi_a);  // (no branch: hi_a may be lo_a)
    const uint64_t px = (((uint64_t)hi << 32) | lo) >> ((a & 3) * 8);  // the pixel's bytes from base on
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = (int)((px >> s.shift[i]) & (BYTES == 1 ? 0xffu : 0xffffu));
  } else {
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = BYTES == 1 ? (int)s.c[i][at] : (int)*reinterpret_cast<const uint16_t *>(s.c[i] + at);
  }
  if constexpr (BYTES == 2) {
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = narrow_word(v[i], d);
  }
  R = v[0]; G = v[1]; B = v[2];
}

__device__ __forceinline__ int rgb_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ---- at the source's size: a pure unpack, one pass, no tables, no LDS ----------------------------------------------------------------------
// A workgroup owns 256 x 4 pixels of a frame; a lane unpacks four neighbouring pixels of a row and stores them as 16 bytes where the
// destination allows it.
constexpr int UNPACK_TW = 256, UNPACK_TH = 4;
template <int BYTES, bool PIX>
__global__ __launch_bounds__(256) void k_rgb_unpack(RgbSrc s, DeepRule deep, int w, int h, int vec_ok, uint32_t *__restrict__ out) {
  const int x = blockIdx.x * UNPACK_TW + (threadIdx.x & 63) * 4, y = blockIdx.y * UNPACK_TH + (threadIdx.x >> 6), frame = blockIdx.z;
  if (x >= w || y >= h) return;
  const int64_t at = (int64_t)frame * s.frame + (int64_t)y * s.row + (int64_t)x * s.step;
  uint32_t px[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (x + j < w) {  // (no pixel past the row's last is fetched)
      int R, G, B;
      fetch_rgb<BYTES, PIX>(s, at + (int64_t)j * s.step, deep, R, G, B);
      px[j] = (uint32_t)R << 16 | (uint32_t)G << 8 | (uint32_t)B;
    }
  uint32_t *o = out + ((int64_t)frame * h + y) * w + x;
  if (vec_ok) *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);  // (w % 4 == 0: the four pixels are inside)
  else
    for (int j = 0; j < 4 && x + j < w; j++) o[j] = px[j];
}

// ---- at another size: k_scale_rgb32_lanczos3's shape (tm_scale.hip), with the descriptor's fetch ----------------------------------------------
// A workgroup owns SC_TW x th output pixels of a frame.  The horizontal pass of the source rows its vertical taps reach goes into LDS as
// three int32 planes -- a source pixel is fetched once and feeds the three channels' sums -- then every lane runs the vertical pass for
// four neighbouring pixels of one row out of LDS and stores them as 16 bytes.  th and the tables are ScaleTables' (SC_HROWS rows of LDS).
template <int BYTES, bool PIX>
__global__ __launch_bounds__(256) void k_rgb_to_rgb32(RgbSrc s, DeepRule deep, AxisTaps ah, AxisTaps av, int dst_w, int dst_h, int th, int vec_ok, uint32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) int32_t hbuf[3][SC_HROWS * SC_TW];
  const int x0 = blockIdx.x * SC_TW, y0 = blockIdx.y * th, frame = blockIdx.z;
  const int y_last = min(y0 + th, dst_h) - 1;
  const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
  const int hx = threadIdx.x & (SC_TW - 1), hr0 = threadIdx.x / SC_TW;  // the horizontal pass: one column, rows hr0, hr0 + 4, ...
  const bool mine = ty < th && y0 + ty <= y_last;
  const int oxc = min(x0 + hx, dst_w - 1), oyc = min(y0 + ty, dst_h - 1);
  const int hfirst = ah.first[oxc], hcount = ah.count[oxc], vfirst = av.first[oyc], vcount = av.count[oyc];
  const int2 span = av.span[blockIdx.y];  // the source rows the tile's samples reach: first row, number of rows
  const int r0 = span.x, rows = span.y;
  if (x0 + hx < dst_w) {
    const int ox = x0 + hx;
    const int64_t col = (int64_t)frame * s.frame + (int64_t)hfirst * s.step;
    constexpr int RS = 256 / SC_TW;
    for (int rb = hr0; rb < rows; rb += 4 * RS) {  // four rows at a time, so that a coefficient is loaded once for twelve products
      const int64_t row = col + (int64_t)(r0 + rb) * s.row;
      int acc[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int k = 0; k < hcount; k++) {
        const int c = ah.coef[(int64_t)k * dst_w + ox];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (rb + i * RS < rows) {
            int R, G, B;
            fetch_rgb<BYTES, PIX>(s, row + (int64_t)i * RS * s.row + (int64_t)k * s.step, deep, R, G, B);
            acc[i][0] += c * R; acc[i][1] += c * G; acc[i][2] += c * B;
          }
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (rb + i * RS < rows) {
#pragma unroll
          for (int ch = 0; ch < 3; ch++) hbuf[ch][(rb + i * RS) * SC_TW + hx] = (acc[i][ch] + 64) >> 7;  // (arithmetic shift, no clamp)
        }
    }
  }
  __syncthreads();
  if (!mine || x0 + tx >= dst_w) return;
  const int oy = y0 + ty, k0 = vfirst - r0;
  int acc[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int k = 0; k < vcount; k++) {
    const int c = av.coef[(int64_t)k * dst_h + oy];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int4 hv = *reinterpret_cast<const int4 *>(&hbuf[ch][(k0 + k) * SC_TW + tx]);
      acc[ch][0] += c * hv.x; acc[ch][1] += c * hv.y; acc[ch][2] += c * hv.z; acc[ch][3] += c * hv.w;
    }
  }
  uint32_t px[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    px[j] = (uint32_t)rgb_clamp255((acc[0][j] + (1 << 20)) >> 21) << 16 | (uint32_t)rgb_clamp255((acc[1][j] + (1 << 20)) >> 21) << 8 |
            (uint32_t)rgb_clamp255((acc[2][j] + (1 << 20)) >> 21);
  uint32_t *o = out + ((int64_t)frame * dst_h + oy) * dst_w + x0 + tx;
  if (vec_ok) *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);  // (dst_w % 4 == 0: the four pixels are inside)
  else
    for (int j = 0; j < 4 && x0 + tx + j < dst_w; j++) o[j] = px[j];
}

// ---- the checks of a lent clip, with no device call: pointers are compared, never read --------------------------------------------------------
int check_rgb_clip(const tm_rgb_clip *c, RgbPlan *out) {
  TM_CHECK(c, TM_E_INVAL, "rgb clip: null descriptor");
  TM_CHECK(c->r && c->g && c->b, TM_E_INVAL, "rgb clip: null %s channel", !c->r ? "r" : !c->g ? "g" : "b");
  TM_CHECK(c->width >= 1 && c->width <= 65536 && c->height >= 1 && c->height <= 65536, TM_E_INVAL, "rgb clip: bad size %dx%d", c->width, c->height);
  TM_CHECK(c->frames >= 1, TM_E_INVAL, "rgb clip: %d frames", c->frames);
  TM_CHECK(c->fps > 0, TM_E_INVAL, "rgb clip: frame rate %g", c->fps);
  TM_CHECK(c->samples >= TM_SAMPLES_U8 && c->samples <= TM_SAMPLES_U16_HIGH, TM_E_INVAL, "rgb clip: unknown sample format %d", c->samples);
  TM_CHECK(c->memory == TM_MEM_HOST || c->memory == TM_MEM_DEVICE, TM_E_INVAL, "rgb clip: unknown memory kind %d", c->memory);
  if (c->samples == TM_SAMPLES_U8) TM_CHECK(c->depth == 8, TM_E_INVAL, "rgb clip: depth %d with 8-bit samples", c->depth);
  else TM_CHECK(c->depth >= 9 && c->depth <= 16, TM_E_INVAL, "rgb clip: depth %d with 16-bit samples (9 .. 16)", c->depth);
  RgbPlan p;
  p.fmt.samples = c->samples; p.fmt.depth = c->depth;
  const int B = p.fmt.bytes();
  TM_CHECK(c->step >= B, TM_E_INVAL, "rgb clip: step %lld is shorter than a sample of %d bytes", (long long)c->step, B);
  // row >= (width - 1) step + B, without the product
  TM_CHECK(c->row >= B && (c->width == 1 || c->step <= (c->row - B) / (c->width - 1)), TM_E_INVAL,
           "rgb clip: the row stride %lld is shorter than a row of (%d - 1) x step %lld + %d bytes", (long long)c->row, c->width, (long long)c->step, B);
  TM_CHECK(c->frame >= 0, TM_E_INVAL, "rgb clip: negative frame stride %lld", (long long)c->frame);
  TM_CHECK(B == 1 || (((uintptr_t)c->r | (uintptr_t)c->g | (uintptr_t)c->b | (uint64_t)c->step | (uint64_t)c->row | (uint64_t)c->frame) & 1) == 0, TM_E_INVAL,
           "rgb clip: an odd pointer, step or stride with 16-bit samples");
  const uintptr_t ptr[3] = {(uintptr_t)c->r, (uintptr_t)c->g, (uintptr_t)c->b};
  const uintptr_t lowest = std::min(ptr[0], std::min(ptr[1], ptr[2])), highest = std::max(ptr[0], std::max(ptr[1], ptr[2]));
  p.base = (const uint8_t *)lowest;
  p.sample_row_bytes = (int64_t)(c->width - 1) * c->step + B;
  if (highest - lowest < (uint64_t)c->step && (uint64_t)(c->row - p.sample_row_bytes) >= highest - lowest) {
    p.interleaved = true;
    for (int i = 0; i < 3; i++) p.off[i] = (int64_t)(ptr[i] - lowest);
    p.span = (int64_t)(highest - lowest) + B;
    p.pixel_row_bytes = p.sample_row_bytes + (int64_t)(highest - lowest);
  }
  if (out) *out = p;
  return TM_OK;
}

template <int BYTES, bool PIX>
static void launch_one(const RgbSrc &s, const DeepRule &deep, const ScaleTables *t, int src_w, int src_h, int nf, int dst_w, int dst_h, int vec_ok, uint32_t *out,
                       hipStream_t stream) {
  if (t == nullptr) {
    const dim3 grid((unsigned)((src_w + UNPACK_TW - 1) / UNPACK_TW), (unsigned)((src_h + UNPACK_TH - 1) / UNPACK_TH), (unsigned)nf);
    hipLaunchKernelGGL((k_rgb_unpack<BYTES, PIX>), grid, dim3(256), 0, stream, s, deep, src_w, src_h, vec_ok, out);
  } else {
    const dim3 grid((unsigned)((dst_w + SC_TW - 1) / SC_TW), (unsigned)((dst_h + t->th - 1) / t->th), (unsigned)nf);
    hipLaunchKernelGGL((k_rgb_to_rgb32<BYTES, PIX>), grid, dim3(256), 0, stream, s, deep, t->taps_h, t->taps_v, dst_w, dst_h, t->th, vec_ok, out);
  }
}

int launch_rgb_to_rgb32(const tm_rgb_clip &c, const RgbPlan &plan, const ScaleTables *tables, int nframes, int dst_w, int dst_h, void *out, hipStream_t stream) {
  if (nframes <= 0) return TM_OK;
  const bool scaled = dst_w != c.width || dst_h != c.height;
  TM_CHECK(scaled == (tables != nullptr), TM_E_INVAL, "rgb_to_rgb32: tables %s for %dx%d -> %dx%d", tables ? "given" : "missing", c.width, c.height, dst_w, dst_h);
  if (tables)
    TM_CHECK(tables->ready && tables->on_device && tables->filter == TM_SCALE_LANCZOS3 && tables->src_w == c.width && tables->src_h == c.height && tables->dst_w == dst_w &&
                 tables->dst_h == dst_h, TM_E_INVAL, "rgb_to_rgb32: the tables on the device are not those of %dx%d -> %dx%d", c.width, c.height, dst_w, dst_h);
  const int B = plan.fmt.bytes();
  // which fetch (fetch_rgb): a pixel at a time where the pixel lies in two neighbouring granules at most -- it measured faster than sample by
  // sample in both kernels
  const bool pix = plan.interleaved && plan.span <= (B == 1 ? 4 : 6);
  RgbSrc s{};
  s.c[0] = (const uint8_t *)c.r; s.c[1] = (const uint8_t *)c.g; s.c[2] = (const uint8_t *)c.b;
  s.base = plan.base; s.step = c.step; s.row = c.row; s.frame = c.frame;
  if (pix) {
    for (int i = 0; i < 3; i++) s.shift[i] = (int)plan.off[i] * 8;
    s.span = (int)plan.span;
  }
  const DeepRule deep = deep_rule_of(plan.fmt);
  const int vec_ok = (dst_w % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  constexpr int LAUNCH_FRAMES = 32768;  // (grid.z; grid.y is at most 65536 / 4 rows of tiles)
  const size_t out_fb = (size_t)dst_w * dst_h;
  for (int f0 = 0; f0 < nframes; f0 += LAUNCH_FRAMES) {
    const int nf = std::min(LAUNCH_FRAMES, nframes - f0);
    RgbSrc sf = s;
    for (int i = 0; i < 3; i++) sf.c[i] += c.frame * f0;
    sf.base += c.frame * f0;
    uint32_t *o = (uint32_t *)out + out_fb * f0;
    if (B == 1) pix ? launch_one<1, true>(sf, deep, tables, c.width, c.height, nf, dst_w, dst_h, vec_ok, o, stream)
                    : launch_one<1, false>(sf, deep, tables, c.width, c.height, nf, dst_w, dst_h, vec_ok, o, stream);
    else pix ? launch_one<2, true>(sf, deep, tables, c.width, c.height, nf, dst_w, dst_h, vec_ok, o, stream)
             : launch_one<2, false>(sf, deep, tables, c.width, c.height, nf, dst_w, dst_h, vec_ok, o, stream);
  }
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_rgb_clip_host(const tm_rgb_clip *clip, double scaling, int *dst_width, int *dst_height) {
  TM_TRY(check_rgb_clip(clip, nullptr));
  int dw = 0, dh = 0;
  TM_TRY(scaled_size(clip->width, clip->height, scaling, &dw, &dh));
  if (dst_width) *dst_width = dw;
  if (dst_height) *dst_height = dh;
  return TM_OK;
}

int tm_rgb_to_rgb32_host(const tm_rgb_clip *clip, int first_frame, int frame_count, int dst_w, int dst_h, uint32_t *out) {
  RgbPlan plan;
  TM_TRY(check_rgb_clip(clip, &plan));
  TM_CHECK(clip->memory == TM_MEM_HOST, TM_E_INVAL, "rgb_to_rgb32_host: the clip is not host memory");
  TM_CHECK(out && dst_w >= 1 && dst_h >= 1, TM_E_INVAL, "rgb_to_rgb32_host: bad destination");
  TM_CHECK(first_frame >= 0 && frame_count >= 0 && (int64_t)first_frame + frame_count <= clip->frames, TM_E_INVAL, "rgb_to_rgb32_host: frames [%d,+%d) of %d", first_frame,
           frame_count, clip->frames);
  const int w = clip->width, h = clip->height, B = plan.fmt.bytes();
  const bool scaled = dst_w != w || dst_h != h;
  if (scaled) TM_TRY(tm_probe_scale_host(w, h, dst_w, dst_h, TM_SCALE_LANCZOS3));
  const DeepRule deep = deep_rule_of(plan.fmt);
  const uint8_t *ch[3] = {(const uint8_t *)clip->r, (const uint8_t *)clip->g, (const uint8_t *)clip->b};
  std::vector<uint32_t> frame(scaled ? (size_t)w * h : 0);
  for (int f = 0; f < frame_count; f++) {
    uint32_t *dst = out + (size_t)dst_w * dst_h * f, *px = scaled ? frame.data() : dst;
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const int64_t at = (int64_t)(first_frame + f) * clip->frame + (int64_t)y * clip->row + (int64_t)x * clip->step;
        uint32_t v = 0;
        for (int i = 0; i < 3; i++) {
          int p = ch[i][at];
          if (B == 2) p = narrow_word(p | (int)ch[i][at + 1] << 8, deep);  // little-endian words
          v = v << 8 | (uint32_t)p;
        }
        px[(size_t)y * w + x] = v;
      }
    if (scaled) TM_TRY(tm_scale_rgb32_host(px, w, w, h, dst, dst_w, dst_w, dst_h, TM_SCALE_LANCZOS3));
  }
  return TM_OK;
}

int tm_stage_rgb_to_rgb32(const tm_rgb_clip *clip, int dst_w, int dst_h, void *out_rgb32, void *stream) {
  RgbPlan plan;
  TM_TRY(check_rgb_clip(clip, &plan));
  TM_CHECK(clip->memory == TM_MEM_DEVICE, TM_E_INVAL, "rgb_to_rgb32: the clip's memory kind must be TM_MEM_DEVICE");
  TM_CHECK(out_rgb32 && dst_w >= 1 && dst_h >= 1, TM_E_INVAL, "rgb_to_rgb32: bad destination");
  const bool scaled = dst_w != clip->width || dst_h != clip->height;
  ScaleTables t;
  if (scaled) TM_TRY(t.prepare(clip->width, clip->height, dst_w, dst_h, TM_SCALE_LANCZOS3));  // (every refusal of the size pair)
  knobs_reload();
  TM_TRY(require_device());
  if (scaled) TM_TRY(t.upload((hipStream_t)stream));
  TM_TRY(launch_rgb_to_rgb32(*clip, plan, scaled ? &t : nullptr, clip->frames, dst_w, dst_h, out_rgb32, (hipStream_t)stream));
  if (scaled) TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the tables are freed on return
  return TM_OK;
}

}  // extern "C"
