// tm_scale.hip -- decoded frames at a caller's size: RGB32 frames resampled on the device.  A frame is uint32
// 0x00RRGGBB; R, G and B are three planes at luma positions (s = 1, o = 0 in section 17's terms).  Two filters:
//   TM_SCALE_LANCZOS3  section 17's rule per channel, tables of resample_taps(n, m, n, 1, 0) (tm_resample.hip): horizontal pass first,
//                      h = (sum c p + 64) >> 7, then v = clamp((sum c h + 2^20) >> 21, 0, 255); shrinking an axis by more than 8 is refused
//   TM_SCALE_NEAREST   output sample j of m takes source sample ((2 j + 1) n) / (2 m), per axis; no shrink limit
// The output's top byte is 0 whatever the source's holds.  The host twin (tm_scale_rgb32_host) is plain loops over the same tables.
#include "tm_internal.h"

namespace tmx {

// ---- the Lanczos kernel ------------------------------------------------------------------------------------------------------------------
// A workgroup owns SC_TW x th output pixels of one frame.  The horizontal pass of the source rows its vertical taps reach goes into LDS as
// three int32 planes (the rule keeps 7 extra bits between the passes: a sum reaches 1.55 x 16384 x 255 / 128, beyond int16): a source word
// is fetched once and feeds the three channels' sums.  Then every lane runs the vertical pass for four neighbouring pixels of one row out of
// LDS, for the three channels at once, and stores them as 16 bytes.  Nothing goes to HBM between the passes.  The host picks th so that the
// rows a tile reaches fit SC_HROWS (resample_tile_rows); 3 x 80 x 64 x 4 bytes = 60 KB of LDS, two workgroups to a CU.
// (SC_TW = 64, SC_HROWS = 80: tm_internal.h, beside the tables that are sized for them; tm_rgb_in.hip's kernel shares both)
struct ScaleGeom { int64_t src_row, src_frame, dst_row, dst_frame; int src_w, src_h, dst_w, dst_h, th, vec_ok; };  // strides in pixels

__device__ __forceinline__ int sc_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ __launch_bounds__(256) void k_scale_rgb32_lanczos3(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, AxisTaps ah, AxisTaps av, ScaleGeom g) {
  __shared__ __attribute__((aligned(16))) int32_t hbuf[3][SC_HROWS * SC_TW];
  const int x0 = blockIdx.x * SC_TW, y0 = blockIdx.y * g.th, frame = blockIdx.z;
  const int y_last = min(y0 + g.th, g.dst_h) - 1;
  const int tx = (threadIdx.x & 15) * 4, ty = threadIdx.x >> 4;
  const int hx = threadIdx.x & (SC_TW - 1), hr0 = threadIdx.x / SC_TW;  // the horizontal pass: one column, rows hr0, hr0 + 4, ...
  const bool mine = ty < g.th && y0 + ty <= y_last;
  const int oxc = min(x0 + hx, g.dst_w - 1), oyc = min(y0 + ty, g.dst_h - 1);
  const int hfirst = ah.first[oxc], hcount = ah.count[oxc], vfirst = av.first[oyc], vcount = av.count[oyc];
  const int2 span = av.span[blockIdx.y];  // the source rows the tile's samples reach: first row, number of rows
  const int r0 = span.x, rows = span.y;
  if (x0 + hx < g.dst_w) {
    const int ox = x0 + hx;
    const uint32_t *col = src + (int64_t)frame * g.src_frame + hfirst;
    constexpr int RS = 256 / SC_TW;
    for (int rb = hr0; rb < rows; rb += 4 * RS) {  // four rows at a time, so that a coefficient is loaded once for twelve products
      const uint32_t *row = col + (int64_t)(r0 + rb) * g.src_row;
      int acc[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int k = 0; k < hcount; k++) {
        const int c = ah.coef[(int64_t)k * g.dst_w + ox];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (rb + i * RS < rows) {
            const uint32_t p = row[(int64_t)i * RS * g.src_row + k];
            acc[i][0] += c * (int)((p >> 16) & 0xff); acc[i][1] += c * (int)((p >> 8) & 0xff); acc[i][2] += c * (int)(p & 0xff);
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
  if (!mine || x0 + tx >= g.dst_w) return;
  const int oy = y0 + ty, k0 = vfirst - r0;
  int acc[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int k = 0; k < vcount; k++) {
    const int c = av.coef[(int64_t)k * g.dst_h + oy];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int4 h = *reinterpret_cast<const int4 *>(&hbuf[ch][(k0 + k) * SC_TW + tx]);
      acc[ch][0] += c * h.x; acc[ch][1] += c * h.y; acc[ch][2] += c * h.z; acc[ch][3] += c * h.w;
    }
  }
  uint32_t px[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    px[j] = (uint32_t)sc_clamp255((acc[0][j] + (1 << 20)) >> 21) << 16 | (uint32_t)sc_clamp255((acc[1][j] + (1 << 20)) >> 21) << 8 |
            (uint32_t)sc_clamp255((acc[2][j] + (1 << 20)) >> 21);
  uint32_t *o = dst + (int64_t)frame * g.dst_frame + (int64_t)oy * g.dst_row + x0 + tx;
  if (g.vec_ok) *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[1], px[2], px[3]);  // (dst_w % 4 == 0: the four pixels are inside)
  else
    for (int j = 0; j < 4 && x0 + tx + j < g.dst_w; j++) o[j] = px[j];
}

// ---- the nearest filter: a gather, one output pixel per lane ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scale_rgb32_nearest(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, ScaleGeom g) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, frame = blockIdx.z;
  if (x >= g.dst_w) return;
  // (2 j + 1) n < 2^32 for sizes up to 32768
  const uint32_t sx = ((uint32_t)(2 * x + 1) * (uint32_t)g.src_w) / (uint32_t)(2 * g.dst_w), sy = ((uint32_t)(2 * y + 1) * (uint32_t)g.src_h) / (uint32_t)(2 * g.dst_h);
  dst[(int64_t)frame * g.dst_frame + (int64_t)y * g.dst_row + x] = src[(int64_t)frame * g.src_frame + (int64_t)sy * g.src_row + sx] & 0x00ffffffu;
}

// ---- checks (no device call) ---------------------------------------------------------------------------------------------------------------
int probe_scale(int src_w, int src_h, int dst_w, int dst_h, int filter) {
  TM_CHECK(src_w >= 1 && src_h >= 1 && dst_w >= 1 && dst_h >= 1, TM_E_INVAL, "scale: bad size %dx%d -> %dx%d", src_w, src_h, dst_w, dst_h);
  TM_CHECK(filter == TM_SCALE_LANCZOS3 || filter == TM_SCALE_NEAREST, TM_E_INVAL, "scale: unknown filter %d", filter);
  TM_CHECK(src_w <= TM_SCALE_MAX_SIZE && src_h <= TM_SCALE_MAX_SIZE && dst_w <= TM_SCALE_MAX_SIZE && dst_h <= TM_SCALE_MAX_SIZE, TM_E_UNSUPPORTED,
           "scale: %dx%d -> %dx%d: a size above %d", src_w, src_h, dst_w, dst_h, TM_SCALE_MAX_SIZE);
  if (filter == TM_SCALE_LANCZOS3)
    TM_CHECK((int64_t)src_w <= 8 * (int64_t)dst_w && (int64_t)src_h <= 8 * (int64_t)dst_h, TM_E_UNSUPPORTED,
             "scale: Lanczos-3 %dx%d -> %dx%d shrinks an axis by more than 8 (more than %d taps)", src_w, src_h, dst_w, dst_h, TM_RESAMPLE_MAX_TAPS);
  return TM_OK;
}

// the sizes and the filter, the pointers, the strides (in pixels) and that the two ranges of memory do not meet
int check_scale_args(const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, int src_w, int src_h, const void *dst, int64_t dst_stride_px,
                     int64_t dst_frame_px, int dst_w, int dst_h, int filter) {
  TM_TRY(probe_scale(src_w, src_h, dst_w, dst_h, filter));
  TM_CHECK(src && dst, TM_E_INVAL, "scale: null pointer");
  TM_CHECK((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, TM_E_INVAL, "scale: the frames must be 4-byte aligned");
  TM_CHECK(nframes >= 0, TM_E_INVAL, "scale: %d frames", nframes);
  TM_CHECK(src_stride_px >= src_w && dst_stride_px >= dst_w, TM_E_INVAL, "scale: a row stride (%lld, %lld pixels) is shorter than its row (%d, %d)",
           (long long)src_stride_px, (long long)dst_stride_px, src_w, dst_w);
  const int64_t src_px = src_stride_px * (src_h - 1) + src_w, dst_px = dst_stride_px * (dst_h - 1) + dst_w;  // of one frame, first to last pixel
  TM_CHECK(nframes <= 1 || (src_frame_px >= src_px && dst_frame_px >= dst_px), TM_E_INVAL, "scale: a frame stride (%lld, %lld pixels) is shorter than its frame (%lld, %lld)",
           (long long)src_frame_px, (long long)dst_frame_px, (long long)src_px, (long long)dst_px);
  if (nframes >= 1) {
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)(src_frame_px * (nframes - 1) + src_px) * 4, d0 = (uintptr_t)dst, d1 = d0 + (size_t)(dst_frame_px * (nframes - 1) + dst_px) * 4;
    TM_CHECK(s1 <= d0 || d1 <= s0, TM_E_INVAL, "scale: source and destination overlap");
  }
  return TM_OK;
}

// ---- the tables of one size pair ---------------------------------------------------------------------------------------------------------
static int scale_tables_host(int src_w, int src_h, int dst_w, int dst_h, AxisTable *h, AxisTable *v, int *th) {
  TM_TRY(h->make(src_w, dst_w, src_w, 1, 0));
  TM_TRY(v->make(src_h, dst_h, src_h, 1, 0));
  TM_TRY(check_resample_sums(*h, *v, src_w, src_h, dst_w, dst_h));
  h->trim(); v->trim();
  const AxisTable *const vert[1] = {v};
  *th = resample_tile_rows(vert, 1, SC_HROWS);
  TM_CHECK(*th > 0, TM_E_UNSUPPORTED, "scale: %d -> %d rows reach too many source rows per tile", src_h, dst_h);
  return TM_OK;
}

int ScaleTables::prepare(int sw, int sh, int dw, int dh, int flt) {
  TM_TRY(probe_scale(sw, sh, dw, dh, flt));
  if (ready && sw == src_w && sh == src_h && dw == dst_w && dh == dst_h && flt == filter) return TM_OK;
  AxisTable nh, nv;
  int nth = 0;
  if (flt == TM_SCALE_LANCZOS3) TM_TRY(scale_tables_host(sw, sh, dw, dh, &nh, &nv, &nth));
  h = std::move(nh); v = std::move(nv); th = nth;
  src_w = sw; src_h = sh; dst_w = dw; dst_h = dh; filter = flt;
  ready = true; on_device = false;
  return TM_OK;
}

int ScaleTables::upload(hipStream_t stream) {
  if (on_device || filter != TM_SCALE_LANCZOS3) return TM_OK;
  const AxisTable *const axes[2] = {&h, &v};
  AxisTaps out[2];
  TM_TRY(upload_axis_tables(axes, 2, th, SC_HROWS, &dev, out, stream));
  taps_h = out[0]; taps_v = out[1];
  on_device = true;
  return TM_OK;
}

// nframes frames; the tables are prepared and uploaded, the arguments checked (check_scale_args)
int launch_scale_rgb32(const ScaleTables &t, const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, void *dst, int64_t dst_stride_px, int64_t dst_frame_px,
                       hipStream_t stream) {
  if (nframes <= 0) return TM_OK;
  TM_CHECK(t.ready && (t.on_device || t.filter != TM_SCALE_LANCZOS3), TM_E_INVAL, "scale: the tables are not on the device");
  ScaleGeom g{src_stride_px, src_frame_px, dst_stride_px, dst_frame_px, t.src_w, t.src_h, t.dst_w, t.dst_h, t.th, 0};
  g.vec_ok = (t.dst_w % 4 == 0 && ((uintptr_t)dst & 15) == 0 && dst_stride_px % 4 == 0 && (nframes == 1 || dst_frame_px % 4 == 0)) ? 1 : 0;
  constexpr int LAUNCH_FRAMES = 32768;  // (grid.z)
  for (int f0 = 0; f0 < nframes; f0 += LAUNCH_FRAMES) {
    const int nf = std::min(LAUNCH_FRAMES, nframes - f0);
    const uint32_t *s = (const uint32_t *)src + src_frame_px * f0;
    uint32_t *d = (uint32_t *)dst + dst_frame_px * f0;
    if (t.filter == TM_SCALE_LANCZOS3) {
      const dim3 grid((unsigned)((t.dst_w + SC_TW - 1) / SC_TW), (unsigned)((t.dst_h + t.th - 1) / t.th), (unsigned)nf);
      hipLaunchKernelGGL(k_scale_rgb32_lanczos3, grid, dim3(256), 0, stream, s, d, t.taps_h, t.taps_v, g);
    } else {
      const dim3 grid((unsigned)((t.dst_w + 255) / 256), (unsigned)t.dst_h, (unsigned)nf);
      hipLaunchKernelGGL(k_scale_rgb32_nearest, grid, dim3(256), 0, stream, s, d, g);
    }
  }
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_scale_host(int src_w, int src_h, int dst_w, int dst_h, int filter) { return probe_scale(src_w, src_h, dst_w, dst_h, filter); }

int tm_scale_rgb32_host(const uint32_t *src, int64_t src_stride_px, int src_w, int src_h, uint32_t *dst, int64_t dst_stride_px, int dst_w, int dst_h, int filter) {
  TM_TRY(check_scale_args(src, src_stride_px, 0, 1, src_w, src_h, dst, dst_stride_px, 0, dst_w, dst_h, filter));
  if (filter == TM_SCALE_NEAREST) {
    for (int y = 0; y < dst_h; y++) {
      const uint32_t *row = src + (((int64_t)(2 * y + 1) * src_h) / (2 * (int64_t)dst_h)) * src_stride_px;
      for (int x = 0; x < dst_w; x++) dst[y * dst_stride_px + x] = row[((int64_t)(2 * x + 1) * src_w) / (2 * (int64_t)dst_w)] & 0x00ffffffu;
    }
    return TM_OK;
  }
  ScaleTables t;
  TM_TRY(t.prepare(src_w, src_h, dst_w, dst_h, filter));
  std::vector<int32_t> hb((size_t)src_h * dst_w * 3);  // the horizontal pass of every source row
  for (int y = 0; y < src_h; y++)
    for (int x = 0; x < dst_w; x++) {
      const int32_t *c = &t.h.coef[(size_t)x * TM_RESAMPLE_MAX_TAPS];
      const uint32_t *p = src + y * src_stride_px + t.h.first[x];
      int32_t acc[3] = {0, 0, 0};
      for (int k = 0; k < t.h.count[x]; k++) { acc[0] += c[k] * (int32_t)((p[k] >> 16) & 0xff); acc[1] += c[k] * (int32_t)((p[k] >> 8) & 0xff); acc[2] += c[k] * (int32_t)(p[k] & 0xff); }
      for (int ch = 0; ch < 3; ch++) hb[((size_t)y * dst_w + x) * 3 + ch] = (acc[ch] + 64) >> 7;
    }
  for (int y = 0; y < dst_h; y++) {
    const int32_t *c = &t.v.coef[(size_t)y * TM_RESAMPLE_MAX_TAPS];
    for (int x = 0; x < dst_w; x++) {
      int32_t acc[3] = {0, 0, 0};
      for (int k = 0; k < t.v.count[y]; k++)
        for (int ch = 0; ch < 3; ch++) acc[ch] += c[k] * hb[((size_t)(t.v.first[y] + k) * dst_w + x) * 3 + ch];
      uint32_t px = 0;
      for (int ch = 0; ch < 3; ch++) px = px << 8 | (uint32_t)std::min(255, std::max(0, (acc[ch] + (1 << 20)) >> 21));
      dst[y * dst_stride_px + x] = px;
    }
  }
  return TM_OK;
}

int tm_stage_scale_rgb32(const void *src, int64_t src_stride_px, int64_t src_frame_px, int nframes, int src_w, int src_h, void *dst, int64_t dst_stride_px,
                         int64_t dst_frame_px, int dst_w, int dst_h, int filter, void *stream) {
  TM_TRY(check_scale_args(src, src_stride_px, src_frame_px, nframes, src_w, src_h, dst, dst_stride_px, dst_frame_px, dst_w, dst_h, filter));
  ScaleTables t;
  TM_TRY(t.prepare(src_w, src_h, dst_w, dst_h, filter));  // (the last refusal: sums beyond 32 bits)
  knobs_reload();
  TM_TRY(require_device());
  TM_TRY(t.upload((hipStream_t)stream));
  TM_TRY(launch_scale_rgb32(t, src, src_stride_px, src_frame_px, nframes, dst, dst_stride_px, dst_frame_px, (hipStream_t)stream));
  if (filter == TM_SCALE_LANCZOS3) TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the tables are freed on return
  return TM_OK;
}

}  // extern "C"
