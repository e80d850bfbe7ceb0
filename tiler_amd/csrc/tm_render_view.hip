// tm_render_view.hip -- Render's other views on the device (tilingencoder.pas:3455-3736 with its switches): the Output page under
// FRenderPredicted / FRenderMirrored / FRenderOutputDithered / FRenderUseGamma / FRenderPaletteIndex, the Input page, the Tiles page.
// The rule is stated once, in include/tilemotion.h (tm_render_view); DESIGN.md section 26 has the kernels and their measurement.
//
// A lane draws four neighbouring pixels of one row -- they lie in one tile-map item, whose fields it reads once -- and writes them as one
// 16-byte store.  The switches are template parameters of the Output and Input kernels: the default instantiation is px_output's work
// (tm_render.hip), per group of four.  Predicted chains are resolved per pixel, as there.  The gamma table travels as a
// kernel argument and is put into LDS once per workgroup.
#include <cmath>

#include "tm_device.h"
#include "tm_encoder.h"

namespace tmx {
namespace {

constexpr uint32_t MAGENTA = 0x00FF00FFu, AQUA = 0x0000FFFFu;
constexpr uint32_t TF_ACTIVE = 1, TF_RGB = 2, TF_PAL = 4;  // tm_tile_hdr.Flags; bits 3 and 4: H / VMirror_Initial
enum { SW_PRED = 1, SW_MIR = 2, SW_DITH = 4, SW_GAMMA = 8, SW_FILTER = 16, SW_COUNT = 32 };  // FILTER: palette_index >= 0 (with DITH only)

struct GammaLut { uint32_t w[64]; };  // lut[256], four entries a word

struct RenderViewMap {  // RenderMap and what the views read beside it
  RenderMap m;
  const uint32_t *rgb_px;          // [ntiles][64] 0x00BBGGRR
  const uint32_t *tile_flags;      // [ntiles] tm_tile_hdr.Flags bits; null: tile_flags_all | tile_mir[t] << 3 (the encoder's tiles)
  const uint8_t *tile_mir;         // [ntiles] bit 0 HMirror_Initial, bit 1 VMirror_Initial (read where tile_flags is null)
  uint32_t tile_flags_all;
  const int32_t *pal_idx_initial;  // [ntiles]; null: -1 everywhere
  int palette_index;               // the filter (Output) / the palette (Tiles); < 0: none
};

__device__ __forceinline__ uint32_t tile_flags_of(const RenderViewMap &v, int64_t t) {
  return v.tile_flags ? v.tile_flags[t] : (v.tile_flags_all | ((uint32_t)v.tile_mir[t] << 3));
}
__device__ __forceinline__ uint32_t tile_has_of(const RenderViewMap &v, int64_t t) {  // the Active / Has* bits alone: no load for the encoder's tiles
  return v.tile_flags ? v.tile_flags[t] : v.tile_flags_all;
}
__device__ __forceinline__ uint32_t gamma_px(const uint8_t *lut, uint32_t c) {
  return ((uint32_t)lut[(c >> 16) & 0xff] << 16) | ((uint32_t)lut[(c >> 8) & 0xff] << 8) | lut[c & 0xff];
}
__device__ __forceinline__ void load_lut(uint8_t *s_lut, const GammaLut &lut) {  // once per workgroup of 256
  if (threadIdx.x < 64) reinterpret_cast<uint32_t *>(s_lut)[threadIdx.x] = lut.w[threadIdx.x];
  __syncthreads();
}
// the four pixels at out[0..3]: one 16-byte store where `wide` (the destination is 16-byte aligned; the group's index is a multiple of 4)
__device__ __forceinline__ void store4(uint32_t *out, bool wide, const uint32_t c[4]) {
  if (wide) *reinterpret_cast<uint4 *>(out) = make_uint4(c[0], c[1], c[2], c[3]);
  else { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3]; }
}

// DrawTile (3457-3506) for pixels (ty, tx0 .. tx0 + 3) of a cell showing tile t through palette `pal` (null: the RGB pixels), tx0 = 0 or 4
template <bool GAMMA>
__device__ __forceinline__ void draw_tile4(const RenderViewMap &v, int64_t t, uint32_t tf, const int32_t *pal, int mir, int ty, int tx0,
                                           const uint8_t *lut, uint32_t c[4]) {
  const int sy = (mir & 2) ? 7 - ty : ty, sx0 = (mir & 1) ? 4 - tx0 : tx0;  // the four pixels in stored order; reversed when mirrored
  for (int k = 0; k < 4; k++) c[k] = MAGENTA;
  if (pal) {
    if (tf & TF_PAL) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(v.m.pal_px + t * 64 + sy * 8 + sx0);
      for (int k = 0; k < 4; k++) {
        const int ci = (w >> (8 * ((mir & 1) ? 3 - k : k))) & 0xff;
        c[k] = ci < v.m.pal_size ? swap_rb((uint32_t)pal[ci]) : 0u;
      }
    }
  } else if (tf & TF_RGB) {
    const uint4 w = *reinterpret_cast<const uint4 *>(v.rgb_px + t * 64 + sy * 8 + sx0);
    const uint32_t a[4] = {w.x, w.y, w.z, w.w};
    for (int k = 0; k < 4; k++) c[k] = swap_rb(a[(mir & 1) ? 3 - k : k]);
  }
  if (GAMMA)
    for (int k = 0; k < 4; k++) c[k] = gamma_px(lut, c[k]);
}

// the palette of Output item i under the view: false = the item is not drawn (background)
template <int SW>
__device__ __forceinline__ bool item_palette(const RenderViewMap &v, int64_t i, const int32_t **pal) {
  *pal = nullptr;
  if (!(SW & SW_DITH)) return true;
  const int32_t p = v.m.pal[i];
  if (SW & SW_FILTER) {
    if (p != v.palette_index) return false;  // (the probe holds palette_index below npal)
  } else if (p < 0 || p >= v.m.npal) return false;
  *pal = v.m.palettes + (int64_t)p * v.m.pal_size;
  return true;
}

// Output page, one pixel: the chain of predicted items back to the item that is drawn, then that item's colour under the view.  The loop
// ends at frame 0 whatever the switches: f only falls.
template <int SW>
__device__ uint32_t view_px(const RenderViewMap &v, const uint8_t *lut, int64_t f, int y, int x) {
  const RenderMap &m = v.m;
  const int64_t per = (int64_t)m.tm_w * m.tm_h;
  const int sw = m.tm_w * 8, sh = m.tm_h * 8;
  for (; f >= 0; f--) {
    const int64_t i = f * per + (int64_t)(y >> 3) * m.tm_w + (x >> 3);
    if ((SW & SW_PRED) && m.pred && (m.pred[i] & m.pred_mask)) {  // 3595-3606
      y = min(max(y + (int)m.py[i], 0), sh - 1);
      x = min(max(x + (int)m.px[i], 0), sw - 1);
      continue;
    }
    const int64_t t = m.tile[i];
    if (t < 0 || t >= m.ntiles) return 0;
    const int32_t *pal;
    if (!item_palette<SW>(v, i, &pal)) return 0;
    const int mir = (SW & SW_MIR) ? m.mir[i] : 0, ty = y & 7, tx = x & 7;
    const int o = (((mir & 2) ? 7 - ty : ty) << 3) + ((mir & 1) ? 7 - tx : tx);
    uint32_t c = MAGENTA;
    if (SW & SW_DITH) {
      if (tile_has_of(v, t) & TF_PAL) {
        const int ci = m.pal_px[t * 64 + o];
        c = ci < m.pal_size ? swap_rb((uint32_t)pal[ci]) : 0u;
      }
    } else if (tile_has_of(v, t) & TF_RGB) {
      c = swap_rb(v.rgb_px[t * 64 + o]);
    }
    return (SW & SW_GAMMA) ? gamma_px(lut, c) : c;
  }
  return 0;  // before frame 0
}

template <int SW>
__global__ __launch_bounds__(256) void k_render_view_output(RenderViewMap v, GammaLut lut, int first, int64_t n4, int wide,
                                                            uint32_t *__restrict__ out) {
  __shared__ uint8_t s_lut[256];
  if (SW & SW_GAMMA) load_lut(s_lut, lut);
  const RenderMap &m = v.m;
  const int sw4 = m.tm_w * 2;  // groups of four pixels in a row
  const int64_t per = (int64_t)m.tm_w * m.tm_h, f4 = (int64_t)sw4 * m.tm_h * 8;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t fr = e / f4, r = e - fr * f4, f = first + fr;
    const int y = (int)(r / sw4), g = (int)(r - (int64_t)y * sw4), x = g * 4;
    const int64_t i = f * per + (int64_t)(y >> 3) * m.tm_w + (g >> 1);
    uint32_t c[4] = {0, 0, 0, 0};
    if ((SW & SW_PRED) && m.pred && (m.pred[i] & m.pred_mask)) {  // predicted: every pixel traces its own chain
      for (int k = 0; k < 4; k++) c[k] = view_px<SW>(v, s_lut, f, y, x + k);
    } else {
      const int64_t t = m.tile[i];
      const int32_t *pal;
      if (t >= 0 && t < m.ntiles && item_palette<SW>(v, i, &pal))
        draw_tile4<(SW & SW_GAMMA) != 0>(v, t, tile_has_of(v, t), pal, (SW & SW_MIR) ? m.mir[i] : 0, y & 7, x & 7, s_lut, c);
    }
    store4(out + e * 4, wide != 0, c);
  }
}

template <bool MIR, bool GAMMA>
__global__ __launch_bounds__(256) void k_render_view_input(RenderInput in, GammaLut lut, int first, int64_t n4, int wide, uint32_t *__restrict__ out) {
  __shared__ uint8_t s_lut[256];
  if (GAMMA) load_lut(s_lut, lut);
  const int sw4 = in.tm_w * 2;
  const int64_t per = (int64_t)in.tm_w * in.tm_h, f4 = (int64_t)sw4 * in.tm_h * 8;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t fr = e / f4, r = e - fr * f4;
    const int y = (int)(r / sw4), g = (int)(r - (int64_t)y * sw4), ty = y & 7, tx0 = (g & 1) * 4;
    const int64_t i = (first + fr) * per + (int64_t)(y >> 3) * in.tm_w + (g >> 1);
    const int mir = MIR ? in.flags[i] : 0;
    const uint4 w = *reinterpret_cast<const uint4 *>(in.tiles + i * 64 + ((mir & 2) ? 7 - ty : ty) * 8 + ((mir & 1) ? 4 - tx0 : tx0));
    const uint32_t a[4] = {w.x, w.y, w.z, w.w};
    uint32_t c[4];
    for (int k = 0; k < 4; k++) {
      c[k] = swap_rb(a[(mir & 1) ? 3 - k : k]);  // (forceActive, no palette: the frame tiles all hold RGB pixels)
      if (GAMMA) c[k] = gamma_px(s_lut, c[k]);
    }
    store4(out + e * 4, wide != 0, c);
  }
}

// Tiles page (3678-3707): page first + p shows tiles [per * (first + p), +per), aqua beyond the last.  sw: SW_MIR | SW_DITH | SW_GAMMA, uniform,
// tested once per group of four pixels.
__global__ __launch_bounds__(256) void k_render_tile_page(RenderViewMap v, GammaLut lut, int sw, int first, int64_t n4, int wide,
                                                          uint32_t *__restrict__ out) {
  __shared__ uint8_t s_lut[256];
  if (sw & SW_GAMMA) load_lut(s_lut, lut);
  const RenderMap &m = v.m;
  const int sw4 = m.tm_w * 2;
  const int64_t per = (int64_t)m.tm_w * m.tm_h, f4 = (int64_t)sw4 * m.tm_h * 8;
  const bool with_pal = (sw & SW_DITH) && m.npal > 0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pg = e / f4, r = e - pg * f4;
    const int y = (int)(r / sw4), g = (int)(r - (int64_t)y * sw4);
    const int64_t t = (first + pg) * per + (int64_t)(y >> 3) * m.tm_w + (g >> 1);
    uint32_t c[4] = {AQUA, AQUA, AQUA, AQUA};
    if (t < m.ntiles) {
      const uint32_t tf = tile_flags_of(v, t);
      const int mir = (sw & SW_MIR) ? (int)((tf >> 3) & 3) : 0;
      const int32_t *pal = nullptr;
      bool drawn = true;
      if (with_pal) {
        const int p = v.palette_index >= 0 ? v.palette_index : max(0, v.pal_idx_initial ? v.pal_idx_initial[t] : -1);
        drawn = p < m.npal;
        if (drawn) pal = m.palettes + (int64_t)p * m.pal_size;
      }
      if (!drawn) c[0] = c[1] = c[2] = c[3] = 0;
      else if (sw & SW_GAMMA) draw_tile4<true>(v, t, (tf & TF_ACTIVE) ? tf : 0u, pal, mir, y & 7, (g & 1) * 4, s_lut, c);
      else draw_tile4<false>(v, t, (tf & TF_ACTIVE) ? tf : 0u, pal, mir, y & 7, (g & 1) * 4, s_lut, c);
    }
    store4(out + e * 4, wide != 0, c);
  }
}

inline int grid_of(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 64)); }
inline int wide_ok(const void *out) { return ((uintptr_t)out & 15) == 0; }  // rows are multiples of 8 pixels: every group of four is aligned with `out`

// the switches of a view as the kernels' word, and its gamma table (all zeros without gamma: never read)
int switches_of(const tm_render_view &view) {
  int sw = (view.predicted ? SW_PRED : 0) | (view.mirrored ? SW_MIR : 0) | (view.dithered ? SW_DITH : 0) | (view.use_gamma ? SW_GAMMA : 0);
  if (view.dithered && view.palette_index >= 0) sw |= SW_FILTER;
  return sw;
}
GammaLut lut_of(const tm_render_view &view) {
  GammaLut l{};
  if (view.use_gamma) {
    uint8_t b[256];
    (void)tm_render_gamma_lut_host(view.gamma, b);
    memcpy(l.w, b, 256);
  }
  return l;
}

template <int SW>
void launch_output_sw(const RenderViewMap &v, const GammaLut &lut, int first, int64_t n4, void *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_render_view_output<SW>, dim3(grid_of(n4)), dim3(256), 0, stream, v, lut, first, n4, wide_ok(out), (uint32_t *)out);
}
template <int... SW>
void launch_output_any(std::integer_sequence<int, SW...>, int sw, const RenderViewMap &v, const GammaLut &lut, int first, int64_t n4, void *out,
                       hipStream_t stream) {
  using Fn = void (*)(const RenderViewMap &, const GammaLut &, int, int64_t, void *, hipStream_t);
  static const Fn table[] = {&launch_output_sw<(SW & SW_DITH) ? SW : (SW & ~SW_FILTER)>...};  // (no filter without a palette: 24 kernels)
  table[sw](v, lut, first, n4, out, stream);
}

int launch_view_output(const RenderViewMap &v, const tm_render_view &view, int first, int count, void *out, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  const int64_t n4 = (int64_t)count * v.m.tm_w * 2 * v.m.tm_h * 8;
  launch_output_any(std::make_integer_sequence<int, SW_COUNT>{}, switches_of(view), v, lut_of(view), first, n4, out, stream);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_view_input(const RenderInput &in, const tm_render_view &view, int first, int count, void *out, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  const int64_t n4 = (int64_t)count * in.tm_w * 2 * in.tm_h * 8;
  const GammaLut lut = lut_of(view);
  const dim3 grid(grid_of(n4)), block(256);
  const int wide = wide_ok(out);
  if (view.mirrored && view.use_gamma) hipLaunchKernelGGL((k_render_view_input<true, true>), grid, block, 0, stream, in, lut, first, n4, wide, (uint32_t *)out);
  else if (view.mirrored) hipLaunchKernelGGL((k_render_view_input<true, false>), grid, block, 0, stream, in, lut, first, n4, wide, (uint32_t *)out);
  else if (view.use_gamma) hipLaunchKernelGGL((k_render_view_input<false, true>), grid, block, 0, stream, in, lut, first, n4, wide, (uint32_t *)out);
  else hipLaunchKernelGGL((k_render_view_input<false, false>), grid, block, 0, stream, in, lut, first, n4, wide, (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_tile_pages(const RenderViewMap &v, const tm_render_view &view, int first, int count, void *out, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  const int64_t n4 = (int64_t)count * v.m.tm_w * 2 * v.m.tm_h * 8;
  hipLaunchKernelGGL(k_render_tile_page, dim3(grid_of(n4)), dim3(256), 0, stream, v, lut_of(view), switches_of(view), first, n4, wide_ok(out),
                     (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int64_t tile_pages_of(int64_t ntiles, int tm_w, int tm_h) {
  const int64_t per = (int64_t)tm_w * tm_h;
  return per > 0 ? (ntiles + per - 1) / per : 0;
}

// the encoder's tiles beside a RenderMap: their RGB pixels, header flags (tm_get_tiles' bits, HasRGBPixels false after ReloadGTM) and first palettes
RenderViewMap view_map_of(tm_encoder *e, const RenderMap &m, const tm_render_view &view) {
  const bool prepared = e->gpal_idx.p && (e->steps_done & (1 << TM_STEP_PREPARE_PALETTES));
  return RenderViewMap{m, e->gtiles.as<uint32_t>(), nullptr, e->gflags.as<uint8_t>(),
                       TF_ACTIVE | (e->gtiles_have_rgb ? TF_RGB : 0u) | (e->has_pal_px ? TF_PAL : 0u), prepared ? e->gpal_idx.as<int32_t>() : nullptr,
                       view.palette_index};
}

// draws into `out` (device) or through a device buffer of the call's (host), as tm_render_frames does; blocking
template <class Launch>
int deliver(tm_encoder *e, int count, void *out, int out_on_device, const Launch &launch) {
  const size_t bytes = (size_t)count * e->tm_w * 8 * e->tm_h * 8 * 4;
  DevBuf tmp;
  void *dst = out;
  if (!out_on_device) {
    TM_TRY(tmp.alloc(bytes));
    dst = tmp.p;
  }
  TM_TRY(launch(dst));
  if (!out_on_device) TM_HIP(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

}  // namespace
}  // namespace tmx

extern "C" {

int tm_render_view_default(tm_render_view *view) {
  TM_CHECK(view, TM_E_INVAL, "render view: null struct");
  *view = tm_render_view{TM_RENDER_PAGE_OUTPUT, 1, 1, 1, 0, -1, 0.6};
  return TM_OK;
}

int tm_probe_render_view_host(const tm_render_view *view, int pal_count) {
  TM_CHECK(view, TM_E_INVAL, "render view: null struct");
  TM_CHECK(view->page == TM_RENDER_PAGE_INPUT || view->page == TM_RENDER_PAGE_OUTPUT || view->page == TM_RENDER_PAGE_TILES, TM_E_INVAL,
           "render view: unknown page %d", view->page);
  TM_CHECK(!std::isnan(view->gamma), TM_E_INVAL, "render view: gamma is not a number");
  TM_CHECK(view->palette_index < pal_count, TM_E_INVAL, "render view: palette %d of %d", view->palette_index, std::max(pal_count, 0));
  return TM_OK;
}

int tm_render_gamma_lut_host(double gamma, uint8_t lut[256]) {
  TM_CHECK(lut && !std::isnan(gamma), TM_E_INVAL, "gamma table: %s", lut ? "gamma is not a number" : "null table");
  const double g = std::max(0.0, gamma);  // SetRenderGammaValue, 3024-3027
  for (int i = 0; i < 256; i++) lut[i] = (uint8_t)std::nearbyint(std::pow(i / 255.0, g) * 255.0);  // round: half to even
  return TM_OK;
}

int tm_render_view_frames(tm_encoder *e, const tm_render_view *view, int first_frame, int frame_count, void *out, int out_on_device) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(view, TM_E_INVAL, "render view: null struct");
  TM_CHECK(view->page != TM_RENDER_PAGE_TILES, TM_E_INVAL, "render view: the Tiles page is drawn by tm_render_tile_pages");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  RenderMap m{};
  RenderInput in{};
  const bool input = view->page == TM_RENDER_PAGE_INPUT;
  if (input) {
    TM_TRY(tm_probe_render_view_host(view, INT32_MAX));  // (the Input page ignores the palette)
    TM_TRY(render_input_src(e, first_frame, frame_count, &in));
  } else {
    TM_TRY(render_output_map(e, &m));
    TM_TRY(tm_probe_render_view_host(view, m.npal));
  }
  if (frame_count == 0) return TM_OK;
  TM_HIP(hipSetDevice(e->device));
  return deliver(e, frame_count, out, out_on_device, [&](void *dst) {
    return input ? launch_view_input(in, *view, first_frame, frame_count, dst, e->stream)
                 : launch_view_output(view_map_of(e, m, *view), *view, first_frame, frame_count, dst, e->stream);
  });
}

int tm_get_tile_page_count(tm_encoder *e, int *pages) {
  TM_CHECK(e && pages, TM_E_INVAL, "null argument");
  TM_CHECK(e->t > 0 && e->tm_size() > 0 && e->gtiles.p && e->gflags.p && (e->steps_done & (1 << TM_STEP_REDUCE)), TM_E_INVAL,
           "tile pages: there are no tiles yet (run Reduce, or ReloadGTM)");
  *pages = (int)tile_pages_of(e->t, e->tm_w, e->tm_h);
  return TM_OK;
}

int tm_render_tile_pages(tm_encoder *e, const tm_render_view *view, int first_page, int page_count, void *out, int out_on_device) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(view, TM_E_INVAL, "render view: null struct");
  int pages = 0;
  TM_TRY(tm_get_tile_page_count(e, &pages));
  TM_CHECK(first_page >= 0 && page_count >= 0 && (int64_t)first_page + page_count <= pages, TM_E_INVAL, "tile page range [%d,+%d) outside 0..%d",
           first_page, page_count, pages);
  // the palettes as made (none before PreparePalettes: the tiles' RGB pixels are shown); palette indices exist once Dither has run
  const bool pals = e->palettes_dev.p && !e->palettes_host.empty() && e->gpal_px.p && e->has_pal_px;
  const int npal = pals ? (int)std::min<int64_t>(e->s.PaletteCount, (int64_t)e->palettes_host.size() / std::max(1, e->s.PaletteSize)) : 0;
  TM_TRY(tm_probe_render_view_host(view, npal));
  if (page_count == 0) return TM_OK;
  RenderMap m{};
  m.pal_px = e->gpal_px.as<uint8_t>();
  m.ntiles = e->t;
  m.palettes = e->palettes_dev.as<int32_t>();
  m.npal = npal; m.pal_size = e->s.PaletteSize; m.tm_w = e->tm_w; m.tm_h = e->tm_h;
  TM_HIP(hipSetDevice(e->device));
  return deliver(e, page_count, out, out_on_device,
                 [&](void *dst) { return launch_tile_pages(view_map_of(e, m, *view), *view, first_page, page_count, dst, e->stream); });
}

int tm_stage_render_view(const tm_render_view *view, const void *tile_idx, const void *pal_idx, const void *item_flags, const void *px, const void *py,
                         int tm_w, int tm_h, int nframes, const void *pal_px, const void *rgb_px, const void *tile_flags, const void *pal_idx_initial,
                         int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_TRY(tm_probe_render_view_host(view, npal));
  TM_CHECK(view->page != TM_RENDER_PAGE_INPUT, TM_E_INVAL, "render view: the stage seam draws the Output and Tiles pages");
  const bool tiles_page = view->page == TM_RENDER_PAGE_TILES;
  TM_CHECK(out && tm_w > 0 && tm_h > 0 && nframes >= 0 && ntiles >= 0 && npal >= 0 && pal_size > 0 && (palettes || npal == 0) &&
               ((pal_px && rgb_px && tile_flags && pal_idx_initial) || ntiles == 0) && (tiles_page || (tile_idx && pal_idx && item_flags && px && py)),
           TM_E_INVAL, "render view: bad arguments");
  TM_CHECK(((uintptr_t)rgb_px & 15) == 0 && ((uintptr_t)pal_px & 3) == 0, TM_E_INVAL, "render view: rgb_px must be 16-byte aligned, pal_px 4-byte aligned");
  TM_CHECK(!tiles_page || nframes <= tile_pages_of(ntiles, tm_w, tm_h), TM_E_INVAL, "render view: %d tile pages asked for, the tiles fill %lld", nframes,
           (long long)tile_pages_of(ntiles, tm_w, tm_h));
  const RenderMap m{(const int32_t *)tile_idx, (const int32_t *)pal_idx, (const uint8_t *)item_flags, (const uint8_t *)item_flags, 4,
                    (const int8_t *)px, (const int8_t *)py, (const uint8_t *)pal_px, ntiles, (const int32_t *)palettes, npal, pal_size, tm_w, tm_h};
  const RenderViewMap v{m, (const uint32_t *)rgb_px, (const uint32_t *)tile_flags, nullptr, 0, (const int32_t *)pal_idx_initial, view->palette_index};
  return tiles_page ? launch_tile_pages(v, *view, 0, nframes, out, (hipStream_t)stream) : launch_view_output(v, *view, 0, nframes, out, (hipStream_t)stream);
}

}  // extern "C"
