// tm_render_api.hip -- the decoded and the source frames on the device as a caller asks for them: tm_render_frames, as YUV, at a caller's size,
// and tm_get_frame_quality.  What a render checks and reads of the encoder is here too (RenderSource and the chunk rule: tm_encoder.h); the
// kernels are tm_render.hip's, tm_yuv_out.hip's and tm_scale.hip's.  The exports draw the same frames (tm_export.hip).
#include <cmath>

#include "tm_encoder.h"

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

extern "C" {

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
  RenderSource src{input != 0};
  TM_TRY(src.prepare(e, first_frame, frame_count));
  if (frame_count == 0) return TM_OK;
  const size_t bytes = (size_t)frame_count * e->tm_w * 8 * e->tm_h * 8 * 4;
  DevBuf tmp;
  void *dst = out;
  if (!out_on_device) {
    TM_TRY(tmp.alloc(bytes));
    dst = tmp.p;
  }
  TM_TRY(src.draw(first_frame, frame_count, dst, e->stream));
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
  RenderSource src{input != 0};
  TM_TRY(src.prepare(e, first_frame, frame_count));
  const bool to_device = dst->memory == TM_MEM_DEVICE;
  if (to_device) TM_TRY(yuv_out_is_device(*dst, e->device));
  if (frame_count == 0) return TM_OK;
  // a chunk of frames is drawn as RGB32 and converted behind the render; host planes go through a packed chunk, one copy per plane
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  const size_t fbytes = (size_t)sw * sh * 4;
  const int chunk = render_chunk_frames(frame_count, fbytes);
  DevBuf rgb, packed;
  TM_TRY(rgb.alloc(fbytes * chunk));
  if (!to_device) TM_TRY(packed.alloc((size_t)plan.frame_bytes() * chunk));
  for (int f0 = 0; f0 < frame_count; f0 += chunk) {
    const int nf = std::min(chunk, frame_count - f0);
    TM_TRY(src.draw(first_frame + f0, nf, rgb.p, e->stream));
    TM_TRY(launch_rgb32_to_yuv(plan, rgb.p, sw, nf, to_device ? yuv_dst_of(*dst, f0) : yuv_dst_packed(plan, packed.as<uint8_t>(), chunk, 0), e->stream));
    if (!to_device) TM_TRY(yuv_copy_out(plan, packed.as<uint8_t>(), chunk, *dst, f0, nf, e->stream));
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

// ---- the same frames at a caller's size (tm_scale.hip): drawn natively a chunk at a time -- render_chunk_frames of
// the larger of the two sizes -- scaled behind the render on the encoder's stream, then delivered or converted
int tm_render_frames_scaled(tm_encoder *e, int first_frame, int frame_count, int input, int out_w, int out_h, int filter, void *out, int out_on_device) {
  TM_CHECK(e && (out || frame_count == 0), TM_E_INVAL, "null argument");
  TM_TRY(render_range_ok(e, first_frame, frame_count));
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  ScaleTables tables;
  TM_TRY(tables.prepare(sw, sh, out_w, out_h, filter));
  const bool gathered = e->grp && input && e->load_sharded;  // tm_render_frames asks every shard for its piece (and makes the checks there)
  RenderSource src{input != 0};
  if (!gathered) TM_TRY(src.prepare(e, first_frame, frame_count));
  if (frame_count == 0) return TM_OK;
  TM_HIP(hipSetDevice(e->device));
  const int64_t spx = (int64_t)sw * sh, opx = (int64_t)out_w * out_h;
  const int chunk = render_chunk_frames(frame_count, (size_t)std::max(spx, opx) * 4);
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
  RenderSource src{input != 0};
  TM_TRY(src.prepare(e, first_frame, frame_count));  // (shard 0 of a group, as tm_render_frames_yuv reads)
  TM_HIP(hipSetDevice(e->device));
  const bool to_device = dst->memory == TM_MEM_DEVICE;
  if (to_device) TM_TRY(yuv_out_is_device(*dst, e->device));
  if (frame_count == 0) return TM_OK;
  const int64_t spx = (int64_t)sw * sh, opx = (int64_t)ow * oh;
  const int chunk = render_chunk_frames(frame_count, (size_t)std::max(spx, opx) * 4);
  DevBuf native, scaled, packed;
  TM_TRY(native.alloc((size_t)spx * 4 * chunk));
  TM_TRY(scaled.alloc((size_t)opx * 4 * chunk));
  if (!to_device) TM_TRY(packed.alloc((size_t)plan.frame_bytes() * chunk));
  TM_TRY(tables.upload(e->stream));
  for (int f0 = 0; f0 < frame_count; f0 += chunk) {
    const int nf = std::min(chunk, frame_count - f0);
    TM_TRY(src.draw(first_frame + f0, nf, native.p, e->stream));
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
