// tm_gtm_api.hip -- the encoder's side of a .gtm: Save hands the encode to the writer (write_gtm, tm_gtm.hip), ReloadGTM takes what the reader
// (read_gtm, tm_gtm_reload.hip) found.  The writer, the reader and the player link without the encoder; what touches tm_encoder is here.
#include "tm_encoder.h"
#include "tm_gtm.h"

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

extern "C" {

int tm_save_gtm(tm_encoder *e, const char *path) {
  TM_CHECK(e && path, TM_E_INVAL, "null argument");
  return save_to(e, path);
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

}  // extern "C"
