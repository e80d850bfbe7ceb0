// tm_encoder.hip -- coarse seam: the TTilingEncoder object behind tm_create/tm_run (include/tilemotion.h).
//
// Mirrors TTilingEncoder (tilingencoder.pas:308-568): settings with the reference's clamps (2919-3047) and INI keys
// (3745-3770), Run(step) walking esLoad..esSave (5529-5554), read-only Tiles/Frames/Palettes views.  Everything a
// step computes stays resident in HBM between steps; only small control data (correlations, digit plans, palette
// colours, counts) crosses to the host.  Every step of Run(esAll) is built (motion prediction, the extended-palette
// re-rank, OptimizePalettes, the .gtm writer and reader included); what stays outside the path is listed in DESIGN.md "Scope".
//
// This file: create / destroy, the settings and their INI text, the video and its frames, tm_run and the read-back views.  The steps are in
// tm_steps.hip, tm_reduce.hip and tm_reconstruct.hip, the multi-GPU side in tm_shard.hip, Save / ReloadGTM in tm_gtm_api.hip, the device render entry points in tm_render_api.hip, the exports in tm_export.hip.
#include <cmath>
#include <fstream>
#include <map>
#include <sstream>

#include "tm_encoder.h"

// ---- settings ------------------------------------------------------------------------------------------------
static int equal_quality_tile_count(double tc) {  // EqualQualityTileCount, utils.pas:1038-1041 (TFloat argument)
  const float f = (float)tc;
  return (int)llrint(std::sqrt((double)f) * std::log2(1 + (double)f));
}

static int clampi(int64_t v, int lo, int hi) { return (int)std::min<int64_t>(hi, std::max<int64_t>(lo, v)); }

void recompute_auto_tile_count(tm_encoder *e) {  // SetGlobalTilingQualityBasedTileCount, tilingencoder.pas:2937-2948
  const int64_t raw = (int64_t)e->nframes * e->tm_size();
  const int eqtc = equal_quality_tile_count((double)raw);
  e->s.GlobalTilingTileCount = (int)std::min<int64_t>(llrint(e->s.GlobalTilingQualityBasedTileCount * eqtc), raw);
}

static int set_number(tm_encoder *e, const std::string &k, double v, bool is_int_like) {
  Settings &s = e->s;
  (void)is_int_like;
  if (k == "StartFrame") s.StartFrame = std::max(0, (int)v);
  else if (k == "FrameCount") s.FrameCount = std::max(0, (int)v);
  else if (k == "Scaling") s.Scaling = std::max(0.01, v);
  else if (k == "MotionPredictRadius") s.MotionPredictRadius = clampi((int64_t)v, 0, 128);  // 3046 clamps to 1..128; 0 = motion prediction off (build extension: the reference code paths for <= 0 exist, 1972, 1496)
  else if (k == "GlobalTilingUseTargetPSNR") s.GlobalTilingUseTargetPSNR = v != 0;
  else if (k == "GlobalTilingTargetPSNR") s.GlobalTilingTargetPSNR = std::min(10 * std::log(255 * 255 / 0.5) / std::log(10.0), std::max(0.0, v));
  else if (k == "GlobalTilingQualityBasedTileCount") { s.GlobalTilingQualityBasedTileCount = v; e->auto_tile_count = true; if (e->nframes) recompute_auto_tile_count(e); }
  else if (k == "GlobalTilingTileCount") {  // SetGlobalTilingTileCount, 2974-2986: has priority over the quality-based value
    const int64_t raw = (int64_t)e->nframes * e->tm_size();
    s.GlobalTilingTileCount = raw ? clampi((int64_t)v, 0, (int)std::min<int64_t>(raw, INT32_MAX)) : std::max(0, (int)v);
    e->auto_tile_count = s.GlobalTilingTileCount <= 0;
  }
  else if (k == "PaletteSize") s.PaletteSize = clampi((int64_t)v, 2, 64);
  else if (k == "PaletteCount") s.PaletteCount = clampi((int64_t)v, 1, 65536);
  else if (k == "DitheringMode") s.DitheringMode = clampi((int64_t)v, 0, 4);
  else if (k == "DitheringUseThomasKnoll") s.DitheringUseThomasKnoll = v != 0;
  else if (k == "DitheringYliluoma2MixedColors") s.DitheringYliluoma2MixedColors = clampi((int64_t)v, 1, 16);
  else if (k == "FrameTilingExtendedPaletteUsage") s.FrameTilingExtendedPaletteUsage = v != 0;
  else if (k == "MaxThreadCount") s.MaxThreadCount = std::max(1, (int)v);
  else if (k == "ShotTransMaxSecondsPerKF") s.ShotTransMaxSecondsPerKF = std::max(0.0, v);
  else if (k == "ShotTransMinSecondsPerKF") s.ShotTransMinSecondsPerKF = std::max(0.0, v);
  else if (k == "ShotTransCorrelLoThres") s.ShotTransCorrelLoThres = std::min(1.0, std::max(-1.0, v));
  else { set_error("unknown setting '%s'", k.c_str()); return TM_E_INVAL; }
  return TM_OK;
}

static int get_number(tm_encoder *e, const std::string &k, double *v) {
  const Settings &s = e->s;
  if (k == "StartFrame") *v = s.StartFrame;
  else if (k == "FrameCount") *v = s.FrameCount;
  else if (k == "Scaling") *v = s.Scaling;
  else if (k == "MotionPredictRadius") *v = s.MotionPredictRadius;
  else if (k == "GlobalTilingUseTargetPSNR") *v = s.GlobalTilingUseTargetPSNR;
  else if (k == "GlobalTilingTargetPSNR") *v = s.GlobalTilingTargetPSNR;
  else if (k == "GlobalTilingQualityBasedTileCount") *v = s.GlobalTilingQualityBasedTileCount;
  else if (k == "GlobalTilingTileCount") *v = s.GlobalTilingTileCount;
  else if (k == "PaletteSize") *v = s.PaletteSize;
  else if (k == "PaletteCount") *v = s.PaletteCount;
  else if (k == "DitheringMode") *v = s.DitheringMode;
  else if (k == "DitheringUseThomasKnoll") *v = s.DitheringUseThomasKnoll;
  else if (k == "DitheringYliluoma2MixedColors") *v = s.DitheringYliluoma2MixedColors;
  else if (k == "FrameTilingExtendedPaletteUsage") *v = s.FrameTilingExtendedPaletteUsage;
  else if (k == "MaxThreadCount") *v = s.MaxThreadCount;
  else if (k == "ShotTransMaxSecondsPerKF") *v = s.ShotTransMaxSecondsPerKF;
  else if (k == "ShotTransMinSecondsPerKF") *v = s.ShotTransMinSecondsPerKF;
  else if (k == "ShotTransCorrelLoThres") *v = s.ShotTransCorrelLoThres;
  else { set_error("unknown setting '%s'", k.c_str()); return TM_E_INVAL; }
  return TM_OK;
}

std::string settings_text(const Settings &s) {  // GetSettings -> SaveSettings, tilingencoder.pas:2255, 3738-3775 (TMemIniFile layout)
  // Sections in the order of their first write, keys in write order inside a section (the ShotTrans* keys are written last but belong
  // to [Load]), a blank line after every section but the last, WriteBool as 0/1, WriteFloat in the shortest form -- and the line
  // ends of the Win64 build that is the reference (CR LF): the text of the reference's own demo streams, line for line, for every key
  // this snapshot still writes (tests/test_gtm.py::test_settings_text_matches_the_demo_streams_line_for_line).
  char buf[2048];
  auto flt = [](double v) { char b[64]; snprintf(b, sizeof(b), "%.15g", v); return std::string(b); };
  snprintf(buf, sizeof(buf),
           "[Load]\nInputFileName=%s\nOutputFileName=%s\nStartFrame=%d\nFrameCount=%d\nScaling=%s\nShotTransMaxSecondsPerKF=%s\n"
           "ShotTransMinSecondsPerKF=%s\nShotTransCorrelLoThres=%s\n\n[MotionPredict]\nMotionPredictRadius=%d\n\n"
           "[GlobalTiling]\nGlobalTilingUseTargetPSNR=%d\nGlobalTilingTargetPSNR=%s\nGlobalTilingQualityBasedTileCount=%s\n"
           "GlobalTilingTileCount=%d\n\n[Dither]\nPaletteSize=%d\nPaletteCount=%d\nDitheringMode=%d\nDitheringUseThomasKnoll=%d\n"
           "DitheringYliluoma2MixedColors=%d\n\n[FrameTiling]\nFrameTilingExtendedPaletteUsage=%d\n\n[Misc]\nMaxThreadCount=%d\n",
           s.InputFileName.c_str(), s.OutputFileName.c_str(), s.StartFrame, s.FrameCount, flt(s.Scaling).c_str(),
           flt(s.ShotTransMaxSecondsPerKF).c_str(), flt(s.ShotTransMinSecondsPerKF).c_str(), flt(s.ShotTransCorrelLoThres).c_str(),
           s.MotionPredictRadius, (int)s.GlobalTilingUseTargetPSNR, flt(s.GlobalTilingTargetPSNR).c_str(),
           flt(s.GlobalTilingQualityBasedTileCount).c_str(), s.GlobalTilingTileCount, s.PaletteSize, s.PaletteCount, s.DitheringMode,
           (int)s.DitheringUseThomasKnoll, s.DitheringYliluoma2MixedColors, (int)s.FrameTilingExtendedPaletteUsage, s.MaxThreadCount);
  std::string out;
  for (const char *c = buf; *c; c++) { if (*c == '\n') out += '\r'; out += *c; }
  return out;
}

extern "C" {

tm_encoder *tm_create(void) {
  if (require_device() != TM_OK) return nullptr;
  tm_encoder *e = new tm_encoder();
  if (hipGetDevice(&e->device) != hipSuccess) e->device = 0;
  return e;
}

void tm_destroy(tm_encoder *e) {
  if (e && e->grp) group_teardown(e);  // every shard frees its memory on its own thread
  delete e;
  pool_trim();  // the calling thread's cached device blocks go back to the driver with the encoder
}

int tm_set_device(tm_encoder *e, int device) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_set_device: the encoder is a device group (tm_set_devices)");
  TM_HIP(hipSetDevice(device));
  e->device = device;
  return TM_OK;
}

int tm_load_default_settings(tm_encoder *e) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (e->grp) return group_each(e, [](tm_encoder *s) { return tm_load_default_settings(s); });
  e->s = Settings();
  e->auto_tile_count = true;
  return TM_OK;
}

static int load_settings_from(tm_encoder *e, std::istream &in) {  // LoadSettings, tilingencoder.pas:3777-3815
  tm_load_default_settings(e);
  std::map<std::string, std::string> kv;
  std::string line;
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty() || line[0] == '[' || line[0] == ';') continue;  // key names are unique across sections
    const size_t eq = line.find('=');
    if (eq == std::string::npos) continue;
    kv[line.substr(0, eq)] = line.substr(eq + 1);
  }
  // GlobalTilingTileCount after GlobalTilingQualityBasedTileCount: it has priority (3796)
  static const char *order[] = {"StartFrame", "FrameCount", "Scaling", "MotionPredictRadius", "GlobalTilingUseTargetPSNR",
                                "GlobalTilingTargetPSNR", "GlobalTilingQualityBasedTileCount", "GlobalTilingTileCount", "PaletteSize",
                                "PaletteCount", "DitheringMode", "DitheringUseThomasKnoll", "DitheringYliluoma2MixedColors",
                                "FrameTilingExtendedPaletteUsage", "MaxThreadCount", "ShotTransMaxSecondsPerKF",
                                "ShotTransMinSecondsPerKF", "ShotTransCorrelLoThres"};
  for (const char *k : order) {
    auto it = kv.find(k);
    if (it == kv.end()) continue;
    std::string v = it->second;
    std::replace(v.begin(), v.end(), ',', '.');
    TM_TRY(set_number(e, k, atof(v.c_str()), false));
  }
  if (kv.count("InputFileName")) e->s.InputFileName = kv["InputFileName"];
  if (kv.count("OutputFileName")) e->s.OutputFileName = kv["OutputFileName"];
  return TM_OK;
}

int tm_load_settings_ini(tm_encoder *e, const char *path) {
  TM_CHECK(e && path, TM_E_INVAL, "null argument");
  if (e->grp) return group_each(e, [path](tm_encoder *s) { return tm_load_settings_ini(s, path); });
  std::ifstream in(path);
  TM_CHECK(in.good(), TM_E_IO, "cannot open %s", path);
  return load_settings_from(e, in);
}

int tm_save_settings_ini(tm_encoder *e, const char *path) {  // SaveSettings, tilingencoder.pas:3738-3775
  TM_CHECK(e && path, TM_E_INVAL, "null argument");
  std::ofstream out(path, std::ios::binary);
  TM_CHECK(out.good(), TM_E_IO, "cannot create %s", path);
  const std::string t = settings_text(e->s);
  out.write(t.data(), (std::streamsize)t.size());
  TM_CHECK(out.good(), TM_E_IO, "cannot write %s", path);
  return TM_OK;
}

// LoadSettings then SaveSettings on text, no device and no encoder needed: what an INI text becomes once the setters have clamped it
// (the embedded settings of a .gtm, tilingencoder.pas:5331-5335, are this text)
int tm_settings_text_host(const char *ini_text, char *out, int64_t cap, int64_t *out_len) {
  TM_CHECK(ini_text && out_len, TM_E_INVAL, "null argument");
  tm_encoder *e = new tm_encoder();  // host state only: nothing here touches a device
  std::istringstream in(ini_text);
  const int rc = load_settings_from(e, in);
  std::string t;
  if (rc == TM_OK) t = settings_text(e->s);
  delete e;
  TM_TRY(rc);
  *out_len = (int64_t)t.size();
  if (out && cap > 0) {
    const size_t n = std::min<size_t>(t.size(), (size_t)cap - 1);
    memcpy(out, t.data(), n);
    out[n] = 0;
  }
  return TM_OK;
}

// (a device group: every setter reaches every shard)
int tm_set_int(tm_encoder *e, const char *key, int64_t v) {
  TM_CHECK(e && key, TM_E_INVAL, "null argument");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return set_number(s, key, (double)v, true); });
  return set_number(e, key, (double)v, true);
}
int tm_set_float(tm_encoder *e, const char *key, double v) {
  TM_CHECK(e && key, TM_E_INVAL, "null argument");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return set_number(s, key, v, false); });
  return set_number(e, key, v, false);
}
int tm_set_bool(tm_encoder *e, const char *key, int v) {
  TM_CHECK(e && key, TM_E_INVAL, "null argument");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return set_number(s, key, v ? 1 : 0, true); });
  return set_number(e, key, v ? 1 : 0, true);
}
int tm_set_str(tm_encoder *e, const char *key, const char *v) {
  TM_CHECK(e && key && v, TM_E_INVAL, "null argument");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_str(s, key, v); });
  if (!strcmp(key, "InputFileName")) e->s.InputFileName = v;
  else if (!strcmp(key, "OutputFileName")) e->s.OutputFileName = v;
  else { set_error("unknown string setting '%s'", key); return TM_E_INVAL; }
  return TM_OK;
}
int tm_get_int(tm_encoder *e, const char *key, int64_t *v) {
  TM_CHECK(e && key && v, TM_E_INVAL, "null argument");
  double d;
  TM_TRY(get_number(e, key, &d));
  *v = (int64_t)llrint(d);
  return TM_OK;
}
int tm_get_float(tm_encoder *e, const char *key, double *v) { TM_CHECK(e && key && v, TM_E_INVAL, "null argument"); return get_number(e, key, v); }

int tm_set_progress_cb(tm_encoder *e, tm_progress_cb cb, void *user) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  e->cb = cb;
  e->cb_user = user;
  return TM_OK;
}

int tm_set_video(tm_encoder *e, int width, int height, double fps, int frame_count) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(width > 0 && height > 0 && frame_count > 0 && fps >= 0, TM_E_INVAL, "bad video geometry %dx%d x%d", width, height, frame_count);
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_video(s, width, height, fps, frame_count); });
  TM_HIP(hipSetDevice(e->device));
  e->frames_peer = nullptr;
  e->input = InputInfo();  // the frames come from memory again, the key frames from the automatic rule
  e->width = width; e->height = height; e->fps = fps; e->nframes = frame_count;
  e->tm_w = (width - 1) / 8 + 1;   // ReframeUI((DstWidth - 1) div cTileWidth + 1, ...), tilingencoder.pas:1776
  e->tm_h = (height - 1) / 8 + 1;
  e->frames = nullptr;
  e->frames_host = nullptr;
  e->frames_owned.release();
  if (e->copy_stream) TM_HIP(hipStreamSynchronize(e->copy_stream));  // a prefetch of the old geometry may still be running
  if (e->stream_aux) TM_HIP(hipStreamSynchronize(e->stream_aux));    // and so may the old clip's correlation
  e->load_tail_pending = false;
  for (tm_encoder::HostClip &c : e->hclip) { c.buf.release(); c.pending = false; c.host = nullptr; }
  e->hclip_cur = -1;
  e->steps_done = 0;
  e->src_tiles = false;
  if (e->auto_tile_count) recompute_auto_tile_count(e);
  return TM_OK;
}

int tm_push_frame_rgb32(tm_encoder *e, int index, const uint32_t *pixels, int stride_px) {
  TM_CHECK(e && pixels, TM_E_INVAL, "null argument");
  TM_CHECK(e->nframes > 0, TM_E_INVAL, "tm_set_video has not been called");
  TM_CHECK(index >= 0 && index < e->nframes && stride_px >= e->width, TM_E_INVAL, "bad frame index/stride");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_push_frame_rgb32(s, index, pixels, stride_px); });
  TM_HIP(hipSetDevice(e->device));
  const size_t fbytes = (size_t)e->width * e->height * 4;
  e->input = InputInfo();
  e->frames_host = nullptr;
  e->frames_peer = nullptr;
  e->hclip_cur = -1;
  if (!e->frames_owned.p || e->frames != e->frames_owned.p) {
    TM_TRY(e->frames_owned.alloc(fbytes * e->nframes));
    TM_HIP(hipMemsetAsync(e->frames_owned.p, 0, fbytes * e->nframes, e->stream));
    e->frames = e->frames_owned.p;
  }
  TM_HIP(hipMemcpy2DAsync(e->frames_owned.as<uint8_t>() + fbytes * index, (size_t)e->width * 4, pixels, (size_t)stride_px * 4,
                          (size_t)e->width * 4, e->height, hipMemcpyHostToDevice, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));  // caller's buffer is only valid during the call (extern.pas:883-892)
  return TM_OK;
}

int tm_set_frames_device(tm_encoder *e, const void *dev_frames) {
  TM_CHECK(e && dev_frames, TM_E_INVAL, "null argument");
  TM_CHECK(e->nframes > 0, TM_E_INVAL, "tm_set_video has not been called");
  if (e->grp) {  // the clip lives on the first listed device: shards there read it, shards elsewhere pull what their Load reads
    const int home = e->device;  // (the group's first device)
    return group_each(e, [=](tm_encoder *s) -> int {
      TM_TRY(tm_set_frames_device(s, dev_frames));
      if (s->device != home) { s->frames = nullptr; s->frames_peer = dev_frames; s->frames_peer_dev = home; }
      return (int)TM_OK;
    });
  }
  e->frames_owned.release();
  e->input = InputInfo();
  e->frames = dev_frames;
  e->frames_host = nullptr;
  e->frames_peer = nullptr;
  e->hclip_cur = -1;
  return TM_OK;
}

int tm_set_frames_host(tm_encoder *e, const uint32_t *host_frames) {
  TM_CHECK(e && host_frames, TM_E_INVAL, "null argument");
  TM_CHECK(e->nframes > 0, TM_E_INVAL, "tm_set_video has not been called");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_set_frames_host(s, host_frames); });  // every shard loads the whole clip
  e->frames_peer = nullptr;
  e->input = InputInfo();
  e->frames_host = host_frames;
  e->frames = nullptr;
  e->hclip_cur = -1;
  return TM_OK;
}

int tm_prefetch_frames_host(tm_encoder *e, const uint32_t *host_frames) {
  TM_CHECK(e && host_frames, TM_E_INVAL, "null argument");
  TM_CHECK(e->nframes > 0, TM_E_INVAL, "tm_set_video has not been called");
  if (e->grp) return group_each(e, [=](tm_encoder *s) { return tm_prefetch_frames_host(s, host_frames); });
  TM_HIP(hipSetDevice(e->device));
  // the buffer to fill: one that neither holds a clip waiting for its Load nor the clip the steps in flight may still read from --
  // unless both are taken, in which case the clip of the last Load gives way (its steps have returned: tm_run blocks)
  int slot = -1;
  for (int i = 0; i < 2; i++)
    if (!e->hclip[i].pending && i != e->hclip_cur) slot = i;
  if (slot < 0 && e->hclip_cur >= 0 && !e->hclip[e->hclip_cur].pending) {
    slot = e->hclip_cur;
    e->hclip_cur = -1;
    if (e->frames == e->hclip[slot].buf.p) e->frames = nullptr;  // a Load without new frames would read a clip being overwritten
  }
  TM_CHECK(slot >= 0, TM_E_INVAL, "tm_prefetch_frames_host: two clips are already waiting for their Load");
  TM_HIP(hipStreamSynchronize(e->stream));  // nothing queued on the encoder's stream still reads (or the pool just handed out) that buffer
  return queue_host_clip(e, slot, host_frames);
}

int tm_run(tm_encoder *e, int step) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  knobs_reload();  // the environment switches are sampled here, once per Run; the steps read the sampled set
  // Load takes nothing but the settings (1764-1820): with no video described yet it opens InputFileName itself
  if ((step == TM_STEP_LOAD || step == TM_STEP_ALL) && e->nframes == 0 && !e->s.InputFileName.empty()) TM_TRY(tm_open_input(e));
  if (e->grp) {  // every step on every shard at once; Save is shard 0's (every shard holds the merged state)
    if (step == TM_STEP_ALL) {
      for (int s = TM_STEP_LOAD; s <= TM_STEP_REINDEX; s++) TM_TRY(group_run_step(e, s));
      if (!e->s.OutputFileName.empty()) TM_TRY(run_step(e, TM_STEP_SAVE));
      return TM_OK;
    }
    if (step == TM_STEP_SAVE) return run_step(e, step);
    TM_CHECK(step >= TM_STEP_LOAD && step < TM_STEP_SAVE, TM_E_INVAL, "bad step %d", step);
    return group_run_step(e, step);
  }
  if (step == TM_STEP_ALL) {  // Run(esAll): every step in order (5535-5553); Save only once an output name is set
    for (int s = TM_STEP_LOAD; s <= TM_STEP_REINDEX; s++) TM_TRY(run_step(e, s));
    if (!e->s.OutputFileName.empty()) TM_TRY(run_step(e, TM_STEP_SAVE));
    return TM_OK;
  }
  return run_step(e, step);
}

int tm_get_counts(tm_encoder *e, int64_t *tiles, int *frames, int *palettes, int *tm_w, int *tm_h, int *keyframes) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (tiles) *tiles = e->t;
  if (frames) *frames = e->nframes;
  if (palettes) *palettes = e->palettes_host.empty() ? 0 : e->s.PaletteCount;
  if (tm_w) *tm_w = e->tm_w;
  if (tm_h) *tm_h = e->tm_h;
  if (keyframes) { TM_TRY(load_tail(e)); *keyframes = (int)e->kf_start.size(); }
  return TM_OK;
}

int tm_get_tiles(tm_encoder *e, int64_t first, int64_t count, tm_tile_hdr *hdrs, uint8_t *pal_px, uint32_t *rgb_px) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(first >= 0 && count >= 0 && first + count <= e->t, TM_E_INVAL, "tile range [%lld,+%lld) outside 0..%lld", (long long)first,
           (long long)count, (long long)e->t);
  if (count == 0) return TM_OK;
  TM_HIP(hipSetDevice(e->device));
  if (rgb_px) TM_HIP(hipMemcpy(rgb_px, e->gtiles.as<uint8_t>() + first * 256, (size_t)count * 256, hipMemcpyDeviceToHost));
  if (pal_px) {
    if (e->has_pal_px) TM_HIP(hipMemcpy(pal_px, e->gpal_px.as<uint8_t>() + first * 64, (size_t)count * 64, hipMemcpyDeviceToHost));
    else memset(pal_px, 0, (size_t)count * 64);
  }
  if (hdrs) {
    std::vector<uint32_t> use(count);
    std::vector<int32_t> pi(count, -1);
    std::vector<uint8_t> fl(count);
    TM_HIP(hipMemcpy(use.data(), e->guse.as<uint8_t>() + first * 4, (size_t)count * 4, hipMemcpyDeviceToHost));
    TM_HIP(hipMemcpy(fl.data(), e->gflags.as<uint8_t>() + first, (size_t)count, hipMemcpyDeviceToHost));
    if (e->gpal_idx.p && (e->steps_done & (1 << TM_STEP_PREPARE_PALETTES)))
      TM_HIP(hipMemcpy(pi.data(), e->gpal_idx.as<uint8_t>() + first * 4, (size_t)count * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; i++) {
      hdrs[i].UseCount = use[i];
      hdrs[i].TmpIndex = (int32_t)(first + i);
      hdrs[i].MergeIndex = -1;
      hdrs[i].PalIdx_Initial = pi[i];
      hdrs[i].Flags = 1u | 2u | 4u | ((fl[i] & 1) ? 8u : 0u) | ((fl[i] & 2) ? 16u : 0u);  // Active, HasRGB, HasPal, H/V mirror
    }
  }
  return TM_OK;
}

int tm_get_tile(tm_encoder *e, int64_t i, tm_tile_hdr *hdr, uint8_t pal_px[64], uint32_t rgb_px[64]) {
  return tm_get_tiles(e, i, 1, hdr, pal_px, rgb_px);
}

// The tile maps as the reference's consumers read them (Frames[i].TileMap, tilingencoder.pas:178-184, 509-512): the packed 18-byte items are
// put together on the device -- TMI^.PSNR := EuclideanToPSNR(knnErr | mpErr) (1619 / 1644; after PredictMotion alone: of its best error, 1250)
// in double precision there, compared with a tolerance like every PSNR -- and cross PCIe in ONE copy.
__global__ __launch_bounds__(256) void k_pack_tilemap(const int32_t *__restrict__ ti, const int32_t *__restrict__ pi, const uint32_t *__restrict__ er,
                                                      const int8_t *__restrict__ px, const int8_t *__restrict__ py, const uint8_t *__restrict__ pr,
                                                      const uint8_t *__restrict__ ff, int with_psnr, int64_t n, uint32_t *__restrict__ out) {
  __shared__ uint32_t s_items[256 * 18 / 4 + 2];
  const int64_t base = (int64_t)blockIdx.x * 256, i = base + threadIdx.x;
  if (i < n) {
    uint8_t *o = reinterpret_cast<uint8_t *>(s_items) + threadIdx.x * 18;
    const int32_t t = ti[i], p = pi[i];
    float ps = 0.0f;
    if (with_psnr) {  // EuclideanToPSNR, utils.pas:1074-1078
      const float r = (float)((double)er[i] * (1.0 / 192));
      const float m = r > 0.5f ? r : 0.5f;
      ps = (float)(10 * log10(255 * 255 / (double)m));
    }
    const uint8_t f = ff[i];
    const uint32_t fl = (f & 1 ? 1u : 0u) | (f & 2 ? 2u : 0u) | ((pr && pr[i]) ? 4u : 0u);
    memcpy(o, &t, 4); memcpy(o + 4, &p, 4);
    o[8] = (uint8_t)(px ? px[i] : 0); o[9] = (uint8_t)(py ? py[i] : 0);
    memcpy(o + 10, &ps, 4); memcpy(o + 14, &fl, 4);
  }
  __syncthreads();
  const int64_t cnt = min((int64_t)256, n - base);
  const int words = (int)((cnt * 18 + 3) / 4);  // 256 items = 1152 whole words; the last workgroup's tail word is padded inside the staging buffer
  uint32_t *dst = out + base * 18 / 4;          // base * 18 is a multiple of 4
  for (int w = threadIdx.x; w < words; w += 256) dst[w] = s_items[w];
}

int tm_get_tilemaps(tm_encoder *e, int first_frame, int frame_count, tm_tilemap_item *items) {
  TM_CHECK(e && items, TM_E_INVAL, "null argument");
  TM_CHECK((e->steps_done & 1) && first_frame >= 0 && frame_count >= 0 && first_frame + frame_count <= e->nframes, TM_E_INVAL,
           "frame range [%d,+%d) outside 0..%d (or no Load yet)", first_frame, frame_count, e->nframes);
  if (frame_count == 0) return TM_OK;
  TM_HIP(hipSetDevice(e->device));
  const int64_t per = e->tm_size(), off = (int64_t)first_frame * per, n = per * frame_count;
  DevBuf pack;
  TM_TRY(pack.alloc((size_t)n * 18 + 8));
  const bool pm = e->has_pm;
  const uint32_t *er = (pm && !e->reconstructed) ? e->pm_err.as<uint32_t>() : e->tm_err.as<uint32_t>();
  hipLaunchKernelGGL(k_pack_tilemap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>() + off, e->tm_pal.as<int32_t>() + off,
                     er + off, pm ? e->tm_px.as<int8_t>() + off : nullptr, pm ? e->tm_py.as<int8_t>() + off : nullptr,
                     pm ? e->tm_pred.as<uint8_t>() + off : nullptr, e->fflags.as<uint8_t>() + off, (e->reconstructed || pm) ? 1 : 0, n, pack.as<uint32_t>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipMemcpyAsync(items, pack.p, (size_t)n * 18, hipMemcpyDeviceToHost, e->stream));  // page-locked destination: one DMA at PCIe rate
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

int tm_get_tilemap(tm_encoder *e, int frame, tm_tilemap_item *items) { return tm_get_tilemaps(e, frame, 1, items); }

int tm_get_palette(tm_encoder *e, int i, int32_t *rgb) {
  TM_CHECK(e && rgb, TM_E_INVAL, "null argument");
  TM_CHECK(!e->palettes_host.empty() && i >= 0 && i < e->s.PaletteCount, TM_E_INVAL, "bad palette %d", i);
  memcpy(rgb, &e->palettes_host[(size_t)i * e->s.PaletteSize], (size_t)e->s.PaletteSize * 4);
  return TM_OK;
}

int tm_get_keyframes(tm_encoder *e, int32_t *start_frames) {
  TM_CHECK(e && start_frames, TM_E_INVAL, "null argument");
  TM_TRY(load_tail(e));
  memcpy(start_frames, e->kf_start.data(), e->kf_start.size() * 4);
  return TM_OK;
}

int tm_get_frame_correlations(tm_encoder *e, float *correl) {
  TM_CHECK(e && correl, TM_E_INVAL, "null argument");
  TM_TRY(load_tail(e));
  memcpy(correl, e->correl.data(), e->correl.size() * 4);
  return TM_OK;
}

int tm_get_psnr(tm_encoder *e, double *per_keyframe, double *global_mean) {  // TKeyFrame.LogPSNR, tilingencoder.pas:1006-1028
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_TRY(load_tail(e));
  TM_CHECK(e->reconstructed && e->tm_err.p && !e->kf_start.empty(), TM_E_INVAL, "PSNR: Reconstruct has not been run");
  TM_HIP(hipSetDevice(e->device));
  // ReconstructPSNRCml = sum of the items' PSNR (Single, 1619 / 1644) in a Double (1657); the reference adds in thread order, here
  // in item order.  Per key frame: / (TileMapSize x FrameCount) (1014); all: / (TileMapSize x frames) (1024).
  std::vector<uint32_t> er((size_t)e->q);
  TM_HIP(hipMemcpy(er.data(), e->tm_err.p, (size_t)e->q * 4, hipMemcpyDeviceToHost));
  const int64_t per = e->tm_size();
  double all = 0;
  for (size_t k = 0; k < e->kf_start.size(); k++) {
    const int64_t f0 = e->kf_start[k], f1 = k + 1 < e->kf_start.size() ? e->kf_start[k + 1] : e->nframes;
    double cml = 0;
    for (int64_t i = f0 * per; i < f1 * per; i++) cml += (double)euclidean_to_psnr(er[(size_t)i]);
    if (per_keyframe) per_keyframe[k] = f1 > f0 ? cml / (double)(per * (f1 - f0)) : 0.0;
    all += cml;
  }
  if (global_mean) *global_mean = all / (double)(per * e->nframes);
  return TM_OK;
}

int tm_get_stage_ms(tm_encoder *e, double ms[8]) {
  TM_CHECK(e && ms, TM_E_INVAL, "null argument");
  memcpy(ms, e->stage_ms, sizeof(e->stage_ms));
  return TM_OK;
}

int tm_get_save_stats(tm_encoder *e, tm_save_stats *out) {
  TM_CHECK(e && out, TM_E_INVAL, "null argument");
  TM_CHECK(e->has_save_stats, TM_E_INVAL, "save stats: this encoder has not saved a stream");
  *out = e->save_stats;
  return TM_OK;
}

void *tm_get_stream(tm_encoder *e) { return e ? (void *)e->stream : nullptr; }

int tm_get_device_array(tm_encoder *e, int which, void **ptr, int64_t *count) {
  TM_CHECK(e && ptr && count, TM_E_INVAL, "null argument");
  switch (which) {
    case TM_ARRAY_TILEMAP_TILE: *ptr = e->tm_tile.p; *count = e->q; break;
    case TM_ARRAY_TILEMAP_ERR: *ptr = e->tm_err.p; *count = e->q; break;
    case TM_ARRAY_TILEMAP_PAL: *ptr = e->tm_pal.p; *count = e->q; break;
    case TM_ARRAY_TILEMAP_PRED: *ptr = e->has_pm ? e->tm_pred.p : nullptr; *count = e->has_pm ? e->q : 0; break;
    case TM_ARRAY_TILEMAP_PX: *ptr = e->has_pm ? e->tm_px.p : nullptr; *count = e->has_pm ? e->q : 0; break;
    case TM_ARRAY_TILEMAP_PY: *ptr = e->has_pm ? e->tm_py.p : nullptr; *count = e->has_pm ? e->q : 0; break;
    case TM_ARRAY_PM_ERR: *ptr = e->has_pm ? e->pm_err.p : nullptr; *count = e->has_pm ? e->q : 0; break;
    case TM_ARRAY_TILE_PALPX: *ptr = e->has_pal_px ? e->gpal_px.p : nullptr; *count = e->has_pal_px ? e->t * 64 : 0; break;
    default: set_error("bad array id %d", which); return TM_E_INVAL;
  }
  return TM_OK;
}

int64_t tm_get_knn_queries(tm_encoder *e) { return e ? e->knn_queries : 0; }
int64_t tm_get_dither_pairs(tm_encoder *e) { return e ? e->dither_pairs : 0; }

int tm_get_kmeans_iters(tm_encoder *e, int *tile_iters, int64_t *tile_points, int *pixel_iters, int64_t *pixel_colours, int64_t *pixels, int64_t *pixel_colour_iters) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (tile_iters) *tile_iters = e->km_stats.tile_iters;
  if (tile_points) *tile_points = e->km_stats.tile_points;
  if (pixel_iters) *pixel_iters = e->km_stats.pixel_iters;
  if (pixel_colours) *pixel_colours = e->km_stats.pixel_colours;
  if (pixels) *pixels = e->km_stats.pixels;
  if (pixel_colour_iters) *pixel_colour_iters = e->km_stats.pixel_colour_iters;
  return TM_OK;
}

int tm_get_knn_kernel_split(tm_encoder *e, double ms[3], int64_t pairs[3]) {
  TM_CHECK(e && ms && pairs, TM_E_INVAL, "null argument");
  for (int i = 0; i < 3; i++) ms[i] = e->knn_split_ms[i];
  pairs[0] = e->knn_split_pairs[0]; pairs[1] = e->knn_split_pairs[1]; pairs[2] = e->knn_split_pairs[2];
  return TM_OK;
}

int tm_get_knn_stats(tm_encoder *e, double *kernel_ms, int64_t *pairs, int *launches, int *k_bytes, int64_t *db_rows) {
  if (e && db_rows) *db_rows = e->knn_db_rows;
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (kernel_ms) *kernel_ms = e->knn_ms;
  if (pairs) *pairs = e->knn_pairs;
  if (launches) *launches = e->knn_launches;
  if (k_bytes) *k_bytes = e->knn_kbytes;
  return TM_OK;
}

}  // extern "C"
