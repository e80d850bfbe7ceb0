// tm_gtm.hip -- (f)#2: the .gtm bitstream writer, host code only.
//
// Restates TTilingEncoder.SaveStream (tilingencoder.pas:5177-5482): the header and one entry per key frame (the container: tm_gtm.h), then
// per key frame one LZMA stream (lz_compress, tm_lzma.hip) of 16-bit commands (data << 4 | cmd; 53-86, 5200-5206; the grammar: tm_gtm_walk.h):
// ExtendedCommand(settings) + SetDimensions + TileSet(tiles with UseCount > 1) + LoadPalette x P in the first
// keyframe, then per frame tile-map items / SkipBlocks (5392-5437) and FrameEnd.
//
// The command bytes of every key frame are built first, on the calling thread; the key frames' streams are independent, so they are then
// coded side by side (lz_compress_jobs, tm_lz_matches.hip) and laid into the file in key-frame order.  Two switches, read at each Save:
// TM_HOST_THREADS (parser threads, at most one per key frame and at most 16) and TM_SAVE_FINDER (host | device: where the match lists
// are made; device only where the caller has one).  The file does not depend on either.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "tm_gtm_walk.h"
#include "tm_lz_matches.h"

namespace tmx {
namespace {

struct Stream {
  std::vector<uint8_t> b;
  uint8_t *grow(size_t n) { b.resize(b.size() + n); return &b[b.size() - n]; }
  void u8(uint32_t v) { b.push_back((uint8_t)v); }
  void u16(uint32_t v) { store_u16(grow(2), v); }
  void u32(uint32_t v) { store_u32(grow(4), v); }
  void cmd(int c, uint32_t data) { u16((data << 4) | (uint32_t)c); }  // DoCmd, 5200-5206
};

// What Save's measurement on the MI355X decided: the finder an encoder with a device uses when TM_SAVE_FINDER is not set.
constexpr bool kDeviceFinderByDefault = true;

int save_threads() {  // TM_HOST_THREADS, or the machine's threads, at most 16
  const char *env = getenv("TM_HOST_THREADS");
  const int n = env ? atoi(env) : (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(16, n));
}
bool save_device_finder(bool has_device) {  // TM_SAVE_FINDER
  if (!has_device) return false;
  const char *env = getenv("TM_SAVE_FINDER");
  if (env && !strcmp(env, "host")) return false;
  if (env && !strcmp(env, "device")) return true;
  return kDeviceFinderByDefault;
}
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

int write_gtm(const char *path, const GtmInput &in) {
  TM_CHECK(path && in.tm_w > 0 && in.tm_h > 0 && in.nframes > 0 && in.fps > 0 && !in.kf_start.empty(), TM_E_INVAL, "write_gtm: bad input");
  const auto t_start = std::chrono::steady_clock::now();
  const int tm_size = in.tm_w * in.tm_h, nkf = (int)in.kf_start.size();
  const int64_t ntiles = (int64_t)in.use.size();
  std::vector<uint8_t> file(GTM_HEADER_BYTES + GTM_KF_BYTES * (size_t)nkf, 0);  // (filled in at the end: the sizes are known then)
  GtmHeader head{GTM_HEADER_RIFF, (uint32_t)file.size(), 4 /* EncoderVersion (5351) */, (uint32_t)in.tm_w * 8, (uint32_t)in.tm_h * 8, (uint32_t)nkf, (uint32_t)in.nframes, 0, 0};
  std::vector<GtmKfEntry> entries((size_t)nkf);
  for (int k = 0; k < nkf; k++)
    entries[(size_t)k] = GtmKfEntry{GTM_KF_RIFF, (uint32_t)k, (uint32_t)in.kf_start[k], 0, 0, (uint32_t)llrint(1000.0 * in.kf_start[k] / in.fps)};
  Stream z;
  // WriteSettings (5331-5335): ExtendedCommand 0 + WriteAnsiString(settings)
  z.cmd(gtExtended, 0);
  z.u32((uint32_t)in.settings.size());
  z.b.insert(z.b.end(), in.settings.begin(), in.settings.end());
  // WriteDimensions (5318-5329)
  z.cmd(gtSetDimensions, 0);
  z.u16((uint32_t)in.tm_w);
  z.u16((uint32_t)in.tm_h);
  z.u32(gtm_frame_ns(in.fps));
  z.u32((uint32_t)ntiles);
  // WriteTiles (5292-5316): tiles before the first UseCount = 1 (sorted by use, most used first) go into one TileSet
  // (5296 starts the count at 0, so a table WITHOUT a UseCount = 1 tile got no TileSet at all while all its items name one: a stream nobody
  // can draw.  Such a table goes into the TileSet whole.)
  int64_t reused = ntiles;
  for (int64_t t = 0; t < ntiles; t++)
    if (in.use[t] == 1) { reused = t; break; }
  if (reused > 0) {
    z.cmd(gtTileSet, (uint32_t)in.pal_size);
    z.u32(0);
    z.u32((uint32_t)(reused - 1));
    z.b.insert(z.b.end(), in.pal_px, in.pal_px + reused * 64);
  }
  // WritePalettes (5270-5290)
  for (int p = 0; p < in.pal_count; p++) {
    z.cmd(gtLoadPalette, 0);
    z.u16((uint32_t)p);
    for (int c = 0; c < in.pal_size; c++) {
      uint32_t col = (uint32_t)in.palettes[(size_t)p * in.pal_size + c];
      if ((int32_t)col == TM_NULL_COLOR) col = 0xffffff;
      z.u32(col | 0xff000000u);
    }
  }
  std::vector<std::vector<uint8_t>> raw((size_t)nkf);  // the key frames' command bytes
  for (int k = 0; k < nkf; k++) {
    const int f0 = in.kf_start[k], f1 = (k + 1 < nkf ? in.kf_start[k + 1] : in.nframes) - 1;
    for (int f = f0; f <= f1; f++) {
      const tm_tilemap_item *tm = in.tilemap + (size_t)f * tm_size;
      int cs = 0, skip = 0;
      for (int yx = 0; yx < tm_size; yx++) {
        if (skip > 0) { skip--; continue; }
        int run = 0;  // smoothed = predicted with a zero offset (GetIsSmoothed, 621-624)
        for (int s = yx; s < tm_size; s++) {
          const tm_tilemap_item &it = tm[s];
          if (!((it.Flags & 4) && it.PredictedX == 0 && it.PredictedY == 0)) break;
          run++;
        }
        run = std::min(4096, run);
        if (run >= 4) {  // CMinBlkSkipCount
          z.cmd(gtSkip, (uint32_t)(run - 1));
          cs += run;
          skip = run - 1;
          continue;
        }
        const tm_tilemap_item &it = tm[yx];  // DoTMI, 5208-5268
        if (it.Flags & 4) {
          if (it.PredictedX < -32 || it.PredictedX > 31 || it.PredictedY < -32 || it.PredictedY > 31) {
            z.cmd(gtPredLong, 0);
            z.u8((uint8_t)it.PredictedX);
            z.u8((uint8_t)it.PredictedY);
          } else {
            z.cmd(gtPredShort, ((uint8_t)it.PredictedX & 63u) | (((uint8_t)it.PredictedY & 63u) << 6));
          }
        } else {
          const int32_t tile_idx = it.TileIdx, pal_idx = it.PalIdx;  // (copies: the item is packed, std::max takes references)
          const uint32_t tile = (uint32_t)std::max(0, tile_idx), pal = (uint32_t)std::max(0, pal_idx) & 0xffff;
          const bool intra = (int64_t)tile < ntiles && in.use[tile] <= 1;
          const uint32_t attrs = ((it.Flags & 2) ? 2u : 0u) | ((it.Flags & 1) ? 1u : 0u);
          if (intra) {
            z.cmd(gtIntra, attrs);
            z.u16(pal);
            z.b.insert(z.b.end(), in.pal_px + (size_t)tile * 64, in.pal_px + (size_t)tile * 64 + 64);
          } else if (tile <= 0xffff && pal < 1024) {
            z.cmd(gtShortShort, attrs | (pal << 2));
            z.u16(tile);
          } else if (pal < 1024) {
            z.cmd(gtLongShort, attrs | (pal << 2));
            z.u32(tile);
          } else {
            z.cmd(gtLongLong, attrs);
            z.u16(pal);
            z.u32(tile);
          }
        }
        cs++;
      }
      TM_CHECK(cs == tm_size && skip == 0, TM_E_INVAL, "write_gtm: incomplete tile map (frame %d)", f);
      const bool is_kf_end = f == f1;
      z.cmd(gtFrameEnd, is_kf_end ? 1 : 0);
      if (is_kf_end) { raw[(size_t)k].swap(z.b); z.b.clear(); }
    }
  }
  const double ms_commands = ms_since(t_start);
  std::vector<LzJob> jobs((size_t)nkf);
  for (int k = 0; k < nkf; k++) { jobs[(size_t)k].src = raw[(size_t)k].data(); jobs[(size_t)k].n = raw[(size_t)k].size(); }
  const bool device_finder = save_device_finder(in.has_device);
  LzJobsReport report;
  TM_TRY(lz_compress_jobs(jobs, save_threads(), device_finder, in.stream, &report));
  double avg_bytes = 0;
  uint32_t kf_max = 0;
  int last_kf = 0;
  int64_t raw_sum = 0, comp_sum = 0;
  for (int k = 0; k < nkf; k++) {
    const int f1 = (k + 1 < nkf ? in.kf_start[k + 1] : in.nframes) - 1;
    const int kf_count = f1 - last_kf + 1;
    last_kf = f1 + 1;
    const std::vector<uint8_t> &lz = jobs[(size_t)k].out;
    file.insert(file.end(), lz.begin(), lz.end());
    const uint32_t kf_size = (uint32_t)lz.size();
    entries[(size_t)k].raw_size = (uint32_t)raw[(size_t)k].size();
    entries[(size_t)k].comp_size = kf_size;
    if (k > 0 || nkf == 1) kf_max = std::max(kf_max, (uint32_t)llrint(kf_size * in.fps / kf_count));
    avg_bytes += kf_size;
    raw_sum += (int64_t)raw[(size_t)k].size();
    comp_sum += kf_size;
  }
  head.avg_bytes_per_s = (uint32_t)llrint(avg_bytes * in.fps / in.nframes);
  head.kf_max_bytes_per_s = kf_max;
  encode_gtm_header(head, &file[0]);
  for (int k = 0; k < nkf; k++) encode_gtm_kf_entry(entries[(size_t)k], &file[GTM_HEADER_BYTES + GTM_KF_BYTES * (size_t)k]);
  FILE *fp = fopen(path, "wb");
  TM_CHECK(fp != nullptr, TM_E_IO, "cannot create %s", path);
  const size_t w = fwrite(file.data(), 1, file.size(), fp);
  fclose(fp);
  TM_CHECK(w == file.size(), TM_E_IO, "short write to %s", path);
  if (in.stats)
    *in.stats = tm_save_stats{raw_sum, comp_sum, nkf, report.threads, device_finder ? TM_SAVE_FINDER_DEVICE : TM_SAVE_FINDER_HOST, 0, ms_commands, report.finder_ms,
                              report.parse_ms, ms_since(t_start)};
  return TM_OK;
}

}  // namespace tmx

extern "C" int tm_write_gtm_host(const char *path, int tm_w, int tm_h, int nframes, double fps, const int32_t *kf_start, int nkf,
                                 const uint8_t *pal_px, const uint32_t *use, int64_t ntiles, const int32_t *palettes, int pal_count,
                                 int pal_size, const tm_tilemap_item *tilemap, const char *settings) {
  if (!path || !kf_start || (!pal_px && ntiles) || !palettes || !tilemap) { tmx::set_error("tm_write_gtm_host: null argument"); return TM_E_INVAL; }
  tmx::GtmInput in;
  in.tm_w = tm_w; in.tm_h = tm_h; in.nframes = nframes; in.fps = fps;
  in.kf_start.assign(kf_start, kf_start + nkf);
  in.pal_px = pal_px;
  in.use.assign(use, use + ntiles);
  in.palettes = palettes; in.pal_count = pal_count; in.pal_size = pal_size;
  in.tilemap = tilemap;
  in.settings = settings ? settings : "";
  return tmx::write_gtm(path, in);
}
