// tm_gtm_reload.hip -- tm_reload_gtm's reader, host code only.
//
// LoadStream (tilingencoder.pas:4880-5175): the command streams of all key frames back into tables.  The grammar is walk_gtm_keyframe's
// (tm_gtm_walk.h); this sink is what LoadStream makes of the commands: frames open at their first item, an intra item becomes the next tile
// after the tile sets, SetTMI counts the uses.  It is the lenient reader: a header is taken on its magic and length alone, a stream without
// one is read to its end, tile sets and palettes may come in any key frame (the strict checks are the player's, tm_player_parse.hip).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "tm_gtm_walk.h"

namespace tmx {
namespace {
struct ReloadSink {
  GtmLoaded *out;
  int frm = -1, tm_pos = 0, last_tile = -1, loaded = 0;
  bool frame_open = false;

  int per() const { return out->tm_w * out->tm_h; }
  tm_tilemap_item *item() {  // "next frame if needed" (5091-5093 ...)
    if (!frame_open) { frm++; out->tilemap.resize((size_t)(frm + 1) * per()); frame_open = true; }
    tm_tilemap_item *it = &out->tilemap[(size_t)frm * per() + tm_pos];
    memset(it, 0, sizeof(*it));
    it->TileIdx = -1; it->PalIdx = -1;
    return it;
  }
  bool room() const { return out->tm_w > 0 && tm_pos < per(); }

  int settings(uint32_t kind, const uint8_t *text, size_t n) {
    if (kind != 0) return TM_OK;
    take_settings_text(text, n, &out->settings, &out->pal_size);
    return TM_OK;
  }
  int dimensions(int tm_w, int tm_h, uint32_t ns, uint32_t tc) {
    out->tm_w = tm_w; out->tm_h = tm_h;
    out->fps = gtm_fps(ns);
    out->pal_px.assign((size_t)tc * 64, 0);
    out->use.assign(tc, 0);
    return TM_OK;
  }
  int pal_size() const { return out->pal_size; }
  int tile_set(int pal_size, uint32_t a, uint32_t b, const uint8_t *px) {
    TM_CHECK((size_t)b < out->use.size(), TM_E_IO, "bad tile set");
    memcpy(&out->pal_px[(size_t)a * 64], px, (size_t)(b - a + 1) * 64);
    last_tile = std::max(last_tile, (int)b);
    out->pal_size = pal_size;
    return TM_OK;
  }
  int load_palette(uint32_t pi, const uint8_t *c) {
    if (out->palettes.size() < (size_t)(pi + 1) * out->pal_size) out->palettes.resize((size_t)(pi + 1) * out->pal_size, 0);
    take_palette_words(c, (size_t)out->pal_size, out->palettes.data() + (size_t)pi * out->pal_size);
    return TM_OK;
  }
  int frame_end(bool) {
    TM_CHECK(tm_pos == per(), TM_E_IO, "incomplete tile map");
    tm_pos = 0;
    frame_open = false;
    loaded++;
    return TM_OK;
  }
  int skip(uint32_t count) {
    for (uint32_t k = 0; k < count; k++) {
      TM_CHECK(room(), TM_E_IO, "skip past the tile map");
      item()->Flags = 4;
      tm_pos++;
    }
    return TM_OK;
  }
  int drawn(uint32_t tile, uint32_t pal, uint32_t mirror) {
    TM_CHECK(room(), TM_E_IO, "bad tile-map item");
    tm_tilemap_item *it = item();
    it->TileIdx = (int32_t)tile; it->PalIdx = (int32_t)pal; it->Flags = mirror;
    if ((size_t)tile < out->use.size()) out->use[tile]++;
    tm_pos++;
    return TM_OK;
  }
  int predicted(int ox, int oy) {
    TM_CHECK(room(), TM_E_IO, "bad tile-map item");
    tm_tilemap_item *it = item();
    it->PredictedX = (int8_t)ox; it->PredictedY = (int8_t)oy;
    it->Flags = 4;
    tm_pos++;
    return TM_OK;
  }
  int intra(uint32_t pal, uint32_t mirror, const uint8_t *px) {
    TM_CHECK(room(), TM_E_IO, "bad intra tile");
    last_tile++;
    TM_CHECK((size_t)last_tile < out->use.size(), TM_E_IO, "more intra tiles than the tile count allows");
    memcpy(&out->pal_px[(size_t)last_tile * 64], px, 64);
    tm_tilemap_item *it = item();
    it->TileIdx = last_tile; it->PalIdx = (int32_t)pal; it->Flags = mirror;
    out->use[(size_t)last_tile]++;
    tm_pos++;
    return TM_OK;
  }
};
}  // namespace

int read_gtm(const char *path, GtmLoaded *out) {
  FILE *fp = fopen(path, "rb");
  TM_CHECK(fp != nullptr, TM_E_IO, "cannot open %s", path);
  std::vector<uint8_t> file;
  {
    uint8_t buf[1 << 16];
    size_t r;
    while ((r = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + r);
    fclose(fp);
  }
  size_t pos = 0;
  out->header_frames = -1;
  if (file.size() >= GTM_HEADER_BYTES && gtm_has_magic(file.data(), GTM_HEADER_MAGIC)) {  // 5015-5033
    const GtmHeader h = decode_gtm_header(file.data());
    out->header_w = (int)h.width; out->header_h = (int)h.height; out->header_frames = (int)h.frame_count;
    pos = h.whole_header_size;
  }
  ReloadSink sink{out};
  std::vector<uint8_t> kf;
  while (pos < file.size()) {
    size_t used = 0;
    TM_TRY(lz_decompress(file.data() + pos, file.size() - pos, kf, &used));
    pos += used;
    out->kf_start.push_back(sink.loaded);
    TM_TRY(walk_gtm_keyframe(kf.data(), kf.size(), path, sink));
  }
  out->nframes = sink.loaded;
  out->pal_count = out->pal_size > 0 ? (int)(out->palettes.size() / out->pal_size) : 0;
  TM_CHECK(out->tilemap.size() == (size_t)sink.loaded * out->tm_w * out->tm_h, TM_E_IO, "%s: frame count mismatch", path);
  return TM_OK;
}
}  // namespace tmx
