// tm_gtm_walk.h -- the command grammar of a .gtm key frame's decoded stream (TGTMCommand, tilingencoder.pas:53-86; LoadStream, 4880-5175),
// stated once.  walk_gtm_keyframe reads 16-bit commands (data << 4 | cmd) with their operands up to the FrameEnd that closes the key frame,
// checks that every operand lies inside the stream, and hands each command to a sink.  What a command MEANS -- where an item lands, which
// tile an intra item becomes -- is the sink's: tm_reload_gtm's tables (tm_gtm_reload.hip) and the player's records (tm_player_parse.hip) are two sinks.
//
// A sink has (each returns TM_OK or an error, which ends the walk):
//   int settings(uint32_t kind, const uint8_t *text, size_t n)        ExtendedCommand; kind 0 is the settings text
//   int dimensions(int tm_w, int tm_h, uint32_t frame_ns, uint32_t tile_count)
//   int pal_size() const                                              colours a LoadPalette carries (the last TileSet's data field)
//   int tile_set(int pal_size, uint32_t first, uint32_t last, const uint8_t *px)   px: (last - first + 1) tiles of 64 index bytes
//   int load_palette(uint32_t index, const uint8_t *colours)          pal_size() little-endian 0xAABBGGRR words
//   int frame_end(bool keyframe_end)
//   int skip(uint32_t count)                                          count items predicted with offset (0, 0)
//   int predicted(int ox, int oy)
//   int drawn(uint32_t tile, uint32_t pal, uint32_t mirror)           ShortShort / LongShort / LongLong
//   int intra(uint32_t pal, uint32_t mirror, const uint8_t *px)       px: the 64 index bytes that travel with the item
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "tm_common.h"
#include "tm_gtm.h"

namespace tmx {

enum { gtPredShort = 0, gtPredLong = 1, gtShortShort = 2, gtLongShort = 3, gtLongLong = 4, gtIntra = 5, gtSkip = 6, gtFrameEnd = 11,
       gtLoadPalette = 12, gtTileSet = 13, gtSetDimensions = 14, gtExtended = 15 };  // TGTMCommand, 72-86

// The palette size a stream has before any TileSet names one.  LoadStream reads FPaletteSize colours per LoadPalette (4956); a TileSet sets
// it (4923), and until then it is the encoder's setting.  SaveStream writes no TileSet when no tile is used twice (5307: every item of such a
// stream is intra or predicted), so for a reader without that encoder the setting is the settings text's "PaletteSize=" line (3758).
// 0: the text has none, or none in 1 .. 256.
inline int settings_palette_size(const uint8_t *text, size_t n) {
  static const char key[] = "PaletteSize=";
  const size_t k = sizeof(key) - 1;
  for (size_t i = 0; i + k < n; i++) {
    if ((i > 0 && text[i - 1] != '\n') || memcmp(text + i, key, k) != 0) continue;
    int v = 0;
    for (size_t j = i + k; j < n && text[j] >= '0' && text[j] <= '9' && v <= 256; j++) v = v * 10 + (text[j] - '0');
    return v <= 256 ? v : 0;
  }
  return 0;
}
// what both sinks make of the settings text (ExtendedCommand 0): kept, and the palette size until a TileSet says it -- a stream of intra
// and predicted items has none
inline void take_settings_text(const uint8_t *text, size_t n, std::string *settings, int *pal_size) {
  settings->assign((const char *)text, n);
  if (*pal_size == 0) *pal_size = settings_palette_size(text, n);
}
// what both sinks make of a LoadPalette's n words 0xAABBGGRR: the alpha is stripped (4951)
inline void take_palette_words(const uint8_t *c, size_t n, int32_t *out) {
  for (size_t k = 0; k < n; k++) out[k] = (int32_t)(load_u32(c + 4 * k) & 0xffffffu);
}

template <class Sink>
int walk_gtm_keyframe(const uint8_t *kf, size_t n, const char *name, Sink &s, size_t *end = nullptr) {
  size_t p = 0;
  auto need = [&](size_t k) { return k <= n - p; };  // (p <= n always)
  auto u8 = [&]() { return (uint32_t)kf[p++]; };
  auto u16 = [&]() { const uint32_t v = load_u16(kf + p); p += 2; return v; };
  auto u32 = [&]() { const uint32_t v = load_u32(kf + p); p += 4; return v; };
  bool kf_end = false;
  while (!kf_end) {
    TM_CHECK(need(2), TM_E_IO, "%s: truncated command stream", name);
    const uint32_t w = u16(), cmd = w & 15, data = w >> 4;
    switch (cmd) {
      case gtExtended: {
        TM_CHECK(need(4), TM_E_IO, "truncated");
        const uint32_t k = u32();
        TM_CHECK(need(k), TM_E_IO, "truncated");
        TM_TRY(s.settings(data, kf + p, k));
        p += k;
        break;
      }
      case gtSetDimensions: {
        TM_CHECK(need(12), TM_E_IO, "truncated");
        const int tw = (int)u16(), th = (int)u16();
        const uint32_t ns = u32(), tc = u32();
        TM_CHECK(tw > 0 && th > 0 && ns > 0, TM_E_IO, "bad dimensions");
        TM_TRY(s.dimensions(tw, th, ns, tc));
        break;
      }
      case gtTileSet: {
        TM_CHECK(need(8), TM_E_IO, "truncated");
        const uint32_t a = u32(), b = u32();
        TM_CHECK(b >= a && need((size_t)(b - a + 1) * 64), TM_E_IO, "bad tile set");
        TM_TRY(s.tile_set((int)data, a, b, kf + p));
        p += (size_t)(b - a + 1) * 64;
        break;
      }
      case gtLoadPalette: {
        TM_CHECK(need(2 + (size_t)s.pal_size() * 4), TM_E_IO, "truncated");
        const uint32_t pi = u16();
        TM_TRY(s.load_palette(pi, kf + p));
        p += (size_t)s.pal_size() * 4;
        break;
      }
      case gtFrameEnd:
        kf_end = (data & 1) != 0;
        TM_TRY(s.frame_end(kf_end));
        break;
      case gtSkip:
        TM_TRY(s.skip(data + 1));
        break;
      case gtShortShort: case gtLongShort: case gtLongLong: {
        TM_CHECK(need(cmd == gtShortShort ? 2 : (cmd == gtLongShort ? 4 : 6)), TM_E_IO, "bad tile-map item");
        const uint32_t pal = cmd == gtLongLong ? u16() : (data >> 2) & 1023;
        const uint32_t tile = cmd == gtShortShort ? u16() : u32();
        TM_TRY(s.drawn(tile, pal, data & 3));
        break;
      }
      case gtPredShort:
        TM_TRY(s.predicted((int)(data & 31) - (int)(data & 32), (int)((data >> 6) & 31) - (int)((data >> 6) & 32)));
        break;
      case gtPredLong: {
        TM_CHECK(need(2), TM_E_IO, "bad tile-map item");
        const int ox = (int8_t)u8(), oy = (int8_t)u8();
        TM_TRY(s.predicted(ox, oy));
        break;
      }
      case gtIntra: {
        TM_CHECK(need(66), TM_E_IO, "bad intra tile");
        const uint32_t pal = u16();
        TM_TRY(s.intra(pal, data & 3, kf + p));
        p += 64;
        break;
      }
      default: set_error("%s: unknown command %u", name, cmd); return TM_E_IO;
    }
  }
  if (end) *end = p;
  return TM_OK;
}

}  // namespace tmx
