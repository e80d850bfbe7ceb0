// tm_gtm.h -- what the .gtm files share (tm_gtm.hip the writer, tm_gtm_reload.hip, tm_lzma.hip, tm_player_parse.hip; tm_gtm_walk.h includes it).
// The container, stated once: a 40-byte GTMv header, one 28-byte GTMk entry per key frame, then the key frames' LZMA streams in order
// (tilingencoder.pas:30-51).  Both records are a 4-byte magic followed by little-endian 32-bit words; GtmHeader and GtmKfEntry name those
// words in file order, so a record's layout is its struct.  Decoding and encoding move bytes and check nothing: what a reader accepts is
// the reader's (the player is strict, tm_reload_gtm takes a header on magic and length alone).
#pragma once
#include <cmath>

#include "tm_common.h"

namespace tmx {

// ---- little-endian words
inline uint32_t load_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t load_u32(const uint8_t *p) { return load_u16(p) | (load_u16(p + 2) << 16); }
inline void store_u16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void store_u32(uint8_t *p, uint32_t v) { store_u16(p, v); store_u16(p + 2, v >> 16); }

// ---- the container
constexpr char GTM_HEADER_MAGIC[] = "GTMv", GTM_KF_MAGIC[] = "GTMk";
constexpr size_t GTM_HEADER_BYTES = 40, GTM_KF_BYTES = 28;
constexpr uint32_t GTM_HEADER_RIFF = 32, GTM_KF_RIFF = 20;  // the bytes of a record behind its riff_size word
// (whole_header_size: header + entries, where the first stream starts)
struct GtmHeader { uint32_t riff_size, whole_header_size, encoder_version, width, height, kf_count, frame_count, avg_bytes_per_s, kf_max_bytes_per_s; };
struct GtmKfEntry { uint32_t riff_size, index, frame, raw_size, comp_size, time_ms; };
static_assert(4 + sizeof(GtmHeader) == GTM_HEADER_BYTES && 4 + sizeof(GtmKfEntry) == GTM_KF_BYTES, "a record: its magic and its words");

template <class Rec>
inline Rec gtm_decode(const uint8_t *p) {  // p: the record's bytes, magic included
  uint32_t w[sizeof(Rec) / 4];
  for (size_t i = 0; i < sizeof(Rec) / 4; i++) w[i] = load_u32(p + 4 + 4 * i);
  Rec r;
  memcpy(&r, w, sizeof(r));
  return r;
}
template <class Rec>
inline void gtm_encode(const Rec &r, const char *magic, uint8_t *p) {
  uint32_t w[sizeof(Rec) / 4];
  memcpy(w, &r, sizeof(r));
  memcpy(p, magic, 4);
  for (size_t i = 0; i < sizeof(Rec) / 4; i++) store_u32(p + 4 + 4 * i, w[i]);
}
inline bool gtm_has_magic(const uint8_t *p, const char *magic) { return memcmp(p, magic, 4) == 0; }
inline GtmHeader decode_gtm_header(const uint8_t *p) { return gtm_decode<GtmHeader>(p); }
inline GtmKfEntry decode_gtm_kf_entry(const uint8_t *p) { return gtm_decode<GtmKfEntry>(p); }
inline void encode_gtm_header(const GtmHeader &h, uint8_t *p) { gtm_encode(h, GTM_HEADER_MAGIC, p); }
inline void encode_gtm_kf_entry(const GtmKfEntry &e, uint8_t *p) { gtm_encode(e, GTM_KF_MAGIC, p); }

// ---- SetDimensions carries the frame period in ns: the stream's rate, both ways
constexpr double GTM_NS_PER_S = 1000.0 * 1000 * 1000;
inline double gtm_fps(uint32_t frame_ns) { return GTM_NS_PER_S / frame_ns; }
inline uint32_t gtm_frame_ns(double fps) { return (uint32_t)llrint(GTM_NS_PER_S / fps); }

// ---- tm_gtm.hip (host only): SaveStream restatement, tilingencoder.pas:5177-5482
struct GtmInput {
  int tm_w = 0, tm_h = 0, nframes = 0;
  double fps = 0;
  std::vector<int32_t> kf_start;
  const uint8_t *pal_px = nullptr;   // [ntiles][64], final (Reindex) order
  std::vector<uint32_t> use;         // [ntiles]
  const int32_t *palettes = nullptr; // [pal_count][pal_size]
  int pal_count = 0, pal_size = 0;
  const tm_tilemap_item *tilemap = nullptr;  // [nframes][tm_h*tm_w]
  std::string settings;
  bool has_device = false;          // the caller has set a device for this thread: the device match finder may run (TM_SAVE_FINDER)
  void *stream = nullptr;           // its hipStream_t
  tm_save_stats *stats = nullptr;   // filled when the file has been written
};
int write_gtm(const char *path, const GtmInput &in);
// tm_lzma.hip (host only): LZCompress / LZDecompress, extern.pas:420-458
void lz_compress(const std::vector<uint8_t> &raw, std::vector<uint8_t> &dst);
int lz_decompress(const uint8_t *src, size_t n, std::vector<uint8_t> &dst, size_t *consumed, size_t max_out = (size_t)-1);  // max_out: TM_E_IO once the output passes it
// tm_gtm_reload.hip (host only): LoadStream (tilingencoder.pas:4880-5175)
struct GtmLoaded {
  int header_w = 0, header_h = 0, header_frames = -1;  // from the GTMv header (-1: headerless stream)
  int tm_w = 0, tm_h = 0, nframes = 0, pal_size = 0, pal_count = 0;
  double fps = 0;
  std::vector<int32_t> kf_start;
  std::vector<uint8_t> pal_px;      // [tiles][64]
  std::vector<uint32_t> use;        // UseCount as SetTMI counts it (4968-4969)
  std::vector<int32_t> palettes;    // [pal_count][pal_size], alpha stripped (4951)
  std::vector<tm_tilemap_item> tilemap;  // [nframes][tm_h*tm_w]
  std::string settings;
};
int read_gtm(const char *path, GtmLoaded *out);
// tm_player_parse.hip (host only): a .gtm file's picture size (tm_w * 8 x tm_h * 8), rate and frame count, from its header and first key frame
int probe_gtm(const char *path, int *width, int *height, double *fps, int *frames);

}  // namespace tmx
