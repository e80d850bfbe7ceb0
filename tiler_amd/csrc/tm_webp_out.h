// tm_webp_out.h -- what the WebP writer is, stated once for its host twin (tm_webp_encode_host) and its device form (the kernels of
// tm_webp_out.hip): DESIGN.md section 44.  Written from the format notes of that section.  The independent check is the tests' plain-Python
// restatement and reader (tests/webp_out_ref.py) and Pillow.
//
//   options   tm_webp_options (include/tilemotion.h); webp_options_check refuses what is unknown.
//   rectangle frame 0, and every frame with diff = 0, is coded whole.  Frame i > 0 is the bounding box of the pixels whose 0x00RRGGBB
//             differs from frame i - 1's, its left and top lowered to even (the container stores them halved); no such pixel: the 1 x 1
//             rectangle at (0, 0).
//   pixels    over the rectangle.  Indexed (palette AUTO and at most 256 distinct colours): the distinct colours ascending, a pixel's index
//             is its colour's rank; bundle_of(colours) indices go into the green byte of one coded pixel, lowest bits first, a row's last
//             coded pixel padded with zero bits; red and blue are 0.  Otherwise: R - G, G, B - G.  Alpha is 0xFF.  A coded pixel is the
//             symbol 0xAARRGGBB.
//   match     at position i of an image's n symbols, with cap = min(kMaxLen, segment end - i) >= kMinMatch: the candidates are the earlier
//             positions whose key (three symbols hashed, missing ones read as 0) is the same, nearest first, at most kDepth visited, none
//             further than kMaxDist back.  Length = common run capped at cap.  The longest wins, the nearest among equals; the walk ends once
//             cap is reached.  Below kMinMatch, or kMinMatch and further than kFar3 back: no match.
//   parse     greedy: from the segment's first symbol, a match where there is one (i += length), else a literal (i += 1).  A match never
//             runs past its segment's end, so a segment's parse depends on no other segment's tokens.  lz77 = 0: literals only.
//   codes     one group per image: the histograms of the five alphabets over its tokens, lengths by dfl::code_lengths (15 bits; 7 for the
//             code of the lengths), write_code below.  The colour table is an image n x 1 of differences, literals only.
//   container RIFF / WEBP, VP8X (animation), ANIM, per frame an ANMF with one VP8L chunk.
//
// parse_segment is written against an IO: the symbols, the links, how a common run is measured (the host: a lane; the device: a wave, 64
// symbols a step and a ballot) and where a token goes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tilemotion.h"
#include "tm_gif_out.h"

#if defined(__HIPCC__)
#define TM_WPO_HD __host__ __device__
#else
#define TM_WPO_HD
#endif

namespace tmx {
namespace wpo {

using gfo::Rect;

constexpr uint32_t kMinMatch = 3, kMaxLen = 4096;
constexpr uint32_t kMaxDist = (1u << 20) - 120;
constexpr uint32_t kFar3 = 512;
constexpr int kDepth = 8;
constexpr int kMaxSide = 16384;
constexpr int kMaxChunk = 32;  // frames a chunk: the sort key holds the frame in 5 bits
// the five alphabets of a group behind one another
constexpr uint32_t kGreen = 0, kRed = 280, kBlue = 536, kAlpha = 792, kDist = 1048, kSyms = 1088;
constexpr uint32_t kGreenSyms = 280, kDistSyms = 40;

TM_WPO_HD inline uint32_t bundle_of(uint32_t colours) { return colours <= 2 ? 8u : colours <= 4 ? 4u : colours <= 16 ? 2u : 1u; }
TM_WPO_HD inline uint32_t packed_width(uint32_t w, uint32_t per) { return (w + per - 1) / per; }
TM_WPO_HD inline uint32_t subtract_green(uint32_t c) {
  const uint32_t g = c >> 8 & 255u;
  return 0xff000000u | (((c >> 16) - g) & 255u) << 16 | g << 8 | ((c - g) & 255u);
}
TM_WPO_HD inline uint32_t segment_len(uint32_t n, uint32_t segment_pixels) { return segment_pixels ? segment_pixels : n; }
TM_WPO_HD inline uint32_t segment_count(uint32_t n, uint32_t segment_pixels) { const uint32_t l = segment_len(n, segment_pixels); return (n + l - 1) / l; }
// the key of three symbols: 27 bits (the device's sort key holds the frame above them)
TM_WPO_HD inline uint32_t key_of(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t v = a * 0x9E3779B1u;
  v = (v ^ v >> 15) + b * 0x85EBCA77u;
  v = (v ^ v >> 13) + c * 0xC2B2AE3Du;
  v = (v ^ v >> 16) * 0x27D4EB2Fu;
  return v >> 5;
}
// a length or a distance code v >= 1 as prefix symbol and extra bits
TM_WPO_HD inline void prefix_of(uint32_t v, uint32_t *sym, uint32_t *ebits, uint32_t *eval) {
  if (v <= 4) { *sym = v - 1; *ebits = 0; *eval = 0; return; }
  v -= 1;
  const uint32_t h = 31u - (uint32_t)__builtin_clz(v), s = v >> (h - 1) & 1u;
  *sym = 2 * h + s; *ebits = h - 1; *eval = v & ((1u << (h - 1)) - 1u);
}

// ---- the parse.  IO: uint32_t sym(i), int32_t prev(i) (the nearest earlier position with i's key, or -1), uint32_t common(j, i, cap) (how
// many of sym(j + k) == sym(i + k), k = 0 .. cap - 1, hold from k = 0 on), void literal(symbol), void match(len, dist).
template <class IO>
TM_WPO_HD inline uint32_t best_match(IO &io, uint32_t i, uint32_t end, uint32_t *dist) {
  const uint32_t cap = end - i < kMaxLen ? end - i : kMaxLen;
  if (cap < kMinMatch) return 0;
  uint32_t best = 0, bd = 0;
  int32_t j = io.prev(i);
  for (int d = 0; d < kDepth && j >= 0 && i - (uint32_t)j <= kMaxDist; d++, j = io.prev((uint32_t)j)) {
    if (best && io.sym((uint32_t)j + best) != io.sym(i + best)) continue;  // cannot be longer (best < cap: in bounds)
    const uint32_t l = io.common((uint32_t)j, i, cap);
    if (l > best) {
      best = l; bd = i - (uint32_t)j;
      if (l == cap) break;
    }
  }
  if (best < kMinMatch || (best == kMinMatch && bd > kFar3)) return 0;
  *dist = bd;
  return best;
}
template <class IO>
TM_WPO_HD inline void parse_segment(IO &io, uint32_t begin, uint32_t end, bool lz77) {
  uint32_t i = begin;
  while (i < end) {
    uint32_t dist = 0;
    const uint32_t len = lz77 ? best_match(io, i, end, &dist) : 0u;
    if (len) { io.match(len, dist); i += len; }
    else { io.literal(io.sym(i)); i++; }
  }
}

// a token: x = the literal's symbol, or the match's length; y = 0, or the match's distance
struct Token { uint32_t x, y; };
// a token's bits through a group's table (entry: the code, bits reversed, | its length << 16): at most 4 x 15, or 15 + 10 + 15 + 18
TM_WPO_HD inline uint32_t token_bits(const uint32_t *tab, Token t, uint64_t *val) {
  uint64_t v = 0;
  uint32_t nb = 0;
  if (t.y == 0) {
    const uint32_t e[4] = {tab[kGreen + (t.x >> 8 & 255u)], tab[kRed + (t.x >> 16 & 255u)], tab[kBlue + (t.x & 255u)], tab[kAlpha + (t.x >> 24)]};
    for (int k = 0; k < 4; k++) { v |= (uint64_t)(e[k] & 0xffffu) << nb; nb += e[k] >> 16; }
  } else {
    uint32_t ls, le, lv, ds, de, dv;
    prefix_of(t.x, &ls, &le, &lv);
    prefix_of(t.y + 120, &ds, &de, &dv);
    const uint32_t a = tab[kGreen + 256 + ls], b = tab[kDist + ds];
    v = a & 0xffffu; nb = a >> 16;
    v |= (uint64_t)lv << nb; nb += le;
    v |= (uint64_t)(b & 0xffffu) << nb; nb += b >> 16;
    v |= (uint64_t)dv << nb; nb += de;
  }
  *val = v;
  return nb;
}
// the histogram slots a token counts in (at most 4)
TM_WPO_HD inline int token_slots(Token t, uint32_t *slots) {
  if (t.y == 0) { slots[0] = kGreen + (t.x >> 8 & 255u); slots[1] = kRed + (t.x >> 16 & 255u); slots[2] = kBlue + (t.x & 255u); slots[3] = kAlpha + (t.x >> 24); return 4; }
  uint32_t s, e, v;
  prefix_of(t.x, &s, &e, &v); slots[0] = kGreen + 256 + s;
  prefix_of(t.y + 120, &s, &e, &v); slots[1] = kDist + s;
  return 2;
}

// ---- bits on the host, lowest first
struct BitWriter {
  std::vector<uint32_t> words;
  uint64_t acc = 0, total = 0;
  uint32_t nb = 0;
  void put(uint64_t v, uint32_t n) {  // n <= 32
    acc |= v << nb;
    nb += n; total += n;
    if (nb >= 32) { words.push_back((uint32_t)acc); acc >>= 32; nb -= 32; }
  }
  void finish() { if (nb) { words.push_back((uint32_t)acc); acc = 0; nb = 0; } }
};

// One prefix code from its alphabet's counts: its bits into `bw`, its table entries into entry[nsym].
void write_code(BitWriter &bw, const uint32_t *freq, int nsym, uint32_t *entry);
// An image's bits before its pixels: the signature and sizes, the transforms (colours > 0: indexing with table[colours]; else subtract
// green), no colour cache, no meta codes, the group's five codes from hist[kSyms]; the group's table into tab[kSyms].
void image_header_bits(BitWriter &bw, int w, int h, const uint32_t *table, uint32_t colours, const uint32_t *hist, uint32_t *tab);

// ---- the container (host)
inline void put_le(std::vector<uint8_t> &f, uint32_t v, int bytes) { for (int k = 0; k < bytes; k++) f.push_back((uint8_t)(v >> (8 * k))); }
inline void put_tag(std::vector<uint8_t> &f, const char *tag) { f.insert(f.end(), tag, tag + 4); }
constexpr size_t kFileHeader = 12 + 18 + 14, kFrameHeader = 8 + 16 + 8;
inline void file_header(int w, int h, int loop, std::vector<uint8_t> &f) {
  put_tag(f, "RIFF"); put_le(f, 0, 4); put_tag(f, "WEBP");  // (the size is known at the end: file_close)
  put_tag(f, "VP8X"); put_le(f, 10, 4); put_le(f, 0x02, 4); put_le(f, (uint32_t)w - 1, 3); put_le(f, (uint32_t)h - 1, 3);
  put_tag(f, "ANIM"); put_le(f, 6, 4); put_le(f, 0, 4); put_le(f, (uint32_t)loop, 2);
}
inline void file_close(std::vector<uint8_t> &f) {
  const uint32_t v = (uint32_t)(f.size() - 8);
  for (int k = 0; k < 4; k++) f[4 + (size_t)k] = (uint8_t)(v >> (8 * k));
}
// an ANMF chunk up to the VP8L payload of `payload` bytes; behind the payload goes a 0 when it is odd
inline void frame_header(const Rect &r, int duration, uint64_t payload, std::vector<uint8_t> &f) {
  put_tag(f, "ANMF"); put_le(f, (uint32_t)(16 + 8 + payload + (payload & 1)), 4);
  put_le(f, (uint32_t)r.x / 2, 3); put_le(f, (uint32_t)r.y / 2, 3); put_le(f, (uint32_t)r.w - 1, 3); put_le(f, (uint32_t)r.h - 1, 3); put_le(f, (uint32_t)duration, 3);
  f.push_back(0x02);
  put_tag(f, "VP8L"); put_le(f, (uint32_t)payload, 4);
}

int webp_options_check(const char *who, const tm_webp_options *opt);
// every refusal of the writer that needs no pixel, and the duration (ms) the frames get
int webp_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt, int *duration);
int webp_chunk_frames(int w, int h);

// The device writer: begin, the frames chunk by chunk in order (at most kMaxChunk a chunk), end.  Every chunk appends its bytes to `file`.
// Between chunks the last frame stays on the device for the next chunk's rectangles.
class WebpDeviceEncoder {
 public:
  WebpDeviceEncoder();
  ~WebpDeviceEncoder();
  WebpDeviceEncoder(const WebpDeviceEncoder &) = delete;
  WebpDeviceEncoder &operator=(const WebpDeviceEncoder &) = delete;
  int begin(int w, int h, double fps, const tm_webp_options &opt, void *hip_stream, std::vector<uint8_t> &file);
  int chunk(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, std::vector<uint8_t> &file);
  int end(std::vector<uint8_t> &file);
  tm_webp_export_stats stats{};

 private:
  struct State;
  State *state_;
};

}  // namespace wpo
}  // namespace tmx
