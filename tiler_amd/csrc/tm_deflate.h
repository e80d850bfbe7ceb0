// tm_deflate.h -- what the PNG writer's coder is, stated once for its host form (tm_deflate.hip) and its device form (tm_png_out.hip):
// DESIGN.md section 34.  Written from RFC 1950, RFC 1951 and the PNG specification.
//
// The file of a picture is a function of its pixels and the options alone.
//   stream    the filtered rows of one frame, n = h (1 + 3 w) bytes: a filter type byte, then R, G, B of every pixel.  Filter NONE: type 0 on
//             every row.  ADAPTIVE: per row the type 0..4 with the least sum of |(int8) byte| over its 3 w filtered bytes (bpp 3, the row
//             above row 0 is zeros, ties to the lowest type).
//   segments  kSeg = 32768 stream bytes each (the last one shorter; an empty stream is one empty segment).
//   match     at position i, with cap = min(kMaxMatch, segment end - i) >= 3: the candidates are the earlier positions with the same three
//             bytes, nearest first, at most kDepth visited, none further than kWindow back (earlier segments included, never before the
//             stream).  Length = common prefix capped at cap.  The longest wins, ties to the nearest; the walk ends once cap is reached.  A
//             match of length 3 further than kFar3 back is dropped (its distance bits cost more than three literals).
//   parse     greedy: from the segment's first byte, a match where there is one (i += length), else a literal (i += 1).  A match never
//             runs past its segment's end, so a segment's parse depends on no other segment's.
//   code      per segment one dynamic-Huffman block, or a stored block when that takes no more bytes.  Code lengths: Huffman lengths of
//             the used symbols ordered by (frequency, symbol), then limited (code_lengths below) -- 15 bits for the literal/length and the
//             distance code, 7 for the code-length code; fewer than two used symbols are padded to two.
//   framing   after every segment but the last an empty stored block, so every segment starts on a byte; the last block carries BFINAL.
//             zlib header 78 9C, Adler-32 of the stream, one IDAT.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tilemotion.h"

#if defined(__HIPCC__)
#define TM_DF_HD __host__ __device__
#else
#define TM_DF_HD
#endif

namespace tmx {
namespace dfl {

constexpr uint32_t kSeg = 32768;     // stream bytes per segment
constexpr uint32_t kWindow = 32768;  // the furthest a match may lie
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258;
constexpr int kDepth = 32;           // candidates visited per position (DESIGN.md section 34 has the sizes behind it)
constexpr uint32_t kFar3 = 4096;     // a match of 3 bytes further back than this is not taken
constexpr int kLitSyms = 286, kDistSyms = 30, kClSyms = 19;
constexpr int kHdrWords = 80;        // a dynamic block's header: at most 17 + 19 * 3 + 316 * 7 = 2286 bits
constexpr uint32_t kSlotBytes = kSeg + 16;  // what a segment's blocks can take: 5 + 32768 stored, 5 more for the empty block; a multiple of 4
constexpr uint32_t kAdler = 65521;

enum { kFilterNone = 1, kFilterAdaptive = 2, kFilterSmaller = 3 };  // TM_PNG_FILTER_* (AUTO is resolved before the rule is asked)

TM_DF_HD inline uint32_t seg_count(uint64_t n) { return n ? (uint32_t)((n + kSeg - 1) / kSeg) : 1u; }
TM_DF_HD inline uint32_t seg_end(uint32_t n, uint32_t i) { const uint64_t e = ((uint64_t)(i / kSeg) + 1) * kSeg; return e < n ? (uint32_t)e : n; }
TM_DF_HD inline uint32_t key3(const uint8_t *p) { return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[2]; }

// ---- the filters (PNG specification, 9.2), bpp = 3.  x: the byte, a: 3 to the left, b: above, c: above and 3 to the left
TM_DF_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
TM_DF_HD inline uint8_t filter_byte(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  switch (type) {
    case 1: return (uint8_t)(x - a);
    case 2: return (uint8_t)(x - b);
    case 3: return (uint8_t)(x - ((a + b) >> 1));
    case 4: return (uint8_t)(x - paeth(a, b, c));
    default: return (uint8_t)x;
  }
}
TM_DF_HD inline uint32_t filter_cost(uint8_t v) { return v < 128 ? v : 256u - v; }  // |(int8) v|
// byte k (0 .. 3 w - 1) of a row of 0x00RRGGBB pixels
TM_DF_HD inline uint32_t row_byte(const uint32_t *row, uint32_t k) { return (row[k / 3] >> (16 - 8 * (k % 3))) & 0xffu; }

// ---- the symbols of a match (RFC 1951, 3.2.5)
TM_DF_HD inline uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
TM_DF_HD inline void len_symbol(uint32_t len, uint32_t *sym, uint32_t *ebits, uint32_t *eval) {
  const uint32_t l = len - 3;
  if (l < 8) { *sym = 257 + l; *ebits = 0; *eval = 0; return; }
  if (len == kMaxMatch) { *sym = 285; *ebits = 0; *eval = 0; return; }
  const uint32_t e = log2_floor(l) - 2;
  *sym = 261 + 4 * e + ((l >> e) & 3u); *ebits = e; *eval = l & ((1u << e) - 1);
}
TM_DF_HD inline void dist_symbol(uint32_t dist, uint32_t *sym, uint32_t *ebits, uint32_t *eval) {
  const uint32_t d = dist - 1;
  if (d < 4) { *sym = d; *ebits = 0; *eval = 0; return; }
  const uint32_t k = log2_floor(d), e = k - 1;
  *sym = 2 * k + ((d >> e) & 1u); *ebits = e; *eval = d & ((1u << e) - 1);
}
TM_DF_HD inline uint32_t len_extra_bits(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) >> 2; }
TM_DF_HD inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }

// ---- the match of position i.  s: the stream; prev[j]: the nearest position before j with j's three bytes (-1: none, or j + 3 > n).
// Returns the length (0: none) and *dist.
TM_DF_HD inline uint32_t best_match(const uint8_t *s, uint32_t n, const int32_t *prev, uint32_t i, uint32_t *dist) {
  const uint32_t cap0 = seg_end(n, i) - i, cap = cap0 < kMaxMatch ? cap0 : kMaxMatch;
  if (cap < kMinMatch) return 0;
  uint32_t best = 0, bd = 0;
  int32_t j = prev[i];
  for (int d = 0; d < kDepth && j >= 0 && i - (uint32_t)j <= kWindow; d++, j = prev[j]) {
    if (best >= kMinMatch && s[(uint32_t)j + best] != s[i + best]) continue;  // cannot be longer (best < cap: in bounds)
    uint32_t l = kMinMatch;
    while (l < cap && s[(uint32_t)j + l] == s[i + l]) l++;
    if (l > best) {
      best = l; bd = i - (uint32_t)j;
      if (l == cap) break;
    }
  }
  if (best == kMinMatch && bd > kFar3) return 0;
  *dist = bd;
  return best;
}

// ---- a token's bits.  Table entries: the code, bits reversed so that it goes out lowest bit first, | its length << 16.
TM_DF_HD inline uint32_t literal_bits(const uint32_t *lit, uint32_t byte, uint64_t *val) {
  *val = lit[byte] & 0xffffu;
  return lit[byte] >> 16;
}
TM_DF_HD inline uint32_t match_bits(const uint32_t *lit, const uint32_t *dst, uint32_t len, uint32_t dist, uint64_t *val) {
  uint32_t ls, le, lv, ds, de, dv;
  len_symbol(len, &ls, &le, &lv);
  dist_symbol(dist, &ds, &de, &dv);
  uint64_t v = lit[ls] & 0xffffu;
  uint32_t nb = lit[ls] >> 16;
  v |= (uint64_t)lv << nb; nb += le;
  v |= (uint64_t)(dst[ds] & 0xffffu) << nb; nb += dst[ds] >> 16;
  v |= (uint64_t)dv << nb; nb += de;
  *val = v;
  return nb;  // at most 15 + 5 + 15 + 13
}

// ---- what the coder decides for one segment from its token histograms; plain data, as the device's pack kernel reads it
struct SegTables {
  uint32_t stored;     // 1: a stored block
  uint32_t hdr_nbits;  // of a dynamic block: BFINAL, BTYPE, HLIT, HDIST, HCLEN and the coded lengths
  uint32_t out_bytes;  // the block, and the empty stored block behind it unless the segment is the last
  uint32_t last;
  uint32_t hdr[kHdrWords];
  uint32_t lit[kLitSyms + 2];  // (288: a round number of words)
  uint32_t dist[kDistSyms + 2];
};

// Adler-32 of a stream from its segments' sums: s1 = sum of the bytes, s2 = sum of (len - k) byte[k]
inline void adler_append(uint32_t *a, uint32_t *b, uint64_t s1, uint64_t s2, uint32_t len) {
  *b = (uint32_t)((*b + (uint64_t)len * *a + s2) % kAdler);
  *a = (uint32_t)((*a + s1) % kAdler);
}

// ---- tm_deflate.hip: the host form
// Length-limited code lengths: deterministic; every length <= max_bits, Kraft sum exactly 1; 0 or 1 used symbols are padded to two.
void code_lengths(const uint32_t *freq, int nsym, int max_bits, uint8_t *lens);
// The tables, header bits and size of one segment (lit_hist without the end-of-block symbol: the coder counts it itself)
void plan_segment(const uint32_t *lit_hist, const uint32_t *dist_hist, uint32_t seg_len, bool last, SegTables *out);
// The filtered rows of a frame; filter NONE or ADAPTIVE
void filter_rows(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, uint8_t *stream);
// The deflate blocks of a stream (no zlib header, no Adler-32) appended to out
int deflate_body(const uint8_t *s, uint32_t n, std::vector<uint8_t> &out);
uint32_t adler32(const uint8_t *s, size_t n);
// The framing around a coded body: zlib header + body + Adler-32 as the one IDAT of a w x h RGB picture
void png_wrap(int w, int h, const uint8_t *body, size_t body_n, uint32_t adler, std::vector<uint8_t> &file);
// Level 0: the picture in stored blocks of 65535 bytes, zlib header 78 01 (what GeneratePNGs has always written)
void png_stored(const uint32_t *frame, int64_t stride_px, int w, int h, std::vector<uint8_t> &file);
// One frame at level 1 with filter NONE, ADAPTIVE or SMALLER
int png_encode(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, std::vector<uint8_t> &file);
int64_t png_bound(int w, int h);
// What the entry points refuse, before any device call: level, filter (AUTO allowed), sizes, strides
int png_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt);
int host_threads();  // TM_HOST_THREADS, 1 .. 16 (default 16, at most the machine's)

// ---- tm_png_out.hip: the device form.  nframes pictures in device memory (rows stride_px, frames frame_px pixels apart) at level 1 with
// filter NONE, ADAPTIVE or SMALLER: the files png_encode writes, files[f] of frame f.  Works through the frames in chunks of at most 32
// frames or 256 MB of stream; returns synchronised.
// The encoder keeps its device buffers (the streams, the sort's, the coder's) from one call to the next: an export makes one and hands
// it chunk after chunk.  The buffers go back to the calling thread's pool with it.
class PngDeviceEncoder {
 public:
  PngDeviceEncoder();
  ~PngDeviceEncoder();
  PngDeviceEncoder(const PngDeviceEncoder &) = delete;
  PngDeviceEncoder &operator=(const PngDeviceEncoder &) = delete;
  int encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, int filter, void *hip_stream,
             std::vector<std::vector<uint8_t>> &files);

 private:
  struct State;
  State *state_;
};

}  // namespace dfl
}  // namespace tmx
