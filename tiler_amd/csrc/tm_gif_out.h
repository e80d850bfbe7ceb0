// tm_gif_out.h -- what the GIF writer is, stated once for its host twin (tm_gif_encode_host and the two seams' twins) and its device form
// (the kernels of tm_gif_out.hip): DESIGN.md section 43.  Written from the GIF89a specification.  The independent check is the tests'
// plain-Python restatement (tests/gif_out_ref.py), Pillow and the project's own reader (tm_gif.h).
//
//   options   tm_gif_options (include/tilemotion.h); gif_options_check refuses what is unknown.
//   rectangle frame 0, and every frame with diff = 0, is coded whole.  Frame i > 0 is the bounding box of the pixels whose 0x00RRGGBB
//             differs from frame i - 1's; no such pixel: the 1 x 1 rectangle at (0, 0).
//   table     over the rectangle's pixels.  Exact (at most max_colours distinct colours, unless the options say quantise): the distinct
//             colours ascending, a pixel's index is its colour's rank.  Quantised: median_cut below over 15-bit cells, a pixel's index is
//             its cell's box.
//   lzw       the rectangle's indices in row order are cut into segments of segment_pixels (0: one segment); lzw_segment codes one:
//             greedy longest match, an entry per code, a clear when the table fills.  A segment's bits are its codes at the widths a
//             reader is at; the image's first clear opens segment 0, and the clear that opens segment k + 1 is written behind segment k's
//             last code at the width segment k ended on -- it is part of segment k's bits, so no segment looks at another.  The last
//             segment ends with eoi instead.
//   container GIF89a, no global table, NETSCAPE2.0 as `loop` says; per frame a graphic control (disposal 1, no transparency, the delay),
//             an image descriptor with a local table of the next power of two (at least 2) padded with black, the minimum code size
//             max(2, bits of the table size), the payload in sub-blocks of 255 and a last shorter one, a 0; the trailer.
//
// lzw_segment is written against an IO: where the indices come from, the dictionary (prefix code, byte) -> code, where a code's bits go.
// The host IO is one lane with a stamped array; the device IO is one wave with the same state in every lane and the dictionary in LDS.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tilemotion.h"

#if defined(__HIPCC__)
#define TM_GIFO_HD __host__ __device__
#else
#define TM_GIFO_HD
#endif

namespace tmx {
namespace gfo {

constexpr uint32_t kCells = 32768;      // 15-bit cells of the quantiser
constexpr uint32_t kHashSlots = 1024;   // a frame's table of distinct colours (open addressing; more than 256 colours is all it must tell)
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr uint32_t kNoCode = 0xffffffffu;
constexpr uint32_t kCodes = 4096;
constexpr uint64_t kMaxPixels = (uint64_t)1 << 28;  // of one frame

struct Rect { int32_t x, y, w, h; };

TM_GIFO_HD inline uint32_t rgb_of(uint32_t px) { return px & 0xffffffu; }
TM_GIFO_HD inline uint32_t cell_of(uint32_t c) { return (c >> 19 & 31u) << 10 | (c >> 11 & 31u) << 5 | (c >> 3 & 31u); }
TM_GIFO_HD inline uint32_t colour_hash(uint32_t c) { return (c * 2654435761u) >> 22; }  // 0 .. kHashSlots - 1
// the local table holds 1 << table_bits entries
TM_GIFO_HD inline uint32_t table_bits(uint32_t colours) {
  uint32_t b = 1;
  while ((1u << b) < colours) b++;
  return b;
}
TM_GIFO_HD inline uint32_t min_code_of(uint32_t colours) { const uint32_t b = table_bits(colours); return b < 2 ? 2 : b; }
// the segments of n indices
TM_GIFO_HD inline uint32_t segment_len(uint32_t n, uint32_t segment_pixels) { return segment_pixels ? segment_pixels : n; }
TM_GIFO_HD inline uint32_t segment_count(uint32_t n, uint32_t segment_pixels) { const uint32_t l = segment_len(n, segment_pixels); return (n + l - 1) / l; }
// an upper bound of a segment's bits: a code per index at most, a clear per 4094 of them, the opening and the closing code; 12 bits each
TM_GIFO_HD inline uint64_t segment_bits_bound(uint32_t p) { return 12ull * ((uint64_t)p + p / 4094 + 3); }

// ---- LZW.  IO: uint32_t index(i) (index i of the segment), void reset() (an empty dictionary), uint32_t find(prefix, byte) (the code
// of that string, or kNoCode), void add(prefix, byte, code) (behind a find of the same string that gave kNoCode), void put(code, width).
template <class IO>
TM_GIFO_HD inline void lzw_segment(IO &io, uint32_t n, uint32_t min_code, bool first, bool last) {
  const uint32_t clear = 1u << min_code, eoi = clear + 1;
  uint32_t next = clear + 2;                         // the coder's next free entry
  uint32_t rnext = clear + 2, width = min_code + 1;  // the reader's next free entry (one code behind) and the width it reads at
  bool fresh = true;                                 // the reader has taken no code since the clear
  if (first) io.put(clear, width);
  io.reset();
  uint32_t s = io.index(0);
  for (uint32_t i = 1; i <= n; i++) {
    uint32_t v = 0;
    if (i < n) {
      v = io.index(i);
      const uint32_t c = io.find(s, v);
      if (c != kNoCode) { s = c; continue; }
    }
    io.put(s, width);
    if (fresh) fresh = false;
    else if (rnext < kCodes) { rnext++; if (rnext == (1u << width) && width < 12) width++; }
    if (i == n) break;
    io.add(s, v, next);
    next++;
    s = v;
    if (next == kCodes) {
      io.put(clear, width);
      io.reset();
      next = clear + 2; rnext = clear + 2; width = min_code + 1; fresh = true;
    }
  }
  io.put(last ? eoi : clear, width);
}

// ---- the quantiser (host): a median cut in integers over the 15-bit cells
struct Cell { unsigned long long n, r, g, b; };  // pixels and channel sums
struct Box {
  int lo[3], hi[3];  // R, G, B in cell units, tight
  unsigned long long n, sum[3];
  uint32_t cells;
};
inline void box_tighten(const Cell *cells, Box &b) {
  int lo[3] = {32, 32, 32}, hi[3] = {-1, -1, -1};
  b.n = 0; b.sum[0] = b.sum[1] = b.sum[2] = 0; b.cells = 0;
  for (int r = b.lo[0]; r <= b.hi[0]; r++)
    for (int g = b.lo[1]; g <= b.hi[1]; g++)
      for (int bl = b.lo[2]; bl <= b.hi[2]; bl++) {
        const Cell &c = cells[r << 10 | g << 5 | bl];
        if (!c.n) continue;
        const int at[3] = {r, g, bl};
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], at[a]); hi[a] = std::max(hi[a], at[a]); }
        b.n += c.n; b.sum[0] += c.r; b.sum[1] += c.g; b.sum[2] += c.b; b.cells++;
      }
  for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
}
// table: at most max_colours entries; cell_box[kCells]: the box of every non-empty cell.  At least one cell is non-empty.
inline uint32_t median_cut(const Cell *cells, uint32_t max_colours, uint32_t *table, uint8_t *cell_box) {
  std::vector<Box> boxes(1);
  for (int a = 0; a < 3; a++) { boxes[0].lo[a] = 0; boxes[0].hi[a] = 31; }
  box_tighten(cells, boxes[0]);
  memset(cell_box, 0, kCells);
  while (boxes.size() < max_colours) {
    int pick = -1;  // the splittable box with the most pixels, the lowest number among equals
    for (size_t i = 0; i < boxes.size(); i++)
      if (boxes[i].cells >= 2 && (pick < 0 || boxes[i].n > boxes[(size_t)pick].n)) pick = (int)i;
    if (pick < 0) break;
    const Box b = boxes[(size_t)pick];
    int axis = 1;  // the longest axis: G, then R, then B among equals
    if (b.hi[0] - b.lo[0] > b.hi[axis] - b.lo[axis]) axis = 0;
    if (b.hi[2] - b.lo[2] > b.hi[axis] - b.lo[axis]) axis = 2;
    unsigned long long slice[32] = {0};
    for (int r = b.lo[0]; r <= b.hi[0]; r++)
      for (int g = b.lo[1]; g <= b.hi[1]; g++)
        for (int bl = b.lo[2]; bl <= b.hi[2]; bl++) {
          const int at[3] = {r, g, bl};
          slice[at[axis]] += cells[r << 10 | g << 5 | bl].n;
        }
    const unsigned long long half = (b.n + 1) / 2;
    unsigned long long run = 0;
    int cut = b.lo[axis];
    for (int v = b.lo[axis]; v <= b.hi[axis]; v++) {
      run += slice[v];
      if (run >= half) { cut = v; break; }
    }
    if (cut == b.hi[axis]) cut = b.hi[axis] - 1;  // (the bounds are tight: the last slice is not empty, and neither is what lies below it)
    Box lower = b, upper = b;
    lower.hi[axis] = cut; upper.lo[axis] = cut + 1;
    box_tighten(cells, lower); box_tighten(cells, upper);
    for (int r = upper.lo[0]; r <= upper.hi[0]; r++)
      for (int g = upper.lo[1]; g <= upper.hi[1]; g++)
        for (int bl = upper.lo[2]; bl <= upper.hi[2]; bl++) cell_box[r << 10 | g << 5 | bl] = (uint8_t)boxes.size();
    boxes[(size_t)pick] = lower;
    boxes.push_back(upper);
  }
  for (size_t i = 0; i < boxes.size(); i++) {
    const Box &b = boxes[i];
    uint32_t c = 0;
    for (int a = 0; a < 3; a++) c = c << 8 | (uint32_t)((2 * b.sum[a] + b.n) / (2 * b.n));
    table[i] = c;
  }
  return (uint32_t)boxes.size();
}

// ---- the container (host)
inline void put16(std::vector<uint8_t> &f, uint32_t v) { f.push_back((uint8_t)v); f.push_back((uint8_t)(v >> 8)); }
inline void file_header(int w, int h, int loop, std::vector<uint8_t> &f) {
  const char *sig = "GIF89a";
  f.insert(f.end(), sig, sig + 6);
  put16(f, (uint32_t)w); put16(f, (uint32_t)h);
  f.push_back(0x70); f.push_back(0); f.push_back(0);  // no global table, 8 bits a channel; background index; aspect
  if (loop >= 0) {
    const uint8_t app[] = {0x21, 0xff, 0x0b, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 0x03, 0x01};
    f.insert(f.end(), app, app + sizeof(app));
    put16(f, (uint32_t)loop);
    f.push_back(0);
  }
}
// graphic control, image descriptor, local table, minimum code size
inline void image_header(const Rect &r, const uint32_t *table, uint32_t colours, int delay, std::vector<uint8_t> &f) {
  const uint8_t gce[] = {0x21, 0xf9, 0x04, 0x04};
  f.insert(f.end(), gce, gce + 4);
  put16(f, (uint32_t)delay);
  f.push_back(0); f.push_back(0);
  f.push_back(0x2c);
  put16(f, (uint32_t)r.x); put16(f, (uint32_t)r.y); put16(f, (uint32_t)r.w); put16(f, (uint32_t)r.h);
  const uint32_t bits = table_bits(colours);
  f.push_back((uint8_t)(0x80 | (bits - 1)));
  for (uint32_t i = 0; i < (1u << bits); i++) {
    const uint32_t c = i < colours ? table[i] : 0u;
    f.push_back((uint8_t)(c >> 16)); f.push_back((uint8_t)(c >> 8)); f.push_back((uint8_t)c);
  }
  f.push_back((uint8_t)min_code_of(colours));
}
inline uint64_t sub_blocked_bytes(uint64_t payload) { return payload + (payload + 254) / 255 + 1; }  // length bytes and the terminator

// ---- where a chunk's bits go (k_gif_emit, k_gif_blob)
struct SegPlace { uint64_t bit_off, bits, word_off; };
struct ImagePlace {
  uint64_t payload, pos, word0;  // payload bytes, where the data starts in the chunk's bytes, its first word among the chunk's payload words
  uint32_t seg0, nseg;
};
struct Piece { uint64_t from, to; uint32_t n, pad; };

#if defined(__HIPCC__)
// The launches the WebP writer shares (tm_webp_out.hip), on `stream`, unchanged for this writer.  k_gif_rect: dev_raw[4 f ..] = min x, min y,
// min (65535 - x), min (65535 - y) of frame f's changed pixels, each from 0x7f7f7f7f (the caller fills it); k_gif_colours: per frame the
// open-addressed table of its rectangle's distinct colours (kHashSlots of kEmpty before) and their count, which stops above max_colours;
// k_gif_emit: the segments' bits joined into every image's payload (sub: GIF sub-blocks); k_gif_blob: host-made pieces to their places.
void launch_rect_raw(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, const uint32_t *dev_prev, int has_prev, int w, int h, int32_t *dev_raw,
                     hipStream_t stream);
void launch_colours(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const Rect *dev_rects, uint32_t *dev_tabs, uint32_t *dev_counts,
                    uint32_t max_colours, hipStream_t stream);
void launch_emit(const ImagePlace *dev_images, uint32_t nimages, const SegPlace *dev_segs, const uint32_t *dev_words, uint64_t nwords, uint64_t total_words, uint8_t *dev_out,
                 uint64_t out_bytes, int sub, hipStream_t stream);
void launch_blob(const Piece *dev_pieces, uint32_t npieces, const uint8_t *dev_blob, uint64_t blob_bytes, uint8_t *dev_out, uint64_t out_bytes, hipStream_t stream);
#endif

int gif_options_check(const char *who, const tm_gif_options *opt);
// every refusal of the writer that needs no pixel, and the delay (1/100 s) the frames get
int gif_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt, int *delay);
int gif_chunk_frames(int w, int h);

// The device writer: begin, the frames chunk by chunk in order, end.  Every chunk appends its bytes to `file`.  Between chunks the last
// frame stays on the device for the next chunk's rectangles.
class GifDeviceEncoder {
 public:
  GifDeviceEncoder();
  ~GifDeviceEncoder();
  int begin(int w, int h, double fps, const tm_gif_options &opt, void *hip_stream, std::vector<uint8_t> &file);
  int chunk(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, std::vector<uint8_t> &file);
  int end(std::vector<uint8_t> &file);
  // the two seams (tm_stage_gif_lzw_pack, tm_stage_gif_palettise)
  int pack(const uint8_t *dev_indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes, void *hip_stream);
  int palettise(const uint32_t *dev_frame, int64_t stride_px, int w, int h, const tm_gif_options &opt, uint32_t *table, int *colours, int *exact, uint8_t *indices,
                void *hip_stream);
  tm_gif_export_stats stats{};

 private:
  int tables(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes);
  struct State;
  State *state_;
};

}  // namespace gfo
}  // namespace tmx
