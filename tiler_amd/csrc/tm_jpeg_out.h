// tm_jpeg_out.h -- what the JPEG writer is, stated once for its host form (tm_jpeg_encode_host) and its device form (the k_jpeg_* kernels;
// both in tm_jpeg_out.hip): DESIGN.md section 40.  It is libjpeg's baseline encoder restated from its published description -- the
// quality scaling of the Annex K.1 quantisers, the 16-bit fixed-point YCbCr of JFIF, box-averaged chroma with alternating bias, the
// "islow" forward DCT (Loeffler, Ligtenberg and Moschytz; the 13-bit constants tm_jpeg.h names), quantisation by integer division and the
// Huffman procedures of T.81 Annex F with the tables of Annex K.3 -- in integer arithmetic from the pixels to the file, so that the file
// is a function of the pixels and the options alone, and both forms write libjpeg's bytes.
//
//   pixels    RGB32, 0x00RRGGBB.  A coordinate past the picture reads its last column / last row.
//   planes    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb, Cr likewise with + (128 << 16) + 32767.  Chroma of 4:2:0 is
//             (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2.. along the output columns, of 4:2:2 (a + b + bias) >> 1 with bias 0, 1, 0, 1..
//             Below its last real row a shrunk plane repeats that SHRUNK row (sample_at: the row index is clamped before it is doubled).
//   blocks    a component has ceil(cw / 8) x ceil(ch / 8) real blocks.  The MCU grid may hold more (luma of 4:2:2 and 4:2:0 only): a dummy
//             block has zero AC and the DC of the block before it in its MCU (block_source names the real block whose DC that is).
//   transform samples - 128; rows first (outputs 0 and 4 shifted left by 2, the others descaled by 11), then columns (descaled by 2 and
//             by 15).  Quantisation: qv = 8 q, (|c| + (qv >> 1)) / qv with the sign restored.
//   code      DC differences per component, the prediction 0 at the start of every segment; categories up to 11 (DC) and 10 (AC), which
//             8-bit samples cannot exceed (section 40.1) -- code_block refuses anything else rather than emit a code it has no entry for;
//             ZRL for runs above 15, EOB unless coefficient 63 is set; bits most significant first, a segment padded with 1-bits, FF
//             stuffed with 00, RSTn (n = i & 7) between segments.
//   scan order  block j of a frame: MCU j / bpm, and inside it the luma blocks row by row, then Cb, then Cr (block_at).
//
// block_coefs and code_block are the whole rule; the forms differ in where the 64 coefficients go and in the sink the bits are put to:
// the host appends stuffed bytes, the device first counts (CountSink) and then ORs words into a zeroed stream (PackSink, tm_jpeg_out.hip).
#pragma once
#include "tm_jpeg.h"

namespace tmx {
namespace jpo {

using jpg::descale;
using jpg::zigzag;

enum { kOk = 0, kBadMagnitude = TM_JPG_BAD_MAGNITUDE };

constexpr uint32_t kMaxBlockBits = 27 + 63 * 26;          // a DC code of 16 bits and 11 more, 63 AC codes of 16 bits and 10 more
constexpr uint32_t kMaxBlockBytes = (kMaxBlockBits + 7) / 8;

// what both forms read of the options: 8 x the quantisers in natural order, and the codes as code | length << 16 (0: no such code)
struct Tables {
  uint16_t qv[2][64];   // [0] luma, [1] chroma
  uint32_t dc[2][12];   // by category
  uint32_t ac[2][256];  // by run << 4 | category
};

// a picture's geometry, the same for every frame of a call
struct Plan {
  int32_t w, h;
  uint32_t ncomp, hs, vs;       // 1 or 3 components; the luma blocks of an MCU across and down (1 x 1 for grey)
  uint32_t mcx, mcy, bpm;       // MCUs across and down, blocks per MCU
  uint32_t seg_mcus, segs;      // MCUs per segment, segments per frame
  uint32_t blocks;              // per frame: mcx mcy bpm
  uint32_t header_bytes;
};

struct Block { uint32_t c, bx, by, m; bool dummy; };  // component, the REAL block whose samples are read, the MCU; dummy: only its DC counts

// the real block a block of the MCU grid takes its samples (or, dummy, its DC) from
TM_JPG_HD inline void block_source(const Plan &p, uint32_t c, uint32_t mx, uint32_t my, uint32_t xin, uint32_t yin, Block *b) {
  b->c = c;
  b->bx = mx; b->by = my; b->dummy = false;
  if (c != 0 || p.ncomp == 1) return;  // (chroma and grey have no dummy blocks: ceil(ceil(w / 2) / 8) = ceil(w / 16))
  const uint32_t cols = ((uint32_t)p.w + 7) / 8, rows = ((uint32_t)p.h + 7) / 8;
  uint32_t bx = mx * p.hs + xin, by = my * p.vs + yin;
  if (by >= rows) { by = my * p.vs; bx = mx * p.hs + p.hs - 1; b->dummy = true; }  // a dummy row: the last block of the row above it
  if (bx >= cols) { bx = mx * p.hs; b->dummy = true; }                             // to the right: the block on its left
  b->bx = bx; b->by = by;
}
// block j of a frame in scan order
TM_JPG_HD inline Block block_at(const Plan &p, uint32_t j) {
  Block b;
  b.m = j / p.bpm;
  const uint32_t k = j % p.bpm, nl = p.ncomp == 1 ? 1 : p.hs * p.vs;
  const uint32_t mx = b.m % p.mcx, my = b.m / p.mcx;
  if (k < nl) block_source(p, 0, mx, my, k % p.hs, k / p.hs, &b);
  else block_source(p, 1 + k - nl, mx, my, 0, 0, &b);
  return b;
}
// the block before j of the same component in scan order, or j itself where the segment starts (prediction 0)
TM_JPG_HD inline uint32_t block_before(const Plan &p, uint32_t j) {
  const uint32_t m = j / p.bpm, k = j % p.bpm, nl = p.ncomp == 1 ? 1 : p.hs * p.vs;
  if (k > 0 && k < nl) return j - 1;
  if (m % p.seg_mcus == 0) return j;
  return k == 0 ? (m - 1) * p.bpm + nl - 1 : j - p.bpm;
}
TM_JPG_HD inline bool ends_segment(const Plan &p, uint32_t j) {
  const uint32_t m = j / p.bpm;
  return j % p.bpm == p.bpm - 1 && (m % p.seg_mcus == p.seg_mcus - 1 || m == p.mcx * p.mcy - 1);
}

constexpr int32_t fix16(double x) { return (int32_t)(x * 65536.0 + 0.5); }
TM_JPG_HD inline int32_t component(uint32_t px, uint32_t c) {
  const int32_t r = (int32_t)(px >> 16 & 255u), g = (int32_t)(px >> 8 & 255u), b = (int32_t)(px & 255u);
  if (c == 0) return (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16;
  if (c == 1) return (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16;
  return (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
}

// sample (x, y) of component c's plane as the transform reads it; fh x fv: how far the component is shrunk
TM_JPG_HD inline int32_t sample_at(const uint32_t *frame, int64_t stride_px, const Plan &p, uint32_t c, uint32_t fh, uint32_t fv, uint32_t x, uint32_t y) {
  const uint32_t wl = (uint32_t)p.w - 1, hl = (uint32_t)p.h - 1;
  if (fv == 2) { const uint32_t last = hl / 2; y = y < last ? y : last; }  // (the shrunk plane's last real row: ceil(h / 2) - 1)
  const uint32_t x0 = x * fh < wl ? x * fh : wl, y0 = y * fv < hl ? y * fv : hl;
  int32_t v = component(frame[(int64_t)y0 * stride_px + x0], c);
  if (fh == 1) return v;
  const uint32_t x1 = x0 < wl ? x0 + 1 : wl;
  v += component(frame[(int64_t)y0 * stride_px + x1], c);
  if (fv == 1) return (v + (int32_t)(x & 1u)) >> 1;
  const uint32_t y1 = y0 < hl ? y0 + 1 : hl;
  v += component(frame[(int64_t)y1 * stride_px + x0], c) + component(frame[(int64_t)y1 * stride_px + x1], c);
  return (v + 1 + (int32_t)(x & 1u)) >> 2;
}

// ---- the islow forward DCT: eight outputs from eight inputs; kPass 0: the rows, 1: the columns.  32-bit two's complement that wraps, as
// in tm_jpeg.h (8-bit samples stay far inside it)
template <int kPass>
TM_JPG_HD inline void fdct8(const uint32_t d[8], int32_t out[8]) {
  using namespace jpg;
  constexpr int n = kPass == 0 ? 11 : 15;
  const uint32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  out[0] = kPass == 0 ? (int32_t)((t10 + t11) << 2) : descale(t10 + t11, 2);
  out[4] = kPass == 0 ? (int32_t)((t10 - t11) << 2) : descale(t10 - t11, 2);
  uint32_t z1 = (t12 + t13) * kF0_541;
  out[2] = descale(z1 + t13 * kF0_765, n);
  out[6] = descale(z1 - t12 * kF1_847, n);
  z1 = t4 + t7;
  uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const uint32_t z5 = (z3 + z4) * kF1_175;
  const uint32_t a4 = t4 * kF0_298, a5 = t5 * kF2_053, a6 = t6 * kF3_072, a7 = t7 * kF1_501;
  z1 = 0u - z1 * kF0_899; z2 = 0u - z2 * kF2_562; z3 = 0u - z3 * kF1_961 + z5; z4 = 0u - z4 * kF0_390 + z5;
  out[7] = descale(a4 + z1 + z3, n); out[5] = descale(a5 + z2 + z4, n); out[3] = descale(a6 + z2 + z3, n); out[1] = descale(a7 + z1 + z4, n);
}

// One block's quantised coefficients in zig-zag order.  qv: the component's 64 divisors.  Every index below is a constant once the loops
// are unrolled: the 64 values stay in registers.
TM_JPG_HD inline void block_coefs(const uint32_t *frame, int64_t stride_px, const Plan &p, const Block &b, const uint16_t *qv, int16_t zz[64]) {
  const uint32_t fh = b.c ? p.hs : 1u, fv = b.c ? p.vs : 1u;
  int32_t ws[64];
#pragma unroll
  for (int y = 0; y < 8; y++) {
    uint32_t in[8];
    int32_t row[8];
#pragma unroll
    for (int x = 0; x < 8; x++) in[x] = (uint32_t)(sample_at(frame, stride_px, p, b.c, fh, fv, 8 * b.bx + (uint32_t)x, 8 * b.by + (uint32_t)y) - 128);
    fdct8<0>(in, row);
#pragma unroll
    for (int x = 0; x < 8; x++) ws[8 * y + x] = row[x];
  }
#pragma unroll
  for (int x = 0; x < 8; x++) {
    uint32_t in[8];
    int32_t col[8];
#pragma unroll
    for (int y = 0; y < 8; y++) in[y] = (uint32_t)ws[8 * y + x];
    fdct8<1>(in, col);
#pragma unroll
    for (int y = 0; y < 8; y++) ws[8 * y + x] = col[y];
  }
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const int32_t v = ws[zigzag((uint32_t)k)];
    const uint32_t q = qv[zigzag((uint32_t)k)], t = ((uint32_t)(v < 0 ? -v : v) + (q >> 1)) / q;
    zz[k] = (b.dummy && k) ? (int16_t)0 : (int16_t)(v < 0 ? -(int32_t)t : (int32_t)t);
  }
}

TM_JPG_HD inline uint32_t category(int32_t v) {
  uint32_t a = (uint32_t)(v < 0 ? -v : v), s = 0;
  while (a) { s++; a >>= 1; }  // (at most 16 passes: the values are 16-bit differences)
  return s;
}
TM_JPG_HD inline uint32_t magnitude_bits(int32_t v, uint32_t s) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

// One block's code: diff = its DC less the prediction, coef(k) its coefficient k of the zig-zag sequence.  The sink takes (bits, count),
// count 1 .. 27.  kBadMagnitude, with nothing more put, for a value that 8-bit samples cannot make.
template <class Coef, class Sink>
TM_JPG_HD inline int code_block(const Tables &t, uint32_t cls, int32_t diff, Coef &&coef, Sink &sink) {
  uint32_t s = category(diff);
  if (s > 11) return kBadMagnitude;
  uint32_t e = t.dc[cls][s];
  sink.put((e & 0xffffu) << s | (s ? magnitude_bits(diff, s) : 0u), (e >> 16) + s);
  uint32_t run = 0;
  for (uint32_t k = 1; k < 64; k++) {
    const int32_t v = coef(k);
    if (!v) { run++; continue; }
    for (; run > 15; run -= 16) sink.put(t.ac[cls][0xf0] & 0xffffu, t.ac[cls][0xf0] >> 16);
    s = category(v);
    if (s > 10) return kBadMagnitude;
    e = t.ac[cls][run << 4 | s];
    sink.put((e & 0xffffu) << s | magnitude_bits(v, s), (e >> 16) + s);
    run = 0;
  }
  if (run) sink.put(t.ac[cls][0] & 0xffffu, t.ac[cls][0] >> 16);
  return kOk;
}

struct CountSink {
  uint32_t n = 0;
  TM_JPG_HD void put(uint32_t, uint32_t count) { n += count; }
};

// ---- the host side (tm_jpeg_out.hip)
struct JpegGeometry {  // Plan, Tables and the file header of (w, h, options)
  Plan plan;
  Tables tables;
  std::vector<uint8_t> header;
};
int jpeg_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt);
int jpeg_options_check(const char *who, const tm_jpeg_options *opt);
void jpeg_geometry(int w, int h, const tm_jpeg_options &opt, JpegGeometry *g);
int64_t jpeg_bound(const Plan &p);
int jpeg_encode_one_host(const JpegGeometry &g, const uint32_t *frame, int64_t stride_px, std::vector<uint8_t> &file);
int jpeg_chunk_frames(int w, int h);  // the PNG export's rule: 32 frames or 256 MB of RGB32, whichever is less

// nframes RGB32 pictures [h][w] in DEVICE memory (rows stride_px apart, frames frame_px apart) as the files jpeg_encode_one_host writes,
// files[f] of frame f, a chunk at a time.  Its device buffers are kept from chunk to chunk and from call to call.
class JpegDeviceEncoder {
 public:
  JpegDeviceEncoder();
  ~JpegDeviceEncoder();
  JpegDeviceEncoder(const JpegDeviceEncoder &) = delete;
  JpegDeviceEncoder &operator=(const JpegDeviceEncoder &) = delete;
  int encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options &opt, void *hip_stream,
             std::vector<std::vector<uint8_t>> &files);
 private:
  struct State;
  State *state_;
};

}  // namespace jpo
}  // namespace tmx
