// tm_jpeg.h -- what the JPEG reader's decoder is, stated once for its host form (tm_jpeg_decode_host) and its device form (k_jpeg_decode;
// both in tm_jpeg_in.hip): DESIGN.md section 39.  Written from ITU-T T.81 (the container, the Huffman procedures of Annexes C and F, the
// tables of Annex K.3) and from the published description of the "islow" inverse DCT (Loeffler, Ligtenberg and Moschytz; 13-bit constants).
//
// Accepted: baseline files (SOF0, or SOF1 with 8-bit samples), one component, or three with chroma 1x1 and luma 1x1, 2x1 or 2x2, in one
// interleaved scan; DQT with 8- or 16-bit entries; DHT tables 0..3 per class (none at all: the tables of Annex K.3, as the frames of an
// MJPEG capture rely on); DRI / RSTn; APPn and COM skipped; fill bytes before a marker; anything behind EOI ignored.  The EXIF orientation
// is ignored: the samples come out as they are stored.  What the container walk refuses (parse_jpeg, host only) never reaches a decoder.
//
// The walk cuts the scan into entropy SEGMENTS at every RSTn.  Segment i holds MCUs [i ri, min((i + 1) ri, total)), starts from a zero DC
// prediction and shares nothing with its neighbours: it is one serial chain, and a picture's segments are decoded side by side.
//   bytes     FF 00 is the byte FF.  An FF followed by anything else ends the data (the walk cuts there, so this is a file's cut tail).
//   codes     canonical codes from the counts of lengths 1..16, most significant bit first.  A symbol that needs bits beyond the segment
//             is kTruncated (bits past the end are never taken for zeros); bits that are no code: kBadCode.
//   blocks    DC: category t <= 11 (else kBadMagnitude), t more bits, added to the component's prediction (32 bits, wrapping; the
//             coefficient is its low 16 bits).  AC: run r, category s <= 10 (else kBadMagnitude); r zeros that would take k past 63:
//             kBadRun; 15/0 is sixteen zeros; any other r/0 ends the block.  Bytes behind a segment's last MCU are ignored.
//   samples   coefficient x quantiser, the islow IDCT (columns descaled by 11, rows by 18), + 128, clamped to 0..255.  Every sum and
//             product is 32-bit two's complement that wraps (unsigned arithmetic, arithmetic shifts), the same in both forms.
// A segment that refuses stops there; the others are decoded all the same, so that both forms leave the same bytes.  A file's status is
// that of its first refusing segment.  Every read is checked against the segment's own extent; a block is written inside the extent its
// plane was given (8 bytes a row where the row has room and is aligned, single bytes at a picture's edge).
//
// The text is written against an IO: how many lanes run it together, where the tables and a lane's 64 coefficients live, how a status is
// noted.  The host IO is one lane; the device IO is a workgroup whose lanes each take a segment.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tilemotion.h"

#if defined(__HIPCC__)
#define TM_JPG_HD __host__ __device__
#else
#define TM_JPG_HD
#endif

namespace tmx {
namespace jpg {

// a file's status (TM_JPG_*, include/tilemotion.h)
enum {
  kOk = 0, kTruncated = TM_JPG_TRUNCATED, kBadCode = TM_JPG_BAD_CODE, kBadRun = TM_JPG_BAD_RUN, kBadMagnitude = TM_JPG_BAD_MAGNITUDE,
  kBadRestart = TM_JPG_BAD_RESTART, kBadDesc = TM_JPG_BAD_DESC,
};

constexpr int kFastBits = 9;               // codes up to this long are one look-up; longer ones walk the counts
constexpr int kCodeTables = 8;             // DC 0..3, AC 0..3 (class << 2 | id)
constexpr uint32_t kSlotHalves = 66;       // a lane's 64 coefficients, and two halves so that neighbouring lanes' slots start in different LDS banks
constexpr uint32_t kNoRefusal = 0xffffffffu;

// the descriptor of a batch as both forms read it: segments as spans of the blob, a table set and a frame per file
struct Seg { uint32_t off, len; };
struct TableSet {
  uint16_t q[4][64];                   // quantisers in natural (row-major) order
  uint8_t count[kCodeTables][16];      // codes of length l + 1
  uint8_t symbol[kCodeTables][256];    // in code order
};
struct Frame {
  uint64_t plane_off[3];               // where the file's Y, U, V start in their planes' buffers
  uint32_t plane_stride[3], plane_w[3], plane_h[3];  // bytes from row to row; the extent a block may be written in
  uint32_t seg_first, seg_count;       // its segments in the list
  uint32_t ri;                         // MCUs per segment (the whole scan where there is no DRI)
  uint32_t mcus_x, mcus_total;
  uint32_t ncomp, hs, vs;              // 1 or 3; the luma blocks of an MCU across and down
  uint8_t tq[4], td[4], ta[4];         // a component's quantiser, DC and AC table
  int32_t status0;                     // what the walk found about the restart markers: kOk or kBadRestart (the file is then not decoded)
  uint32_t reserved;
};

// coefficient k of the zig-zag sequence sits at kZigzag[k] of the block
TM_JPG_HD inline uint32_t zigzag(uint32_t k) {
  constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}

// what the kernel checks of a frame before it reads or writes for it (the host entry points make descriptors that pass)
TM_JPG_HD inline bool frame_ok(const Frame &f, uint32_t nsegs, const uint64_t plane_bytes[3]) {
  if (f.ncomp != 1 && f.ncomp != 3) return false;
  if (f.hs < 1 || f.hs > 2 || f.vs < 1 || f.vs > 2 || !f.ri || !f.mcus_x || f.mcus_total % f.mcus_x) return false;
  if (f.seg_first > nsegs || f.seg_count > nsegs - f.seg_first) return false;
#pragma unroll
  for (uint32_t c = 0; c < 3; c++) {  // (unrolled: plane_bytes stays in registers)
    if (c >= f.ncomp) break;
    if (f.tq[c] > 3 || f.td[c] > 3 || f.ta[c] > 3 || !f.plane_w[c] || !f.plane_h[c] || f.plane_stride[c] < f.plane_w[c]) return false;
    const uint64_t last = f.plane_off[c] + (uint64_t)(f.plane_h[c] - 1) * f.plane_stride[c] + f.plane_w[c];
    if (last > plane_bytes[c] || last < f.plane_off[c]) return false;
  }
  return true;
}

// fast[t][p]: symbol << 8 | length for every pattern p of kFastBits bits that begins with a code of table t at most that long, 0 elsewhere
// (no code has length 0).  Run by all lanes together; the fill is shared out.
template <class IO>
TM_JPG_HD inline void build_fast(IO &io, const TableSet &ts, uint16_t *fast /* [kCodeTables][1 << kFastBits] */) {
  for (uint32_t i = io.lane(); i < (uint32_t)kCodeTables << kFastBits; i += io.lanes()) fast[i] = 0;
  io.sync();
  for (int t = 0; t < kCodeTables; t++) {
    uint32_t code = 0, at = 0;
    for (int l = 1; l <= kFastBits; l++) {
      const uint32_t cnt = ts.count[t][l - 1];
      for (uint32_t i = 0; i < cnt && code < (1u << l); i++, code++, at++) {
        const uint32_t e = (uint32_t)ts.symbol[t][at & 255u] << 8 | (uint32_t)l, lo = code << (kFastBits - l), hi = (code + 1) << (kFastBits - l);
        for (uint32_t p = lo + io.lane(); p < hi; p += io.lanes()) fast[((uint32_t)t << kFastBits) + p] = (uint16_t)e;
      }
      code <<= 1;
    }
  }
  io.sync();
}

// one lane's reader of one segment: the bits fetched and not yet used are the low `bc` bits of `bb`, the oldest on top
struct Bits {
  const uint8_t *p;
  uint32_t pos = 0, n;
  uint64_t bb = 0;
  uint32_t bc = 0;
  TM_JPG_HD Bits(const uint8_t *p_, uint32_t n_) : p(p_), n(n_) {}
  TM_JPG_HD void refill() {
    while (bc <= 56 && pos < n) {
      const uint32_t b = p[pos];
      if (b == 0xffu) {
        if (pos + 1 >= n || p[pos + 1] != 0) { n = pos; break; }  // not a stuffed byte: the data ends here
        pos += 2;
      } else pos++;
      bb = bb << 8 | b;
      bc += 8;
    }
  }
  // the next k bits, k <= 16: false when the segment has fewer left
  TM_JPG_HD bool take(uint32_t k, uint32_t *v) {
    if (bc < k) { refill(); if (bc < k) return false; }
    *v = (uint32_t)(bb >> (bc - k)) & ((1u << k) - 1u);
    bc -= k;
    return true;
  }
  // one symbol of table t: >= 0, or -kTruncated / -kBadCode.  It takes at least one bit or none at all.
  TM_JPG_HD int symbol(const TableSet &ts, const uint16_t *fast, uint32_t t) {
    if (bc < 16) refill();
    const uint32_t peek = bc >= (uint32_t)kFastBits ? (uint32_t)(bb >> (bc - kFastBits)) & ((1u << kFastBits) - 1u)
                                                     : ((uint32_t)bb << (kFastBits - bc)) & ((1u << kFastBits) - 1u);
    const uint32_t e = fast[(t << kFastBits) + peek];
    if (e) {
      if ((e & 255u) > bc) return -(int)kTruncated;  // (the code found leans on bits that are not there; no shorter one matched)
      bc -= e & 255u;
      return (int)(e >> 8);
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= 16; l++) {
      if (l > bc) return -(int)kTruncated;
      code = code << 1 | ((uint32_t)(bb >> (bc - l)) & 1u);
      const uint32_t cnt = ts.count[t][l - 1];
      if (code - first < cnt) {
        bc -= l;
        return (int)ts.symbol[t][(index + code - first) & 255u];
      }
      index += cnt;
      first = (first + cnt) << 1;
    }
    return -(int)kBadCode;
  }
};

// s bits as the value of category s (T.81 F.2.2.1's EXTEND); s >= 1
TM_JPG_HD inline int32_t extend(uint32_t v, uint32_t s) { return v < (1u << (s - 1)) ? (int32_t)v - (int32_t)(1u << s) + 1 : (int32_t)v; }

// One block's coefficients into `slot` (64 halves, zeroed here).  Every pass of the loop takes a symbol, which takes a bit or ends the
// block with a status, and moves k on by at least one: at most 63 passes.
TM_JPG_HD inline int decode_block(Bits &b, const TableSet &ts, const uint16_t *fast, uint32_t td, uint32_t ta, uint32_t *pred, int16_t *slot) {
  __builtin_memset(__builtin_assume_aligned(slot, 4), 0, 128);  // (a slot starts on four bytes)
  int t = b.symbol(ts, fast, td);
  if (t < 0) return -t;
  if (t > 11) return kBadMagnitude;
  if (t) {
    uint32_t v;
    if (!b.take((uint32_t)t, &v)) return kTruncated;
    *pred += (uint32_t)extend(v, (uint32_t)t);
  }
  slot[0] = (int16_t)(uint16_t)*pred;
  for (uint32_t k = 1; k < 64;) {
    const int rs = b.symbol(ts, fast, 4u + ta);
    if (rs < 0) return -rs;
    const uint32_t r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
    if (!s) {
      if (r != 15) break;  // end of block
      if (k + 15 > 63) return kBadRun;
      k += 16;
      continue;
    }
    if (s > 10) return kBadMagnitude;
    k += r;
    if (k > 63) return kBadRun;
    uint32_t v;
    if (!b.take(s, &v)) return kTruncated;
    slot[zigzag(k)] = (int16_t)extend(v, s);
    k++;
  }
  return kOk;
}

// ---- the islow inverse DCT: eight samples from eight inputs, descaled by `shift`
constexpr uint32_t kF0_298 = 2446, kF0_390 = 3196, kF0_541 = 4433, kF0_765 = 6270, kF0_899 = 7373, kF1_175 = 9633, kF1_501 = 12299, kF1_847 = 15137,
                   kF1_961 = 16069, kF2_053 = 16819, kF2_562 = 20995, kF3_072 = 25172;
TM_JPG_HD inline int32_t descale(uint32_t v, int shift) { return (int32_t)(v + (1u << (shift - 1))) >> shift; }
TM_JPG_HD inline void idct8(const uint32_t in[8], int shift, int32_t out[8]) {
  uint32_t z2 = in[2], z3 = in[6];
  uint32_t z1 = (z2 + z3) * kF0_541;
  uint32_t tmp2 = z1 - z3 * kF1_847, tmp3 = z1 + z2 * kF0_765;
  uint32_t tmp0 = (in[0] + in[4]) << 13, tmp1 = (in[0] - in[4]) << 13;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  uint32_t z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * kF1_175;
  tmp0 *= kF0_298; tmp1 *= kF2_053; tmp2 *= kF3_072; tmp3 *= kF1_501;
  z1 = 0u - z1 * kF0_899; z2 = 0u - z2 * kF2_562; z3 = 0u - z3 * kF1_961; z4 = 0u - z4 * kF0_390;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  out[0] = descale(tmp10 + tmp3, shift); out[7] = descale(tmp10 - tmp3, shift);
  out[1] = descale(tmp11 + tmp2, shift); out[6] = descale(tmp11 - tmp2, shift);
  out[2] = descale(tmp12 + tmp1, shift); out[5] = descale(tmp12 - tmp1, shift);
  out[3] = descale(tmp13 + tmp0, shift); out[4] = descale(tmp13 - tmp0, shift);
}

// the block in `slot` as samples at (x, y) of a plane, inside the extent w x h
TM_JPG_HD inline void block_to_plane(const int16_t *slot, const uint16_t *q, uint8_t *plane, uint32_t stride, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
  int32_t ws[64];  // (every index below is a constant once the loops are unrolled: registers)
#pragma unroll
  for (int c = 0; c < 8; c++) {
    uint32_t in[8];
    int32_t col[8];
#pragma unroll
    for (int r = 0; r < 8; r++) in[r] = (uint32_t)(int32_t)slot[8 * r + c] * (uint32_t)q[8 * r + c];
    idct8(in, 11, col);
#pragma unroll
    for (int r = 0; r < 8; r++) ws[8 * r + c] = col[r];
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {
    uint32_t in[8];
    int32_t row[8];
#pragma unroll
    for (int c = 0; c < 8; c++) in[c] = (uint32_t)ws[8 * r + c];
    idct8(in, 18, row);
    uint64_t packed = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int32_t v = row[c] + 128;
      packed |= (uint64_t)(uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * c);
    }
    if (y + (uint32_t)r >= h || x >= w) continue;
    uint8_t *to = plane + (uint64_t)(y + (uint32_t)r) * stride + x;
#if defined(__HIP_DEVICE_COMPILE__)
    if (x + 8 <= w && (reinterpret_cast<uintptr_t>(to) & 7u) == 0) { *reinterpret_cast<uint64_t *>(to) = packed; continue; }
#else
    if (x + 8 <= w) { memcpy(to, &packed, 8); continue; }
#endif
    for (uint32_t c = 0; c < w - x && c < 8; c++) to[c] = (uint8_t)(packed >> (8 * c));
  }
}

// Segment i of a frame.  The loops are bounded by the segment's MCUs (at most the frame's), an MCU's blocks (at most 6) and a block's 63
// passes; every symbol takes at least one of the segment's bits or ends the segment, so a segment of n bytes ends after at most 8 n
// symbols whatever its bytes are.
TM_JPG_HD inline int decode_segment(const Frame &f, const TableSet &ts, const uint16_t *fast, const uint8_t *data, uint32_t len, uint32_t i, int16_t *slot,
                                    uint8_t *const planes[3]) {
  const uint64_t m0 = (uint64_t)i * f.ri;
  if (m0 >= f.mcus_total) return kOk;  // (the walk refuses such a list: kBadRestart)
  const uint32_t m1 = (uint32_t)(m0 + f.ri < f.mcus_total ? m0 + f.ri : f.mcus_total);
  Bits bits(data, len);
  uint32_t pred0 = 0, pred1 = 0, pred2 = 0;  // the DC predictions (three names, not an array indexed by the component: registers)
  for (uint32_t m = (uint32_t)m0; m < m1; m++) {
    const uint32_t mx = m % f.mcus_x, my = m / f.mcus_x;
    for (uint32_t c = 0; c < f.ncomp; c++) {
      const uint32_t ch = c == 0 && f.ncomp == 3 ? f.hs : 1u, cv = c == 0 && f.ncomp == 3 ? f.vs : 1u;
      for (uint32_t v = 0; v < cv; v++)
        for (uint32_t h = 0; h < ch; h++) {
          uint32_t pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
          const int rc = decode_block(bits, ts, fast, f.td[c], f.ta[c], &pred, slot);
          if (rc != kOk) return rc;
          if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
          block_to_plane(slot, ts.q[f.tq[c]], planes[c] + f.plane_off[c], f.plane_stride[c], f.plane_w[c], f.plane_h[c], 8 * (mx * ch + h), 8 * (my * cv + v));
        }
    }
  }
  return kOk;
}

// One file: the look-ups, then its segments in rounds of the IO's lanes.  Returns the file's status (the same in every lane).
template <class IO>
TM_JPG_HD inline int decode_frame(IO &io, const Frame &f, const TableSet &ts, const Seg *segs, const uint8_t *blob, uint64_t blob_bytes, uint8_t *const planes[3]) {
  if (f.status0 != kOk) return f.status0;
  uint16_t *fast = io.fast();
  build_fast(io, ts, fast);
  uint32_t my_i = kNoRefusal;  // this lane's first refusing segment and its status
  int my_rc = kOk;
  for (uint32_t i0 = 0; i0 < f.seg_count; i0 += io.lanes()) {
    const uint32_t i = i0 + io.lane();
    if (i >= f.seg_count || i < i0) continue;
    const Seg sg = segs[f.seg_first + i];
    int rc = kBadDesc;
    if (sg.off <= blob_bytes && sg.len <= blob_bytes - sg.off) rc = decode_segment(f, ts, fast, blob + sg.off, sg.len, i, io.slot(), planes);
    if (rc != kOk && my_i == kNoRefusal) { my_i = i; my_rc = rc; }
  }
  if (my_i != kNoRefusal) io.refuse(my_i);
  io.sync();
  if (my_i != kNoRefusal && my_i == io.refusal()) io.set_status(my_rc);
  io.sync();
  return io.status();
}

// ---- the host side (tm_jpeg_in.hip): what the container walk leaves of a file, and a batch's descriptor as it is uploaded
struct JpegInfo {
  int w = 0, h = 0, ncomp = 0, hs = 1, vs = 1, sof = -1;  // hs x vs: the luma blocks of an MCU (1 x 1 for a single component)
  uint32_t ri = 0;                                         // DRI's interval, 0: none
  int status0 = kOk;                                       // kBadRestart: the segment list is not what ri and the size ask for
  uint8_t tq[4] = {0, 0, 0, 0}, td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0};
  TableSet ts;
  std::vector<Seg> segs;                                   // spans of the file; empty with kBadRestart
  uint32_t nsegs = 0;                                      // how many the walk found
  void plane_size(int c, int *pw, int *ph) const;          // ceil(w / hs) x ceil(h / vs) for chroma
  void mcus(uint32_t *across, uint32_t *down) const;
  int layout() const;                                      // TM_CHROMA_444 / _420JPEG / _MONO, or CHROMA_422_CENTRED (tm_input.h)
};
struct PlaneLayout { uint64_t off[3] = {0, 0, 0}; uint32_t stride[3] = {0, 0, 0}, w[3] = {0, 0, 0}, h[3] = {0, 0, 0}; };
int parse_jpeg(const uint8_t *file, size_t n, const char *name, JpegInfo *info);
int jpeg_status_error(int status, const char *name);  // a refused file's status as Load's error (TM_E_INVAL)
struct JpegBatch {
  std::vector<Frame> frames;
  std::vector<TableSet> tables;
  std::vector<Seg> segs;
  void clear();
  void add(const JpegInfo &info, uint64_t at, const PlaneLayout &pl);  // at: where the file starts in the blob
  size_t desc_bytes() const;
  size_t write_desc(uint8_t *to) const;
};
int jpeg_batch_launch(const JpegBatch &b, const uint8_t *dev_blob, size_t blob_bytes, size_t desc_off, uint8_t *y, uint8_t *u, uint8_t *v, const uint64_t plane_bytes[3],
                      int32_t *dev_status, void *hip_stream);
int jpeg_decode_one_host(const JpegInfo &info, const uint8_t *file, size_t n, const PlaneLayout &pl, uint8_t *const planes[3]);

}  // namespace jpg
}  // namespace tmx
