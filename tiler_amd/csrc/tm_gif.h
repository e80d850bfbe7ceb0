// tm_gif.h -- what the GIF reader is, stated once for its host form (tm_gif_lzw_streams_host, tm_gif_decode_host) and its device form
// (k_gif_lzw, k_gif_compose; both in tm_gif_in.hip): DESIGN.md section 42.  Written from the GIF89a specification.  The independent check
// is the tests' plain-Python restatement (tests/gif_ref.py) and Pillow.
//
//   data      the image data is a chain of sub-blocks inside the stream's span: a length byte L, then L bytes; L = 0 ends the data, and so
//             does the end of the span, wherever it falls (a sub-block that the span cuts gives the bytes the span holds).
//   codes     LSB first, min + 1 bits at the start; clear = 1 << min, eoi = clear + 1, the first free entry is clear + 2; the width grows
//             when the next free entry reaches 1 << width, up to 12; a full table goes on at 12 bits and adds nothing (deferred clear).
//             A clear resets table and width; the code behind a clear (or the first code: a missing initial clear is accepted) must be
//             a literal and adds no entry.
//   strings   every string the table gains is the previous string plus the first byte of the current one, and the previous string was just
//             written at output position pp with length pl: the new entry is bytes [pp, pp + pl] of the output.  An entry is (pos, len);
//             expanding a code is a copy out of earlier output, and for code == next free entry the source runs into the bytes being
//             written (period pl).
//   end       decoding stops as soon as npix indices are out; eoi is not required and what follows is not looked at.
//   status    kTruncated: the data or an eoi ends it early; kBadCode: a code above the next free entry, or a non-literal behind a clear.
//             {code, payload bytes taken (whole bytes of the codes read), indices written}.
//
// The text is written against an IO: where the span's bytes come from, where indices go, how many lanes run the text together.  The host
// IO is one lane.  The device IO is one wave with the same state in every lane: the table and a stage of payload bytes live in LDS, a
// string is copied by the whole wave out of the image's own earlier output in memory.
//
// The frames: dispose_pixel, index_at and draw_pixel are one canvas pixel's step from frame i - 1 to frame i (disposal of the frame
// before, then the new rectangle), the same text for the host loop and for k_gif_compose.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/tilemotion.h"

#if defined(__HIPCC__)
#define TM_GIF_HD __host__ __device__
#else
#define TM_GIF_HD
#endif

namespace tmx {
namespace gif {

enum { kOk = 0, kTruncated = TM_GIF_TRUNCATED, kBadCode = TM_GIF_BAD_CODE, kBadDesc = TM_GIF_BAD_DESC };

constexpr uint32_t kTableSize = 4096;
constexpr uint32_t kNone = 0xffffffffu;

// ---- the sub-block chain of a span of `src_bytes` bytes: pos is where the next unread byte of the span lies, left the payload bytes the
// current sub-block still holds
struct Chain {
  uint32_t pos = 0, left = 0;
  bool ended = false;
};
// the next run of at most `want` payload bytes: [*at, *at + *n) of the span with n >= 1, or false when the data has ended.
// byte_at(p) is the span's byte p, p < src_bytes.
template <class ByteAt>
TM_GIF_HD inline bool chain_next_run(Chain &c, uint32_t src_bytes, ByteAt byte_at, uint32_t want, uint32_t *at, uint32_t *n) {
  if (c.ended) return false;
  if (c.left == 0) {
    if (c.pos >= src_bytes) { c.ended = true; return false; }
    const uint32_t len = byte_at(c.pos);
    c.pos++;
    const uint32_t room = src_bytes - c.pos;
    c.left = len < room ? len : room;
    if (c.left == 0) { c.ended = true; return false; }
  }
  *at = c.pos;
  *n = want < c.left ? want : c.left;
  c.pos += *n; c.left -= *n;
  return true;
}

// ---- LZW.  IO: bool next_byte(uint32_t *b) (the payload's next byte; false when the data has ended), void entry_set(i, pos, len), void entry_get(i, &pos, &len), void put(out, v), void copy(out, src, len, period) (bytes
// [out, out + len) become bytes src + (k < period ? k : k - period) of the output; len <= period + 1, src + period <= out), void finish(out).
template <class IO>
TM_GIF_HD inline void lzw_stream(IO &io, uint32_t min_code, uint32_t npix, tm_gif_status *st) {
  const uint32_t clear = 1u << min_code, eoi = clear + 1;
  uint32_t next = clear + 2, width = min_code + 1;
  uint32_t pp = kNone, pl = 0;  // the previous string: where it was written and its length; kNone: behind a clear
  uint32_t out = 0, nbits = 0;
  uint64_t bits_used = 0;
  uint64_t acc = 0;
  int rc = kOk;
  while (out < npix) {
    while (nbits < width) {
      uint32_t b;
      if (!io.next_byte(&b)) break;
      acc |= (uint64_t)b << nbits;
      nbits += 8;
    }
    if (nbits < width) { rc = kTruncated; break; }
    const uint32_t code = (uint32_t)acc & ((1u << width) - 1u);
    acc >>= width; nbits -= width; bits_used += width;
    if (code == clear) { next = clear + 2; width = min_code + 1; pp = kNone; continue; }
    if (code == eoi) { rc = kTruncated; break; }
    if (pp == kNone) {
      if (code > clear) { rc = kBadCode; break; }
      io.put(out, code);
      pp = out; pl = 1; out += 1;
      continue;
    }
    if (code > next || (code == next && next >= kTableSize)) { rc = kBadCode; break; }
    uint32_t len;
    const uint32_t room = npix - out;
    if (code < clear) {
      len = 1;
      io.put(out, code);
    } else {
      uint32_t src, period;
      if (code < next) { io.entry_get(code, &src, &len); period = len; }
      else { src = pp; len = pl + 1; period = pl; }
      io.copy(out, src, len < room ? len : room, period);
    }
    if (next < kTableSize) {
      io.entry_set(next, pp, pl + 1);
      next++;
      if (next == (1u << width) && width < 12) width++;
    }
    pp = out; pl = len;
    out += len < room ? len : room;
  }
  io.finish(out);
  st->code = rc;
  st->in_pos = (uint32_t)((bits_used + 7) / 8);
  st->out_n = out;
}

// ---- frames
// picture row -> stored row of an interlaced image of h rows: rows 0, 8, ... come first, then 4, 12, ..., then 2, 6, ..., then 1, 3, ...
TM_GIF_HD inline uint32_t row_map(uint32_t y, uint32_t h, bool interlaced) {
  if (!interlaced) return y;
  const uint32_t n1 = (h + 7) / 8, n2 = (h + 3) / 8, n3 = (h + 1) / 4;
  if ((y & 7u) == 0) return y >> 3;
  if ((y & 7u) == 4) return n1 + (y >> 3);
  if ((y & 3u) == 2) return n1 + n2 + (y >> 2);
  return n1 + n2 + n3 + (y >> 1);
}

// one image as the compositor takes it (uploaded as it is)
struct FrameDesc {
  int32_t left, top, w, h;
  int32_t disposal, transparent /* -1: none */, interlaced, table_n;
  uint32_t table_off;  // the first of table_n colours (0x00RRGGBB) in the chunk's colour array
  int32_t stream;      // the image's LZW stream in the chunk (its status decides whether the frame is drawn), or -1: descriptor of the frame before the chunk
  uint64_t idx_off;    // where its stored indices start in the chunk's index buffer
  int64_t slot;        // the delivered frame it becomes (frames of frame_px pixels from `out`), or -1: composited, not delivered
};

TM_GIF_HD inline bool in_rect(const FrameDesc &f, int x, int y) { return x >= f.left && x - f.left < f.w && y >= f.top && y - f.top < f.h; }

// the disposal of the frame before, at pixel (x, y)
TM_GIF_HD inline uint32_t dispose_pixel(uint32_t canvas, uint32_t saved, const FrameDesc &prev, int x, int y, uint32_t bg) {
  if (!in_rect(prev, x, y)) return canvas;
  return prev.disposal == 2 ? bg : prev.disposal == 3 ? saved : canvas;
}
// where pixel (x, y) of the canvas reads its index in frame f's stored rows; in_rect(f, x, y)
TM_GIF_HD inline uint64_t index_at(const FrameDesc &f, int x, int y) {
  return f.idx_off + (uint64_t)row_map((uint32_t)(y - f.top), (uint32_t)f.h, f.interlaced != 0) * (uint32_t)f.w + (uint32_t)(x - f.left);
}
// the new rectangle's pixel drawn over the canvas
TM_GIF_HD inline uint32_t draw_pixel(uint32_t canvas, const FrameDesc &f, uint32_t idx, const uint32_t *colours) {
  if ((int32_t)idx == f.transparent) return canvas;
  return idx < (uint32_t)f.table_n ? colours[f.table_off + idx] : 0u;
}

// ---- the container walk (host; tm_gif_in.hip)
struct Image {
  int32_t left, top, w, h, delay, disposal, transparent, interlaced, min_code, local;
  uint32_t table_off, table_n;   // the colours that apply, in GifInfo::colours
  uint64_t data_off, data_bytes;  // the sub-block chain in the file, terminator included
};
struct GifInfo {
  int32_t w = 0, h = 0, version = 0, loop = -1, global_n = 0, bg_index = 0, uniform_delay = 1;
  uint32_t bg = 0;
  double fps = 0;
  std::vector<Image> images;
  std::vector<uint32_t> colours;  // the global table first, then every local one
};
int parse_gif(const uint8_t *file, size_t n, const char *name, GifInfo *info);
int gif_status_error(int status, const char *name, int image);
// frames [first, first + count) of the file on the device into dev_out (tm_stage_gif_decode and Load's device path): the file goes up
// once, then chunk by chunk a descriptor, k_gif_lzw and k_gif_compose.  status: first + count (host).  chunk_frames <= 0: what 1 GiB of
// stored indices holds.  bytes_uploaded: added to, when not null.
int gif_decode_device(const uint8_t *file, size_t size, const GifInfo &info, int first, int count, uint32_t bg, uint32_t *dev_out, int64_t frame_px, int32_t *status,
                      int chunk_frames, void *hip_stream, int64_t *bytes_uploaded);
// the same on the host, the LZW of a chunk's images on `threads` threads (tm_gif_decode_host: 1)
int gif_decode_host(const uint8_t *file, size_t size, const GifInfo &info, int first, int count, uint32_t bg, uint32_t *out, int64_t frame_px, int32_t *status, int threads);
inline uint32_t gif_background(const GifInfo &info, int background) { return background >= 0 ? (uint32_t)background & 0xffffffu : info.bg; }

}  // namespace gif
}  // namespace tmx
