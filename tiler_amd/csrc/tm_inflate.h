// tm_inflate.h -- what the PNG reader's decoder is, stated once for its host form (tm_inflate_streams_host, tm_png_decode_host) and its
// device form (k_inflate, k_png_unfilter; both in tm_png_in.hip): DESIGN.md section 35.  Written from RFC 1950, RFC 1951 and the PNG
// specification.  The independent check is tm_png.hip's reader (tm_inflate_host, tm_read_png_host), which shares no line with this file.
//
// A stream is accepted exactly when that reader accepts it:
//   header    CM 8, CINFO <= 7, FCHECK; FDICT refused; at least 6 bytes.
//   stored    LEN / NLEN checked, a zero-length block allowed.
//   codes     canonical codes by their lengths.  An over-subscribed length set is refused when its table is built; an incomplete one is
//             accepted and refused only when the bits met are no assigned code.  Literal/length symbols 286, 287 and distance symbols
//             30, 31 are refused when met.  The code-length code's repeats (16, 17, 18) run across the boundary between the two tables.
//   window    a distance reaching before the start of the data is refused; so are output past `cap` and input running out.
//   trailer   the Adler-32 of the output on the next byte boundary.
// Every read is checked against the stream's own extent and every write against `cap` before it is made: a damaged stream ends with a
// status {code, input byte position, bytes written}, never with an access outside its buffers.
//
// The text below is written against an IO: where the input bytes come from (a list of spans: the IDAT payloads of a file are not joined),
// where output bytes go, and how many lanes run the text together.  The host IO is one lane writing to the destination.  The device IO is
// one wave: the decode state is the same in every lane, the tables, the 32 KiB window and a stage of input bytes live in LDS, a match is
// copied LDS to LDS by the whole wave, and finished output leaves in 16-byte stores.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tilemotion.h"

#if defined(__HIPCC__)
#define TM_INF_HD __host__ __device__
#else
#define TM_INF_HD
#endif

namespace tmx {
namespace inf {

// tm_inflate_status::code (TM_INF_*, include/tilemotion.h)
enum {
  kOk = TM_INF_OK, kTooShort = TM_INF_TOO_SHORT, kBadHeader = TM_INF_BAD_HEADER, kDict = TM_INF_DICT, kTruncated = TM_INF_TRUNCATED,
  kBlockType = TM_INF_BLOCK_TYPE, kStoredLen = TM_INF_STORED_LEN, kDynHeader = TM_INF_DYN_HEADER, kClCode = TM_INF_CL_CODE,
  kLengths = TM_INF_LENGTHS, kNoEob = TM_INF_NO_EOB, kOverSubscribed = TM_INF_OVER_SUBSCRIBED, kBadCode = TM_INF_BAD_CODE,
  kBadSymbol = TM_INF_BAD_SYMBOL, kDistance = TM_INF_DISTANCE, kOverflow = TM_INF_OVERFLOW, kNoChecksum = TM_INF_NO_CHECKSUM,
  kAdler = TM_INF_ADLER, kBadSpan = TM_INF_BAD_SPAN,
  // of a picture, behind its stream (tm_stage_png_decode, tm_png_decode_host)
  kPngSize = TM_PNG_BAD_SIZE, kPngFilter = TM_PNG_BAD_FILTER, kPngPalette = TM_PNG_BAD_INDEX,
};

constexpr uint32_t kWindow = 32768;
constexpr int kLitFastBits = 9, kDistFastBits = 6;  // codes up to this long are one table look-up; longer ones walk the counts
constexpr uint32_t kAdlerMod = 65521;

// The tables of one block, wherever the IO keeps them.  fast[]: symbol << 4 | length for every pattern of kFastBits stream bits that begins
// with a code of at most that length, 0 elsewhere.  count[l], symbol[]: the canonical code by lengths (symbols in code order).
struct Tables {
  uint16_t *lit_fast;    // [1 << kLitFastBits]
  uint16_t *dist_fast;   // [1 << kDistFastBits]
  uint16_t *lit_count;   // [16]
  uint16_t *lit_symbol;  // [288]
  uint16_t *dist_count;  // [16]
  uint16_t *dist_symbol; // [32]
  uint32_t *work;        // [32]: build_code's running offsets and codes per length
  uint8_t *lens;         // [320]
};
constexpr size_t kTableHalves = ((size_t)1 << kLitFastBits) + ((size_t)1 << kDistFastBits) + 16 + 288 + 16 + 32;  // the uint16_t entries

TM_INF_HD inline uint32_t len_base(uint32_t s) {  // s = symbol - 257, 0 .. 28
  return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3u)) << ((s >> 2) - 1));
}
TM_INF_HD inline uint32_t len_extra(uint32_t s) { return (s < 8 || s == 28) ? 0u : (s >> 2) - 1; }
TM_INF_HD inline uint32_t dist_base(uint32_t s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1u)) << ((s >> 1) - 1)); }  // s 0 .. 29
TM_INF_HD inline uint32_t dist_extra(uint32_t s) { return s < 4 ? 0u : (s >> 1) - 1; }

// Adler-32 over a run of `len` bytes from its sums: s1 = sum of the bytes, s2 = sum of (len - k) byte[k]
TM_INF_HD inline void adler_append(uint32_t *a, uint32_t *b, uint64_t s1, uint64_t s2, uint32_t len) {
  *b = (uint32_t)((*b + (uint64_t)len * *a + s2) % kAdlerMod);
  *a = (uint32_t)((*a + s1) % kAdlerMod);
}

// The canonical code of n lengths (each <= 15): false when over-subscribed.  Run by all lanes together; the table fill is shared out.
template <class IO>
TM_INF_HD inline bool build_code(IO &io, const uint8_t *len, int n, uint16_t *count, uint16_t *symbol, uint16_t *fast, int fast_bits, uint32_t *work) {
  for (int l = 0; l < 16; l++) count[l] = 0;
  for (int i = (int)io.lane(); i < (1 << fast_bits); i += (int)io.lanes()) fast[i] = 0;
  io.sync();
  for (int i = 0; i < n; i++) count[len[i]] = (uint16_t)(count[len[i]] + 1);
  io.sync();
  if (count[0] == n) return true;  // no codes: decoding with it fails, which is what an unused table may do
  int left = 1;
  for (int l = 1; l < 16; l++) {
    left = (left << 1) - (int)count[l];
    if (left < 0) return false;
  }
  uint32_t *offs = work, *next = work + 16;
  offs[1] = 0; next[1] = 0;
  for (int l = 1; l < 15; l++) { offs[l + 1] = offs[l] + count[l]; next[l + 1] = (next[l] + count[l]) << 1; }
  for (int i = 0; i < n; i++) {
    const int l = len[i];
    if (!l) continue;
    symbol[offs[l]++] = (uint16_t)i;
    const uint32_t code = next[l]++;
    if (l > fast_bits) continue;
    uint32_t rev = 0;
    for (int k = 0; k < l; k++) rev |= ((code >> k) & 1u) << (l - 1 - k);
    for (uint32_t t = rev + (io.lane() << l); t < (1u << fast_bits); t += io.lanes() << l) fast[t] = (uint16_t)((uint32_t)i << 4 | (uint32_t)l);
  }
  io.sync();
  return true;
}

template <class IO>
struct Decoder {
  IO &io;
  uint64_t bb = 0;    // the bits fetched and not yet used, lowest first
  uint32_t bc = 0;    // how many
  uint32_t ipos = 0;  // the next input byte to fetch
  uint32_t n;         // input bytes
  uint32_t out = 0;
  TM_INF_HD explicit Decoder(IO &io_) : io(io_), n(io_.in_size()) {}

  TM_INF_HD void refill() {
    while (bc <= 56 && ipos < n) { bb |= (uint64_t)io.in_byte(ipos++) << bc; bc += 8; }
  }
  TM_INF_HD bool take(uint32_t k, uint32_t *v) {  // k <= 16
    if (bc < k) { refill(); if (bc < k) return false; }
    *v = (uint32_t)bb & ((1u << k) - 1u);
    bb >>= k; bc -= k;
    return true;
  }
  TM_INF_HD uint32_t used_bytes() const { return ipos - bc / 8; }  // input bytes begun
  // one symbol of a code: >= 0, or -kTruncated / -kBadCode
  TM_INF_HD int symbol(const uint16_t *fast, int fast_bits, const uint16_t *count, const uint16_t *sym) {
    if (bc < 15) refill();
    const uint32_t peek = (uint32_t)bb & 0x7fffu;  // (bits past the end of the input read as 0 and are never consumed)
    const uint32_t e = fast[peek & ((1u << fast_bits) - 1u)];
    uint32_t l = e & 15u;
    int s = (int)(e >> 4);
    if (!e) {
      int code = 0, first = 0, index = 0;
      s = -1;
      for (l = 1; l < 16; l++) {
        code |= (int)((peek >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - c < first) { s = sym[index + (code - first)]; break; }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
      }
      if (s < 0) return bc < 15 ? -(int)kTruncated : -(int)kBadCode;
    }
    if (l > bc) return -(int)kTruncated;
    bb >>= l; bc -= l;
    return s;
  }

  TM_INF_HD int codes(const Tables &t) {
    const uint32_t cap = io.cap();
    for (;;) {
      io.flush_some(out);
      const int s = symbol(t.lit_fast, kLitFastBits, t.lit_count, t.lit_symbol);
      if (s < 0) return -s;
      if (s < 256) {
        if (out >= cap) return kOverflow;
        io.put(out++, (uint32_t)s);
      } else if (s == 256) {
        return kOk;
      } else {
        if (s >= 286) return kBadSymbol;
        uint32_t ev = 0, dv = 0;
        if (!take(len_extra((uint32_t)s - 257), &ev)) return kTruncated;
        const uint32_t len = len_base((uint32_t)s - 257) + ev;
        const int ds = symbol(t.dist_fast, kDistFastBits, t.dist_count, t.dist_symbol);
        if (ds < 0) return -ds;
        if (ds >= 30) return kBadSymbol;
        if (!take(dist_extra((uint32_t)ds), &dv)) return kTruncated;
        const uint32_t d = dist_base((uint32_t)ds) + dv;
        if (d > out) return kDistance;
        if (len > cap - out) return kOverflow;
        io.copy(out, d, len);
        out += len;
      }
    }
  }

  TM_INF_HD int run(uint32_t *adler_out) {
    const uint32_t cap = io.cap();
    const Tables t = io.tables();
    if (n < 6) return kTooShort;
    const uint32_t h0 = io.in_byte(0), h1 = io.in_byte(1);
    ipos = 2;
    if ((h0 & 0x0fu) != 8 || (h0 >> 4) > 7 || ((h0 << 8) | h1) % 31 != 0) return kBadHeader;
    if (h1 & 0x20u) return kDict;
    for (uint32_t last = 0; !last;) {
      uint32_t type = 0;
      if (!take(1, &last) || !take(2, &type)) return kTruncated;
      if (type == 0) {
        ipos = used_bytes(); bb = 0; bc = 0;  // to the byte boundary
        if (n - ipos < 4) return kTruncated;
        const uint32_t len = io.in_byte(ipos) | io.in_byte(ipos + 1) << 8, nlen = io.in_byte(ipos + 2) | io.in_byte(ipos + 3) << 8;
        ipos += 4;
        if ((len ^ 0xffffu) != nlen) return kStoredLen;
        if (len > n - ipos) return kTruncated;
        if (len > cap - out) return kOverflow;
        for (uint32_t k = 0; k < len;) {  // in pieces the window can hold unflushed
          const uint32_t piece = len - k < 4096u ? len - k : 4096u;
          io.flush_some(out);
          io.put_input(out, ipos, piece);
          out += piece; ipos += piece; k += piece;
        }
      } else if (type == 1) {
        for (int i = (int)io.lane(); i < 320; i += (int)io.lanes()) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
        io.sync();
        build_code(io, t.lens, 288, t.lit_count, t.lit_symbol, t.lit_fast, kLitFastBits, t.work);
        build_code(io, t.lens + 288, 30, t.dist_count, t.dist_symbol, t.dist_fast, kDistFastBits, t.work);
        const int rc = codes(t);
        if (rc) return rc;
      } else if (type == 2) {
        uint32_t a = 0, b = 0, c = 0;
        if (!take(5, &a) || !take(5, &b) || !take(4, &c)) return kTruncated;
        const int nlen = (int)a + 257, ndist = (int)b + 1, ncode = (int)c + 4;
        if (nlen > 286 || ndist > 30) return kDynHeader;
        for (int i = (int)io.lane(); i < 320; i += (int)io.lanes()) t.lens[i] = 0;
        io.sync();
        for (int i = 0; i < ncode; i++) {
          uint32_t v = 0;
          if (!take(3, &v)) return kTruncated;
          const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
          t.lens[at] = (uint8_t)v;
        }
        io.sync();
        // the code-length code borrows the distance code's tables; its lengths are then cleared for the two codes' own
        if (!build_code(io, t.lens, 19, t.dist_count, t.dist_symbol, t.dist_fast, kDistFastBits, t.work)) return kClCode;
        for (int i = (int)io.lane(); i < 320; i += (int)io.lanes()) t.lens[i] = 0;
        io.sync();
        for (int i = 0; i < nlen + ndist;) {
          const int s = symbol(t.dist_fast, kDistFastBits, t.dist_count, t.dist_symbol);
          if (s < 0) return -s;
          if (s < 16) { t.lens[i++] = (uint8_t)s; continue; }
          uint32_t rep = 0, val = 0;
          if (s == 16) {
            if (i == 0) return kLengths;
            io.sync();
            val = t.lens[i - 1];
            if (!take(2, &rep)) return kTruncated;
            rep += 3;
          } else if (s == 17) {
            if (!take(3, &rep)) return kTruncated;
            rep += 3;
          } else {
            if (!take(7, &rep)) return kTruncated;
            rep += 11;
          }
          if (i + (int)rep > nlen + ndist) return kLengths;
          while (rep--) t.lens[i++] = (uint8_t)val;
        }
        io.sync();
        if (t.lens[256] == 0) return kNoEob;
        if (!build_code(io, t.lens, nlen, t.lit_count, t.lit_symbol, t.lit_fast, kLitFastBits, t.work)) return kOverSubscribed;
        if (!build_code(io, t.lens + nlen, ndist, t.dist_count, t.dist_symbol, t.dist_fast, kDistFastBits, t.work)) return kOverSubscribed;
        const int rc = codes(t);
        if (rc) return rc;
      } else {
        return kBlockType;
      }
    }
    const uint32_t tail = used_bytes();
    if (n - tail < 4) return kNoChecksum;
    const uint32_t want = io.in_byte(tail) << 24 | io.in_byte(tail + 1) << 16 | io.in_byte(tail + 2) << 8 | io.in_byte(tail + 3);
    ipos = tail + 4; bb = 0; bc = 0;
    const uint32_t got = io.finish(out);
    *adler_out = got;
    return got == want ? kOk : kAdler;
  }
};

// One stream through an IO.  A refused stream leaves whatever had been decoded and flushed up to the refusal, and reports 0 bytes.
template <class IO>
TM_INF_HD inline void inflate_stream(IO &io, tm_inflate_status *st) {
  Decoder<IO> d(io);
  uint32_t adler = 1;
  const int rc = d.run(&adler);
  st->code = rc;
  st->in_pos = d.used_bytes();
  st->out_n = rc == kOk ? d.out : 0;
}

// ---- the rows of a picture (PNG specification, 9.2).  x: the filtered byte, a: bpp to the left, b: above, c: above and bpp to the left
TM_INF_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
TM_INF_HD inline uint32_t unfilter_byte(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  switch (type) {
    case 1: return (x + a) & 0xffu;
    case 2: return (x + b) & 0xffu;
    case 3: return (x + ((a + b) >> 1)) & 0xffu;
    case 4: return (x + paeth(a, b, c)) & 0xffu;
    default: return x;
  }
}
TM_INF_HD inline int png_bpp(int ctype) { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4; }
// One pixel of `bpp` bytes packed lowest byte first, a, b, c alike: the unfiltered pixel
TM_INF_HD inline uint32_t unfilter_pixel(uint32_t type, int bpp, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0;
  for (int k = 0; k < bpp; k++) {
    const int sh = 8 * k;
    r |= unfilter_byte(type, (x >> sh) & 0xffu, (a >> sh) & 0xffu, (b >> sh) & 0xffu, (c >> sh) & 0xffu) << sh;
  }
  return r;
}
// The 0x00RRGGBB of an unfiltered pixel: grey replicated, alpha dropped, a palette index looked up.  false: the index is beyond PLTE.
// pal: npal entries of 0x00RRGGBB
TM_INF_HD inline bool png_rgb32(int ctype, uint32_t px, const uint32_t *pal, int npal, uint32_t *out) {
  const uint32_t s0 = px & 0xffu;
  if (ctype == 0 || ctype == 4) { *out = s0 * 0x010101u; return true; }
  if (ctype == 3) {
    if ((int)s0 >= npal) { *out = 0; return false; }
    *out = pal[s0];
    return true;
  }
  *out = s0 << 16 | (px & 0xff00u) | ((px >> 16) & 0xffu);
  return true;
}
// What a picture's first refusal is called: the rows are judged top to bottom, a row's filter type before its pixels
TM_INF_HD inline uint32_t row_fault_key(uint32_t row, bool palette) { return row << 1 | (palette ? 1u : 0u); }
constexpr uint32_t kNoRowFault = 0xffffffffu;

// ---- what the kernels and the host twins are handed (plain data, uploaded as it is; offsets below 4 GiB: a batch is one blob)
struct Span { uint32_t off, len; };  // bytes [off, off + len) of the blob
struct Stream {                      // tm_inflate_stream's layout
  uint64_t dst_off;
  uint32_t dst_cap, first_span, span_count, pad;
};
struct Picture {  // one file of a batch: colour type, PLTE entries and where they start in the batch's table of (R, G, B) bytes
  uint32_t ctype, npal, pal_off, pad;
};

// ---- tm_png_in.hip: the host side of the device form
struct PngInfo {  // what the container walk leaves of a file
  int w = 0, h = 0, ctype = -1, npal = 0;
  uint8_t pal3[768];
  std::vector<Span> idat;  // the IDAT payloads, as spans of the file
};
// decode_png's walk (tm_png.hip) with its refusals and codes: signature, chunk extents, CRCs, IHDR, PLTE, unknown critical chunks
int parse_png(const uint8_t *file, size_t n, const char *name, PngInfo *info);
// what lies between the walk and the stream: the sequence's size, a palette picture without PLTE
int png_check_decodable(const PngInfo &info, const char *name, int w, int h);
// TM_OK, or TM_E_INVAL with the error set, for a file's status
int png_status_error(int status, const char *name);
// The descriptors of a batch of files that lie in one blob: file i's bytes start at the offset it was added with.
struct PngBatch {
  std::vector<Span> spans;
  std::vector<Stream> streams;  // dst_off: where the file's rows go in the batch's scratch
  std::vector<Picture> pics;
  std::vector<uint8_t> pal3;
  uint64_t raw_bytes = 0;       // the scratch the batch's inflated rows take: h (1 + row bytes) per file, rounded up to 16
  void clear();
  void add(const PngInfo &info, uint64_t at);
  size_t desc_bytes() const;               // an upper bound of what write_desc writes
  size_t write_desc(uint8_t *to) const;    // streams | pictures | spans | palettes
};
// k_inflate and k_png_unfilter on a batch whose files and descriptor (at desc_off, a multiple of 8) lie in dev_blob; queued on the stream
int png_batch_launch(const PngBatch &b, const uint8_t *dev_blob, size_t blob_bytes, size_t desc_off, uint8_t *dev_raw, tm_inflate_status *dev_inflated, int w, int h,
                     uint32_t *dev_out, int64_t frame_px, int32_t *dev_status, void *hip_stream);

}  // namespace inf
}  // namespace tmx
