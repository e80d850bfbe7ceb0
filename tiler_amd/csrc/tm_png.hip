// tm_png.hip -- host only: the PNG reader behind a numbered PNG sequence (LoadInputVideo, tilingencoder.pas:3340-3353) and the inflate it
// needs.  Like the LZMA coder of tm_lzma.hip and the PNG writer of tm_deflate.hip it links nothing: stored, fixed and dynamic Huffman
// blocks (RFC 1951), the zlib wrapper with its Adler-32 (RFC 1950), chunk CRCs and the five row filters (PNG 1.2, sections 3, 6).
// Every read is checked against the end of its buffer; a stream that is cut short or damaged is refused, never followed.
#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

namespace {

struct BitReader {
  const uint8_t *p;
  size_t n, pos = 0;
  uint32_t buf = 0;
  int cnt = 0;
  bool bad = false;
  uint32_t bits(int k) {  // k <= 16, least significant bit first
    while (cnt < k) {
      if (pos >= n) { bad = true; return 0; }
      buf |= (uint32_t)p[pos++] << cnt;
      cnt += 8;
    }
    const uint32_t v = buf & ((1u << k) - 1u);
    buf >>= k;
    cnt -= k;
    return v;
  }
};

struct Huffman {  // canonical code by lengths: count[len] codes of every length, symbols in code order
  uint16_t count[16], symbol[288];
  bool build(const uint8_t *len, int n) {
    memset(count, 0, sizeof(count));
    for (int i = 0; i < n; i++) count[len[i]]++;
    if (count[0] == n) return true;  // no codes: decoding with it fails, which is what an unused table may do
    int left = 1;
    for (int l = 1; l < 16; l++) {
      left = (left << 1) - count[l];
      if (left < 0) return false;  // over-subscribed
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int i = 0; i < n; i++)
      if (len[i]) symbol[offs[len[i]]++] = (uint16_t)i;
    return true;
  }
  int decode(BitReader &br) const {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
      code |= (int)br.bits(1);
      if (br.bad) return -1;
      const int c = count[l];
      if (code - c < first) return symbol[index + (code - first)];
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    return -1;
  }
};

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

int inflate_codes(BitReader &br, const Huffman &lit, const Huffman &dist, uint8_t *dst, size_t cap, size_t &out) {
  for (;;) {
    const int sym = lit.decode(br);
    TM_CHECK(sym >= 0, TM_E_INVAL, "inflate: bad literal/length code or truncated stream");
    if (sym < 256) {
      TM_CHECK(out < cap, TM_E_INVAL, "inflate: the data does not fit the buffer");
      dst[out++] = (uint8_t)sym;
    } else if (sym == 256) {
      return TM_OK;
    } else {
      TM_CHECK(sym < 286, TM_E_INVAL, "inflate: bad length symbol %d", sym);
      const int len = kLenBase[sym - 257] + (int)br.bits(kLenExtra[sym - 257]);
      const int ds = dist.decode(br);
      TM_CHECK(ds >= 0 && ds < 30, TM_E_INVAL, "inflate: bad distance code or truncated stream");
      const size_t d = kDistBase[ds] + (size_t)br.bits(kDistExtra[ds]);
      TM_CHECK(!br.bad, TM_E_INVAL, "inflate: truncated stream");
      TM_CHECK(d <= out, TM_E_INVAL, "inflate: a match reaches before the start of the data");
      TM_CHECK(out + (size_t)len <= cap, TM_E_INVAL, "inflate: the data does not fit the buffer");
      for (int i = 0; i < len; i++, out++) dst[out] = dst[out - d];  // (overlapping on purpose)
    }
  }
}

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

}  // namespace

// the CRC of PNG chunks (and of zip, gzip: polynomial 0xEDB88320), for the reader here and the writer in tm_deflate.hip
uint32_t crc32_ieee(const uint8_t *p, size_t n) {
  struct Table { uint32_t v[256]; };
  static const Table tb = [] {
    Table t;
    for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; t.v[i] = c; }
    return t;
  }();
  const uint32_t *table = tb.v;
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}
// a zlib stream (RFC 1950) into dst; *out_n = bytes written.  TM_E_INVAL: damaged, cut short, a preset dictionary, or more than cap bytes
int inflate_zlib(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n) {
  *out_n = 0;
  TM_CHECK(n >= 6, TM_E_INVAL, "inflate: %zu bytes are no zlib stream", n);
  TM_CHECK((src[0] & 0x0f) == 8 && (src[0] >> 4) <= 7 && (((unsigned)src[0] << 8) | src[1]) % 31 == 0, TM_E_INVAL, "inflate: bad zlib header");
  TM_CHECK(!(src[1] & 0x20), TM_E_INVAL, "inflate: preset dictionary");
  BitReader br{src + 2, n - 2};
  size_t out = 0;
  for (int last = 0; !last;) {
    last = (int)br.bits(1);
    const int type = (int)br.bits(2);
    TM_CHECK(!br.bad, TM_E_INVAL, "inflate: truncated stream");
    if (type == 0) {
      br.buf = 0; br.cnt = 0;  // to the byte boundary
      TM_CHECK(br.pos + 4 <= br.n, TM_E_INVAL, "inflate: truncated stored block");
      const unsigned len = br.p[br.pos] | br.p[br.pos + 1] << 8, nlen = br.p[br.pos + 2] | br.p[br.pos + 3] << 8;
      br.pos += 4;
      TM_CHECK((len ^ 0xffffu) == nlen, TM_E_INVAL, "inflate: stored block length check failed");
      TM_CHECK(br.pos + len <= br.n, TM_E_INVAL, "inflate: truncated stored block");
      TM_CHECK(out + len <= cap, TM_E_INVAL, "inflate: the data does not fit the buffer");
      memcpy(dst + out, br.p + br.pos, len);
      br.pos += len;
      out += len;
    } else if (type == 1) {
      struct Fixed { Huffman lit, dist; };
      static const Fixed fx = [] {  // (initialised once, also under several shards' threads)
        Fixed f;
        uint8_t l[288], d[30];
        for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        for (int i = 0; i < 30; i++) d[i] = 5;
        f.lit.build(l, 288); f.dist.build(d, 30);
        return f;
      }();
      const Huffman &lit = fx.lit, &dist = fx.dist;
      TM_TRY(inflate_codes(br, lit, dist, dst, cap, out));
    } else if (type == 2) {
      const int nlen = (int)br.bits(5) + 257, ndist = (int)br.bits(5) + 1, ncode = (int)br.bits(4) + 4;
      TM_CHECK(!br.bad && nlen <= 286 && ndist <= 30, TM_E_INVAL, "inflate: bad dynamic block header");
      static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      uint8_t lens[320];
      memset(lens, 0, sizeof(lens));
      for (int i = 0; i < ncode; i++) lens[order[i]] = (uint8_t)br.bits(3);
      Huffman cl;
      TM_CHECK(!br.bad && cl.build(lens, 19), TM_E_INVAL, "inflate: bad code-length code");
      memset(lens, 0, sizeof(lens));
      for (int i = 0; i < nlen + ndist;) {
        const int sym = cl.decode(br);
        TM_CHECK(sym >= 0, TM_E_INVAL, "inflate: bad code length or truncated stream");
        if (sym < 16) { lens[i++] = (uint8_t)sym; continue; }
        int rep, val = 0;
        if (sym == 16) { TM_CHECK(i > 0, TM_E_INVAL, "inflate: repeat without a length before it"); val = lens[i - 1]; rep = 3 + (int)br.bits(2); }
        else if (sym == 17) rep = 3 + (int)br.bits(3);
        else rep = 11 + (int)br.bits(7);
        TM_CHECK(!br.bad && i + rep <= nlen + ndist, TM_E_INVAL, "inflate: code lengths run past their table");
        while (rep--) lens[i++] = (uint8_t)val;
      }
      TM_CHECK(lens[256] != 0, TM_E_INVAL, "inflate: no end-of-block code");
      Huffman lit, dist;
      TM_CHECK(lit.build(lens, nlen) && dist.build(lens + nlen, ndist), TM_E_INVAL, "inflate: over-subscribed code");
      TM_TRY(inflate_codes(br, lit, dist, dst, cap, out));
    } else {
      set_error("inflate: reserved block type");
      return TM_E_INVAL;
    }
  }
  // the Adler-32 of the data follows on the next byte boundary
  size_t tail = br.pos - (size_t)(br.cnt / 8);
  TM_CHECK(tail + 4 <= br.n, TM_E_INVAL, "inflate: the checksum is missing");
  uint32_t a = 1, b = 0;
  for (size_t i = 0; i < out;) {
    const size_t stop = std::min(out, i + 5552);  // (the longest run whose sums fit 32 bits)
    for (; i < stop; i++) { a += dst[i]; b += a; }
    a %= 65521u; b %= 65521u;
  }
  TM_CHECK(be32(br.p + tail) == ((b << 16) | a), TM_E_INVAL, "inflate: Adler-32 mismatch");
  *out_n = out;
  return TM_OK;
}

// a PNG file's bytes -> 0x00RRGGBB pixels.  out may be null (size only).  Non-interlaced, 8 bits per sample: grey, grey + alpha, RGB, RGBA,
// palette; alpha is dropped.
int decode_png(const uint8_t *file, size_t n, const char *name, uint32_t *out, int64_t cap_px, int *w_out, int *h_out) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  TM_CHECK(n >= 8 + 25 && !memcmp(file, sig, 8), TM_E_UNSUPPORTED, "%s is not a PNG file", name);
  size_t pos = 8;
  int w = 0, h = 0, ctype = -1;
  uint8_t pal[256][3];
  int npal = 0;
  std::vector<uint8_t> z;
  bool end = false;
  while (!end) {
    TM_CHECK(pos + 12 <= n, TM_E_INVAL, "%s: truncated (no IEND chunk)", name);
    const size_t len = be32(file + pos);
    TM_CHECK(len <= n - pos - 12, TM_E_INVAL, "%s: a chunk runs past the end of the file", name);
    const uint8_t *type = file + pos + 4, *data = file + pos + 8;
    TM_CHECK(crc32_ieee(type, len + 4) == be32(data + len), TM_E_INVAL, "%s: CRC mismatch in chunk %.4s", name, (const char *)type);
    if (pos == 8) TM_CHECK(!memcmp(type, "IHDR", 4) && len == 13, TM_E_INVAL, "%s: the first chunk is not IHDR", name);
    if (!memcmp(type, "IHDR", 4)) {
      TM_CHECK(pos == 8, TM_E_INVAL, "%s: a second IHDR", name);
      const uint32_t ww = be32(data), hh = be32(data + 4);
      TM_CHECK(ww > 0 && hh > 0 && ww <= 65536 && hh <= 65536, TM_E_INVAL, "%s: bad size %ux%u", name, ww, hh);
      w = (int)ww; h = (int)hh; ctype = data[9];
      TM_CHECK(data[8] == 8, TM_E_UNSUPPORTED, "%s: %d bits per sample (8 only)", name, data[8]);
      TM_CHECK(ctype == 0 || ctype == 2 || ctype == 3 || ctype == 4 || ctype == 6, TM_E_INVAL, "%s: bad colour type %d", name, ctype);
      TM_CHECK(data[10] == 0 && data[11] == 0, TM_E_INVAL, "%s: unknown compression or filter method", name);
      TM_CHECK(data[12] == 0, TM_E_UNSUPPORTED, "%s: interlaced (Adam7) images are not read", name);
    } else if (!memcmp(type, "PLTE", 4)) {
      TM_CHECK(len % 3 == 0 && len <= 768, TM_E_INVAL, "%s: bad PLTE chunk", name);
      npal = (int)(len / 3);
      memcpy(pal, data, len);
    } else if (!memcmp(type, "IDAT", 4)) {
      z.insert(z.end(), data, data + len);
    } else if (!memcmp(type, "IEND", 4)) {
      end = true;
    } else {
      TM_CHECK(type[0] & 0x20, TM_E_UNSUPPORTED, "%s: unknown critical chunk %.4s", name, (const char *)type);
    }
    pos += 12 + len;
  }
  *w_out = w; *h_out = h;
  if (!out) return TM_OK;
  TM_CHECK((int64_t)w * h <= cap_px, TM_E_INVAL, "%s: %dx%d pixels do not fit the buffer", name, w, h);
  TM_CHECK(ctype != 3 || npal > 0, TM_E_INVAL, "%s: palette image without PLTE", name);
  const int bpp = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
  const size_t stride = (size_t)w * bpp, need = (stride + 1) * h;
  std::vector<uint8_t> raw(need);
  size_t got = 0;
  TM_TRY(inflate_zlib(z.data(), z.size(), raw.data(), need, &got));
  TM_CHECK(got == need, TM_E_INVAL, "%s: %zu bytes of image data, %zu expected", name, got, need);
  std::vector<uint8_t> zero(stride, 0);
  for (int y = 0; y < h; y++) {
    uint8_t *row = &raw[(size_t)y * (stride + 1) + 1];
    const uint8_t *up = y ? row - (stride + 1) : zero.data();
    const int ft = row[-1];
    TM_CHECK(ft <= 4, TM_E_INVAL, "%s: bad filter type %d in row %d", name, ft, y);
    for (size_t i = 0; i < stride; i++) {
      const int a = i >= (size_t)bpp ? row[i - bpp] : 0, b = up[i], c = i >= (size_t)bpp ? up[i - bpp] : 0;
      int pred = 0;
      if (ft == 1) pred = a;
      else if (ft == 2) pred = b;
      else if (ft == 3) pred = (a + b) >> 1;
      else if (ft == 4) {
        const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
      }
      row[i] = (uint8_t)(row[i] + pred);
    }
    uint32_t *o = out + (size_t)y * w;
    for (int x = 0; x < w; x++) {
      const uint8_t *s = row + (size_t)x * bpp;
      if (ctype == 0 || ctype == 4) o[x] = (uint32_t)s[0] * 0x010101u;
      else if (ctype == 3) {
        TM_CHECK(s[0] < npal, TM_E_INVAL, "%s: palette index %d beyond the %d entries of PLTE", name, s[0], npal);
        o[x] = (uint32_t)pal[s[0]][0] << 16 | (uint32_t)pal[s[0]][1] << 8 | pal[s[0]][2];
      } else o[x] = (uint32_t)s[0] << 16 | (uint32_t)s[1] << 8 | s[2];
    }
  }
  return TM_OK;
}

int read_file_bytes(const char *path, std::vector<uint8_t> *out) {
  FILE *f = fopen(path, "rb");
  TM_CHECK(f, TM_E_IO, "cannot open %s", path);
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (sz < 0) { fclose(f); set_error("cannot size %s", path); return TM_E_IO; }
  out->resize((size_t)sz);
  const size_t got = sz ? fread(out->data(), 1, (size_t)sz, f) : 0;
  fclose(f);
  TM_CHECK(got == (size_t)sz, TM_E_IO, "cannot read %s", path);
  return TM_OK;
}

int read_png(const char *path, uint32_t *out, int64_t cap_px, int *w, int *h) {
  std::vector<uint8_t> bytes;
  TM_TRY(read_file_bytes(path, &bytes));
  return decode_png(bytes.data(), bytes.size(), path, out, cap_px, w, h);
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_inflate_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *out_n) {
  TM_CHECK((src || n == 0) && (dst || cap == 0) && out_n, TM_E_INVAL, "null argument");
  return inflate_zlib(src, n, dst, cap, out_n);
}

int tm_read_png_host(const char *path, uint32_t *out_rgb32, int64_t cap_px, int *w, int *h) {
  TM_CHECK(path && w && h, TM_E_INVAL, "null argument");
  return read_png(path, out_rgb32, cap_px, w, h);
}

}  // extern "C"
