// tm_png_in.hip -- the PNG reader on the device.  The rule is tm_inflate.h's; the host twins (tm_inflate_streams_host,
// tm_png_decode_host) run the same text on one lane, and tm_png.hip's reader is the independent check.
//
//   host      parse_png walks a file's chunks as decode_png does (signature, CRCs, IHDR, PLTE; same refusals, same codes) and leaves a
//             descriptor: the IDAT payloads as spans of the file, the colour type, the palette.  The payloads are not joined.
//   inflate   k_inflate, one wave (one workgroup) per stream, every stream of a batch in one launch.  The decode state is the same in every
//             lane.  In LDS: the 32 KiB window, a stage of 1 KiB of input gathered through the span list, the tables (37 KB in all: four
//             workgroups to a compute unit's 160 KB).  A match is copied window to window by the whole wave; output leaves the window in
//             16-byte stores, and its Adler-32 sums are taken as it leaves.
//   unfilter  k_png_unfilter, one wave per picture: lanes on 64 consecutive rows, lane l one pixel behind lane l - 1, so that `up` and
//             `up-left` are lane l - 1's last two pixels (a cross-lane move).  The last row of a pass is written back unfiltered into the
//             inflated rows, where the next pass's first lane reads its `up`.  The pixel leaves as 0x00RRGGBB in the destination frame.
//
// Every loop is bounded by a stream's input, its destination's cap or the picture's size; plain launches, nothing waits on another workgroup.
#include "tm_common.h"
#include "tm_internal.h"
#include "tm_inflate.h"

namespace tmx {
namespace inf {
namespace {

constexpr uint32_t kStage = 1024;          // input bytes staged in LDS
constexpr uint32_t kFlushAt = 16384;       // finished bytes the window holds before they leave
constexpr uint32_t kMask = kWindow - 1;

// ---- the host IO: one lane, the destination itself is the window
struct HostIO {
  const uint8_t *blob;
  const Span *spans;
  uint32_t total;
  uint8_t *dst;
  uint32_t cap_;
  uint32_t si = 0, sstart = 0;  // the span the last byte came from and the input position it starts at
  uint16_t halves[kTableHalves];
  uint32_t work[32];
  uint8_t lens[320];
  uint32_t lane() const { return 0; }
  uint32_t lanes() const { return 1; }
  void sync() {}
  uint32_t in_size() const { return total; }
  uint32_t cap() const { return cap_; }
  Tables tables() {
    uint16_t *h = halves;
    Tables t;
    t.lit_fast = h; h += 1 << kLitFastBits;
    t.dist_fast = h; h += 1 << kDistFastBits;
    t.lit_count = h; h += 16;
    t.lit_symbol = h; h += 288;
    t.dist_count = h; h += 16;
    t.dist_symbol = h;
    t.work = work; t.lens = lens;
    return t;
  }
  uint32_t in_byte(uint32_t pos) {  // pos < total
    if (pos < sstart) { si = 0; sstart = 0; }
    while (pos - sstart >= spans[si].len) { sstart += spans[si].len; si++; }
    return blob[(size_t)spans[si].off + (pos - sstart)];
  }
  void flush_some(uint32_t) {}
  void put(uint32_t out, uint32_t v) { dst[out] = (uint8_t)v; }
  void copy(uint32_t out, uint32_t d, uint32_t len) {
    for (uint32_t k = 0; k < len; k++) dst[out + k] = dst[out - d + (d >= len ? k : k % d)];
  }
  void put_input(uint32_t out, uint32_t pos, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) dst[out + k] = (uint8_t)in_byte(pos + k);
  }
  uint32_t finish(uint32_t out) {
    uint32_t a = 1, b = 0;
    for (uint32_t i = 0; i < out;) {
      const uint32_t stop = out - i < 4096u ? out : i + 4096u;
      uint64_t s1 = 0, s2 = 0;
      for (uint32_t k = i; k < stop; k++) { s1 += dst[k]; s2 += (uint64_t)(stop - k) * dst[k]; }
      adler_append(&a, &b, s1, s2, stop - i);
      i = stop;
    }
    return b << 16 | a;
  }
};

// ---- the device IO: one wave
struct WaveLds {
  uint8_t ring[kWindow];   // the window: byte p of the output at (p + skew) & kMask, skew = the destination's address & 15
  uint8_t stage[kStage];
  uint16_t halves[kTableHalves];
  uint32_t work[32];
  uint8_t lens[320];
};

struct WaveIO {
  WaveLds &m;
  const uint8_t *blob;
  uint64_t blob_bytes;
  const Span *spans;  // the stream's own
  uint32_t total;
  uint8_t *dst;
  uint32_t cap_, skew, lane_;
  uint32_t si = 0, sstart = 0;          // as HostIO's
  uint32_t sbase = 0, slen = 0;         // the staged input positions [sbase, sbase + slen)
  uint32_t fl = 0, ad_a = 1, ad_b = 0;  // output bytes that have left, and their Adler-32 sums
  __device__ WaveIO(WaveLds &m_, const uint8_t *blob_, uint64_t blob_bytes_, const Span *spans_, uint32_t total_, uint8_t *dst_, uint32_t cap)
      : m(m_), blob(blob_), blob_bytes(blob_bytes_), spans(spans_), total(total_), dst(dst_), cap_(cap), skew((uint32_t)(reinterpret_cast<uintptr_t>(dst_) & 15u)),
        lane_(threadIdx.x) {}
  __device__ uint32_t lane() const { return lane_; }
  __device__ uint32_t lanes() const { return 64; }
  __device__ void sync() { __syncthreads(); }  // (the workgroup is this wave)
  __device__ uint32_t in_size() const { return total; }
  __device__ uint32_t cap() const { return cap_; }
  __device__ Tables tables() {
    uint16_t *h = m.halves;
    Tables t;
    t.lit_fast = h; h += 1 << kLitFastBits;
    t.dist_fast = h; h += 1 << kDistFastBits;
    t.lit_count = h; h += 16;
    t.lit_symbol = h; h += 288;
    t.dist_count = h; h += 16;
    t.dist_symbol = h;
    t.work = m.work; t.lens = m.lens;
    return t;
  }
  // input positions [pos, pos + kStage) into LDS, gathered through the span list; pos < total
  __device__ void restage(uint32_t pos) {
    __syncthreads();
    if (pos < sstart) { si = 0; sstart = 0; }
    while (pos - sstart >= spans[si].len) { sstart += spans[si].len; si++; }
    uint32_t j = si, s = sstart;
    for (uint32_t k = lane_; k < kStage; k += 64) {
      const uint32_t q = pos + k;
      uint8_t v = 0;
      if (q < total && q >= pos) {
        while (q - s >= spans[j].len) { s += spans[j].len; j++; }
        const uint64_t at = (uint64_t)spans[j].off + (q - s);
        if (at < blob_bytes) v = blob[at];
      }
      m.stage[k] = v;
    }
    sbase = pos;
    slen = total - pos < kStage ? total - pos : kStage;
    __syncthreads();
  }
  __device__ uint32_t in_byte(uint32_t pos) {
    if (pos - sbase >= slen) restage(pos);
    return m.stage[pos - sbase];
  }
  // output bytes [fl, upto) leave the window: whole 16-byte units of the destination, single bytes before the first and, when the
  // stream has ended, behind the last
  __device__ void flush(uint32_t out, bool final) {
    uint32_t upto = out;
    if (!final) upto -= (skew + out) & 15u;
    if (upto <= fl || upto > cap_) return;
    __syncthreads();
    const uint32_t cnt = upto - fl;
    uint32_t head = (16u - ((skew + fl) & 15u)) & 15u;
    if (head > cnt) head = cnt;
    const uint32_t units = (cnt - head) / 16u, tail = cnt - head - units * 16u;
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t k = lane_; k < head + tail; k += 64) {
      const uint32_t at = k < head ? k : cnt - tail + (k - head);
      const uint32_t v = m.ring[(fl + at + skew) & kMask];
      dst[fl + at] = (uint8_t)v;
      s1 += v; s2 += (uint64_t)(cnt - at) * v;
    }
    for (uint32_t u = lane_; u < units; u += 64) {
      const uint32_t at = head + u * 16u;
      const uint4 v = *reinterpret_cast<const uint4 *>(&m.ring[(fl + at + skew) & kMask]);
      *reinterpret_cast<uint4 *>(dst + fl + at) = v;
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
      uint32_t b1 = 0, bk = 0;  // sum of the 16 bytes, and of k byte[k]
      for (int i = 0; i < 4; i++)
        for (int k = 0; k < 4; k++) { const uint32_t b = (w4[i] >> (8 * k)) & 0xffu; b1 += b; bk += (uint32_t)(4 * i + k) * b; }
      s1 += b1; s2 += (uint64_t)(cnt - at) * b1 - bk;
    }
    for (int off = 32; off > 0; off >>= 1) {
      s1 += (uint64_t)__shfl_xor((unsigned long long)s1, off);
      s2 += (uint64_t)__shfl_xor((unsigned long long)s2, off);
    }
    adler_append(&ad_a, &ad_b, s1, s2, cnt);
    fl = upto;
    __syncthreads();
  }
  __device__ void flush_some(uint32_t out) { if (out - fl >= kFlushAt) flush(out, false); }
  __device__ void put(uint32_t out, uint32_t v) { m.ring[(out + skew) & kMask] = (uint8_t)v; }  // (every lane writes the same byte)
  __device__ void copy(uint32_t out, uint32_t d, uint32_t len) {
    __syncthreads();
    for (uint32_t k = lane_; k < len; k += 64) m.ring[(out + k + skew) & kMask] = m.ring[(out - d + (d >= len ? k : k % d) + skew) & kMask];
    __syncthreads();
  }
  __device__ void put_input(uint32_t out, uint32_t pos, uint32_t n) {
    while (n) {
      if (pos - sbase >= slen) restage(pos);
      const uint32_t have = sbase + slen - pos, piece = n < have ? n : have;
      for (uint32_t k = lane_; k < piece; k += 64) m.ring[(out + k + skew) & kMask] = m.stage[pos - sbase + k];
      out += piece; pos += piece; n -= piece;
    }
    __syncthreads();
  }
  __device__ uint32_t finish(uint32_t out) {
    flush(out, true);
    return ad_b << 16 | ad_a;
  }
};

// One wave per stream.  A stream whose spans or destination do not lie inside what the launch was given is refused untouched.
__global__ __launch_bounds__(64) void k_inflate(const uint8_t *__restrict__ blob, uint64_t blob_bytes, const Span *__restrict__ spans, uint32_t nspans,
                                                const Stream *__restrict__ streams, uint8_t *dst, uint64_t dst_bytes, tm_inflate_status *__restrict__ status) {
  __shared__ __align__(16) WaveLds lds;
  const Stream st = streams[blockIdx.x];
  tm_inflate_status res{kBadSpan, 0, 0};
  uint64_t total = 0;
  bool ok = st.first_span <= nspans && st.span_count <= nspans - st.first_span && st.dst_off <= dst_bytes && st.dst_cap <= dst_bytes - st.dst_off;
  if (ok)
    for (uint32_t j = 0; j < st.span_count; j++) {
      const Span sp = spans[st.first_span + j];
      ok = ok && sp.off <= blob_bytes && sp.len <= blob_bytes - sp.off;
      total += sp.len;
    }
  if (ok && total < ((uint64_t)1 << 32)) {
    WaveIO io(lds, blob, blob_bytes, spans + st.first_span, (uint32_t)total, dst + st.dst_off, st.dst_cap);
    inflate_stream(io, &res);
  }
  if (threadIdx.x == 0) status[blockIdx.x] = res;
}

// One wave per picture.  raw: the inflated rows of picture p at streams[p].dst_off, h (1 + w bpp) bytes when status[p] says so.
__global__ __launch_bounds__(64) void k_png_unfilter(uint8_t *raw_base, const Stream *__restrict__ streams, const Picture *__restrict__ pics,
                                                     const uint8_t *__restrict__ pal3, const tm_inflate_status *__restrict__ inflated, int w, int h,
                                                     uint32_t *__restrict__ out, int64_t frame_px, int32_t *__restrict__ status) {
  __shared__ uint32_t pal[256];
  __shared__ uint32_t s_fault;
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  const Picture pic = pics[p];
  const tm_inflate_status in = inflated[p];
  const int ctype = (int)pic.ctype, bpp = png_bpp(ctype), npal = (int)(pic.npal < 256u ? pic.npal : 256u);
  const uint64_t stride = (uint64_t)w * bpp, need = (stride + 1) * (uint64_t)h;
  if (in.code != kOk || in.out_n != need || streams[p].dst_cap < need) {  // (the same in every lane)
    if (lane == 0) status[p] = in.code != kOk ? in.code : (int32_t)kPngSize;
    return;
  }
  for (int i = (int)lane; i < 256; i += 64) {
    const uint8_t *e = pal3 + pic.pal_off + 3 * (size_t)i;
    pal[i] = i < npal ? ((uint32_t)e[0] << 16 | (uint32_t)e[1] << 8 | e[2]) : 0u;
  }
  if (lane == 0) s_fault = kNoRowFault;
  __syncthreads();
  uint8_t *raw = raw_base + streams[p].dst_off;
  uint32_t *frame = out + (int64_t)p * frame_px;
  for (int r0 = 0; r0 < h; r0 += 64) {
    const int r = r0 + (int)lane;
    const bool row_ok = r < h;
    uint8_t *row = raw + (uint64_t)(row_ok ? r : 0) * (stride + 1) + 1;
    const uint8_t *above = raw + (uint64_t)(r0 > 0 ? r0 - 1 : 0) * (stride + 1) + 1;  // lane 0's `up`: the last row of the pass before
    uint32_t ft = row_ok ? row[-1] : 0u;
    if (ft > 4) { atomicMin(&s_fault, row_fault_key((uint32_t)r, false)); ft = 0; }
    uint32_t left = 0, mine = 0, up_before = 0;
    for (int t = 0; t < w + 63; t++) {
      const int x = t - (int)lane;
      const bool on = row_ok && x >= 0 && x < w;
      uint32_t up = __shfl_up(mine, 1);  // lane l - 1's pixel x, made one step ago
      if (lane == 0) {
        up = 0;
        if (r0 > 0 && on)
          for (int k = 0; k < bpp; k++) up |= (uint32_t)above[(uint64_t)x * bpp + k] << (8 * k);
      }
      if (on) {
        uint32_t v = 0;
        for (int k = 0; k < bpp; k++) v |= (uint32_t)row[(uint64_t)x * bpp + k] << (8 * k);
        const uint32_t px = unfilter_pixel(ft, bpp, v, x > 0 ? left : 0u, up, x > 0 ? up_before : 0u);
        left = px; mine = px;
        uint32_t rgb;
        if (!png_rgb32(ctype, px, pal, npal, &rgb)) atomicMin(&s_fault, row_fault_key((uint32_t)r, true));
        frame[(int64_t)r * w + x] = rgb;
        if (lane == 63)
          for (int k = 0; k < bpp; k++) row[(uint64_t)x * bpp + k] = (uint8_t)(px >> (8 * k));
      }
      up_before = up;
    }
    __syncthreads();  // the written-back row is the next pass's `up`
  }
  if (lane == 0) status[p] = s_fault == kNoRowFault ? (int32_t)kOk : (s_fault & 1u) ? (int32_t)kPngPalette : (int32_t)kPngFilter;
}

// the rows of one picture on the host: the same rule, one row after the other.  raw is unfiltered in place.
int unfilter_host(uint8_t *raw, int w, int h, int ctype, const uint32_t *pal, int npal, uint32_t *out) {
  const int bpp = png_bpp(ctype);
  const size_t stride = (size_t)w * bpp;
  for (int y = 0; y < h; y++) {
    uint8_t *row = raw + (size_t)y * (stride + 1) + 1;
    const uint8_t *above = y ? row - (stride + 1) : nullptr;
    const uint32_t ft = row[-1];
    if (ft > 4) return kPngFilter;
    uint32_t left = 0, up_before = 0;
    for (int x = 0; x < w; x++) {
      uint32_t v = 0, up = 0;
      for (int k = 0; k < bpp; k++) {
        v |= (uint32_t)row[(size_t)x * bpp + k] << (8 * k);
        if (above) up |= (uint32_t)above[(size_t)x * bpp + k] << (8 * k);
      }
      const uint32_t px = unfilter_pixel(ft, bpp, v, x > 0 ? left : 0u, up, x > 0 ? up_before : 0u);
      for (int k = 0; k < bpp; k++) row[(size_t)x * bpp + k] = (uint8_t)(px >> (8 * k));
      left = px; up_before = up;
      if (!png_rgb32(ctype, px, pal, npal, &out[(size_t)y * w + x])) return kPngPalette;
    }
  }
  return kOk;
}

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// what the entry points refuse about a batch of streams, and the spans as the rule takes them
int check_streams(const char *who, const uint8_t *blob, size_t blob_bytes, const tm_inflate_span *spans, int nspans, const tm_inflate_stream *streams, int nstreams,
                  const void *dst, size_t dst_bytes, const tm_inflate_status *status, std::vector<Span> *packed) {
  TM_CHECK((blob || !blob_bytes) && (spans || !nspans) && (streams || !nstreams) && (dst || !dst_bytes) && (status || !nstreams) && nspans >= 0 && nstreams >= 0, TM_E_INVAL,
           "%s: null argument", who);
  TM_CHECK(blob_bytes < ((size_t)1 << 32), TM_E_UNSUPPORTED, "%s: a blob of %zu bytes (below 4 GiB)", who, blob_bytes);
  packed->resize((size_t)nspans);
  for (int j = 0; j < nspans; j++) {
    TM_CHECK(spans[j].off <= blob_bytes && spans[j].len <= blob_bytes - spans[j].off, TM_E_INVAL, "%s: span %d lies outside the blob", who, j);
    (*packed)[(size_t)j] = Span{(uint32_t)spans[j].off, spans[j].len};
  }
  for (int s = 0; s < nstreams; s++) {
    const tm_inflate_stream &st = streams[s];
    TM_CHECK(st.first_span <= (uint32_t)nspans && st.span_count <= (uint32_t)nspans - st.first_span, TM_E_INVAL, "%s: stream %d names spans outside the list", who, s);
    uint64_t total = 0;
    for (uint32_t j = 0; j < st.span_count; j++) total += spans[st.first_span + j].len;
    TM_CHECK(total < ((uint64_t)1 << 32), TM_E_INVAL, "%s: stream %d has %llu input bytes (below 4 GiB)", who, s, (unsigned long long)total);
    TM_CHECK(st.dst_off <= dst_bytes && st.dst_cap <= dst_bytes - st.dst_off, TM_E_INVAL, "%s: stream %d's destination lies outside the %zu bytes given", who, s, dst_bytes);
  }
  return TM_OK;
}

void inflate_one_host(const uint8_t *blob, const Span *spans, uint32_t count, uint8_t *dst, uint32_t cap, tm_inflate_status *st) {
  uint64_t total = 0;
  for (uint32_t j = 0; j < count; j++) total += spans[j].len;
  HostIO io{blob, spans, (uint32_t)total, dst, cap};
  inflate_stream(io, st);
}

}  // namespace

// ---- the container walk: decode_png's (tm_png.hip), leaving a descriptor in place of pixels
int parse_png(const uint8_t *file, size_t n, const char *name, PngInfo *info) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  TM_CHECK(n >= 8 + 25 && !memcmp(file, sig, 8), TM_E_UNSUPPORTED, "%s is not a PNG file", name);
  TM_CHECK(n < ((size_t)1 << 32), TM_E_UNSUPPORTED, "%s: a file of %zu bytes (below 4 GiB)", name, n);
  size_t pos = 8;
  info->w = info->h = 0; info->ctype = -1; info->npal = 0;
  info->idat.clear();
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
      info->w = (int)ww; info->h = (int)hh; info->ctype = data[9];
      TM_CHECK(data[8] == 8, TM_E_UNSUPPORTED, "%s: %d bits per sample (8 only)", name, data[8]);
      TM_CHECK(info->ctype == 0 || info->ctype == 2 || info->ctype == 3 || info->ctype == 4 || info->ctype == 6, TM_E_INVAL, "%s: bad colour type %d", name, info->ctype);
      TM_CHECK(data[10] == 0 && data[11] == 0, TM_E_INVAL, "%s: unknown compression or filter method", name);
      TM_CHECK(data[12] == 0, TM_E_UNSUPPORTED, "%s: interlaced (Adam7) images are not read", name);
    } else if (!memcmp(type, "PLTE", 4)) {
      TM_CHECK(len % 3 == 0 && len <= 768, TM_E_INVAL, "%s: bad PLTE chunk", name);
      info->npal = (int)(len / 3);
      memcpy(info->pal3, data, len);
    } else if (!memcmp(type, "IDAT", 4)) {
      info->idat.push_back(Span{(uint32_t)(pos + 8), (uint32_t)len});
    } else if (!memcmp(type, "IEND", 4)) {
      end = true;
    } else {
      TM_CHECK(type[0] & 0x20, TM_E_UNSUPPORTED, "%s: unknown critical chunk %.4s", name, (const char *)type);
    }
    pos += 12 + len;
  }
  return TM_OK;
}
// what decode_png refuses between the walk and the stream, in its order
int png_check_decodable(const PngInfo &info, const char *name, int w, int h) {
  TM_CHECK(info.w == w && info.h == h, TM_E_INVAL, "%s is %dx%d, the sequence's first frame is %dx%d", name, info.w, info.h, w, h);
  TM_CHECK(info.ctype != 3 || info.npal > 0, TM_E_INVAL, "%s: palette image without PLTE", name);
  TM_CHECK(((uint64_t)w * png_bpp(info.ctype) + 1) * (uint64_t)h < ((uint64_t)1 << 32), TM_E_UNSUPPORTED, "%s: %dx%d is 4 GiB of rows or more", name, w, h);
  return TM_OK;
}
// a refused file's status as the error decode_png would have set
int png_status_error(int status, const char *name) {
  if (status == kOk) return TM_OK;
  if (status == kPngSize) set_error("%s: the image data is not the picture's size", name);
  else if (status == kPngFilter) set_error("%s: bad filter type in a row", name);
  else if (status == kPngPalette) set_error("%s: a palette index beyond the entries of PLTE", name);
  else set_error("%s: inflate: the stream is damaged or cut short (code %d)", name, status);
  return TM_E_INVAL;
}

void PngBatch::clear() { spans.clear(); streams.clear(); pics.clear(); pal3.clear(); raw_bytes = 0; }
void PngBatch::add(const PngInfo &info, uint64_t at) {
  const uint64_t need = ((uint64_t)info.w * png_bpp(info.ctype) + 1) * (uint64_t)info.h;
  Stream st{raw_bytes, (uint32_t)need, (uint32_t)spans.size(), (uint32_t)info.idat.size(), 0};
  for (const Span &sp : info.idat) spans.push_back(Span{(uint32_t)(at + sp.off), sp.len});
  Picture pic{(uint32_t)info.ctype, info.ctype == 3 ? (uint32_t)info.npal : 0u, (uint32_t)pal3.size(), 0};
  if (info.ctype == 3) pal3.insert(pal3.end(), info.pal3, info.pal3 + 3 * (size_t)info.npal);
  streams.push_back(st); pics.push_back(pic);
  raw_bytes += (need + 15) & ~(uint64_t)15;
}
size_t PngBatch::desc_bytes() const { return streams.size() * (sizeof(Stream) + sizeof(Picture)) + spans.size() * sizeof(Span) + ((pal3.size() + 15) & ~(size_t)15) + 16; }
// streams | pictures | spans | palette bytes, each part on 8 bytes
size_t PngBatch::write_desc(uint8_t *to) const {
  size_t at = 0;
  memcpy(to + at, streams.data(), streams.size() * sizeof(Stream)); at += streams.size() * sizeof(Stream);
  memcpy(to + at, pics.data(), pics.size() * sizeof(Picture)); at += pics.size() * sizeof(Picture);
  memcpy(to + at, spans.data(), spans.size() * sizeof(Span)); at += spans.size() * sizeof(Span);
  if (!pal3.empty()) memcpy(to + at, pal3.data(), pal3.size());
  at += pal3.size();
  return at;
}

// the two kernels on a batch whose files and descriptor (write_desc at desc_off) lie in the device blob; raw: raw_bytes of scratch
int png_batch_launch(const PngBatch &b, const uint8_t *dev_blob, size_t blob_bytes, size_t desc_off, uint8_t *raw, tm_inflate_status *dev_inflated, int w, int h,
                     uint32_t *dev_out, int64_t frame_px, int32_t *dev_status, void *hip_stream) {
  hipStream_t stream = (hipStream_t)hip_stream;
  const int n = (int)b.streams.size();
  if (!n) return TM_OK;
  const uint8_t *d = dev_blob + desc_off;
  const Stream *streams = reinterpret_cast<const Stream *>(d);
  const Picture *pics = reinterpret_cast<const Picture *>(d + (size_t)n * sizeof(Stream));
  const Span *spans = reinterpret_cast<const Span *>(d + (size_t)n * (sizeof(Stream) + sizeof(Picture)));
  const uint8_t *pal3 = d + (size_t)n * (sizeof(Stream) + sizeof(Picture)) + b.spans.size() * sizeof(Span);
  hipLaunchKernelGGL(k_inflate, dim3((unsigned)n), dim3(64), 0, stream, dev_blob, (uint64_t)blob_bytes, spans, (uint32_t)b.spans.size(), streams, raw, (uint64_t)b.raw_bytes,
                     dev_inflated);
  hipLaunchKernelGGL(k_png_unfilter, dim3((unsigned)n), dim3(64), 0, stream, raw, streams, pics, pal3, dev_inflated, w, h, dev_out, frame_px, dev_status);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace inf
}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_inflate_streams_host(const uint8_t *blob, size_t blob_bytes, const tm_inflate_span *spans, int nspans, const tm_inflate_stream *streams, int nstreams, uint8_t *dst,
                            size_t dst_bytes, tm_inflate_status *status) {
  std::vector<inf::Span> packed;
  TM_TRY(inf::check_streams("tm_inflate_streams_host", blob, blob_bytes, spans, nspans, streams, nstreams, dst, dst_bytes, status, &packed));
  for (int s = 0; s < nstreams; s++)
    inf::inflate_one_host(blob, packed.data() + streams[s].first_span, streams[s].span_count, dst + streams[s].dst_off, streams[s].dst_cap, &status[s]);
  return TM_OK;
}

int tm_stage_inflate(const uint8_t *blob, size_t blob_bytes, const tm_inflate_span *spans, int nspans, const tm_inflate_stream *streams, int nstreams, uint8_t *dev_dst,
                     size_t dst_bytes, tm_inflate_status *status, void *stream) {
  std::vector<inf::Span> packed;
  TM_TRY(inf::check_streams("tm_stage_inflate", blob, blob_bytes, spans, nspans, streams, nstreams, dev_dst, dst_bytes, status, &packed));
  TM_TRY(require_device());
  if (!nstreams) return TM_OK;
  hipStream_t hs = (hipStream_t)stream;
  static_assert(sizeof(inf::Stream) == sizeof(tm_inflate_stream), "the stream descriptor is uploaded as it is given");
  DevBuf d_blob, d_spans, d_streams, d_status;
  TM_TRY(d_blob.alloc(blob_bytes)); TM_TRY(d_spans.alloc(packed.size() * sizeof(inf::Span))); TM_TRY(d_streams.alloc((size_t)nstreams * sizeof(inf::Stream)));
  TM_TRY(d_status.alloc((size_t)nstreams * sizeof(tm_inflate_status)));
  if (blob_bytes) TM_HIP(hipMemcpyAsync(d_blob.p, blob, blob_bytes, hipMemcpyHostToDevice, hs));
  if (!packed.empty()) TM_HIP(hipMemcpyAsync(d_spans.p, packed.data(), packed.size() * sizeof(inf::Span), hipMemcpyHostToDevice, hs));
  TM_HIP(hipMemcpyAsync(d_streams.p, streams, (size_t)nstreams * sizeof(inf::Stream), hipMemcpyHostToDevice, hs));
  hipLaunchKernelGGL(inf::k_inflate, dim3((unsigned)nstreams), dim3(64), 0, hs, d_blob.as<uint8_t>(), (uint64_t)blob_bytes, d_spans.as<inf::Span>(), (uint32_t)nspans,
                     d_streams.as<inf::Stream>(), dev_dst, (uint64_t)dst_bytes, d_status.as<tm_inflate_status>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipMemcpyAsync(status, d_status.p, (size_t)nstreams * sizeof(tm_inflate_status), hipMemcpyDeviceToHost, hs));
  TM_HIP(hipStreamSynchronize(hs));
  return TM_OK;
}

static int check_png_files(const char *who, const void *const *files, const size_t *sizes, int nfiles, int w, int h, const void *out, int64_t frame_px, const int32_t *status) {
  TM_CHECK(files && sizes && out && status && nfiles >= 0, TM_E_INVAL, "%s: null argument", who);
  TM_CHECK(w >= 1 && h >= 1 && w <= 65536 && h <= 65536 && frame_px >= (int64_t)w * h, TM_E_INVAL, "%s: bad size %dx%d or frames %lld pixels apart", who, w, h, (long long)frame_px);
  for (int i = 0; i < nfiles; i++) TM_CHECK(files[i], TM_E_INVAL, "%s: file %d is null", who, i);
  return TM_OK;
}

int tm_png_decode_host(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint32_t *out, int64_t frame_px, int32_t *status) {
  TM_TRY(check_png_files("tm_png_decode_host", files, sizes, nfiles, w, h, out, frame_px, status));
  std::vector<inf::PngInfo> infos((size_t)nfiles);
  for (int i = 0; i < nfiles; i++) {
    char name[32];
    snprintf(name, sizeof(name), "file %d", i);
    TM_TRY(inf::parse_png((const uint8_t *)files[i], sizes[i], name, &infos[(size_t)i]));
    TM_TRY(inf::png_check_decodable(infos[(size_t)i], name, w, h));
  }
  std::vector<uint8_t> raw;
  for (int i = 0; i < nfiles; i++) {
    const inf::PngInfo &info = infos[(size_t)i];
    const size_t need = ((size_t)w * inf::png_bpp(info.ctype) + 1) * (size_t)h;
    raw.assign(need, 0);
    tm_inflate_status st;
    inf::inflate_one_host((const uint8_t *)files[i], info.idat.data(), (uint32_t)info.idat.size(), raw.data(), (uint32_t)need, &st);
    if (st.code != inf::kOk) { status[i] = st.code; continue; }
    if (st.out_n != need) { status[i] = inf::kPngSize; continue; }
    uint32_t pal[256] = {0};
    for (int k = 0; k < info.npal; k++) pal[k] = (uint32_t)info.pal3[3 * k] << 16 | (uint32_t)info.pal3[3 * k + 1] << 8 | info.pal3[3 * k + 2];
    status[i] = inf::unfilter_host(raw.data(), w, h, info.ctype, pal, info.npal, out + (int64_t)i * frame_px);
  }
  return TM_OK;
}

int tm_stage_png_decode(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint32_t *dev_out, int64_t frame_px, int32_t *status, void *stream) {
  TM_TRY(check_png_files("tm_stage_png_decode", files, sizes, nfiles, w, h, dev_out, frame_px, status));
  inf::PngBatch batch;
  inf::PngInfo info;
  uint64_t at = 0;
  std::vector<uint64_t> where((size_t)nfiles);
  for (int i = 0; i < nfiles; i++) {
    char name[32];
    snprintf(name, sizeof(name), "file %d", i);
    TM_TRY(inf::parse_png((const uint8_t *)files[i], sizes[i], name, &info));
    TM_TRY(inf::png_check_decodable(info, name, w, h));
    where[(size_t)i] = at;
    batch.add(info, at);
    at += (sizes[i] + 15) & ~(size_t)15;
  }
  TM_CHECK(at + batch.desc_bytes() < ((uint64_t)1 << 32), TM_E_UNSUPPORTED, "tm_stage_png_decode: a batch of %llu bytes (below 4 GiB)", (unsigned long long)at);
  TM_TRY(require_device());
  if (!nfiles) return TM_OK;
  hipStream_t hs = (hipStream_t)stream;
  std::vector<uint8_t> blob((size_t)at + batch.desc_bytes());
  for (int i = 0; i < nfiles; i++) memcpy(blob.data() + where[(size_t)i], files[i], sizes[i]);
  const size_t used = (size_t)at + batch.write_desc(blob.data() + at);
  DevBuf d_blob, d_raw, d_inflated, d_status;
  TM_TRY(d_blob.alloc(used)); TM_TRY(d_raw.alloc(batch.raw_bytes)); TM_TRY(d_inflated.alloc((size_t)nfiles * sizeof(tm_inflate_status))); TM_TRY(d_status.alloc((size_t)nfiles * 4));
  TM_HIP(hipMemcpyAsync(d_blob.p, blob.data(), used, hipMemcpyHostToDevice, hs));
  TM_TRY(inf::png_batch_launch(batch, d_blob.as<uint8_t>(), used, (size_t)at, d_raw.as<uint8_t>(), d_inflated.as<tm_inflate_status>(), w, h, dev_out, frame_px,
                               d_status.as<int32_t>(), hs));
  TM_HIP(hipMemcpyAsync(status, d_status.p, (size_t)nfiles * 4, hipMemcpyDeviceToHost, hs));
  TM_HIP(hipStreamSynchronize(hs));
  return TM_OK;
}

}  // extern "C"
