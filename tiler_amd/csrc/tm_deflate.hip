// tm_deflate.hip -- the host form of the PNG writer's coder (the rule: tm_deflate.h): the row filters, the match
// finder and greedy parse, the length-limited code lengths, a segment's tables and header, and the file framing.  Host code only; the
// device form (tm_png_out.hip) shares best_match, the symbol and bit rules and plan_segment, and writes the same bytes.
#include <cstdlib>
#include <thread>

#include "tm_common.h"
#include "tm_deflate.h"
#include "tm_internal.h"

namespace tmx {
namespace dfl {
namespace {

struct BitWriter {  // lowest bit first (RFC 1951, 3.1.1)
  std::vector<uint8_t> &out;
  uint64_t acc = 0;
  uint32_t fill = 0;
  explicit BitWriter(std::vector<uint8_t> &o) : out(o) {}
  void put(uint64_t v, uint32_t nbits) {  // nbits <= 48
    acc |= v << fill;
    fill += nbits;
    while (fill >= 8) { out.push_back((uint8_t)acc); acc >>= 8; fill -= 8; }
  }
  void align() { if (fill) { out.push_back((uint8_t)acc); acc = 0; fill = 0; } }
};

uint32_t reverse_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int b = 0; b < len; b++) r |= ((code >> b) & 1u) << (len - 1 - b);
  return r;
}
// canonical codes of RFC 1951, 3.2.2 as table entries: reversed code | length << 16
void canonical(const uint8_t *lens, int nsym, uint32_t *entries) {
  uint32_t count[16] = {0}, next[16] = {0};
  for (int s = 0; s < nsym; s++) count[lens[s]]++;
  count[0] = 0;
  uint32_t code = 0;
  for (int b = 1; b <= 15; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
  for (int s = 0; s < nsym; s++) entries[s] = lens[s] ? (reverse_bits(next[lens[s]]++, lens[s]) | ((uint32_t)lens[s] << 16)) : 0u;
}

// prev[j]: the nearest position before j with j's three bytes.  A stable sort of the positions by their three bytes (three counting
// passes) puts that position just below j.
void link_positions(const uint8_t *s, uint32_t n, std::vector<int32_t> &prev) {
  prev.assign(n, -1);
  if (n < 3) return;
  const uint32_t m = n - 2;
  std::vector<uint32_t> a(m), b(m);
  for (uint32_t i = 0; i < m; i++) a[i] = i;
  for (int byte = 2; byte >= 0; byte--) {
    uint32_t count[257] = {0};
    for (uint32_t i = 0; i < m; i++) count[s[a[i] + byte] + 1]++;
    for (int v = 0; v < 256; v++) count[v + 1] += count[v];
    for (uint32_t i = 0; i < m; i++) b[count[s[a[i] + byte]]++] = a[i];
    a.swap(b);
  }
  for (uint32_t r = 1; r < m; r++)
    if (key3(s + a[r]) == key3(s + a[r - 1])) prev[a[r]] = (int32_t)a[r - 1];
}

}  // namespace

int host_threads() {
  const char *env = getenv("TM_HOST_THREADS");
  const int n = env ? atoi(env) : (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(16, n));
}

void code_lengths(const uint32_t *freq, int nsym, int max_bits, uint8_t *lens) {
  memset(lens, 0, (size_t)nsym);
  int used[288], nu = 0;
  for (int s = 0; s < nsym; s++) if (freq[s]) used[nu++] = s;
  if (nu == 0) { lens[0] = lens[1] = 1; return; }
  if (nu == 1) { lens[used[0]] = 1; lens[used[0] == 0 ? 1 : 0] = 1; return; }
  std::sort(used, used + nu, [&](int x, int y) { return freq[x] != freq[y] ? freq[x] < freq[y] : x < y; });
  // Huffman's tree over the sorted leaves with two queues: leaves 0 .. nu - 1, inner nodes nu .. 2 nu - 2 in the order they are made (their
  // weights never decrease); of two equal weights the leaf goes first
  uint64_t weight[576];
  int parent[576];
  for (int k = 0; k < nu; k++) weight[k] = freq[used[k]];
  int leaf = 0, inner = nu;
  for (int made = nu; made < 2 * nu - 1; made++) {
    uint64_t sum = 0;
    for (int pick = 0; pick < 2; pick++) {
      const bool take_leaf = leaf < nu && (inner >= made || weight[leaf] <= weight[inner]);
      const int node = take_leaf ? leaf++ : inner++;
      sum += weight[node];
      parent[node] = made;
    }
    weight[made] = sum;
  }
  int depth[576];
  uint32_t count[64] = {0};
  depth[2 * nu - 2] = 0;
  for (int node = 2 * nu - 3; node >= 0; node--) {
    depth[node] = depth[parent[node]] + 1;
    if (node < nu) count[std::min(depth[node], max_bits)]++;  // (a leaf deeper than the limit is counted at the limit)
  }
  // the limit: lengths beyond it were cut to it, which oversubscribes the code by `total - 2^max_bits` units of 2^-max_bits.  One unit is
  // paid back by taking a leaf off the last level and putting it beside a leaf of the deepest level above that has one, which moves down
  uint32_t total = 0;
  for (int b = 1; b <= max_bits; b++) total += count[b] << (max_bits - b);
  while (total > (1u << max_bits)) {
    count[max_bits]--;
    for (int b = max_bits - 1; b >= 1; b--)
      if (count[b]) { count[b]--; count[b + 1] += 2; break; }
    total--;
  }
  // the longest codes to the rarest symbols
  int k = 0;
  for (int b = max_bits; b >= 1; b--)
    for (uint32_t c = 0; c < count[b]; c++) lens[used[k++]] = (uint8_t)b;
}

void plan_segment(const uint32_t *lit_hist, const uint32_t *dist_hist, uint32_t seg_len, bool last, SegTables *t) {
  memset(t, 0, sizeof(*t));
  t->last = last ? 1 : 0;
  uint32_t lf[kLitSyms];
  memcpy(lf, lit_hist, sizeof(lf));
  lf[256] = 1;  // the end of the block
  uint8_t ll[kLitSyms], dl[kDistSyms], cl[kClSyms];
  code_lengths(lf, kLitSyms, 15, ll);
  code_lengths(dist_hist, kDistSyms, 15, dl);
  canonical(ll, kLitSyms, t->lit);
  canonical(dl, kDistSyms, t->dist);
  int hlit = kLitSyms, hdist = kDistSyms;
  while (hlit > 257 && !ll[hlit - 1]) hlit--;
  while (hdist > 1 && !dl[hdist - 1]) hdist--;
  // the lengths of both codes as one sequence, run-length coded (3.2.7): a run of zeros as 18s (11 .. 138) while 11 or more are left, then
  // one 17 (3 .. 10) or the zeros themselves; a run of a length as itself once, then 16s (3 .. 6) while 3 or more are left, then itself
  uint8_t seq[kLitSyms + kDistSyms];
  memcpy(seq, ll, (size_t)hlit);
  memcpy(seq + hlit, dl, (size_t)hdist);
  const int nseq = hlit + hdist;
  struct Rle { uint8_t sym, ebits, eval; };
  Rle rle[kLitSyms + kDistSyms];
  int nrle = 0;
  uint32_t cf[kClSyms] = {0};
  auto emit = [&](int sym, int ebits, int eval) { rle[nrle++] = Rle{(uint8_t)sym, (uint8_t)ebits, (uint8_t)eval}; cf[sym]++; };
  for (int at = 0; at < nseq;) {
    const int v = seq[at];
    int run = 1;
    while (at + run < nseq && seq[at + run] == v) run++;
    at += run;
    if (v == 0) {
      while (run >= 11) { const int r = std::min(run, 138); emit(18, 7, r - 11); run -= r; }
      if (run >= 3) { emit(17, 3, run - 3); run = 0; }
    } else {
      emit(v, 0, 0); run--;
      while (run >= 3) { const int r = std::min(run, 6); emit(16, 2, r - 3); run -= r; }
    }
    for (; run > 0; run--) emit(v, 0, 0);
  }
  code_lengths(cf, kClSyms, 7, cl);
  uint32_t ce[kClSyms];
  canonical(cl, kClSyms, ce);
  static const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = kClSyms;
  while (hclen > 4 && !cl[order[hclen - 1]]) hclen--;
  uint32_t nb = 0;
  auto put = [&](uint32_t v, uint32_t bits) {
    for (uint32_t b = 0; b < bits; b++, nb++) t->hdr[nb >> 5] |= ((v >> b) & 1u) << (nb & 31);
  };
  put(last ? 1 : 0, 1); put(2, 2);
  put((uint32_t)hlit - 257, 5); put((uint32_t)hdist - 1, 5); put((uint32_t)hclen - 4, 4);
  for (int k = 0; k < hclen; k++) put(cl[order[k]], 3);
  for (int k = 0; k < nrle; k++) { put(ce[rle[k].sym] & 0xffffu, ce[rle[k].sym] >> 16); put(rle[k].eval, rle[k].ebits); }
  t->hdr_nbits = nb;
  uint64_t bits = nb;
  for (int s = 0; s < kLitSyms; s++) bits += (uint64_t)lf[s] * (ll[s] + (s > 256 ? len_extra_bits((uint32_t)s) : 0u));
  for (int s = 0; s < kDistSyms; s++) bits += (uint64_t)dist_hist[s] * (dl[s] + dist_extra_bits((uint32_t)s));
  const uint64_t dyn_bytes = (bits + 7) / 8, stored_bytes = 5 + (uint64_t)seg_len;
  t->stored = stored_bytes <= dyn_bytes ? 1 : 0;
  if (t->stored) t->out_bytes = (uint32_t)(stored_bytes + (last ? 0 : 5));
  else t->out_bytes = (uint32_t)(last ? dyn_bytes : (bits + 3 + 7) / 8 + 4);
}

void filter_rows(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, uint8_t *stream) {
  const uint32_t rb = 3u * (uint32_t)w;
  std::vector<uint32_t> zeros((size_t)w, 0);
  for (int y = 0; y < h; y++) {
    const uint32_t *row = frame + (int64_t)y * stride_px, *up = y ? row - stride_px : zeros.data();
    uint8_t *out = stream + (size_t)y * (1 + rb);
    int type = 0;
    if (filter == kFilterAdaptive) {
      uint64_t cost[5] = {0, 0, 0, 0, 0};
      for (uint32_t k = 0; k < rb; k++) {
        const uint32_t x = row_byte(row, k), a = k >= 3 ? row_byte(row, k - 3) : 0, b = row_byte(up, k), c = k >= 3 ? row_byte(up, k - 3) : 0;
        for (int t = 0; t < 5; t++) cost[t] += filter_cost(filter_byte(t, x, a, b, c));
      }
      for (int t = 1; t < 5; t++) if (cost[t] < cost[type]) type = t;
    }
    out[0] = (uint8_t)type;
    for (uint32_t k = 0; k < rb; k++)
      out[1 + k] = filter_byte(type, row_byte(row, k), k >= 3 ? row_byte(row, k - 3) : 0, row_byte(up, k), k >= 3 ? row_byte(up, k - 3) : 0);
  }
}

int deflate_body(const uint8_t *s, uint32_t n, std::vector<uint8_t> &out) {
  std::vector<int32_t> prev;
  link_positions(s, n, prev);
  const uint32_t nseg = seg_count(n);
  std::vector<uint32_t> tokens;  // length | distance << 16 (a literal: length 0)
  SegTables t;
  BitWriter bw(out);
  for (uint32_t g = 0; g < nseg; g++) {
    const uint32_t first = g * kSeg, end = std::min<uint64_t>(n, (uint64_t)first + kSeg);
    const bool last = g + 1 == nseg;
    uint32_t lit_hist[kLitSyms] = {0}, dist_hist[kDistSyms] = {0};
    tokens.clear();
    for (uint32_t i = first; i < end;) {
      uint32_t dist = 0, sym, eb, ev;
      const uint32_t len = best_match(s, n, prev.data(), i, &dist);
      if (len) {
        len_symbol(len, &sym, &eb, &ev); lit_hist[sym]++;
        dist_symbol(dist, &sym, &eb, &ev); dist_hist[sym]++;
        tokens.push_back(len | (dist << 16));
        i += len;
      } else {
        lit_hist[s[i]]++;
        tokens.push_back(0);
        i++;
      }
    }
    plan_segment(lit_hist, dist_hist, end - first, last, &t);
    const size_t before = out.size();
    if (t.stored) {
      const uint32_t len = end - first;
      out.push_back(last ? 1 : 0);
      out.push_back(len & 0xff); out.push_back(len >> 8); out.push_back(~len & 0xff); out.push_back((~len >> 8) & 0xff);
      out.insert(out.end(), s + first, s + end);
    } else {
      for (uint32_t b = 0; b < t.hdr_nbits; b += 32) bw.put(t.hdr[b >> 5], std::min(32u, t.hdr_nbits - b));
      uint32_t i = first;
      uint64_t v;
      for (uint32_t tok : tokens) {
        const uint32_t nb = tok ? match_bits(t.lit, t.dist, tok & 0xffffu, tok >> 16, &v) : literal_bits(t.lit, s[i], &v);
        bw.put(v, nb);
        i += tok ? tok & 0xffffu : 1;
      }
      bw.put(t.lit[256] & 0xffffu, t.lit[256] >> 16);
    }
    if (!last) { bw.put(0, 3); bw.align(); out.push_back(0); out.push_back(0); out.push_back(0xff); out.push_back(0xff); }
    else bw.align();
    // the size the plan announced is the size the device form lays the segments out by
    TM_CHECK(out.size() - before == t.out_bytes, TM_E_INTERNAL, "deflate: segment %u took %zu bytes, its plan said %u", g, out.size() - before, t.out_bytes);
  }
  return TM_OK;
}

uint32_t adler32(const uint8_t *s, size_t n) {
  uint32_t a = 1, b = 0;
  for (size_t at = 0; at < n; at += kSeg) {
    const uint32_t len = (uint32_t)std::min<size_t>(kSeg, n - at);
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t k = 0; k < len; k++) { s1 += s[at + k]; s2 += (uint64_t)(len - k) * s[at + k]; }
    adler_append(&a, &b, s1, s2, len);
  }
  return (b << 16) | a;
}

static void png_chunk(std::vector<uint8_t> &out, const char *type, const uint8_t *data, size_t n) {
  auto be32 = [&](uint32_t v) { out.push_back(v >> 24); out.push_back(v >> 16); out.push_back(v >> 8); out.push_back(v); };
  be32((uint32_t)n);
  const size_t at = out.size();
  out.insert(out.end(), type, type + 4);
  out.insert(out.end(), data, data + n);
  be32(crc32_ieee(out.data() + at, out.size() - at));
}
static void png_frame(int w, int h, const std::vector<uint8_t> &z, std::vector<uint8_t> &file) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  file.assign(sig, sig + 8);
  file.reserve(z.size() + 64);
  const uint8_t ihdr[13] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, 8, 2, 0, 0, 0};
  png_chunk(file, "IHDR", ihdr, 13);
  png_chunk(file, "IDAT", z.data(), z.size());
  png_chunk(file, "IEND", nullptr, 0);
}

void png_wrap(int w, int h, const uint8_t *body, size_t body_n, uint32_t adler, std::vector<uint8_t> &file) {
  std::vector<uint8_t> z;
  z.reserve(body_n + 6);
  z.push_back(0x78); z.push_back(0x9c);
  z.insert(z.end(), body, body + body_n);
  z.push_back(adler >> 24); z.push_back(adler >> 16); z.push_back(adler >> 8); z.push_back(adler);
  png_frame(w, h, z, file);
}

// 24-bit RGB PNG (pf24bit, tilingencoder.pas:2086) of 0x00RRGGBB pixels; the image data travels in stored deflate blocks
void png_stored(const uint32_t *frame, int64_t stride_px, int w, int h, std::vector<uint8_t> &file) {
  std::vector<uint8_t> raw((size_t)h * (1 + (size_t)w * 3));
  filter_rows(frame, stride_px, w, h, kFilterNone, raw.data());
  std::vector<uint8_t> z = {0x78, 0x01};
  const uint32_t ad = adler32(raw.data(), raw.size());
  for (size_t off = 0; off < raw.size() || off == 0; off += 65535) {
    const size_t n = std::min<size_t>(65535, raw.size() - off);
    z.push_back(off + n >= raw.size() ? 1 : 0);
    z.push_back(n & 0xff); z.push_back(n >> 8); z.push_back(~n & 0xff); z.push_back((~n >> 8) & 0xff);
    z.insert(z.end(), raw.begin() + off, raw.begin() + off + n);
    if (raw.empty()) break;
  }
  z.push_back(ad >> 24); z.push_back(ad >> 16); z.push_back(ad >> 8); z.push_back(ad);
  png_frame(w, h, z, file);
}

int png_encode(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, std::vector<uint8_t> &file) {
  const uint32_t n = (uint32_t)((uint64_t)h * (1 + 3 * (uint64_t)w));
  std::vector<uint8_t> stream(n), body;
  auto one = [&](int flt, std::vector<uint8_t> &f) -> int {
    filter_rows(frame, stride_px, w, h, flt, stream.data());
    body.clear();
    TM_TRY(deflate_body(stream.data(), n, body));
    png_wrap(w, h, body.data(), body.size(), adler32(stream.data(), n), f);
    return TM_OK;
  };
  if (filter != kFilterSmaller) return one(filter == kFilterAdaptive ? kFilterAdaptive : kFilterNone, file);
  std::vector<uint8_t> other;
  TM_TRY(one(kFilterNone, file));
  TM_TRY(one(kFilterAdaptive, other));
  if (other.size() < file.size()) file.swap(other);
  return TM_OK;
}

int64_t png_bound(int w, int h) {
  const int64_t n = (int64_t)h * (1 + 3 * (int64_t)w);
  // signature 8, IHDR 25, IDAT 12 + zlib header 2 + Adler-32 4, IEND 12; a segment: at most its bytes stored (5) and the empty block (5)
  return 63 + n + 10 * (int64_t)seg_count((uint64_t)n);
}

int png_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt) {
  TM_CHECK(opt, TM_E_INVAL, "%s: null options", who);
  TM_CHECK(opt->level == 0 || opt->level == 1, TM_E_INVAL, "%s: unknown level %d (0 or 1)", who, opt->level);
  TM_CHECK(opt->filter >= TM_PNG_FILTER_AUTO && opt->filter <= TM_PNG_FILTER_SMALLER, TM_E_INVAL, "%s: unknown filter %d", who, opt->filter);
  TM_CHECK(w >= 1 && h >= 1 && w <= 32768 && h <= 32768, TM_E_INVAL, "%s: a picture of %d x %d (1 .. 32768 each)", who, w, h);
  TM_CHECK((int64_t)h * (1 + 3 * (int64_t)w) < ((int64_t)1 << 31), TM_E_INVAL, "%s: %d x %d makes a stream of 2^31 bytes or more", who, w, h);
  TM_CHECK(nframes >= 0, TM_E_INVAL, "%s: %d frames", who, nframes);
  TM_CHECK(frames || nframes == 0, TM_E_INVAL, "%s: null frames", who);
  TM_CHECK(h == 1 || stride_px >= w, TM_E_INVAL, "%s: a row stride of %lld pixels for rows of %d", who, (long long)stride_px, w);
  TM_CHECK(nframes <= 1 || frame_px >= (int64_t)(h - 1) * stride_px + w, TM_E_INVAL, "%s: a frame stride of %lld pixels for frames of %lld", who,
           (long long)frame_px, (long long)((int64_t)(h - 1) * stride_px + w));
  return TM_OK;
}

}  // namespace dfl
}  // namespace tmx

extern "C" {

int tm_deflate_code_lengths_host(const uint32_t *freq, int nsym, int max_bits, uint8_t *lens) {
  using namespace tmx;
  TM_CHECK(freq && lens, TM_E_INVAL, "tm_deflate_code_lengths_host: null argument");
  TM_CHECK(nsym >= 2 && nsym <= 288 && max_bits >= 1 && max_bits <= 15 && (1 << max_bits) >= nsym, TM_E_INVAL,
           "tm_deflate_code_lengths_host: %d symbols in %d bits", nsym, max_bits);
  dfl::code_lengths(freq, nsym, max_bits, lens);
  return TM_OK;
}

int tm_png_filter_rows_host(const uint32_t *frame, int64_t stride_px, int w, int h, int filter, uint8_t *stream) {
  using namespace tmx;
  TM_CHECK(stream, TM_E_INVAL, "tm_png_filter_rows_host: null stream");
  TM_CHECK(filter == TM_PNG_FILTER_NONE || filter == TM_PNG_FILTER_ADAPTIVE, TM_E_INVAL, "tm_png_filter_rows_host: filter %d (NONE or ADAPTIVE)", filter);
  const tm_png_options opt = {1, filter};
  TM_TRY(dfl::png_check("tm_png_filter_rows_host", frame, stride_px, 0, 1, w, h, &opt));
  dfl::filter_rows(frame, stride_px, w, h, filter, stream);
  return TM_OK;
}

int tm_zlib_compress_host(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int64_t *out_n) {
  using namespace tmx;
  TM_CHECK((src || !n) && out_n && (out || !cap), TM_E_INVAL, "tm_zlib_compress_host: null argument");
  TM_CHECK(n >= 0 && n < ((int64_t)1 << 31) && cap >= 0, TM_E_INVAL, "tm_zlib_compress_host: a stream of %lld bytes (0 .. 2^31 - 1)", (long long)n);
  std::vector<uint8_t> z = {0x78, 0x9c};
  TM_TRY(dfl::deflate_body(src, (uint32_t)n, z));
  const uint32_t ad = dfl::adler32(src, (size_t)n);
  z.push_back(ad >> 24); z.push_back(ad >> 16); z.push_back(ad >> 8); z.push_back(ad);
  *out_n = (int64_t)z.size();
  TM_CHECK(cap >= (int64_t)z.size(), TM_E_INVAL, "tm_zlib_compress_host: %zu bytes needed, %lld given", z.size(), (long long)cap);
  memcpy(out, z.data(), z.size());
  return TM_OK;
}

int tm_png_bound_host(int w, int h, int64_t *bytes) {
  using namespace tmx;
  TM_CHECK(bytes, TM_E_INVAL, "tm_png_bound_host: null argument");
  const tm_png_options opt = {1, TM_PNG_FILTER_NONE};
  TM_TRY(dfl::png_check("tm_png_bound_host", nullptr, w, 0, 0, w, h, &opt));
  *bytes = dfl::png_bound(w, h);
  return TM_OK;
}

int tm_png_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt, uint8_t *out,
                       int64_t cap, int64_t *offsets) {
  using namespace tmx;
  TM_TRY(dfl::png_check("tm_png_encode_host", frames, stride_px, frame_px, nframes, w, h, opt));
  TM_CHECK(offsets && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_png_encode_host: null argument");
  std::vector<std::vector<uint8_t>> files((size_t)nframes);
  int64_t total = 0;
  for (int f = 0; f < nframes; f++) {
    const uint32_t *fr = frames + (int64_t)f * frame_px;
    if (opt->level == 0) dfl::png_stored(fr, stride_px, w, h, files[(size_t)f]);
    else TM_TRY(dfl::png_encode(fr, stride_px, w, h, opt->filter == TM_PNG_FILTER_AUTO ? TM_PNG_FILTER_NONE : opt->filter, files[(size_t)f]));
    total += (int64_t)files[(size_t)f].size();
  }
  if (total > cap) {
    offsets[nframes] = total;
    TM_CHECK(false, TM_E_INVAL, "tm_png_encode_host: %lld bytes needed, %lld given", (long long)total, (long long)cap);
  }
  int64_t at = 0;
  for (int f = 0; f < nframes; f++) {
    offsets[f] = at;
    memcpy(out + at, files[(size_t)f].data(), files[(size_t)f].size());
    at += (int64_t)files[(size_t)f].size();
  }
  offsets[nframes] = at;
  return TM_OK;
}

}  // extern "C"
