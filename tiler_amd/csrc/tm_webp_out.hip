// tm_webp_out.hip -- the WebP writer on the device and its host twin.  The rule is tm_webp_out.h's; both forms write
// the same bytes.  A chunk of frames goes through these stages on the caller's stream, every frame of the chunk in the same launches:
//
//   rect      k_gif_rect (tm_gif_out.hip's, shared) and k_webp_rect_fix, which makes the rule's rectangle with its even corner.
//   colours   k_gif_colours (shared): per frame the open-addressed table of the rectangle's distinct colours and a count that stops above
//             256.  Rectangles, tables and counts come to the host (read-back 1), which sorts an indexed frame's colours into its table and
//             a rank per slot.
//   symbols   k_webp_symbols: a lane per coded pixel: the ranks of its bundle's pixels, or the green-subtracted colour.
//   links     k_webp_keys: a lane per position, the key of its three symbols under its frame's number; one stable radix sort (rocPRIM) of
//             all positions of the chunk; k_webp_links: the entry below in sorted order is the nearest earlier position with the same key.
//   parse     k_webp_parse: one wave (one workgroup) per segment, every segment of the chunk in one launch.  The parse's state is the same
//             in every lane and lives in registers (position, best length and distance, token count); a common run is measured 64 symbols
//             a step with one ballot.  In LDS (4352 bytes): the segment's histograms of the five alphabets, added to its image's with one
//             atomic per used symbol at the end.  Output: the segment's tokens in a span of its own, their count (read-back 2, with the
//             histograms).
//   codes     the host: per image the five codes' lengths, its header bits and its table of codes.
//   pack      k_webp_pack: a workgroup of 256 per segment, a lane per token: its bits through the image's table (in LDS), a scan of the
//             bit counts over the workgroup, the bits or-ed into 514 words of LDS and stored 256 tokens at a time.  Output: the segment's
//             bits in a span of its own and its bit count (read-back 3).
//   place     the host adds the bit counts up; an image's header bits are one more span in front of its segments'.
//   emit      k_gif_emit (shared): a lane per four payload bytes, each piece by a funnel shift of two words; k_gif_blob (shared) copies
//             the chunk headers and pad bytes.  One copy brings the chunk's bytes back (read-back 4).
//
// Every loop is bounded by the rectangle, the segment, the depth or the grid; plain launches, nothing waits on another workgroup; every
// store is checked against the buffer it goes to.
#include <chrono>

#include <rocprim/device/device_radix_sort.hpp>

#include "tm_common.h"
#include "tm_deflate.h"
#include "tm_webp_out.h"

namespace tmx {
namespace wpo {
namespace {

using gfo::ImagePlace;
using gfo::kEmpty;
using gfo::kHashSlots;
using gfo::Piece;
using gfo::SegPlace;

constexpr int32_t kRectInit = 0x7f7f7f7f;
constexpr uint32_t kBatch = 256;          // tokens the pack kernel joins at a time
constexpr uint32_t kPackWords = 2 * kBatch + 2;  // 31 bits carried + 256 tokens of at most 60 bits, and two words a token may reach into

struct FrameJob {
  Rect r;
  uint64_t sym_off;  // its symbols among the chunk's
  uint32_t n, pw, per, colours;  // symbols, coded pixels a row, pixels a coded pixel, the table's colours (0: subtract green)
};
struct SegJob {
  uint64_t sym_off, word_off;  // the image's symbols; the segment's span of words
  uint32_t n, begin, end, frame, cap_words, pad;
};

inline unsigned blocks_of(uint64_t n, unsigned most) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, most)); }
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// whole: the chunk's first frame is the file's first
__global__ void k_webp_rect_fix(int nf, int whole_first, int diff, int w, int h, const int32_t *__restrict__ raw, Rect *__restrict__ rects) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= nf) return;
  Rect r{0, 0, w, h};
  if (diff && !(whole_first && f == 0)) {
    if (raw[f * 4] == kRectInit) r = Rect{0, 0, 1, 1};
    else {
      const int x0 = raw[f * 4] & ~1, y0 = raw[f * 4 + 1] & ~1;
      r = Rect{x0, y0, 65535 - raw[f * 4 + 2] - x0 + 1, 65535 - raw[f * 4 + 3] - y0 + 1};
    }
  }
  rects[f] = r;
}

// ---- pixels -> symbols
__global__ __launch_bounds__(256) void k_webp_symbols(const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, const FrameJob *__restrict__ jobs,
                                                      const uint32_t *__restrict__ tabs, const uint8_t *__restrict__ ranks, uint32_t *__restrict__ sym, uint64_t total,
                                                      int32_t *__restrict__ status) {
  const uint32_t f = blockIdx.y;
  const FrameJob j = jobs[f];
  const uint32_t *cur = frames + (int64_t)f * frame_px;
  const uint32_t *tab = tabs + (size_t)f * kHashSlots;
  const uint32_t bits = 8 / j.per;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < j.n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t y = (uint32_t)(i / j.pw), px = (uint32_t)(i % j.pw);
    const uint32_t *row = cur + (int64_t)(j.r.y + (int)y) * stride_px + j.r.x;
    uint32_t v;
    if (j.colours) {
      uint32_t g = 0;
      for (uint32_t k = 0; k < j.per; k++) {
        const uint32_t x = px * j.per + k;
        if (x >= (uint32_t)j.r.w) break;
        const uint32_t c = gfo::rgb_of(row[x]);
        uint32_t slot = gfo::colour_hash(c), probe = 0;
        while (probe < kHashSlots && tab[slot] != c) { probe++; slot = (slot + 1) & (kHashSlots - 1); }
        if (probe < kHashSlots) g |= (uint32_t)ranks[(size_t)f * kHashSlots + slot] << (k * bits);
        else atomicMax(status, 1);
      }
      v = 0xff000000u | g << 8;
    } else {
      v = subtract_green(gfo::rgb_of(row[px]));
    }
    if (j.sym_off + i < total) sym[j.sym_off + i] = v;
  }
}

// ---- links
__global__ __launch_bounds__(256) void k_webp_keys(const FrameJob *__restrict__ jobs, const uint32_t *__restrict__ sym, uint64_t total, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ pos) {
  const uint32_t f = blockIdx.y;
  const FrameJob j = jobs[f];
  if (j.sym_off > total || j.n > total - j.sym_off) return;
  const uint32_t *s = sym + j.sym_off;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < j.n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t a = s[i], b = i + 1 < j.n ? s[i + 1] : 0u, c = i + 2 < j.n ? s[i + 2] : 0u;
    keys[j.sym_off + i] = f << 27 | key_of(a, b, c);
    pos[j.sym_off + i] = (uint32_t)(j.sym_off + i);
  }
}
// sorted by (frame, key, position): the entry below is the nearest earlier position of the frame with the same key
__global__ __launch_bounds__(256) void k_webp_links(const FrameJob *__restrict__ jobs, const uint32_t *__restrict__ keys_sorted, const uint32_t *__restrict__ ord, uint32_t total,
                                                    int32_t *__restrict__ prev) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < total; r += (uint64_t)gridDim.x * 256) {
    const uint32_t at = ord[r];
    if (at >= total) continue;
    const uint32_t off = (uint32_t)jobs[keys_sorted[r] >> 27].sym_off;
    prev[at] = (r > 0 && keys_sorted[r - 1] == keys_sorted[r] && ord[r - 1] >= off && ord[r - 1] < at) ? (int32_t)(ord[r - 1] - off) : -1;
  }
}

// ---- the parse: the device IO, one wave
struct WaveParse {
  const uint32_t *s;
  const int32_t *links;
  Token *tok;
  uint32_t tok_cap;
  uint32_t *hist;  // LDS, kSyms
  uint32_t lane;
  uint32_t ntok = 0, nmatch = 0;
  __device__ WaveParse(const uint32_t *s_, const int32_t *links_, Token *tok_, uint32_t cap_, uint32_t *hist_) : s(s_), links(links_), tok(tok_), tok_cap(cap_), hist(hist_), lane(threadIdx.x) {}
  __device__ uint32_t sym(uint32_t i) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)s[i]); }
  // (a link that does not point back ends the walk: every read stays below i)
  __device__ int32_t prev(uint32_t i) const { const int32_t j = __builtin_amdgcn_readfirstlane(links[i]); return j < (int32_t)i ? j : -1; }
  __device__ uint32_t common(uint32_t j, uint32_t i, uint32_t cap) const {
    for (uint32_t k = 0; k < cap; k += 64) {
      const uint32_t kk = k + lane;
      const unsigned long long differ = __ballot(kk < cap && s[j + kk] != s[i + kk]);
      if (differ) return k + (uint32_t)(__ffsll((long long)differ) - 1);
    }
    return cap;
  }
  __device__ void emit(Token t) {
    if (lane == 0) {
      if (ntok < tok_cap) tok[ntok] = t;
      uint32_t slots[4];
      const int ns = token_slots(t, slots);
      for (int k = 0; k < ns; k++) hist[slots[k]]++;
    }
    ntok++;
  }
  __device__ void literal(uint32_t v) { emit(Token{v, 0}); }
  __device__ void match(uint32_t len, uint32_t dist) { emit(Token{len, dist}); nmatch++; }
};

__global__ __launch_bounds__(64) void k_webp_parse(const SegJob *__restrict__ jobs, const uint32_t *__restrict__ sym, const int32_t *__restrict__ prev, uint64_t total, int lz77,
                                                   Token *__restrict__ tok, uint32_t *__restrict__ hists, uint32_t nframes, uint32_t *__restrict__ ntoks,
                                                   uint32_t *__restrict__ nmatches, int32_t *__restrict__ status) {
  __shared__ uint32_t hist[kSyms];
  const SegJob j = jobs[blockIdx.x];
  // a job that points outside what the launch was given is refused untouched
  if (j.sym_off > total || j.n > total - j.sym_off || j.begin >= j.end || j.end > j.n || j.frame >= nframes) {
    if (threadIdx.x == 0) { ntoks[blockIdx.x] = 0; nmatches[blockIdx.x] = 0; atomicMax(status, 2); }
    return;
  }
  for (uint32_t k = threadIdx.x; k < kSyms; k += 64) hist[k] = 0;
  __syncthreads();
  WaveParse io(sym + j.sym_off, prev + j.sym_off, tok + j.sym_off + j.begin, j.end - j.begin, hist);
  parse_segment(io, j.begin, j.end, lz77 != 0);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kSyms; k += 64)
    if (hist[k]) atomicAdd(&hists[(size_t)j.frame * kSyms + k], hist[k]);
  if (threadIdx.x == 0) { ntoks[blockIdx.x] = io.ntok; nmatches[blockIdx.x] = io.nmatch; }
}

// ---- the tokens' bits
__global__ __launch_bounds__(256) void k_webp_pack(const SegJob *__restrict__ jobs, const Token *__restrict__ tok, uint64_t total, const uint32_t *__restrict__ ntoks,
                                                   const uint32_t *__restrict__ tabs, uint32_t nframes, uint32_t *__restrict__ words, uint64_t nwords,
                                                   unsigned long long *__restrict__ bits, int32_t *__restrict__ status) {
  __shared__ uint32_t tab[kSyms];
  __shared__ uint32_t lw[kPackWords];
  __shared__ uint32_t scan[kBatch];
  const SegJob j = jobs[blockIdx.x];
  const uint32_t nt = ntoks[blockIdx.x], tid = threadIdx.x;
  if (j.sym_off > total || j.end > j.n || j.n > total - j.sym_off || j.begin >= j.end || nt > j.end - j.begin || j.frame >= nframes || j.word_off > nwords ||
      j.cap_words > nwords - j.word_off) {
    if (tid == 0) { bits[blockIdx.x] = 0; atomicMax(status, 3); }
    return;
  }
  for (uint32_t k = tid; k < kSyms; k += 256) tab[k] = tabs[(size_t)j.frame * kSyms + k];
  for (uint32_t k = tid; k < kPackWords; k += 256) lw[k] = 0;
  __syncthreads();
  const Token *t = tok + j.sym_off + j.begin;
  uint32_t *out = words + j.word_off;
  uint32_t written = 0, carry = 0;  // whole words stored; bits waiting in lw[0]
  bool over = false;
  for (uint32_t base = 0; base < nt; base += kBatch) {
    uint64_t val = 0;
    const uint32_t nb = base + tid < nt ? token_bits(tab, t[base + tid], &val) : 0u;
    scan[tid] = nb;
    __syncthreads();
    for (uint32_t step = 1; step < kBatch; step <<= 1) {
      const uint32_t add = tid >= step ? scan[tid - step] : 0u;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    const uint32_t at = carry + scan[tid] - nb, all = carry + scan[kBatch - 1];
    if (nb) {
      const uint32_t wi = at >> 5, sh = at & 31u;
      const uint64_t lo = val << sh;
      const uint32_t hi = sh ? (uint32_t)(val >> (64 - sh)) : 0u;
      if ((uint32_t)lo) atomicOr(&lw[wi], (uint32_t)lo);
      if ((uint32_t)(lo >> 32)) atomicOr(&lw[wi + 1], (uint32_t)(lo >> 32));
      if (hi) atomicOr(&lw[wi + 2], hi);
    }
    __syncthreads();
    const uint32_t full = all >> 5;
    for (uint32_t k = tid; k < full; k += 256) {
      if (written + k < j.cap_words) out[written + k] = lw[k]; else over = true;
    }
    const uint32_t rest = lw[full];
    __syncthreads();
    for (uint32_t k = tid; k < full + 3 && k < kPackWords; k += 256) lw[k] = k == 0 ? rest : 0u;
    __syncthreads();
    written += full;
    carry = all & 31u;
  }
  if (tid == 0) {
    if (carry) { if (written < j.cap_words) out[written] = lw[0]; else over = true; }
    bits[blockIdx.x] = (unsigned long long)written * 32 + carry;
  }
  if (over) atomicMax(status, 4);
}

// ---- what both forms share on the host
void canonical(const uint8_t *lens, int nsym, uint32_t *entries) {
  uint32_t count[16] = {0}, next[16] = {0};
  for (int s = 0; s < nsym; s++) count[lens[s]]++;
  count[0] = 0;
  uint32_t code = 0;
  for (int b = 1; b <= 15; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
  for (int s = 0; s < nsym; s++) {
    entries[s] = 0;
    if (!lens[s]) continue;
    const uint32_t c = next[lens[s]]++;
    uint32_t r = 0;
    for (int b = 0; b < lens[s]; b++) r |= ((c >> b) & 1u) << (lens[s] - 1 - b);
    entries[s] = r | (uint32_t)lens[s] << 16;
  }
}
void put_token(BitWriter &bw, const uint32_t *tab, Token t) {
  uint64_t v;
  const uint32_t nb = token_bits(tab, t, &v);
  bw.put(v & 0xffffffffu, std::min(nb, 32u));
  if (nb > 32) bw.put(v >> 32, nb - 32);
}
const uint32_t kAlphabet[5][2] = {{kGreen, kGreenSyms}, {kRed, 256}, {kBlue, 256}, {kAlpha, 256}, {kDist, kDistSyms}};
void write_group(BitWriter &bw, const uint32_t *hist, uint32_t *tab) {
  for (int a = 0; a < 5; a++) write_code(bw, hist + kAlphabet[a][0], (int)kAlphabet[a][1], tab + kAlphabet[a][0]);
}

struct Palette {
  uint32_t table[256];
  uint32_t colours = 0;  // 0: subtract green
  uint8_t rank[kHashSlots];
};
inline bool takes_index(const tm_webp_options &opt, uint32_t count) { return opt.palette == TM_WEBP_PALETTE_AUTO && count <= 256; }
void palette_of_slots(const uint32_t *slots, Palette &p) {
  p.colours = 0;
  for (uint32_t s = 0; s < kHashSlots; s++) if (slots[s] != kEmpty && p.colours < 256) p.table[p.colours++] = slots[s];
  std::sort(p.table, p.table + p.colours);
  memset(p.rank, 0, sizeof(p.rank));
  for (uint32_t s = 0; s < kHashSlots; s++)
    if (slots[s] != kEmpty) p.rank[s] = (uint8_t)(std::lower_bound(p.table, p.table + p.colours, slots[s]) - p.table);
}

Rect rect_host(const uint32_t *cur, int64_t stride_px, const uint32_t *old, int w, int h) {
  int x0 = w, y0 = h, x1 = -1, y1 = -1;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++)
      if (gfo::rgb_of(cur[(int64_t)y * stride_px + x]) != gfo::rgb_of(old[(int64_t)y * stride_px + x])) {
        x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
      }
  if (x1 < 0) return Rect{0, 0, 1, 1};
  x0 &= ~1; y0 &= ~1;
  return Rect{x0, y0, x1 - x0 + 1, y1 - y0 + 1};
}

// ---- the host IO: one lane
struct HostParse {
  const uint32_t *s = nullptr;
  const int32_t *links = nullptr;
  std::vector<Token> *tok = nullptr;
  int64_t nmatch = 0;
  uint32_t sym(uint32_t i) const { return s[i]; }
  int32_t prev(uint32_t i) const { return links[i]; }
  uint32_t common(uint32_t j, uint32_t i, uint32_t cap) const {
    uint32_t l = 0;
    while (l < cap && s[j + l] == s[i + l]) l++;
    return l;
  }
  void literal(uint32_t v) { tok->push_back(Token{v, 0}); }
  void match(uint32_t len, uint32_t dist) { tok->push_back(Token{len, dist}); nmatch++; }
};
void links_host(const uint32_t *s, uint32_t n, std::vector<int32_t> &prev) {
  prev.assign(n, -1);
  std::vector<uint64_t> order(n);  // key << 32 | position
  for (uint32_t i = 0; i < n; i++) order[i] = (uint64_t)key_of(s[i], i + 1 < n ? s[i + 1] : 0u, i + 2 < n ? s[i + 2] : 0u) << 32 | i;
  std::sort(order.begin(), order.end());
  for (uint32_t r = 1; r < n; r++)
    if (order[r] >> 32 == order[r - 1] >> 32) prev[(uint32_t)order[r]] = (int32_t)(uint32_t)order[r - 1];
}

int deliver(const char *who, const std::vector<uint8_t> &file, uint8_t *out, int64_t cap, int64_t *bytes) {
  *bytes = (int64_t)file.size();
  TM_CHECK((int64_t)file.size() <= cap, TM_E_INVAL, "%s: %lld bytes needed, %lld given", who, (long long)file.size(), (long long)cap);
  if (!file.empty()) memcpy(out, file.data(), file.size());
  return TM_OK;
}

}  // namespace

void write_code(BitWriter &bw, const uint32_t *freq, int nsym, uint32_t *entry) {
  memset(entry, 0, (size_t)nsym * 4);
  int used[2] = {0, 0}, nu = 0;
  bool small = true;
  for (int s = 0; s < nsym; s++)
    if (freq[s]) {
      if (nu < 2) used[nu] = s;
      nu++;
      if (s >= 256) small = false;
    }
  if (nu <= 2 && small) {  // a simple code; no used symbol: symbol 0 alone
    if (nu == 0) nu = 1;
    bw.put(1, 1); bw.put((uint32_t)nu - 1, 1);
    const bool wide = used[0] > 1;
    bw.put(wide ? 1 : 0, 1); bw.put((uint32_t)used[0], wide ? 8 : 1);
    if (nu == 2) {
      bw.put((uint32_t)used[1], 8);
      entry[used[0]] = 0u | 1u << 16; entry[used[1]] = 1u | 1u << 16;
    }
    return;
  }
  uint8_t lens[kGreenSyms];
  dfl::code_lengths(freq, nsym, 15, lens);
  canonical(lens, nsym, entry);
  // the lengths through a code of their own: a run of zeros as 18s (11 .. 138) while 11 or more are left, then one 17 (3 .. 10) or the
  // zeros themselves; every other length as itself (16 is not used)
  struct Item { uint8_t sym, ebits, eval; };
  Item items[kGreenSyms];
  int ni = 0;
  uint32_t cf[19] = {0};
  for (int s = 0; s < nsym;) {
    if (lens[s]) { items[ni++] = Item{lens[s], 0, 0}; cf[lens[s]]++; s++; continue; }
    int run = 1;
    while (s + run < nsym && !lens[s + run]) run++;
    s += run;
    while (run >= 11) { const int take = std::min(run, 138); items[ni++] = Item{18, 7, (uint8_t)(take - 11)}; cf[18]++; run -= take; }
    if (run >= 3) { items[ni++] = Item{17, 3, (uint8_t)(run - 3)}; cf[17]++; run = 0; }
    for (; run > 0; run--) { items[ni++] = Item{0, 0, 0}; cf[0]++; }
  }
  uint8_t cl[19];
  uint32_t ce[19];
  dfl::code_lengths(cf, 19, 7, cl);
  canonical(cl, 19, ce);
  static const int order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  int count = 19;
  while (count > 4 && !cl[order[count - 1]]) count--;
  bw.put(0, 1); bw.put((uint32_t)count - 4, 4);
  for (int k = 0; k < count; k++) bw.put(cl[order[k]], 3);
  bw.put(0, 1);  // the whole alphabet follows
  for (int k = 0; k < ni; k++) {
    bw.put(ce[items[k].sym] & 0xffffu, ce[items[k].sym] >> 16);
    if (items[k].ebits) bw.put(items[k].eval, items[k].ebits);
  }
}

void image_header_bits(BitWriter &bw, int w, int h, const uint32_t *table, uint32_t colours, const uint32_t *hist, uint32_t *tab) {
  bw.put(0x2f, 8); bw.put((uint32_t)w - 1, 14); bw.put((uint32_t)h - 1, 14); bw.put(0, 1); bw.put(0, 3);
  if (colours) {
    bw.put(1, 1); bw.put(3, 2); bw.put(colours - 1, 8);
    uint32_t diff[256], ph[kSyms] = {0}, pt[kSyms];
    uint32_t before = 0;
    for (uint32_t i = 0; i < colours; i++) {
      const uint32_t c = 0xff000000u | table[i];
      uint32_t d = 0;
      for (int b = 0; b < 32; b += 8) d |= (((c >> b) - (before >> b)) & 255u) << b;
      diff[i] = d; before = c;
      uint32_t slots[4];
      token_slots(Token{d, 0}, slots);
      for (int k = 0; k < 4; k++) ph[slots[k]]++;
    }
    bw.put(0, 1);  // no colour cache
    write_group(bw, ph, pt);
    for (uint32_t i = 0; i < colours; i++) put_token(bw, pt, Token{diff[i], 0});
  } else {
    bw.put(1, 1); bw.put(2, 2);
  }
  bw.put(0, 1);  // no further transform
  bw.put(0, 1);  // no colour cache
  bw.put(0, 1);  // no meta codes
  write_group(bw, hist, tab);
}

int webp_options_check(const char *who, const tm_webp_options *opt) {
  TM_CHECK(opt, TM_E_INVAL, "%s: null options", who);
  TM_CHECK(opt->diff == 0 || opt->diff == 1, TM_E_INVAL, "%s: diff %d (0 or 1)", who, opt->diff);
  TM_CHECK(opt->palette == TM_WEBP_PALETTE_AUTO || opt->palette == TM_WEBP_PALETTE_OFF, TM_E_INVAL, "%s: unknown palette %d", who, opt->palette);
  TM_CHECK(opt->lz77 == 0 || opt->lz77 == 1, TM_E_INVAL, "%s: lz77 %d (0 or 1)", who, opt->lz77);
  TM_CHECK(opt->segment_pixels >= 0, TM_E_INVAL, "%s: segment_pixels %d (0 and more)", who, opt->segment_pixels);
  TM_CHECK(opt->loop >= 0 && opt->loop <= 65535, TM_E_INVAL, "%s: loop %d (0 .. 65535)", who, opt->loop);
  TM_CHECK(opt->duration_ms >= 0 && opt->duration_ms <= (1 << 24) - 1, TM_E_INVAL, "%s: duration_ms %d (0 .. 2^24 - 1)", who, opt->duration_ms);
  return TM_OK;
}

int webp_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt, int *duration) {
  TM_TRY(webp_options_check(who, opt));
  TM_CHECK(w >= 1 && h >= 1, TM_E_INVAL, "%s: a picture of %d x %d", who, w, h);
  TM_CHECK(w <= kMaxSide && h <= kMaxSide, TM_E_UNSUPPORTED, "%s: a picture of %d x %d (%d a side at most)", who, w, h, kMaxSide);
  TM_CHECK(nframes >= 1, TM_E_INVAL, "%s: %d frames", who, nframes);
  TM_CHECK(frames, TM_E_INVAL, "%s: null frames", who);
  TM_CHECK(h == 1 || stride_px >= w, TM_E_INVAL, "%s: a row stride of %lld pixels for rows of %d", who, (long long)stride_px, w);
  TM_CHECK(nframes <= 1 || frame_px >= (int64_t)(h - 1) * stride_px + w, TM_E_INVAL, "%s: a frame stride of %lld pixels for frames of %lld", who, (long long)frame_px,
           (long long)((int64_t)(h - 1) * stride_px + w));
  int d = opt->duration_ms;
  if (!d) {
    TM_CHECK(fps > 0 && fps == fps, TM_E_INVAL, "%s: a rate of %g", who, fps);
    const double v = std::floor(1000.0 / fps + 0.5);
    TM_CHECK(v <= (double)((1 << 24) - 1), TM_E_INVAL, "%s: a rate of %g is a duration above 2^24 - 1", who, fps);
    d = std::max(1, (int)v);
  }
  *duration = d;
  return TM_OK;
}

int webp_chunk_frames(int w, int h) { return (int)std::max<size_t>(1, std::min<size_t>(kMaxChunk, ((size_t)256 << 20) / ((size_t)w * h * 4))); }

// per frame: the chunk headers and a pad byte; at most 31 300 header bits (two groups of codes with every length in 7 bits, a table of 256
// differences); a token of at most 60 bits per pixel
static int64_t webp_bound(int w, int h, int nframes) {
  return (int64_t)kFileHeader + (int64_t)nframes * (int64_t)(kFrameHeader + 1 + 4096 + (60ull * (uint64_t)w * h + 7) / 8);
}

// ---- the host twin
static int webp_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, int duration, const tm_webp_options &opt,
                            std::vector<uint8_t> &file, uint32_t *canvas, tm_webp_export_stats *st) {
  file.clear();
  file_header(w, h, opt.loop, file);
  std::vector<uint32_t> px, sym;
  std::vector<int32_t> links;
  std::vector<Token> tok;
  for (int f = 0; f < nframes; f++) {
    const uint32_t *cur = frames + (int64_t)f * frame_px;
    const Rect r = opt.diff && f > 0 ? rect_host(cur, stride_px, cur - frame_px, w, h) : Rect{0, 0, w, h};
    px.clear();
    for (int y = r.y; y < r.y + r.h; y++)
      for (int x = r.x; x < r.x + r.w; x++) px.push_back(gfo::rgb_of(cur[(int64_t)y * stride_px + x]));
    std::vector<uint32_t> table(px);
    std::sort(table.begin(), table.end());
    table.erase(std::unique(table.begin(), table.end()), table.end());
    const uint32_t colours = takes_index(opt, (uint32_t)std::min<size_t>(table.size(), 257)) ? (uint32_t)table.size() : 0u;
    const uint32_t per = colours ? bundle_of(colours) : 1u, pw = packed_width((uint32_t)r.w, per), n = pw * (uint32_t)r.h, bits = 8 / per;
    sym.assign(n, 0);
    for (uint32_t y = 0; y < (uint32_t)r.h; y++)
      for (uint32_t p = 0; p < pw; p++) {
        uint32_t v;
        if (colours) {
          uint32_t g = 0;
          for (uint32_t k = 0; k < per && p * per + k < (uint32_t)r.w; k++)
            g |= (uint32_t)(std::lower_bound(table.begin(), table.end(), px[(size_t)y * r.w + p * per + k]) - table.begin()) << (k * bits);
          v = 0xff000000u | g << 8;
        } else {
          v = subtract_green(px[(size_t)y * r.w + p]);
        }
        sym[(size_t)y * pw + p] = v;
      }
    if (opt.lz77) links_host(sym.data(), n, links);
    tok.clear();
    HostParse io;
    io.s = sym.data(); io.links = links.data(); io.tok = &tok;
    const uint32_t len = segment_len(n, (uint32_t)opt.segment_pixels), count = segment_count(n, (uint32_t)opt.segment_pixels);
    for (uint32_t s = 0; s < count; s++) parse_segment(io, s * len, std::min(n, (s + 1) * len), opt.lz77 != 0);
    uint32_t hist[kSyms] = {0}, tab[kSyms];
    for (const Token &t : tok) {
      uint32_t slots[4];
      const int ns = token_slots(t, slots);
      for (int k = 0; k < ns; k++) hist[slots[k]]++;
    }
    BitWriter bw;
    image_header_bits(bw, r.w, r.h, table.data(), colours, hist, tab);
    for (const Token &t : tok) put_token(bw, tab, t);
    bw.finish();
    const uint64_t payload = (bw.total + 7) / 8;
    frame_header(r, duration, payload, file);
    for (uint64_t k = 0; k < payload; k++) file.push_back((uint8_t)(bw.words[(size_t)(k / 4)] >> (8 * (k % 4))));
    if (payload & 1) file.push_back(0);
    st->frames++; st->frames_indexed += colours ? 1 : 0; st->segments += count; st->tokens += (int64_t)tok.size(); st->matches += io.nmatch;
    if (canvas) {
      uint32_t *c = canvas + (size_t)f * w * h;
      if (f > 0) memcpy(c, c - (size_t)w * h, (size_t)w * h * 4);
      for (int y = 0; y < r.h; y++)
        for (int x = 0; x < r.w; x++) c[(size_t)(r.y + y) * w + r.x + x] = px[(size_t)y * r.w + x];
    }
  }
  file_close(file);
  st->file_bytes = (int64_t)file.size();
  return TM_OK;
}

// ---- the device writer
struct WebpDeviceEncoder::State {
  DevBuf prev, raw, rects, tabs, counts, ranks, jobs, sym, keys, pos, keys_sorted, ord, tmp, links, segjobs, tok, hists, ntoks, nmatches, codes, words, bits, status, places,
      images, pieces, blob, out;
  std::vector<Rect> h_rects;
  std::vector<uint32_t> h_tabs, h_counts, h_hists, h_ntoks, h_nmatches, h_codes, h_header;
  std::vector<unsigned long long> h_bits;
  std::vector<uint8_t> h_out;
  int w = 0, h = 0, duration = 0, frame_no = 0;
  tm_webp_options opt{};
  hipStream_t stream = nullptr;
};
WebpDeviceEncoder::WebpDeviceEncoder() : state_(new State) {}
WebpDeviceEncoder::~WebpDeviceEncoder() { delete state_; }

int WebpDeviceEncoder::begin(int w, int h, double fps, const tm_webp_options &opt, void *hip_stream, std::vector<uint8_t> &file) {
  State &d = *state_;
  uint32_t dummy = 0;
  TM_TRY(webp_out_check("webp out", &dummy, w, (int64_t)w * h, 1, w, h, fps, &opt, &d.duration));
  d.w = w; d.h = h; d.opt = opt; d.stream = (hipStream_t)hip_stream; d.frame_no = 0;
  stats = tm_webp_export_stats{};
  file_header(w, h, opt.loop, file);
  return TM_OK;
}

int WebpDeviceEncoder::chunk(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nf, std::vector<uint8_t> &file) {
  State &d = *state_;
  hipStream_t stream = d.stream;
  const int w = d.w, h = d.h;
  const tm_webp_options &opt = d.opt;
  if (nf <= 0) return TM_OK;
  TM_CHECK(nf <= kMaxChunk, TM_E_INVAL, "webp out: a chunk of %d frames (%d at most)", nf, kMaxChunk);
  auto t0 = std::chrono::steady_clock::now();
  // rectangles and distinct colours
  TM_TRY(d.raw.alloc((size_t)nf * 16)); TM_TRY(d.rects.alloc((size_t)nf * sizeof(Rect))); TM_TRY(d.tabs.alloc((size_t)nf * kHashSlots * 4)); TM_TRY(d.counts.alloc((size_t)nf * 4));
  TM_TRY(d.prev.alloc((size_t)w * h * 4)); TM_TRY(d.status.alloc(4));
  TM_HIP(hipMemsetAsync(d.raw.p, 0x7f, (size_t)nf * 16, stream));
  TM_HIP(hipMemsetAsync(d.tabs.p, 0xff, (size_t)nf * kHashSlots * 4, stream));
  TM_HIP(hipMemsetAsync(d.counts.p, 0, (size_t)nf * 4, stream));
  TM_HIP(hipMemsetAsync(d.status.p, 0, 4, stream));
  if (opt.diff) gfo::launch_rect_raw(dev_frames, stride_px, frame_px, nf, d.prev.as<uint32_t>(), d.frame_no > 0 ? 1 : 0, w, h, d.raw.as<int32_t>(), stream);
  hipLaunchKernelGGL(k_webp_rect_fix, dim3((unsigned)(nf + 63) / 64), dim3(64), 0, stream, nf, d.frame_no == 0 ? 1 : 0, opt.diff, w, h, d.raw.as<int32_t>(), d.rects.as<Rect>());
  gfo::launch_colours(dev_frames, stride_px, frame_px, nf, w, h, d.rects.as<Rect>(), d.tabs.as<uint32_t>(), d.counts.as<uint32_t>(), 256, stream);
  TM_HIP(hipGetLastError());
  d.h_rects.resize((size_t)nf); d.h_tabs.resize((size_t)nf * kHashSlots); d.h_counts.resize((size_t)nf);
  TM_HIP(hipMemcpyAsync(d.h_rects.data(), d.rects.p, (size_t)nf * sizeof(Rect), hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_tabs.data(), d.tabs.p, (size_t)nf * kHashSlots * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_counts.data(), d.counts.p, (size_t)nf * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));
  std::vector<Palette> pals((size_t)nf);
  std::vector<FrameJob> jobs((size_t)nf);
  std::vector<uint8_t> ranks((size_t)nf * kHashSlots, 0);
  std::vector<SegJob> segs;
  std::vector<uint32_t> seg0((size_t)nf + 1, 0);
  uint64_t total = 0, nwords = 0;
  for (int f = 0; f < nf; f++) {
    const Rect &r = d.h_rects[(size_t)f];
    TM_CHECK(r.x >= 0 && r.y >= 0 && r.w >= 1 && r.h >= 1 && r.x + r.w <= w && r.y + r.h <= h && !(r.x & 1) && !(r.y & 1), TM_E_INTERNAL,
             "webp out: frame %d has a rectangle outside the picture", d.frame_no + f);
    Palette &p = pals[(size_t)f];
    if (takes_index(opt, d.h_counts[(size_t)f])) {
      palette_of_slots(d.h_tabs.data() + (size_t)f * kHashSlots, p);
      memcpy(ranks.data() + (size_t)f * kHashSlots, p.rank, kHashSlots);
    }
    const uint32_t per = p.colours ? bundle_of(p.colours) : 1u, pw = packed_width((uint32_t)r.w, per), n = pw * (uint32_t)r.h;
    jobs[(size_t)f] = FrameJob{r, total, n, pw, per, p.colours};
    const uint32_t len = segment_len(n, (uint32_t)opt.segment_pixels), count = segment_count(n, (uint32_t)opt.segment_pixels);
    for (uint32_t s = 0; s < count; s++) {
      const uint32_t begin = s * len, end = std::min(n, (s + 1) * len), cap = 2 * (end - begin) + 2;
      segs.push_back(SegJob{total, nwords, n, begin, end, (uint32_t)f, cap, 0});
      nwords += cap;
    }
    seg0[(size_t)f + 1] = (uint32_t)segs.size();
    total += n;
    stats.frames++; stats.frames_indexed += p.colours ? 1 : 0;
  }
  const size_t ns = segs.size();
  TM_CHECK(total < ((uint64_t)1 << 31) && ns < ((size_t)1 << 31), TM_E_UNSUPPORTED, "webp out: a chunk of %llu coded pixels in %zu segments", (unsigned long long)total, ns);
  stats.ms_colours += ms_since(t0); t0 = std::chrono::steady_clock::now();
  // symbols and links
  const unsigned fb = blocks_of((uint64_t)w * h, 1024);
  TM_TRY(d.jobs.alloc((size_t)nf * sizeof(FrameJob))); TM_TRY(d.ranks.alloc(ranks.size())); TM_TRY(d.sym.alloc(total * 4)); TM_TRY(d.links.alloc(total * 4));
  TM_HIP(hipMemcpyAsync(d.jobs.p, jobs.data(), (size_t)nf * sizeof(FrameJob), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.ranks.p, ranks.data(), ranks.size(), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_webp_symbols, dim3(fb, (unsigned)nf), dim3(256), 0, stream, dev_frames, stride_px, frame_px, d.jobs.as<FrameJob>(), d.tabs.as<uint32_t>(),
                     d.ranks.as<uint8_t>(), d.sym.as<uint32_t>(), total, d.status.as<int32_t>());
  if (opt.lz77) {
    TM_TRY(d.keys.alloc(total * 4)); TM_TRY(d.pos.alloc(total * 4)); TM_TRY(d.keys_sorted.alloc(total * 4)); TM_TRY(d.ord.alloc(total * 4));
    hipLaunchKernelGGL(k_webp_keys, dim3(fb, (unsigned)nf), dim3(256), 0, stream, d.jobs.as<FrameJob>(), d.sym.as<uint32_t>(), total, d.keys.as<uint32_t>(), d.pos.as<uint32_t>());
    TM_HIP(hipGetLastError());
    TM_TRY(with_temp(d.tmp, "webp out: radix sort of the positions", [&](void *t, size_t &b) {
      return rocprim::radix_sort_pairs(t, b, d.keys.as<uint32_t>(), d.keys_sorted.as<uint32_t>(), d.pos.as<uint32_t>(), d.ord.as<uint32_t>(), (size_t)total, 0, 32, stream);
    }));
    hipLaunchKernelGGL(k_webp_links, dim3(blocks_of(total, 16384)), dim3(256), 0, stream, d.jobs.as<FrameJob>(), d.keys_sorted.as<uint32_t>(), d.ord.as<uint32_t>(), (uint32_t)total,
                       d.links.as<int32_t>());
  }
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(stream));  // (jobs and ranks are read by then; the stage's time)
  stats.ms_match += ms_since(t0); t0 = std::chrono::steady_clock::now();
  // the parse and the histograms
  TM_TRY(d.segjobs.alloc(ns * sizeof(SegJob))); TM_TRY(d.tok.alloc(total * sizeof(Token))); TM_TRY(d.hists.alloc((size_t)nf * kSyms * 4)); TM_TRY(d.ntoks.alloc(ns * 4));
  TM_TRY(d.nmatches.alloc(ns * 4));
  TM_HIP(hipMemcpyAsync(d.segjobs.p, segs.data(), ns * sizeof(SegJob), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemsetAsync(d.hists.p, 0, (size_t)nf * kSyms * 4, stream));
  hipLaunchKernelGGL(k_webp_parse, dim3((unsigned)ns), dim3(64), 0, stream, d.segjobs.as<SegJob>(), d.sym.as<uint32_t>(), d.links.as<int32_t>(), total, opt.lz77, d.tok.as<Token>(),
                     d.hists.as<uint32_t>(), (uint32_t)nf, d.ntoks.as<uint32_t>(), d.nmatches.as<uint32_t>(), d.status.as<int32_t>());
  TM_HIP(hipGetLastError());
  d.h_hists.resize((size_t)nf * kSyms); d.h_ntoks.resize(ns); d.h_nmatches.resize(ns);
  int32_t rc = 0;
  TM_HIP(hipMemcpyAsync(d.h_hists.data(), d.hists.p, (size_t)nf * kSyms * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_ntoks.data(), d.ntoks.p, ns * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_nmatches.data(), d.nmatches.p, ns * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(&rc, d.status.p, 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));
  TM_CHECK(rc == 0, TM_E_INTERNAL, "webp out: the parse refused a segment or a colour (status %d)", rc);
  for (size_t s = 0; s < ns; s++) {
    TM_CHECK(d.h_ntoks[s] >= 1 && d.h_ntoks[s] <= segs[s].end - segs[s].begin, TM_E_INTERNAL, "webp out: a segment of %u tokens", d.h_ntoks[s]);
    stats.tokens += d.h_ntoks[s]; stats.matches += d.h_nmatches[s];
  }
  stats.segments += (int64_t)ns;
  stats.ms_parse += ms_since(t0); t0 = std::chrono::steady_clock::now();
  // the codes and the header bits: every image's header is one more span of words behind the segments'
  d.h_codes.resize((size_t)nf * kSyms);
  d.h_header.clear();
  std::vector<SegPlace> places;
  std::vector<uint64_t> header_bits((size_t)nf), header_off((size_t)nf);
  for (int f = 0; f < nf; f++) {
    BitWriter bw;
    image_header_bits(bw, d.h_rects[(size_t)f].w, d.h_rects[(size_t)f].h, pals[(size_t)f].table, pals[(size_t)f].colours, d.h_hists.data() + (size_t)f * kSyms,
                      d.h_codes.data() + (size_t)f * kSyms);
    bw.finish();
    header_bits[(size_t)f] = bw.total; header_off[(size_t)f] = nwords + d.h_header.size();
    d.h_header.insert(d.h_header.end(), bw.words.begin(), bw.words.end());
  }
  const uint64_t all_words = nwords + d.h_header.size();
  stats.ms_codes += ms_since(t0); t0 = std::chrono::steady_clock::now();
  // the bits
  TM_TRY(d.codes.alloc((size_t)nf * kSyms * 4)); TM_TRY(d.words.alloc(all_words * 4)); TM_TRY(d.bits.alloc(ns * 8));
  TM_HIP(hipMemcpyAsync(d.codes.p, d.h_codes.data(), (size_t)nf * kSyms * 4, hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.words.as<uint32_t>() + nwords, d.h_header.data(), d.h_header.size() * 4, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_webp_pack, dim3((unsigned)ns), dim3(256), 0, stream, d.segjobs.as<SegJob>(), d.tok.as<Token>(), total, d.ntoks.as<uint32_t>(), d.codes.as<uint32_t>(),
                     (uint32_t)nf, d.words.as<uint32_t>(), nwords, d.bits.as<unsigned long long>(), d.status.as<int32_t>());
  TM_HIP(hipGetLastError());
  d.h_bits.resize(ns);
  TM_HIP(hipMemcpyAsync(d.h_bits.data(), d.bits.p, ns * 8, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(&rc, d.status.p, 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));
  TM_CHECK(rc == 0, TM_E_INTERNAL, "webp out: the packer refused a segment (status %d)", rc);
  // places: per image its header, then its segments; the chunk's bytes: per image its chunk headers, its payload, a 0 when that is odd
  std::vector<ImagePlace> images((size_t)nf);
  std::vector<uint8_t> blob_bytes(1, 0);
  std::vector<Piece> pcs;
  uint64_t word0 = 0, at = 0;
  for (int f = 0; f < nf; f++) {
    ImagePlace &im = images[(size_t)f];
    im.seg0 = (uint32_t)places.size(); im.nseg = seg0[(size_t)f + 1] - seg0[(size_t)f] + 1;
    uint64_t bit = header_bits[(size_t)f];
    places.push_back(SegPlace{0, bit, header_off[(size_t)f]});
    for (uint32_t s = seg0[(size_t)f]; s < seg0[(size_t)f + 1]; s++) {
      TM_CHECK(d.h_bits[s] <= (uint64_t)segs[s].cap_words * 32, TM_E_INTERNAL, "webp out: a segment of %llu bits, above its bound", d.h_bits[s]);
      places.push_back(SegPlace{bit, d.h_bits[s], segs[s].word_off});
      bit += d.h_bits[s];
    }
    im.payload = (bit + 7) / 8;
    im.word0 = word0;
    word0 += (im.payload + 3) / 4;
    const size_t from = blob_bytes.size();
    frame_header(d.h_rects[(size_t)f], d.duration, im.payload, blob_bytes);
    pcs.push_back(Piece{from, at, (uint32_t)(blob_bytes.size() - from), 0});
    at += blob_bytes.size() - from;
    im.pos = at;
    at += im.payload;
    if (im.payload & 1) { pcs.push_back(Piece{0, at, 1, 0}); at++; }
  }
  TM_TRY(d.places.alloc(places.size() * sizeof(SegPlace))); TM_TRY(d.images.alloc(images.size() * sizeof(ImagePlace))); TM_TRY(d.out.alloc(at));
  TM_TRY(d.pieces.alloc(pcs.size() * sizeof(Piece))); TM_TRY(d.blob.alloc(blob_bytes.size()));
  TM_HIP(hipMemcpyAsync(d.places.p, places.data(), places.size() * sizeof(SegPlace), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.images.p, images.data(), images.size() * sizeof(ImagePlace), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.pieces.p, pcs.data(), pcs.size() * sizeof(Piece), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.blob.p, blob_bytes.data(), blob_bytes.size(), hipMemcpyHostToDevice, stream));
  gfo::launch_emit(d.images.as<ImagePlace>(), (uint32_t)nf, d.places.as<SegPlace>(), d.words.as<uint32_t>(), all_words, word0, d.out.as<uint8_t>(), at, 0, stream);
  gfo::launch_blob(d.pieces.as<Piece>(), (uint32_t)pcs.size(), d.blob.as<uint8_t>(), (uint64_t)blob_bytes.size(), d.out.as<uint8_t>(), at, stream);
  TM_HIP(hipGetLastError());
  d.h_out.resize(at);
  TM_HIP(hipMemcpyAsync(d.h_out.data(), d.out.p, at, hipMemcpyDeviceToHost, stream));
  // the last frame stays for the next chunk's first rectangle
  TM_HIP(hipMemcpy2DAsync(d.prev.p, (size_t)w * 4, dev_frames + (int64_t)(nf - 1) * frame_px, (size_t)(h == 1 ? w : stride_px) * 4, (size_t)w * 4, (size_t)h,
                          hipMemcpyDeviceToDevice, stream));
  TM_HIP(hipStreamSynchronize(stream));
  file.insert(file.end(), d.h_out.begin(), d.h_out.end());
  d.frame_no += nf;
  stats.ms_emit += ms_since(t0);
  return TM_OK;
}

int WebpDeviceEncoder::end(std::vector<uint8_t> &file) {
  file_close(file);
  stats.file_bytes = (int64_t)file.size();
  return TM_OK;
}

}  // namespace wpo
}  // namespace tmx

extern "C" {

int tm_webp_bound_host(int w, int h, int nframes, const tm_webp_options *opt, int64_t *bytes) {
  using namespace tmx;
  TM_CHECK(bytes, TM_E_INVAL, "tm_webp_bound_host: null argument");
  uint32_t dummy = 0;
  int duration;
  TM_TRY(wpo::webp_out_check("tm_webp_bound_host", &dummy, w, (int64_t)w * h, nframes, w, h, 10.0, opt, &duration));
  *bytes = wpo::webp_bound(w, h, nframes);
  return TM_OK;
}

int tm_webp_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt, uint8_t *out,
                        int64_t cap, int64_t *bytes, uint32_t *canvas, tm_webp_export_stats *stats) {
  using namespace tmx;
  int duration;
  TM_TRY(wpo::webp_out_check("tm_webp_encode_host", frames, stride_px, frame_px, nframes, w, h, fps, opt, &duration));
  TM_CHECK(bytes && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_webp_encode_host: null argument");
  std::vector<uint8_t> file;
  tm_webp_export_stats st{};
  TM_TRY(wpo::webp_encode_host(frames, stride_px, frame_px, nframes, w, h, duration, *opt, file, canvas, &st));
  if (stats) *stats = st;
  return wpo::deliver("tm_webp_encode_host", file, out, cap, bytes);
}

int tm_stage_webp_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_webp_options *opt, int chunk_frames,
                         uint8_t *out, int64_t cap, int64_t *bytes, tm_webp_export_stats *stats, void *stream) {
  using namespace tmx;
  int duration;
  TM_TRY(wpo::webp_out_check("tm_stage_webp_encode", dev_frames, stride_px, frame_px, nframes, w, h, fps, opt, &duration));
  TM_CHECK(bytes && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_stage_webp_encode: null argument");
  TM_TRY(require_device());
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> file;
  wpo::WebpDeviceEncoder encoder;
  TM_TRY(encoder.begin(w, h, fps, *opt, stream, file));
  const int chunk = chunk_frames > 0 ? std::min(chunk_frames, (int)wpo::kMaxChunk) : wpo::webp_chunk_frames(w, h);
  for (int f0 = 0; f0 < nframes; f0 += chunk) TM_TRY(encoder.chunk(dev_frames + (int64_t)f0 * frame_px, stride_px, frame_px, std::min(chunk, nframes - f0), file));
  TM_TRY(encoder.end(file));
  encoder.stats.ms_device = encoder.stats.ms_wall = wpo::ms_since(t0);
  if (stats) *stats = encoder.stats;
  return wpo::deliver("tm_stage_webp_encode", file, out, cap, bytes);
}

}  // extern "C"
