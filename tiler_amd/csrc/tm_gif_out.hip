// tm_gif_out.hip -- the GIF writer on the device and its host twin.  The rule is tm_gif_out.h's; both forms write
// the same bytes.  A chunk of frames goes through these stages on the caller's stream, every frame of the chunk in the same launches:
//
//   rect      k_gif_rect: a frame's changed pixels against the frame before (the chunk's first against the frame kept from the chunk
//             before), min / max in LDS and one set of atomics a workgroup; k_gif_rect_fix makes the rule's rectangle of it.
//   colours   k_gif_colours: per frame an open-addressed table of the rectangle's distinct colours, one compare-and-swap per probe, and
//             a count that stops above max_colours.  Rectangles, tables and counts come to the host (read-back 1), which sorts the exact
//             frames' colours into a table and a rank per slot.  For the frames to quantise k_gif_hist fills the 32 768 cells (read-back
//             1b, only then) and the host runs the cut: a table and a cell -> box map.
//   map       k_gif_map: pixel -> stored index of the rectangle (the rank of its slot, or its cell's box).
//   lzw       k_gif_lzw_pack: one wave (one workgroup) per segment, every segment of the chunk in one launch; the coder's state is the
//             same in every lane.  In LDS (25 088 bytes: six workgroups to a compute unit): the dictionary, 96 buckets of 64 slots of
//             (prefix code, byte, code); a lookup is one LDS access of the whole bucket, a lane a slot, and a ballot -- lane l only ever
//             reads and writes column l, so nothing but the ballot crosses lanes; a full bucket passes on to the next.  256 staged
//             indices, and 64 words of output that the lanes store together.  Output: the segment's bits in a span of its own, sized by
//             the bound, and its bit count (read-back 2).
//   place     the host adds the bit counts up (a few thousand at most): each segment's bit offset in its image, each image's payload and
//             place in the chunk's bytes; it also makes the blob of headers and tables.
//   emit      k_gif_emit: a lane per four payload bytes: the 32 bits at its offset out of the one or more segments that hold them, each
//             piece by a funnel shift of two words; payload byte j goes to base + j + j / 255 + 1, the sub-block lengths between.
//             k_gif_blob copies headers, tables, terminators and the trailer.  One copy brings the chunk's bytes back (read-back 3).
//
// Every loop is bounded by the rectangle, the segment, the table or the grid; plain launches, nothing waits on another workgroup; every
// store is checked against the buffer it goes to.
#include <chrono>

#include "tm_common.h"
#include "tm_gif_out.h"

namespace tmx {
namespace gfo {
namespace {

constexpr uint32_t kBuckets = 96;  // of 64 slots: 6144 slots for at most 4094 entries
constexpr uint32_t kStage = 256;
constexpr int32_t kRectInit = 0x7f7f7f7f;

struct FrameJob {
  Rect r;
  uint64_t idx_off;  // its stored indices in the chunk's index buffer
  int32_t exact;
  uint32_t map;      // quantised: which cell -> box map
};
struct SegJob {
  uint64_t idx_off, word_off;
  uint32_t n, min_code, first, last, cap_words, pad;
};

inline unsigned blocks_of(uint64_t n, unsigned most) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, most)); }
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// ---- rectangles.  raw: per frame min x, min y, min (65535 - x), min (65535 - y), each from kRectInit
__global__ __launch_bounds__(256) void k_gif_rect(const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, const uint32_t *__restrict__ prev, int has_prev,
                                                  int w, int h, int32_t *__restrict__ raw) {
  __shared__ int32_t box[4];
  const uint32_t f = blockIdx.y;
  if (threadIdx.x < 4) box[threadIdx.x] = kRectInit;
  __syncthreads();
  if (f > 0 || has_prev) {
    const uint32_t *cur = frames + (int64_t)f * frame_px;
    const uint32_t *old = f > 0 ? cur - frame_px : prev;
    const int64_t old_stride = f > 0 ? stride_px : (int64_t)w;
    const uint64_t n = (uint64_t)w * h;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
      const int x = (int)(i % (uint32_t)w), y = (int)(i / (uint32_t)w);
      if (rgb_of(cur[(int64_t)y * stride_px + x]) != rgb_of(old[(int64_t)y * old_stride + x])) {
        atomicMin(&box[0], x); atomicMin(&box[1], y); atomicMin(&box[2], 65535 - x); atomicMin(&box[3], 65535 - y);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && box[threadIdx.x] != kRectInit) atomicMin(&raw[f * 4 + threadIdx.x], box[threadIdx.x]);
}
// whole: the chunk's first frame is the file's first
__global__ void k_gif_rect_fix(int nf, int whole_first, int diff, int w, int h, const int32_t *__restrict__ raw, Rect *__restrict__ rects) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= nf) return;
  Rect r{0, 0, w, h};
  if (diff && !(whole_first && f == 0)) {
    if (raw[f * 4] == kRectInit) r = Rect{0, 0, 1, 1};
    else r = Rect{raw[f * 4], raw[f * 4 + 1], 65535 - raw[f * 4 + 2] - raw[f * 4] + 1, 65535 - raw[f * 4 + 3] - raw[f * 4 + 1] + 1};
  }
  rects[f] = r;
}

// ---- distinct colours
__global__ __launch_bounds__(256) void k_gif_colours(const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, const Rect *__restrict__ rects,
                                                     uint32_t *tabs, uint32_t *counts, uint32_t max_colours) {
  const uint32_t f = blockIdx.y;
  const Rect r = rects[f];
  const uint32_t *cur = frames + (int64_t)f * frame_px;
  uint32_t *tab = tabs + (size_t)f * kHashSlots;
  const uint64_t n = (uint64_t)r.w * r.h;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = rgb_of(cur[(int64_t)(r.y + (int)(i / (uint32_t)r.w)) * stride_px + r.x + (int)(i % (uint32_t)r.w)]);
    uint32_t slot = colour_hash(c);
    for (uint32_t probe = 0; probe < kHashSlots; probe++, slot = (slot + 1) & (kHashSlots - 1)) {
      uint32_t at = __atomic_load_n(&tab[slot], __ATOMIC_RELAXED);
      if (at == c) break;
      if (at != kEmpty) continue;
      if (__atomic_load_n(&counts[f], __ATOMIC_RELAXED) > max_colours) break;  // (it has told all it must)
      at = atomicCAS(&tab[slot], kEmpty, c);
      if (at == kEmpty) { atomicAdd(&counts[f], 1u); break; }
      if (at == c) break;
    }
  }
}

__global__ __launch_bounds__(256) void k_gif_hist(const uint32_t *__restrict__ frame, int64_t stride_px, Rect r, Cell *__restrict__ cells) {
  const uint64_t n = (uint64_t)r.w * r.h;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = rgb_of(frame[(int64_t)(r.y + (int)(i / (uint32_t)r.w)) * stride_px + r.x + (int)(i % (uint32_t)r.w)]);
    Cell *cell = cells + cell_of(c);
    atomicAdd(&cell->n, 1ull); atomicAdd(&cell->r, (unsigned long long)(c >> 16)); atomicAdd(&cell->g, (unsigned long long)(c >> 8 & 255u));
    atomicAdd(&cell->b, (unsigned long long)(c & 255u));
  }
}

// ---- pixels -> stored indices
__global__ __launch_bounds__(256) void k_gif_map(const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, const FrameJob *__restrict__ jobs,
                                                 const uint32_t *__restrict__ tabs, const uint8_t *__restrict__ ranks, const uint8_t *__restrict__ cellmaps,
                                                 uint8_t *__restrict__ idx, uint64_t idx_bytes, int32_t *__restrict__ status) {
  const uint32_t f = blockIdx.y;
  const FrameJob j = jobs[f];
  const uint32_t *cur = frames + (int64_t)f * frame_px;
  const uint32_t *tab = tabs + (size_t)f * kHashSlots;
  const uint64_t n = (uint64_t)j.r.w * j.r.h;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = rgb_of(cur[(int64_t)(j.r.y + (int)(i / (uint32_t)j.r.w)) * stride_px + j.r.x + (int)(i % (uint32_t)j.r.w)]);
    uint32_t v = 0;
    if (j.exact) {
      uint32_t slot = colour_hash(c), probe = 0;
      while (probe < kHashSlots && tab[slot] != c) { probe++; slot = (slot + 1) & (kHashSlots - 1); }
      if (probe < kHashSlots) v = ranks[(size_t)f * kHashSlots + slot];
      else atomicMax(status, 1);
    } else {
      v = cellmaps[(size_t)j.map * kCells + cell_of(c)];
    }
    if (j.idx_off + i < idx_bytes) idx[j.idx_off + i] = (uint8_t)v;
  }
}

// ---- LZW: the device IO, one wave
struct PackLds {
  uint32_t slots[kBuckets * 64];  // key << 12 | code, key = prefix << 8 | byte
  uint32_t outw[64];
  uint8_t stage[kStage];
};
struct WavePack {
  PackLds &m;
  const uint8_t *idx;
  uint32_t n;
  uint32_t *words;
  uint32_t cap;
  uint32_t lane;
  uint32_t window = 0xffffffffu;  // the first of the staged indices
  uint32_t ins = 0;               // where the string of the last failed find goes
  uint64_t acc = 0, total = 0;
  uint32_t nb = 0, nw = 0, written = 0;
  __device__ WavePack(PackLds &m_, const uint8_t *idx_, uint32_t n_, uint32_t *words_, uint32_t cap_) : m(m_), idx(idx_), n(n_), words(words_), cap(cap_), lane(threadIdx.x) {}
  __device__ uint32_t index(uint32_t i) {
    const uint32_t at = i & ~(kStage - 1);
    if (at != window) {
      __syncthreads();
      for (uint32_t k = lane; k < kStage; k += 64) m.stage[k] = at + k < n ? idx[at + k] : (uint8_t)0;
      __syncthreads();
      window = at;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)m.stage[i & (kStage - 1)]);
  }
  __device__ void reset() {
    for (uint32_t b = 0; b < kBuckets; b++) m.slots[b * 64 + lane] = kEmpty;
  }
  __device__ uint32_t find(uint32_t prefix, uint32_t byte) {
    const uint32_t key = prefix << 8 | byte;
    uint32_t b = ((key * 2654435761u) >> 20) % kBuckets;
    for (uint32_t probe = 0; probe < kBuckets; probe++) {
      const uint32_t v = m.slots[b * 64 + lane];
      const unsigned long long hit = __ballot(v != kEmpty && (v >> 12) == key);
      if (hit) return (uint32_t)__builtin_amdgcn_readlane((int)v, __ffsll((long long)hit) - 1) & 4095u;
      const unsigned long long free_ = __ballot(v == kEmpty);
      if (free_) { ins = b * 64 + (uint32_t)(__ffsll((long long)free_) - 1); return kNoCode; }
      b = b + 1 == kBuckets ? 0 : b + 1;
    }
    ins = kBuckets * 64;  // (cannot be: 6144 slots, 4094 entries)
    return kNoCode;
  }
  __device__ void add(uint32_t prefix, uint32_t byte, uint32_t code) {
    if (ins < kBuckets * 64 && (ins & 63u) == lane) m.slots[ins] = (prefix << 8 | byte) << 12 | code;
  }
  __device__ void flush() {
    if (lane < nw && written + lane < cap) words[written + lane] = m.outw[lane];  // (outw[lane]: every lane wrote it itself)
    written += nw;
    nw = 0;
  }
  __device__ void put(uint32_t code, uint32_t width) {
    acc |= (uint64_t)code << nb;
    nb += width; total += width;
    if (nb >= 32) {
      m.outw[nw++] = (uint32_t)acc;  // (every lane writes the same value)
      acc >>= 32; nb -= 32;
      if (nw == 64) flush();
    }
  }
  __device__ void finish() {
    if (nb) { m.outw[nw++] = (uint32_t)acc; nb = 0; }
    flush();
  }
};

__global__ __launch_bounds__(64) void k_gif_lzw_pack(const SegJob *__restrict__ jobs, const uint8_t *__restrict__ idx, uint64_t idx_bytes, uint32_t *__restrict__ words,
                                                     uint64_t nwords, unsigned long long *__restrict__ bits, int32_t *__restrict__ status) {
  __shared__ __align__(16) PackLds lds;
  const SegJob j = jobs[blockIdx.x];
  // a job that points outside what the launch was given is refused untouched
  if (j.n == 0 || j.idx_off > idx_bytes || j.n > idx_bytes - j.idx_off || j.word_off > nwords || j.cap_words > nwords - j.word_off || j.min_code < 2 || j.min_code > 8) {
    if (threadIdx.x == 0) { bits[blockIdx.x] = 0; atomicMax(status, 2); }
    return;
  }
  WavePack io(lds, idx + j.idx_off, j.n, words + j.word_off, j.cap_words);
  lzw_segment(io, j.n, j.min_code, j.first != 0, j.last != 0);
  io.finish();
  if (threadIdx.x == 0) {
    bits[blockIdx.x] = io.total;
    if (io.written > j.cap_words) atomicMax(status, 3);
  }
}

// ---- the bits to their place
__global__ __launch_bounds__(256) void k_gif_emit(const ImagePlace *__restrict__ images, uint32_t nimages, const SegPlace *__restrict__ segs, const uint32_t *__restrict__ words,
                                                  uint64_t nwords, uint64_t total_words, uint8_t *__restrict__ out, uint64_t out_bytes, int sub) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total_words; t += (uint64_t)gridDim.x * 256) {
    uint32_t lo = 0, hi = nimages;  // the last image that starts at or before word t
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (images[mid].word0 <= t) lo = mid; else hi = mid;
    }
    const ImagePlace im = images[lo];
    const uint64_t k = t - im.word0;
    if (4 * k >= im.payload) continue;
    const SegPlace *sg = segs + im.seg0;
    uint32_t s0 = 0, s1 = im.nseg;  // the last segment that starts at or before bit 32 k
    while (s1 - s0 > 1) {
      const uint32_t mid = s0 + (s1 - s0) / 2;
      if (sg[mid].bit_off <= 32 * k) s0 = mid; else s1 = mid;
    }
    uint32_t v = 0;
    uint64_t pos = 32 * k;
    const uint64_t end = 32 * k + 32;
    while (pos < end && s0 < im.nseg) {
      const SegPlace p = sg[s0];
      const uint64_t in = pos - p.bit_off;
      const uint32_t take = (uint32_t)(end - pos < p.bits - in ? end - pos : p.bits - in);
      const uint64_t wd = p.word_off + (in >> 5);
      const uint32_t sh = (uint32_t)in & 31u;
      const uint32_t a = wd < nwords ? words[wd] : 0u;
      const uint32_t b = sh + take > 32 && wd + 1 < nwords ? words[wd + 1] : 0u;
      uint32_t piece = __funnelshift_r(a, b, sh);
      if (take < 32) piece &= (1u << take) - 1u;
      v |= piece << (uint32_t)(pos - 32 * k);
      pos += take;
      s0++;
    }
    for (uint32_t q = 0; q < 4; q++) {
      const uint64_t j = 4 * k + q;
      if (j >= im.payload) break;
      const uint64_t to = sub ? im.pos + j + j / 255 + 1 : im.pos + j;
      if (to < out_bytes) out[to] = (uint8_t)(v >> (8 * q));
      if (sub && j % 255 == 0 && to - 1 < out_bytes) out[to - 1] = (uint8_t)(im.payload - j < 255 ? im.payload - j : 255);
    }
  }
}
__global__ __launch_bounds__(256) void k_gif_blob(const Piece *__restrict__ pieces, const uint8_t *__restrict__ blob, uint64_t blob_bytes, uint8_t *__restrict__ out,
                                                  uint64_t out_bytes) {
  const Piece p = pieces[blockIdx.x];
  for (uint32_t k = threadIdx.x; k < p.n; k += 256)
    if (p.from + k < blob_bytes && p.to + k < out_bytes) out[p.to + k] = blob[p.from + k];
}

}  // namespace

// ---- the launches another writer shares (tm_gif_out.h)
void launch_rect_raw(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, const uint32_t *dev_prev, int has_prev, int w, int h, int32_t *dev_raw,
                     hipStream_t stream) {
  hipLaunchKernelGGL(k_gif_rect, dim3(blocks_of((uint64_t)w * h, 1024), (unsigned)nframes), dim3(256), 0, stream, dev_frames, stride_px, frame_px, dev_prev, has_prev, w, h, dev_raw);
}
void launch_colours(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const Rect *dev_rects, uint32_t *dev_tabs, uint32_t *dev_counts,
                    uint32_t max_colours, hipStream_t stream) {
  hipLaunchKernelGGL(k_gif_colours, dim3(blocks_of((uint64_t)w * h, 1024), (unsigned)nframes), dim3(256), 0, stream, dev_frames, stride_px, frame_px, dev_rects, dev_tabs, dev_counts,
                     max_colours);
}
void launch_emit(const ImagePlace *dev_images, uint32_t nimages, const SegPlace *dev_segs, const uint32_t *dev_words, uint64_t nwords, uint64_t total_words, uint8_t *dev_out,
                 uint64_t out_bytes, int sub, hipStream_t stream) {
  hipLaunchKernelGGL(k_gif_emit, dim3(blocks_of(total_words, 16384)), dim3(256), 0, stream, dev_images, nimages, dev_segs, dev_words, nwords, total_words, dev_out, out_bytes, sub);
}
void launch_blob(const Piece *dev_pieces, uint32_t npieces, const uint8_t *dev_blob, uint64_t blob_bytes, uint8_t *dev_out, uint64_t out_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(k_gif_blob, dim3(npieces), dim3(256), 0, stream, dev_pieces, dev_blob, blob_bytes, dev_out, out_bytes);
}

namespace {

// ---- what both forms share on the host
struct Palette {
  uint32_t table[256];
  uint32_t colours = 0;
  bool exact = true;
  uint8_t rank[kHashSlots];           // exact: the rank of every slot's colour
  std::vector<uint8_t> cell_box;      // quantised
};
void exact_palette(const uint32_t *slots, Palette &p) {
  p.exact = true; p.colours = 0;
  for (uint32_t s = 0; s < kHashSlots; s++) if (slots[s] != kEmpty && p.colours < 256) p.table[p.colours++] = slots[s];
  std::sort(p.table, p.table + p.colours);
  memset(p.rank, 0, sizeof(p.rank));
  for (uint32_t s = 0; s < kHashSlots; s++)
    if (slots[s] != kEmpty) p.rank[s] = (uint8_t)(std::lower_bound(p.table, p.table + p.colours, slots[s]) - p.table);
}
void quantised_palette(const Cell *cells, uint32_t max_colours, Palette &p) {
  p.exact = false;
  p.cell_box.resize(kCells);
  p.colours = median_cut(cells, max_colours, p.table, p.cell_box.data());
}
inline bool takes_exact(const tm_gif_options &opt, uint32_t count) { return opt.colours != TM_GIF_COLOURS_QUANTISE && count <= (uint32_t)opt.max_colours; }

// the host's table of a rectangle's distinct colours; the count stops above max_colours
void colours_host(const uint32_t *frame, int64_t stride_px, const Rect &r, uint32_t max_colours, uint32_t *slots, uint32_t *count) {
  std::fill(slots, slots + kHashSlots, kEmpty);
  *count = 0;
  for (int y = r.y; y < r.y + r.h && *count <= max_colours; y++)
    for (int x = r.x; x < r.x + r.w && *count <= max_colours; x++) {
      const uint32_t c = rgb_of(frame[(int64_t)y * stride_px + x]);
      uint32_t slot = colour_hash(c);
      while (slots[slot] != kEmpty && slots[slot] != c) slot = (slot + 1) & (kHashSlots - 1);
      if (slots[slot] == kEmpty) { slots[slot] = c; (*count)++; }
    }
}
size_t distinct_host(const uint32_t *frame, int64_t stride_px, const Rect &r) {
  std::vector<uint32_t> v;
  v.reserve((size_t)r.w * r.h);
  for (int y = r.y; y < r.y + r.h; y++)
    for (int x = r.x; x < r.x + r.w; x++) v.push_back(rgb_of(frame[(int64_t)y * stride_px + x]));
  std::sort(v.begin(), v.end());
  return (size_t)(std::unique(v.begin(), v.end()) - v.begin());
}
Rect rect_host(const uint32_t *cur, int64_t stride_px, const uint32_t *old, int64_t old_stride, int w, int h) {
  int x0 = w, y0 = h, x1 = -1, y1 = -1;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++)
      if (rgb_of(cur[(int64_t)y * stride_px + x]) != rgb_of(old[(int64_t)y * old_stride + x])) {
        x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
      }
  if (x1 < 0) return Rect{0, 0, 1, 1};
  return Rect{x0, y0, x1 - x0 + 1, y1 - y0 + 1};
}
// table and stored indices of one frame's rectangle
int palettise_host(const char *who, const uint32_t *frame, int64_t stride_px, const Rect &r, const tm_gif_options &opt, int frame_no, Palette &p, std::vector<uint8_t> &idx) {
  uint32_t slots[kHashSlots], count;
  colours_host(frame, stride_px, r, (uint32_t)opt.max_colours, slots, &count);
  idx.resize((size_t)r.w * r.h);
  size_t at = 0;
  if (takes_exact(opt, count)) {
    exact_palette(slots, p);
    for (int y = r.y; y < r.y + r.h; y++)
      for (int x = r.x; x < r.x + r.w; x++) {
        const uint32_t c = rgb_of(frame[(int64_t)y * stride_px + x]);
        uint32_t slot = colour_hash(c);
        while (slots[slot] != c) slot = (slot + 1) & (kHashSlots - 1);
        idx[at++] = p.rank[slot];
      }
    return TM_OK;
  }
  TM_CHECK(opt.colours != TM_GIF_COLOURS_EXACT, TM_E_UNSUPPORTED, "%s: frame %d holds %zu colours, a table %d", who, frame_no, distinct_host(frame, stride_px, r),
           opt.max_colours);
  std::vector<Cell> cells(kCells, Cell{0, 0, 0, 0});
  for (int y = r.y; y < r.y + r.h; y++)
    for (int x = r.x; x < r.x + r.w; x++) {
      const uint32_t c = rgb_of(frame[(int64_t)y * stride_px + x]);
      Cell &cell = cells[cell_of(c)];
      cell.n++; cell.r += c >> 16; cell.g += c >> 8 & 255u; cell.b += c & 255u;
    }
  quantised_palette(cells.data(), (uint32_t)opt.max_colours, p);
  for (int y = r.y; y < r.y + r.h; y++)
    for (int x = r.x; x < r.x + r.w; x++) idx[at++] = p.cell_box[cell_of(rgb_of(frame[(int64_t)y * stride_px + x]))];
  return TM_OK;
}

// ---- the host IO: one lane; an image's segments share the bit stream
struct HostPack {
  const uint8_t *idx = nullptr;
  std::vector<uint32_t> tab = std::vector<uint32_t>((size_t)kCodes * 256, 0u);  // stamp << 12 | code
  uint32_t stamp = 0;
  std::vector<uint8_t> *out = nullptr;
  uint64_t acc = 0;
  uint32_t nb = 0;
  uint32_t index(uint32_t i) const { return idx[i]; }
  void reset() { stamp++; }
  uint32_t find(uint32_t prefix, uint32_t byte) const { const uint32_t v = tab[(size_t)prefix << 8 | byte]; return (v >> 12) == stamp ? (v & 4095u) : kNoCode; }
  void add(uint32_t prefix, uint32_t byte, uint32_t code) { tab[(size_t)prefix << 8 | byte] = stamp << 12 | code; }
  void put(uint32_t code, uint32_t width) {
    acc |= (uint64_t)code << nb;
    nb += width;
    while (nb >= 8) { out->push_back((uint8_t)acc); acc >>= 8; nb -= 8; }
  }
  void finish() { if (nb) { out->push_back((uint8_t)acc); acc = 0; nb = 0; } }
};
// the payload of n indices, before sub-blocks
void lzw_pack_host(HostPack &io, const uint8_t *idx, uint32_t n, uint32_t min_code, uint32_t segment_pixels, std::vector<uint8_t> &payload, int64_t *segments) {
  payload.clear();
  io.out = &payload;
  const uint32_t len = segment_len(n, segment_pixels), count = segment_count(n, segment_pixels);
  for (uint32_t s = 0; s < count; s++) {
    if (io.stamp >= (1u << 20) - 2) { std::fill(io.tab.begin(), io.tab.end(), 0u); io.stamp = 0; }
    io.idx = idx + (size_t)s * len;
    lzw_segment(io, std::min(len, n - s * len), min_code, s == 0, s + 1 == count);
  }
  io.finish();
  if (segments) *segments += count;
}
void put_sub_blocks(const std::vector<uint8_t> &payload, std::vector<uint8_t> &f) {
  for (size_t at = 0; at < payload.size(); at += 255) {
    const size_t n = std::min<size_t>(255, payload.size() - at);
    f.push_back((uint8_t)n);
    f.insert(f.end(), payload.begin() + (ptrdiff_t)at, payload.begin() + (ptrdiff_t)(at + n));
  }
  f.push_back(0);
}

int deliver(const char *who, const std::vector<uint8_t> &file, uint8_t *out, int64_t cap, int64_t *bytes) {
  *bytes = (int64_t)file.size();
  TM_CHECK((int64_t)file.size() <= cap, TM_E_INVAL, "%s: %lld bytes needed, %lld given", who, (long long)file.size(), (long long)cap);
  if (!file.empty()) memcpy(out, file.data(), file.size());
  return TM_OK;
}

}  // namespace

int gif_options_check(const char *who, const tm_gif_options *opt) {
  TM_CHECK(opt, TM_E_INVAL, "%s: null options", who);
  TM_CHECK(opt->colours >= TM_GIF_COLOURS_AUTO && opt->colours <= TM_GIF_COLOURS_QUANTISE, TM_E_INVAL, "%s: unknown colours %d", who, opt->colours);
  TM_CHECK(opt->max_colours >= 2 && opt->max_colours <= 256, TM_E_INVAL, "%s: max_colours %d (2 .. 256)", who, opt->max_colours);
  TM_CHECK(opt->diff == 0 || opt->diff == 1, TM_E_INVAL, "%s: diff %d (0 or 1)", who, opt->diff);
  TM_CHECK(opt->segment_pixels == 0 || opt->segment_pixels >= 256, TM_E_INVAL, "%s: segment_pixels %d (0, or 256 and more)", who, opt->segment_pixels);
  TM_CHECK(opt->loop >= -1 && opt->loop <= 65535, TM_E_INVAL, "%s: loop %d (-1 .. 65535)", who, opt->loop);
  TM_CHECK(opt->delay_cs == 0 || (opt->delay_cs >= 2 && opt->delay_cs <= 65535), TM_E_INVAL, "%s: delay_cs %d (0, or 2 .. 65535)", who, opt->delay_cs);
  return TM_OK;
}

int gif_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt, int *delay) {
  TM_TRY(gif_options_check(who, opt));
  TM_CHECK(w >= 1 && h >= 1, TM_E_INVAL, "%s: a picture of %d x %d", who, w, h);
  TM_CHECK(w <= 65535 && h <= 65535, TM_E_UNSUPPORTED, "%s: a picture of %d x %d (65535 a side at most)", who, w, h);
  TM_CHECK((uint64_t)w * (uint64_t)h <= kMaxPixels, TM_E_UNSUPPORTED, "%s: a picture of %d x %d (2^28 pixels at most)", who, w, h);
  TM_CHECK(nframes >= 1, TM_E_INVAL, "%s: %d frames", who, nframes);
  TM_CHECK(frames, TM_E_INVAL, "%s: null frames", who);
  TM_CHECK(h == 1 || stride_px >= w, TM_E_INVAL, "%s: a row stride of %lld pixels for rows of %d", who, (long long)stride_px, w);
  TM_CHECK(nframes <= 1 || frame_px >= (int64_t)(h - 1) * stride_px + w, TM_E_INVAL, "%s: a frame stride of %lld pixels for frames of %lld", who, (long long)frame_px,
           (long long)((int64_t)(h - 1) * stride_px + w));
  int d = opt->delay_cs;
  if (!d) {
    TM_CHECK(fps > 0 && fps == fps, TM_E_INVAL, "%s: a rate of %g", who, fps);
    const double v = std::floor(100.0 / fps + 0.5);
    TM_CHECK(v <= 65535.0, TM_E_INVAL, "%s: a rate of %g is a delay above 65535", who, fps);
    d = std::max(2, (int)v);
  }
  *delay = d;
  return TM_OK;
}

int gif_chunk_frames(int w, int h) { return (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)256 << 20) / ((size_t)w * h * 4))); }

static int64_t gif_bound(int w, int h, int nframes, const tm_gif_options &opt) {
  const uint32_t n = (uint32_t)((uint64_t)w * h), len = segment_len(n, (uint32_t)opt.segment_pixels), count = segment_count(n, (uint32_t)opt.segment_pixels);
  const uint64_t bits = (uint64_t)(count - 1) * segment_bits_bound(len) + segment_bits_bound(n - (count - 1) * len);
  return 13 + 19 + (int64_t)nframes * (int64_t)(8 + 10 + 768 + 1 + sub_blocked_bytes((bits + 7) / 8)) + 1;
}

// ---- the host twin
static int gif_encode_host(const char *who, const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, int delay, const tm_gif_options &opt,
                           std::vector<uint8_t> &file, uint32_t *canvas, tm_gif_export_stats *st) {
  file.clear();
  file_header(w, h, opt.loop, file);
  HostPack io;
  Palette pal;
  std::vector<uint8_t> idx, payload;
  for (int f = 0; f < nframes; f++) {
    const uint32_t *cur = frames + (int64_t)f * frame_px;
    const Rect r = opt.diff && f > 0 ? rect_host(cur, stride_px, cur - frame_px, stride_px, w, h) : Rect{0, 0, w, h};
    TM_TRY(palettise_host(who, cur, stride_px, r, opt, f, pal, idx));
    image_header(r, pal.table, pal.colours, delay, file);
    lzw_pack_host(io, idx.data(), (uint32_t)idx.size(), min_code_of(pal.colours), (uint32_t)opt.segment_pixels, payload, &st->segments);
    put_sub_blocks(payload, file);
    st->frames++;
    (pal.exact ? st->frames_exact : st->frames_quantised)++;
    if (canvas) {
      uint32_t *c = canvas + (size_t)f * w * h;
      if (f > 0) memcpy(c, c - (size_t)w * h, (size_t)w * h * 4);
      for (int y = 0; y < r.h; y++)
        for (int x = 0; x < r.w; x++) c[(size_t)(r.y + y) * w + r.x + x] = pal.table[idx[(size_t)y * r.w + x]];
    }
  }
  file.push_back(0x3b);
  st->file_bytes = (int64_t)file.size();
  return TM_OK;
}

// ---- the device writer
struct GifDeviceEncoder::State {
  DevBuf prev, raw, rects, tabs, counts, ranks, cells, cellmaps, jobs, idx, segjobs, words, bits, status, places, images, pieces, blob, out;
  std::vector<Rect> h_rects;
  std::vector<uint32_t> h_tabs, h_counts;
  std::vector<unsigned long long> h_bits;
  std::vector<SegPlace> h_places;
  std::vector<uint8_t> h_out;
  int w = 0, h = 0, delay = 0, frame_no = 0;
  tm_gif_options opt{};
  hipStream_t stream = nullptr;
  // the segments of `n` images (idx_off, n, min_code each) coded in one launch: their places (bit_off inside their image) and every image's payload bytes
  struct ImageIn { uint64_t idx_off; uint32_t n, min_code; };
  int code(const std::vector<ImageIn> &ims, const uint8_t *dev_idx, uint64_t idx_bytes, uint32_t segment_pixels, std::vector<ImagePlace> &images, uint64_t *nwords_out) {
    std::vector<SegJob> jobs;
    uint64_t word = 0;
    images.clear();
    for (const ImageIn &im : ims) {
      const uint32_t len = segment_len(im.n, segment_pixels), count = segment_count(im.n, segment_pixels);
      images.push_back(ImagePlace{0, 0, 0, (uint32_t)jobs.size(), count});
      for (uint32_t s = 0; s < count; s++) {
        const uint32_t p = std::min(len, im.n - s * len);
        const uint64_t cap = (segment_bits_bound(p) + 31) / 32 + 1;
        jobs.push_back(SegJob{im.idx_off + (uint64_t)s * len, word, p, im.min_code, s == 0 ? 1u : 0u, s + 1 == count ? 1u : 0u, (uint32_t)cap, 0});
        word += cap;
      }
    }
    const size_t ns = jobs.size();
    TM_CHECK(ns < ((size_t)1 << 31), TM_E_UNSUPPORTED, "gif out: a chunk of %zu segments", ns);
    TM_TRY(segjobs.alloc(ns * sizeof(SegJob))); TM_TRY(words.alloc(word * 4)); TM_TRY(bits.alloc(ns * 8)); TM_TRY(status.alloc(4));
    TM_HIP(hipMemcpyAsync(segjobs.p, jobs.data(), ns * sizeof(SegJob), hipMemcpyHostToDevice, stream));
    TM_HIP(hipMemsetAsync(status.p, 0, 4, stream));
    hipLaunchKernelGGL(k_gif_lzw_pack, dim3((unsigned)ns), dim3(64), 0, stream, segjobs.as<SegJob>(), dev_idx, idx_bytes, words.as<uint32_t>(), word,
                       bits.as<unsigned long long>(), status.as<int32_t>());
    TM_HIP(hipGetLastError());
    h_bits.resize(ns);
    int32_t rc = 0;
    TM_HIP(hipMemcpyAsync(h_bits.data(), bits.p, ns * 8, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipMemcpyAsync(&rc, status.p, 4, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    TM_CHECK(rc == 0, TM_E_INTERNAL, "gif out: the coder refused a segment or a colour (status %d)", rc);
    h_places.resize(ns);
    uint64_t word0 = 0;
    for (ImagePlace &im : images) {
      uint64_t bit = 0;
      for (uint32_t s = im.seg0; s < im.seg0 + im.nseg; s++) {
        TM_CHECK(h_bits[s] > 0 && h_bits[s] <= (uint64_t)jobs[s].cap_words * 32, TM_E_INTERNAL, "gif out: a segment of %llu bits, above its bound", h_bits[s]);
        h_places[s] = SegPlace{bit, h_bits[s], jobs[s].word_off};
        bit += h_bits[s];
      }
      im.payload = (bit + 7) / 8;
      im.word0 = word0;
      word0 += (im.payload + 3) / 4;
    }
    TM_TRY(places.alloc(ns * sizeof(SegPlace)));
    TM_HIP(hipMemcpyAsync(places.p, h_places.data(), ns * sizeof(SegPlace), hipMemcpyHostToDevice, stream));
    *nwords_out = word;
    stats_segments += (int64_t)ns;
    return TM_OK;
  }
  // the images' bits and the blob's pieces into `total` bytes, and those to the host
  int emit(std::vector<ImagePlace> &ims, uint64_t nwords, const std::vector<Piece> &pcs, const std::vector<uint8_t> &blob_bytes, uint64_t total, int sub) {
    TM_TRY(images.alloc(ims.size() * sizeof(ImagePlace))); TM_TRY(out.alloc(total));
    TM_HIP(hipMemcpyAsync(images.p, ims.data(), ims.size() * sizeof(ImagePlace), hipMemcpyHostToDevice, stream));
    const uint64_t total_words = ims.back().word0 + (ims.back().payload + 3) / 4;
    hipLaunchKernelGGL(k_gif_emit, dim3(blocks_of(total_words, 16384)), dim3(256), 0, stream, images.as<ImagePlace>(), (uint32_t)ims.size(), places.as<SegPlace>(),
                       words.as<uint32_t>(), nwords, total_words, out.as<uint8_t>(), total, sub);
    if (!pcs.empty()) {
      TM_TRY(pieces.alloc(pcs.size() * sizeof(Piece))); TM_TRY(blob.alloc(blob_bytes.size()));
      TM_HIP(hipMemcpyAsync(pieces.p, pcs.data(), pcs.size() * sizeof(Piece), hipMemcpyHostToDevice, stream));
      TM_HIP(hipMemcpyAsync(blob.p, blob_bytes.data(), blob_bytes.size(), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(k_gif_blob, dim3((unsigned)pcs.size()), dim3(256), 0, stream, pieces.as<Piece>(), blob.as<uint8_t>(), (uint64_t)blob_bytes.size(), out.as<uint8_t>(),
                         total);
    }
    TM_HIP(hipGetLastError());
    h_out.resize(total);
    TM_HIP(hipMemcpyAsync(h_out.data(), out.p, total, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    return TM_OK;
  }
  int64_t stats_segments = 0;
  std::vector<Palette> pals;
  std::vector<ImageIn> ims;
  uint64_t idx_bytes = 0;
};
GifDeviceEncoder::GifDeviceEncoder() : state_(new State) {}
GifDeviceEncoder::~GifDeviceEncoder() { delete state_; }

int GifDeviceEncoder::begin(int w, int h, double fps, const tm_gif_options &opt, void *hip_stream, std::vector<uint8_t> &file) {
  State &d = *state_;
  uint32_t dummy = 0;
  TM_TRY(gif_out_check("gif out", &dummy, w, (int64_t)w * h, 1, w, h, fps, &opt, &d.delay));
  d.w = w; d.h = h; d.opt = opt; d.stream = (hipStream_t)hip_stream; d.frame_no = 0; d.stats_segments = 0;
  stats = tm_gif_export_stats{};
  file_header(w, h, opt.loop, file);
  return TM_OK;
}

// rectangles, tables and stored indices of a chunk's frames: State::pals, ims, idx_bytes and the index buffer
int GifDeviceEncoder::tables(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nf) {
  State &d = *state_;
  hipStream_t stream = d.stream;
  const int w = d.w, h = d.h;
  const tm_gif_options &opt = d.opt;
  auto t0 = std::chrono::steady_clock::now();
  // rectangles and distinct colours
  const unsigned fb = blocks_of((uint64_t)w * h, 1024);
  TM_TRY(d.raw.alloc((size_t)nf * 16)); TM_TRY(d.rects.alloc((size_t)nf * sizeof(Rect))); TM_TRY(d.tabs.alloc((size_t)nf * kHashSlots * 4)); TM_TRY(d.counts.alloc((size_t)nf * 4));
  TM_TRY(d.prev.alloc((size_t)w * h * 4));
  TM_HIP(hipMemsetAsync(d.raw.p, 0x7f, (size_t)nf * 16, stream));
  TM_HIP(hipMemsetAsync(d.tabs.p, 0xff, (size_t)nf * kHashSlots * 4, stream));
  TM_HIP(hipMemsetAsync(d.counts.p, 0, (size_t)nf * 4, stream));
  if (opt.diff)
    hipLaunchKernelGGL(k_gif_rect, dim3(fb, (unsigned)nf), dim3(256), 0, stream, dev_frames, stride_px, frame_px, d.prev.as<uint32_t>(), d.frame_no > 0 ? 1 : 0, w, h,
                       d.raw.as<int32_t>());
  hipLaunchKernelGGL(k_gif_rect_fix, dim3((unsigned)(nf + 63) / 64), dim3(64), 0, stream, nf, d.frame_no == 0 ? 1 : 0, opt.diff, w, h, d.raw.as<int32_t>(), d.rects.as<Rect>());
  hipLaunchKernelGGL(k_gif_colours, dim3(fb, (unsigned)nf), dim3(256), 0, stream, dev_frames, stride_px, frame_px, d.rects.as<Rect>(), d.tabs.as<uint32_t>(),
                     d.counts.as<uint32_t>(), (uint32_t)opt.max_colours);
  TM_HIP(hipGetLastError());
  d.h_rects.resize((size_t)nf); d.h_tabs.resize((size_t)nf * kHashSlots); d.h_counts.resize((size_t)nf);
  TM_HIP(hipMemcpyAsync(d.h_rects.data(), d.rects.p, (size_t)nf * sizeof(Rect), hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_tabs.data(), d.tabs.p, (size_t)nf * kHashSlots * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(d.h_counts.data(), d.counts.p, (size_t)nf * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));
  for (int f = 0; f < nf; f++) {
    const Rect &r = d.h_rects[(size_t)f];
    TM_CHECK(r.x >= 0 && r.y >= 0 && r.w >= 1 && r.h >= 1 && r.x + r.w <= w && r.y + r.h <= h, TM_E_INTERNAL, "gif out: frame %d has a rectangle outside the picture",
             d.frame_no + f);
  }
  // which frames are exact; the others' cells
  std::vector<Palette> &pals = d.pals;
  pals.assign((size_t)nf, Palette());
  std::vector<int> quant;
  for (int f = 0; f < nf; f++) {
    if (takes_exact(opt, d.h_counts[(size_t)f])) { exact_palette(d.h_tabs.data() + (size_t)f * kHashSlots, pals[(size_t)f]); continue; }
    if (opt.colours == TM_GIF_COLOURS_EXACT) {  // the refusal names the count: the frame comes to the host for it
      std::vector<uint32_t> px((size_t)w * h);
      TM_HIP(hipMemcpy2D(px.data(), (size_t)w * 4, dev_frames + (int64_t)f * frame_px, (size_t)(h == 1 ? w : stride_px) * 4, (size_t)w * 4, (size_t)h, hipMemcpyDeviceToHost));
      TM_CHECK(false, TM_E_UNSUPPORTED, "gif out: frame %d holds %zu colours, a table %d", d.frame_no + f, distinct_host(px.data(), w, d.h_rects[(size_t)f]), opt.max_colours);
    }
    quant.push_back(f);
  }
  if (!quant.empty()) {
    TM_TRY(d.cells.alloc(quant.size() * kCells * sizeof(Cell))); TM_TRY(d.cellmaps.alloc(quant.size() * kCells));
    TM_HIP(hipMemsetAsync(d.cells.p, 0, quant.size() * kCells * sizeof(Cell), stream));
    for (size_t q = 0; q < quant.size(); q++) {
      const Rect &r = d.h_rects[(size_t)quant[q]];
      hipLaunchKernelGGL(k_gif_hist, dim3(blocks_of((uint64_t)r.w * r.h, 1024)), dim3(256), 0, stream, dev_frames + (int64_t)quant[q] * frame_px, stride_px, r,
                         d.cells.as<Cell>() + q * kCells);
    }
    TM_HIP(hipGetLastError());
    std::vector<Cell> cells(quant.size() * kCells);
    TM_HIP(hipMemcpyAsync(cells.data(), d.cells.p, cells.size() * sizeof(Cell), hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    stats.ms_colours += ms_since(t0); t0 = std::chrono::steady_clock::now();
    for (size_t q = 0; q < quant.size(); q++) {
      quantised_palette(cells.data() + q * kCells, (uint32_t)opt.max_colours, pals[(size_t)quant[q]]);
      TM_HIP(hipMemcpyAsync(d.cellmaps.as<uint8_t>() + q * kCells, pals[(size_t)quant[q]].cell_box.data(), kCells, hipMemcpyHostToDevice, stream));
    }
  } else {
    stats.ms_colours += ms_since(t0); t0 = std::chrono::steady_clock::now();
  }
  // the jobs
  std::vector<FrameJob> jobs((size_t)nf);
  std::vector<uint8_t> ranks((size_t)nf * kHashSlots);
  std::vector<State::ImageIn> &ims = d.ims;
  ims.resize((size_t)nf);
  uint64_t idx_bytes = 0;
  size_t q = 0;
  for (int f = 0; f < nf; f++) {
    const Rect &r = d.h_rects[(size_t)f];
    const Palette &p = pals[(size_t)f];
    jobs[(size_t)f] = FrameJob{r, idx_bytes, p.exact ? 1 : 0, p.exact ? 0u : (uint32_t)q};
    if (p.exact) memcpy(ranks.data() + (size_t)f * kHashSlots, p.rank, kHashSlots); else q++;
    ims[(size_t)f] = State::ImageIn{idx_bytes, (uint32_t)((uint64_t)r.w * r.h), min_code_of(p.colours)};
    idx_bytes += (uint64_t)r.w * r.h;
    stats.frames++;
    (p.exact ? stats.frames_exact : stats.frames_quantised)++;
  }
  TM_TRY(d.jobs.alloc((size_t)nf * sizeof(FrameJob))); TM_TRY(d.ranks.alloc(ranks.size())); TM_TRY(d.idx.alloc(idx_bytes)); TM_TRY(d.status.alloc(4));
  TM_TRY(d.cellmaps.alloc(16));
  TM_HIP(hipMemcpyAsync(d.jobs.p, jobs.data(), (size_t)nf * sizeof(FrameJob), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.ranks.p, ranks.data(), ranks.size(), hipMemcpyHostToDevice, stream));
  stats.ms_tables += ms_since(t0); t0 = std::chrono::steady_clock::now();
  TM_HIP(hipMemsetAsync(d.status.p, 0, 4, stream));
  hipLaunchKernelGGL(k_gif_map, dim3(fb, (unsigned)nf), dim3(256), 0, stream, dev_frames, stride_px, frame_px, d.jobs.as<FrameJob>(), d.tabs.as<uint32_t>(), d.ranks.as<uint8_t>(),
                     d.cellmaps.as<uint8_t>(), d.idx.as<uint8_t>(), idx_bytes, d.status.as<int32_t>());
  TM_HIP(hipGetLastError());
  int32_t map_rc = 0;
  TM_HIP(hipMemcpyAsync(&map_rc, d.status.p, 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));  // (the host's copies above are read by then, and status is free for the coder)
  TM_CHECK(map_rc == 0, TM_E_INTERNAL, "gif out: a pixel's colour is not in its frame's table");
  d.idx_bytes = idx_bytes;
  stats.ms_lzw += ms_since(t0);
  return TM_OK;
}

int GifDeviceEncoder::chunk(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nf, std::vector<uint8_t> &file) {
  State &d = *state_;
  hipStream_t stream = d.stream;
  const int w = d.w, h = d.h;
  const tm_gif_options &opt = d.opt;
  if (nf <= 0) return TM_OK;
  TM_TRY(tables(dev_frames, stride_px, frame_px, nf));
  auto t0 = std::chrono::steady_clock::now();
  const std::vector<Palette> &pals = d.pals;
  std::vector<ImagePlace> images;
  uint64_t nwords = 0;
  TM_TRY(d.code(d.ims, d.idx.as<uint8_t>(), d.idx_bytes, (uint32_t)opt.segment_pixels, images, &nwords));
  stats.ms_lzw += ms_since(t0); t0 = std::chrono::steady_clock::now();
  // the chunk's bytes: per image its header, its data, a 0
  std::vector<uint8_t> blob_bytes(1, 0);
  std::vector<Piece> pcs;
  uint64_t at = 0;
  for (int f = 0; f < nf; f++) {
    const size_t from = blob_bytes.size();
    image_header(d.h_rects[(size_t)f], pals[(size_t)f].table, pals[(size_t)f].colours, d.delay, blob_bytes);
    pcs.push_back(Piece{from, at, (uint32_t)(blob_bytes.size() - from), 0});
    at += blob_bytes.size() - from;
    images[(size_t)f].pos = at;
    at += sub_blocked_bytes(images[(size_t)f].payload);
    pcs.push_back(Piece{0, at - 1, 1, 0});
  }
  TM_TRY(d.emit(images, nwords, pcs, blob_bytes, at, 1));
  file.insert(file.end(), d.h_out.begin(), d.h_out.end());
  // the last frame stays for the next chunk's first rectangle
  TM_HIP(hipMemcpy2DAsync(d.prev.p, (size_t)w * 4, dev_frames + (int64_t)(nf - 1) * frame_px, (size_t)(h == 1 ? w : stride_px) * 4, (size_t)w * 4, (size_t)h,
                          hipMemcpyDeviceToDevice, stream));
  TM_HIP(hipStreamSynchronize(stream));
  d.frame_no += nf;
  stats.segments = d.stats_segments;
  stats.ms_emit += ms_since(t0);
  return TM_OK;
}

int GifDeviceEncoder::pack(const uint8_t *dev_indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes, void *hip_stream) {
  State &d = *state_;
  d.stream = (hipStream_t)hip_stream;
  std::vector<ImagePlace> images;
  uint64_t nwords = 0;
  TM_TRY(d.code({State::ImageIn{0, n, (uint32_t)min_code}}, dev_indices, n, (uint32_t)segment_pixels, images, &nwords));
  images[0].pos = 0;
  TM_TRY(d.emit(images, nwords, {}, {}, images[0].payload, 0));
  return deliver("tm_stage_gif_lzw_pack", d.h_out, out, cap, bytes);
}

int GifDeviceEncoder::palettise(const uint32_t *dev_frame, int64_t stride_px, int w, int h, const tm_gif_options &opt, uint32_t *table, int *colours, int *exact,
                                uint8_t *indices, void *hip_stream) {
  State &d = *state_;
  std::vector<uint8_t> file;
  tm_gif_options whole = opt;
  whole.diff = 0; whole.delay_cs = 10;
  TM_TRY(begin(w, h, 10.0, whole, hip_stream, file));
  TM_TRY(tables(dev_frame, stride_px, (int64_t)stride_px * h, 1));
  const Palette &p = d.pals[0];
  for (uint32_t i = 0; i < 256; i++) table[i] = i < p.colours ? p.table[i] : 0u;
  *colours = (int)p.colours; *exact = p.exact ? 1 : 0;
  TM_HIP(hipMemcpyAsync(indices, d.idx.p, (size_t)w * h, hipMemcpyDeviceToHost, d.stream));
  TM_HIP(hipStreamSynchronize(d.stream));
  return TM_OK;
}

int GifDeviceEncoder::end(std::vector<uint8_t> &file) {
  file.push_back(0x3b);
  stats.file_bytes = (int64_t)file.size();
  return TM_OK;
}

}  // namespace gfo
}  // namespace tmx

extern "C" {

int tm_gif_bound_host(int w, int h, int nframes, const tm_gif_options *opt, int64_t *bytes) {
  using namespace tmx;
  TM_CHECK(bytes, TM_E_INVAL, "tm_gif_bound_host: null argument");
  uint32_t dummy = 0;
  int delay;
  TM_TRY(gfo::gif_out_check("tm_gif_bound_host", &dummy, w, (int64_t)w * h, nframes, w, h, 10.0, opt, &delay));
  *bytes = gfo::gif_bound(w, h, nframes, *opt);
  return TM_OK;
}

int tm_gif_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt, uint8_t *out,
                       int64_t cap, int64_t *bytes, uint32_t *canvas, tm_gif_export_stats *stats) {
  using namespace tmx;
  int delay;
  TM_TRY(gfo::gif_out_check("tm_gif_encode_host", frames, stride_px, frame_px, nframes, w, h, fps, opt, &delay));
  TM_CHECK(bytes && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_gif_encode_host: null argument");
  std::vector<uint8_t> file;
  tm_gif_export_stats st{};
  TM_TRY(gfo::gif_encode_host("tm_gif_encode_host", frames, stride_px, frame_px, nframes, w, h, delay, *opt, file, canvas, &st));
  if (stats) *stats = st;
  return gfo::deliver("tm_gif_encode_host", file, out, cap, bytes);
}

int tm_stage_gif_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, double fps, const tm_gif_options *opt, int chunk_frames,
                        uint8_t *out, int64_t cap, int64_t *bytes, tm_gif_export_stats *stats, void *stream) {
  using namespace tmx;
  int delay;
  TM_TRY(gfo::gif_out_check("tm_stage_gif_encode", dev_frames, stride_px, frame_px, nframes, w, h, fps, opt, &delay));
  TM_CHECK(bytes && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_stage_gif_encode: null argument");
  TM_TRY(require_device());
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> file;
  gfo::GifDeviceEncoder encoder;
  TM_TRY(encoder.begin(w, h, fps, *opt, stream, file));
  const int chunk = chunk_frames > 0 ? chunk_frames : gfo::gif_chunk_frames(w, h);
  for (int f0 = 0; f0 < nframes; f0 += chunk) TM_TRY(encoder.chunk(dev_frames + (int64_t)f0 * frame_px, stride_px, frame_px, std::min(chunk, nframes - f0), file));
  TM_TRY(encoder.end(file));
  encoder.stats.ms_device = encoder.stats.ms_wall = gfo::ms_since(t0);
  if (stats) *stats = encoder.stats;
  return gfo::deliver("tm_stage_gif_encode", file, out, cap, bytes);
}

static int lzw_pack_check(const char *who, const void *indices, uint32_t n, int min_code, int segment_pixels, const uint8_t *out, int64_t cap, const int64_t *bytes) {
  using namespace tmx;
  TM_CHECK(indices && bytes && (out || !cap) && cap >= 0, TM_E_INVAL, "%s: null argument", who);
  TM_CHECK(n >= 1 && n <= gfo::kMaxPixels, TM_E_INVAL, "%s: %u indices (1 .. 2^28)", who, n);
  TM_CHECK(min_code >= 2 && min_code <= 8, TM_E_INVAL, "%s: a minimum code size of %d (2 .. 8)", who, min_code);
  TM_CHECK(segment_pixels == 0 || segment_pixels >= 256, TM_E_INVAL, "%s: segment_pixels %d (0, or 256 and more)", who, segment_pixels);
  return TM_OK;
}

int tm_gif_lzw_pack_host(const uint8_t *indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes) {
  using namespace tmx;
  TM_TRY(lzw_pack_check("tm_gif_lzw_pack_host", indices, n, min_code, segment_pixels, out, cap, bytes));
  gfo::HostPack io;
  std::vector<uint8_t> payload;
  gfo::lzw_pack_host(io, indices, n, (uint32_t)min_code, (uint32_t)segment_pixels, payload, nullptr);
  return gfo::deliver("tm_gif_lzw_pack_host", payload, out, cap, bytes);
}

int tm_stage_gif_lzw_pack(const uint8_t *dev_indices, uint32_t n, int min_code, int segment_pixels, uint8_t *out, int64_t cap, int64_t *bytes, void *stream) {
  using namespace tmx;
  TM_TRY(lzw_pack_check("tm_stage_gif_lzw_pack", dev_indices, n, min_code, segment_pixels, out, cap, bytes));
  TM_TRY(require_device());
  gfo::GifDeviceEncoder encoder;
  return encoder.pack(dev_indices, n, min_code, segment_pixels, out, cap, bytes, stream);
}

int tm_gif_palettise_host(const uint32_t *frame, int64_t stride_px, int w, int h, const tm_gif_options *opt, uint32_t *table, int *colours, int *exact, uint8_t *indices) {
  using namespace tmx;
  int delay;
  TM_TRY(gfo::gif_out_check("tm_gif_palettise_host", frame, stride_px, (int64_t)stride_px * h, 1, w, h, 10.0, opt, &delay));
  TM_CHECK(table && colours && exact && indices, TM_E_INVAL, "tm_gif_palettise_host: null argument");
  gfo::Palette p;
  std::vector<uint8_t> idx;
  TM_TRY(gfo::palettise_host("tm_gif_palettise_host", frame, stride_px, gfo::Rect{0, 0, w, h}, *opt, 0, p, idx));
  for (uint32_t i = 0; i < 256; i++) table[i] = i < p.colours ? p.table[i] : 0u;
  *colours = (int)p.colours; *exact = p.exact ? 1 : 0;
  memcpy(indices, idx.data(), idx.size());
  return TM_OK;
}

int tm_stage_gif_palettise(const uint32_t *dev_frame, int64_t stride_px, int w, int h, const tm_gif_options *opt, uint32_t *table, int *colours, int *exact, uint8_t *indices,
                           void *stream) {
  using namespace tmx;
  int delay;
  TM_TRY(gfo::gif_out_check("tm_stage_gif_palettise", dev_frame, stride_px, (int64_t)stride_px * h, 1, w, h, 10.0, opt, &delay));
  TM_CHECK(table && colours && exact && indices, TM_E_INVAL, "tm_stage_gif_palettise: null argument");
  TM_TRY(require_device());
  gfo::GifDeviceEncoder encoder;
  return encoder.palettise(dev_frame, stride_px, w, h, *opt, table, colours, exact, indices, stream);
}

}  // extern "C"
