// tm_jpeg_out.hip -- the JPEG writer on the device and its host twin.  The rule is tm_jpeg_out.h's; both forms
// write the same bytes.  A chunk of frames (at most 32, at most 256 MB of RGB32) goes through these stages, all on the caller's stream and
// every picture of the chunk in the same launches; block g = frame * blocks + j, j in scan order, and nothing below depends on where the
// restart markers are, so a file without them is as parallel as one with them:
//
//   blocks    k_jpeg_blocks, a lane per block (component by component, so that a wave's lanes read alike): colour, chroma average, forward
//             DCT and quantisation from the source pixels; 64 int16 coefficients in zig-zag order at coef[k * nblocks + g].
//   count     k_jpeg_count, a lane per block: the block's bit count (CountSink); the DC difference reads the DC of the block before it.
//   offsets   one exclusive scan (rocPRIM) of the bit counts over the whole chunk: S[g].  Segment s (frame * segs + i) starts at bit
//             S[its first block]; its unstuffed bytes start at word (S >> 5) + s of a zeroed stream, which leaves every segment room
//             (section 40.2), and a block's bits start S[g] - S[first] bits into them.
//   pack      k_jpeg_pack, a lane per block: the block's code again (PackSink), 32 bits at a time; the words a block owns whole are
//             stored, its first and last word, which it shares with its neighbours, are merged with atomicOr (a vector atomic).  The
//             last block of a segment adds the 1-bits that pad it to a byte.
//   stuffing  k_jpeg_ff counts the FF bytes of every word; one exclusive scan: F[word].  k_jpeg_sizes, a lane per segment: its bytes with
//             the stuffed zeros, the marker behind it and, for a frame's first, the header; one exclusive scan: where every segment starts.
//   files     the sizes come to the host (the one read-back the coder waits for), the output is allocated to the byte, k_jpeg_emit (a lane
//             per word: its up to four bytes and their stuffed zeros) and k_jpeg_marks (headers, RSTn, EOI) write the files, and one
//             copy brings them back.
//
// Every loop is bounded by the block (63 coefficients), the segment count (a binary search) or the grid; plain launches, nothing waits on
// another workgroup.  Device memory for a chunk of B blocks and G segments: 128 B (coefficients) + 12 B (counts, offsets) + two streams
// of B kMaxBlockBytes + 4 G bytes (unstuffed words and their FF counts, sized by the bound: the bits are not known before they are
// scanned) + the files to the byte.
#include <rocprim/device/device_scan.hpp>

#include "tm_common.h"
#include "tm_jpeg_out.h"

namespace tmx {
namespace jpo {
namespace {

// T.81 Annex K.1 in natural order, and the code tables of Annex K.3 (counts of lengths 1 .. 16, symbols in code order)
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcSymbols[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

void quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int k = 0; k < 64; k++) {
    luma[k] = (uint16_t)std::min(255, std::max(1, (kBaseLuma[k] * scale + 50) / 100));
    chroma[k] = (uint16_t)std::min(255, std::max(1, (kBaseChroma[k] * scale + 50) / 100));
  }
}
// canonical codes from the counts: out[symbol] = code | length << 16
void codes_of(const uint8_t counts[16], const uint8_t *symbols, uint32_t *out) {
  uint32_t code = 0, at = 0;
  for (uint32_t l = 1; l <= 16; l++) {
    for (uint32_t i = 0; i < counts[l - 1]; i++) out[symbols[at++]] = code++ | l << 16;
    code <<= 1;
  }
}

void put_segment(std::vector<uint8_t> &f, uint8_t marker, const std::vector<uint8_t> &body) {
  const size_t n = body.size() + 2;
  f.push_back(0xff); f.push_back(marker); f.push_back((uint8_t)(n >> 8)); f.push_back((uint8_t)n);
  f.insert(f.end(), body.begin(), body.end());
}

// the host's sink: the bytes of one segment, FF stuffed as they are completed
struct ByteSink {
  std::vector<uint8_t> &out;
  uint64_t acc = 0;
  uint32_t n = 0;
  void put(uint32_t bits, uint32_t count) {
    acc = acc << count | bits;
    n += count;
    while (n >= 8) {
      n -= 8;
      const uint8_t b = (uint8_t)(acc >> n);
      out.push_back(b);
      if (b == 0xff) out.push_back(0);
    }
  }
  void pad() { if (n) put((1u << (8 - n)) - 1u, 8 - n); }
};

// ---- the device form
struct Chunk {  // what every kernel of a chunk is given
  Plan p;
  uint32_t nf, nblocks, nsegs;  // frames, blocks and segments of the chunk
};
__device__ inline uint32_t seg_first_block(const Chunk &c, uint32_t s) { return (s / c.p.segs) * c.p.blocks + (s % c.p.segs) * c.p.seg_mcus * c.p.bpm; }
__device__ inline uint32_t seg_end_block(const Chunk &c, uint32_t s) {
  const uint32_t i = s % c.p.segs;
  return i + 1 == c.p.segs ? (s / c.p.segs + 1) * c.p.blocks : seg_first_block(c, s + 1);
}
__device__ inline uint32_t seg_word(const Chunk &c, const unsigned long long *S, uint32_t s) { return (uint32_t)(S[seg_first_block(c, s)] >> 5) + s; }

__global__ __launch_bounds__(256) void k_jpeg_blocks(Chunk c, const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, const Tables *__restrict__ tables,
                                                     int16_t *__restrict__ coef) {
  __shared__ uint16_t qv[2][64];
  if (threadIdx.x < 128) qv[threadIdx.x >> 6][threadIdx.x & 63] = tables->qv[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= c.nblocks) return;
  // lane t of a frame: its luma blocks first, then Cb, then Cr
  const uint32_t f = t / c.p.blocks, r = t % c.p.blocks, mcus = c.p.mcx * c.p.mcy, nl = c.p.bpm - (c.p.ncomp - 1), luma = mcus * nl;
  const uint32_t j = r < luma ? (r / nl) * c.p.bpm + r % nl : ((r - luma) % mcus) * c.p.bpm + nl + (r - luma) / mcus;
  const Block b = block_at(c.p, j);
  int16_t zz[64];
  block_coefs(frames + (int64_t)f * frame_px, stride_px, c.p, b, qv[b.c ? 1 : 0], zz);
  const size_t g = (size_t)f * c.p.blocks + j;
#pragma unroll
  for (int k = 0; k < 64; k++) coef[(size_t)k * c.nblocks + g] = zz[k];
}

// what a lane of k_jpeg_count / k_jpeg_pack codes: block g of the chunk through `sink`
template <class Sink>
__device__ inline int code_one(const Chunk &c, const Tables &t, const int16_t *__restrict__ coef, uint32_t g, Sink &sink) {
  const uint32_t f = g / c.p.blocks, j = g % c.p.blocks, before = block_before(c.p, j);
  const uint32_t k0 = j % c.p.bpm, cls = (c.p.ncomp == 3 && k0 >= c.p.bpm - 2) ? 1u : 0u;
  const int32_t pred = before == j ? 0 : (int32_t)coef[(size_t)f * c.p.blocks + before];
  return code_block(t, cls, (int32_t)coef[g] - pred, [&](uint32_t k) { return (int32_t)coef[(size_t)k * c.nblocks + g]; }, sink);
}
__device__ inline void load_codes(Tables *lds, const Tables *__restrict__ tables) {
  const uint32_t *from = reinterpret_cast<const uint32_t *>(tables);
  uint32_t *to = reinterpret_cast<uint32_t *>(lds);
  for (uint32_t k = threadIdx.x; k < sizeof(Tables) / 4; k += blockDim.x) to[k] = from[k];
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_jpeg_count(Chunk c, const Tables *__restrict__ tables, const int16_t *__restrict__ coef, unsigned long long *__restrict__ bits,
                                                    int32_t *__restrict__ status) {
  __shared__ Tables t;
  load_codes(&t, tables);
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g > c.nblocks) return;
  if (g == c.nblocks) { bits[g] = 0; return; }  // (the scan's last entry: the chunk's bits)
  CountSink sink;
  const int rc = code_one(c, t, coef, g, sink);
  if (rc != kOk) atomicMax(status, rc);
  bits[g] = sink.n;
}

// the bits of one block into the stream of big-endian words: `word` is the word being filled, `n` bits of it are in `acc`
struct PackSink {
  uint32_t *words;
  uint32_t word, limit;
  uint64_t acc = 0;
  uint32_t n;
  bool shared;  // the word being filled holds a neighbour's bits too
  __device__ PackSink(uint32_t *w, uint32_t limit_, uint64_t bit) : words(w), word((uint32_t)(bit >> 5)), limit(limit_), n((uint32_t)bit & 31u), shared(((uint32_t)bit & 31u) != 0) {}
  __device__ void put(uint32_t bits, uint32_t count) {
    acc = acc << count | bits;
    n += count;
    if (n >= 32) {
      n -= 32;
      const uint32_t v = (uint32_t)(acc >> n);
      if (word < limit) { if (shared) atomicOr(&words[word], v); else words[word] = v; }
      word++;
      shared = false;
    }
  }
  __device__ void finish() {
    if (n && word < limit) atomicOr(&words[word], (uint32_t)(acc << (32 - n)));
  }
};

__global__ __launch_bounds__(256) void k_jpeg_pack(Chunk c, const Tables *__restrict__ tables, const int16_t *__restrict__ coef, const unsigned long long *__restrict__ S,
                                                   uint32_t *__restrict__ words, uint32_t nwords) {
  __shared__ Tables t;
  load_codes(&t, tables);
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= c.nblocks) return;
  const uint32_t f = g / c.p.blocks, j = g % c.p.blocks, s = f * c.p.segs + (j / c.p.bpm) / c.p.seg_mcus;
  const unsigned long long in_seg = S[g] - S[seg_first_block(c, s)];
  PackSink sink(words, nwords, (unsigned long long)seg_word(c, S, s) * 32 + in_seg);
  if (code_one(c, t, coef, g, sink) != kOk) return;  // (k_jpeg_count has noted it: the chunk is refused)
  if (ends_segment(c.p, j)) {
    const uint32_t pad = (uint32_t)(0 - (in_seg + (S[g + 1] - S[g]))) & 7u;
    if (pad) sink.put((1u << pad) - 1u, pad);
  }
  sink.finish();
}

// a segment's extent: its unstuffed bytes and where its words start
struct SegExtent { uint32_t word, bytes; };
__device__ inline SegExtent seg_extent(const Chunk &c, const unsigned long long *S, uint32_t s) {
  const uint32_t b0 = seg_first_block(c, s);
  return SegExtent{(uint32_t)(S[b0] >> 5) + s, (uint32_t)((S[seg_end_block(c, s)] - S[b0] + 7) >> 3)};
}
__device__ inline uint32_t ff_bytes(uint32_t v) {
  return (uint32_t)((v >> 24) == 0xffu) + (uint32_t)((v >> 16 & 255u) == 0xffu) + (uint32_t)((v >> 8 & 255u) == 0xffu) + (uint32_t)((v & 255u) == 0xffu);
}
// the word behind the chunk's last segment: the stream is sized by the bound, what the pictures filled of it ends here
__device__ inline uint32_t words_used(const Chunk &c, const unsigned long long *S) {
  const SegExtent e = seg_extent(c, S, c.nsegs - 1);
  return e.word + (e.bytes + 3) / 4;
}
// (bytes past a segment's end are zero, so every FF of a word is a byte of the segment the word belongs to)
__global__ __launch_bounds__(256) void k_jpeg_ff(Chunk c, const unsigned long long *__restrict__ S, const uint32_t *__restrict__ words, uint32_t nwords,
                                                 uint32_t *__restrict__ ff) {
  const uint32_t used = min(words_used(c, S), nwords);
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w <= nwords; w += gridDim.x * 256) ff[w] = w < used ? ff_bytes(words[w]) : 0u;
}

__global__ __launch_bounds__(256) void k_jpeg_sizes(Chunk c, const unsigned long long *__restrict__ S, const uint32_t *__restrict__ F, unsigned long long *__restrict__ sizes) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s > c.nsegs) return;
  if (s == c.nsegs) { sizes[s] = 0; return; }
  const SegExtent e = seg_extent(c, S, s);
  const uint32_t w1 = e.word + (e.bytes + 3) / 4;
  sizes[s] = (unsigned long long)e.bytes + (F[w1] - F[e.word]) + 2 + (s % c.p.segs == 0 ? c.p.header_bytes : 0);
}

// word w of the unstuffed stream to its place in its file
__global__ __launch_bounds__(256) void k_jpeg_emit(Chunk c, const unsigned long long *__restrict__ S, const uint32_t *__restrict__ F, const uint32_t *__restrict__ words,
                                                   uint32_t nwords, const unsigned long long *__restrict__ pos, uint8_t *__restrict__ out, unsigned long long out_bytes) {
  const uint32_t used = min(words_used(c, S), nwords);
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < used; w += gridDim.x * 256) {
    uint32_t lo = 0, hi = c.nsegs;  // the last segment that starts at or before w
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (seg_word(c, S, mid) <= w) lo = mid; else hi = mid;
    }
    const SegExtent e = seg_extent(c, S, lo);
    const uint32_t at = (w - e.word) * 4;
    if (at >= e.bytes) continue;  // (the slack between two segments)
    unsigned long long to = pos[lo] + (lo % c.p.segs == 0 ? c.p.header_bytes : 0) + at + (F[w] - F[e.word]);
    const uint32_t v = words[w];
    for (uint32_t k = 0; k < 4 && at + k < e.bytes; k++) {
      const uint32_t b = v >> (24 - 8 * k) & 255u;
      if (to < out_bytes) out[to] = (uint8_t)b;
      to++;
      if (b == 0xffu) { if (to < out_bytes) out[to] = 0; to++; }
    }
  }
}

// a workgroup per frame: its header, the RSTn behind every segment but the last, EOI
__global__ __launch_bounds__(256) void k_jpeg_marks(Chunk c, const uint8_t *__restrict__ header, const unsigned long long *__restrict__ pos, uint8_t *__restrict__ out,
                                                    unsigned long long out_bytes) {
  const uint32_t f = blockIdx.x, s0 = f * c.p.segs;
  const unsigned long long base = pos[s0];
  for (uint32_t k = threadIdx.x; k < c.p.header_bytes; k += 256) if (base + k < out_bytes) out[base + k] = header[k];
  for (uint32_t i = threadIdx.x; i < c.p.segs; i += 256) {
    const unsigned long long at = pos[s0 + i + 1] - 2;
    if (at + 1 < out_bytes) { out[at] = 0xff; out[at + 1] = (uint8_t)(i + 1 == c.p.segs ? 0xd9 : 0xd0 + (i & 7u)); }
  }
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// ---- what both forms share on the host
int jpeg_options_check(const char *who, const tm_jpeg_options *opt) {
  TM_CHECK(opt, TM_E_INVAL, "%s: null options", who);
  TM_CHECK(opt->quality >= 1 && opt->quality <= 100, TM_E_INVAL, "%s: quality %d (1 .. 100)", who, opt->quality);
  TM_CHECK(opt->sampling >= TM_JPEG_420 && opt->sampling <= TM_JPEG_GREY, TM_E_INVAL, "%s: unknown sampling %d", who, opt->sampling);
  TM_CHECK(opt->restart_rows >= 0, TM_E_INVAL, "%s: restart_rows %d", who, opt->restart_rows);
  return TM_OK;
}

int jpeg_out_check(const char *who, const void *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt) {
  TM_TRY(jpeg_options_check(who, opt));
  TM_CHECK(w >= 1 && h >= 1 && w <= 32768 && h <= 32768, TM_E_INVAL, "%s: a picture of %d x %d (1 .. 32768 each)", who, w, h);
  const int mcu_w = opt->sampling == TM_JPEG_420 || opt->sampling == TM_JPEG_422 ? 16 : 8;
  TM_CHECK((int64_t)opt->restart_rows * ((w + mcu_w - 1) / mcu_w) <= 65535, TM_E_INVAL, "%s: a restart interval of %d rows of %d MCUs (65535 MCUs at most)", who,
           opt->restart_rows, (w + mcu_w - 1) / mcu_w);
  TM_CHECK(nframes >= 0, TM_E_INVAL, "%s: %d frames", who, nframes);
  TM_CHECK(frames || nframes == 0, TM_E_INVAL, "%s: null frames", who);
  TM_CHECK(h == 1 || stride_px >= w, TM_E_INVAL, "%s: a row stride of %lld pixels for rows of %d", who, (long long)stride_px, w);
  TM_CHECK(nframes <= 1 || frame_px >= (int64_t)(h - 1) * stride_px + w, TM_E_INVAL, "%s: a frame stride of %lld pixels for frames of %lld", who,
           (long long)frame_px, (long long)((int64_t)(h - 1) * stride_px + w));
  return TM_OK;
}

void jpeg_geometry(int w, int h, const tm_jpeg_options &opt, JpegGeometry *g) {
  Plan &p = g->plan;
  p.w = w; p.h = h;
  p.ncomp = opt.sampling == TM_JPEG_GREY ? 1 : 3;
  p.hs = opt.sampling == TM_JPEG_420 || opt.sampling == TM_JPEG_422 ? 2 : 1;
  p.vs = opt.sampling == TM_JPEG_420 ? 2 : 1;
  p.mcx = ((uint32_t)w + 8 * p.hs - 1) / (8 * p.hs); p.mcy = ((uint32_t)h + 8 * p.vs - 1) / (8 * p.vs);
  p.bpm = p.ncomp == 1 ? 1 : p.hs * p.vs + 2;
  const uint32_t mcus = p.mcx * p.mcy;
  p.seg_mcus = opt.restart_rows ? std::min<uint32_t>((uint32_t)opt.restart_rows * p.mcx, mcus) : mcus;
  p.segs = (mcus + p.seg_mcus - 1) / p.seg_mcus;
  p.blocks = mcus * p.bpm;
  Tables &t = g->tables;
  memset(&t, 0, sizeof(t));
  uint16_t q[2][64];
  quant_tables(opt.quality, q[0], q[1]);
  const uint8_t dc_symbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  for (int c = 0; c < 2; c++) {
    for (int k = 0; k < 64; k++) t.qv[c][k] = (uint16_t)(8 * q[c][k]);
    codes_of(kDcCounts[c], dc_symbols, t.dc[c]);
    codes_of(kAcCounts[c], kAcSymbols[c], t.ac[c]);
  }
  // the container up to the scan
  std::vector<uint8_t> &f = g->header;
  f = {0xff, 0xd8};
  put_segment(f, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (uint32_t c = 0; c < (p.ncomp == 1 ? 1u : 2u); c++) {
    std::vector<uint8_t> body = {(uint8_t)c};
    for (uint32_t k = 0; k < 64; k++) body.push_back((uint8_t)q[c][zigzag(k)]);
    put_segment(f, 0xdb, body);
  }
  std::vector<uint8_t> sof = {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)p.ncomp};
  for (uint32_t c = 0; c < p.ncomp; c++) { sof.push_back((uint8_t)(c + 1)); sof.push_back((uint8_t)(c ? 0x11 : p.hs << 4 | p.vs)); sof.push_back(c ? 1 : 0); }
  put_segment(f, 0xc0, sof);
  for (uint32_t c = 0; c < (p.ncomp == 1 ? 1u : 2u); c++) {
    std::vector<uint8_t> dc = {(uint8_t)c}, ac = {(uint8_t)(0x10 | c)};
    dc.insert(dc.end(), kDcCounts[c], kDcCounts[c] + 16); dc.insert(dc.end(), dc_symbols, dc_symbols + 12);
    ac.insert(ac.end(), kAcCounts[c], kAcCounts[c] + 16); ac.insert(ac.end(), kAcSymbols[c], kAcSymbols[c] + 162);
    put_segment(f, 0xc4, dc);
    put_segment(f, 0xc4, ac);
  }
  if (opt.restart_rows) { const uint32_t ri = (uint32_t)opt.restart_rows * p.mcx; put_segment(f, 0xdd, {(uint8_t)(ri >> 8), (uint8_t)ri}); }
  std::vector<uint8_t> sos = {(uint8_t)p.ncomp};
  for (uint32_t c = 0; c < p.ncomp; c++) { sos.push_back((uint8_t)(c + 1)); sos.push_back(c ? 0x11 : 0x00); }
  sos.push_back(0); sos.push_back(63); sos.push_back(0);
  put_segment(f, 0xda, sos);
  p.header_bytes = (uint32_t)f.size();
}

// every block at most kMaxBlockBits before stuffing and twice that after; a segment's padding (one byte, stuffed) and its marker
int64_t jpeg_bound(const Plan &p) { return (int64_t)p.header_bytes + 2 * (int64_t)p.blocks * kMaxBlockBytes + 4 * (int64_t)p.segs; }

int jpeg_chunk_frames(int w, int h) { return (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)256 << 20) / ((size_t)w * h * 4))); }

int jpeg_encode_one_host(const JpegGeometry &g, const uint32_t *frame, int64_t stride_px, std::vector<uint8_t> &file) {
  const Plan &p = g.plan;
  file.assign(g.header.begin(), g.header.end());
  ByteSink sink{file};
  std::vector<int16_t> dcs(p.blocks);
  for (uint32_t j = 0; j < p.blocks; j++) {
    const Block b = block_at(p, j);
    int16_t zz[64];
    block_coefs(frame, stride_px, p, b, g.tables.qv[b.c ? 1 : 0], zz);
    dcs[j] = zz[0];
    const uint32_t before = block_before(p, j);
    const int rc = code_block(g.tables, b.c ? 1u : 0u, (int32_t)zz[0] - (before == j ? 0 : (int32_t)dcs[before]), [&](uint32_t k) { return (int32_t)zz[k]; }, sink);
    TM_CHECK(rc == kOk, TM_E_INTERNAL, "jpeg out: block %u holds a value no 8-bit picture makes (status %d)", j, rc);
    if (ends_segment(p, j)) {
      sink.pad();
      const uint32_t i = (j / p.bpm) / p.seg_mcus;
      file.push_back(0xff);
      file.push_back((uint8_t)(i + 1 == p.segs ? 0xd9 : 0xd0 + (i & 7u)));
    }
  }
  return TM_OK;
}

// ---- the device encoder
struct JpegDeviceEncoder::State {
  DevBuf tables, header, coef, bits, S, words, ff, F, sizes, pos, status, tmp, out;
  std::vector<unsigned long long> h_pos;
  std::vector<uint8_t> h_out;
};
JpegDeviceEncoder::JpegDeviceEncoder() : state_(new State) {}
JpegDeviceEncoder::~JpegDeviceEncoder() { delete state_; }

int JpegDeviceEncoder::encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options &opt, void *hip_stream,
                              std::vector<std::vector<uint8_t>> &files) {
  hipStream_t stream = (hipStream_t)hip_stream;
  State &d = *state_;
  files.assign((size_t)nframes, {});
  if (nframes == 0) return TM_OK;
  JpegGeometry geo;
  jpeg_geometry(w, h, opt, &geo);
  const Plan &p = geo.plan;
  const int chunk = std::min(jpeg_chunk_frames(w, h), nframes);
  // the unstuffed stream of a chunk, in words: every block's bound, and a word of slack per segment
  const uint64_t nwords64 = ((uint64_t)chunk * p.blocks * kMaxBlockBytes + 3) / 4 + (uint64_t)chunk * p.segs + 2;
  TM_CHECK(nwords64 < ((uint64_t)1 << 30) && (uint64_t)chunk * p.blocks < ((uint64_t)1 << 31), TM_E_UNSUPPORTED, "jpeg out: a chunk of %llu blocks",
           (unsigned long long)chunk * p.blocks);
  const uint32_t nwords = (uint32_t)nwords64;
  TM_TRY(d.tables.alloc(sizeof(Tables))); TM_TRY(d.header.alloc(geo.header.size())); TM_TRY(d.status.alloc(4));
  TM_TRY(d.coef.alloc((size_t)chunk * p.blocks * 128));
  TM_TRY(d.bits.alloc(((size_t)chunk * p.blocks + 1) * 8)); TM_TRY(d.S.alloc(((size_t)chunk * p.blocks + 1) * 8));
  TM_TRY(d.words.alloc((size_t)nwords * 4)); TM_TRY(d.ff.alloc(((size_t)nwords + 1) * 4)); TM_TRY(d.F.alloc(((size_t)nwords + 1) * 4));
  TM_TRY(d.sizes.alloc(((size_t)chunk * p.segs + 1) * 8)); TM_TRY(d.pos.alloc(((size_t)chunk * p.segs + 1) * 8));
  TM_HIP(hipMemcpyAsync(d.tables.p, &geo.tables, sizeof(Tables), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemcpyAsync(d.header.p, geo.header.data(), geo.header.size(), hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemsetAsync(d.status.p, 0, 4, stream));
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int nf = std::min(chunk, nframes - f0);
    const Chunk c{p, (uint32_t)nf, (uint32_t)nf * p.blocks, (uint32_t)nf * p.segs};
    const Tables *tb = d.tables.as<Tables>();
    unsigned long long *S = d.S.as<unsigned long long>(), *pos = d.pos.as<unsigned long long>();
    hipLaunchKernelGGL(k_jpeg_blocks, dim3(blocks_of(c.nblocks)), dim3(256), 0, stream, c, dev_frames + (int64_t)f0 * frame_px, stride_px, frame_px, tb, d.coef.as<int16_t>());
    hipLaunchKernelGGL(k_jpeg_count, dim3(blocks_of((uint64_t)c.nblocks + 1)), dim3(256), 0, stream, c, tb, d.coef.as<int16_t>(), d.bits.as<unsigned long long>(), d.status.as<int32_t>());
    TM_HIP(hipGetLastError());
    TM_TRY(with_temp(d.tmp, "jpeg out: scan of the blocks' bit counts", [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, d.bits.as<unsigned long long>(), S, 0ull, (size_t)c.nblocks + 1, rocprim::plus<unsigned long long>(), stream);
    }));
    TM_HIP(hipMemsetAsync(d.words.p, 0, (size_t)nwords * 4, stream));
    hipLaunchKernelGGL(k_jpeg_pack, dim3(blocks_of(c.nblocks)), dim3(256), 0, stream, c, tb, d.coef.as<int16_t>(), S, d.words.as<uint32_t>(), nwords);
    hipLaunchKernelGGL(k_jpeg_ff, dim3(std::min(blocks_of((uint64_t)nwords + 1), 16384u)), dim3(256), 0, stream, c, S, d.words.as<uint32_t>(), nwords, d.ff.as<uint32_t>());
    TM_HIP(hipGetLastError());
    TM_TRY(with_temp(d.tmp, "jpeg out: scan of the words' FF counts", [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, d.ff.as<uint32_t>(), d.F.as<uint32_t>(), 0u, (size_t)nwords + 1, rocprim::plus<uint32_t>(), stream);
    }));
    hipLaunchKernelGGL(k_jpeg_sizes, dim3(blocks_of((uint64_t)c.nsegs + 1)), dim3(256), 0, stream, c, S, d.F.as<uint32_t>(), d.sizes.as<unsigned long long>());
    TM_HIP(hipGetLastError());
    TM_TRY(with_temp(d.tmp, "jpeg out: scan of the segments' sizes", [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, d.sizes.as<unsigned long long>(), pos, 0ull, (size_t)c.nsegs + 1, rocprim::plus<unsigned long long>(), stream);
    }));
    // where every file starts, the chunk's bytes and the coder's status: the one read-back the host waits for before the files themselves
    d.h_pos.resize((size_t)c.nsegs + 1);
    int32_t status = 0;
    TM_HIP(hipMemcpyAsync(d.h_pos.data(), pos, d.h_pos.size() * 8, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipMemcpyAsync(&status, d.status.p, 4, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    TM_CHECK(status == 0, TM_E_INTERNAL, "jpeg out: a block holds a value no 8-bit picture makes (status %d)", status);
    const unsigned long long total = d.h_pos[c.nsegs];
    TM_CHECK(total <= (unsigned long long)nf * (unsigned long long)jpeg_bound(p), TM_E_INTERNAL, "jpeg out: %llu bytes, above the bound", total);
    TM_TRY(d.out.alloc(total));
    hipLaunchKernelGGL(k_jpeg_emit, dim3(std::min(blocks_of(nwords), 16384u)), dim3(256), 0, stream, c, S, d.F.as<uint32_t>(), d.words.as<uint32_t>(), nwords, pos,
                       d.out.as<uint8_t>(), total);
    hipLaunchKernelGGL(k_jpeg_marks, dim3((unsigned)nf), dim3(256), 0, stream, c, d.header.as<uint8_t>(), pos, d.out.as<uint8_t>(), total);
    TM_HIP(hipGetLastError());
    d.h_out.resize(total);
    TM_HIP(hipMemcpyAsync(d.h_out.data(), d.out.p, total, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    for (int f = 0; f < nf; f++) {
      const unsigned long long from = d.h_pos[(size_t)f * p.segs], to = d.h_pos[(size_t)(f + 1) * p.segs];
      files[(size_t)(f0 + f)].assign(d.h_out.begin() + (ptrdiff_t)from, d.h_out.begin() + (ptrdiff_t)to);
    }
  }
  return TM_OK;
}

namespace {
// the files behind one another in `out`, as tm_stage_png_encode lays them
int lay_out(const char *who, const std::vector<std::vector<uint8_t>> &files, uint8_t *out, int64_t cap, int64_t *offsets) {
  const int nframes = (int)files.size();
  int64_t total = 0;
  for (const auto &f : files) total += (int64_t)f.size();
  if (total > cap) {
    offsets[nframes] = total;
    TM_CHECK(false, TM_E_INVAL, "%s: %lld bytes needed, %lld given", who, (long long)total, (long long)cap);
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
}  // namespace

}  // namespace jpo
}  // namespace tmx

extern "C" {

int tm_jpeg_quant_tables_host(int quality, uint16_t *luma, uint16_t *chroma) {
  using namespace tmx;
  TM_CHECK(luma && chroma, TM_E_INVAL, "tm_jpeg_quant_tables_host: null argument");
  TM_CHECK(quality >= 1 && quality <= 100, TM_E_INVAL, "tm_jpeg_quant_tables_host: quality %d (1 .. 100)", quality);
  jpo::quant_tables(quality, luma, chroma);
  return TM_OK;
}

int tm_jpeg_bound_host(int w, int h, const tm_jpeg_options *opt, int64_t *bytes) {
  using namespace tmx;
  TM_CHECK(bytes, TM_E_INVAL, "tm_jpeg_bound_host: null argument");
  TM_TRY(jpo::jpeg_out_check("tm_jpeg_bound_host", nullptr, w, 0, 0, w, h, opt));
  jpo::JpegGeometry g;
  jpo::jpeg_geometry(w, h, *opt, &g);
  *bytes = jpo::jpeg_bound(g.plan);
  return TM_OK;
}

int tm_jpeg_encode_host(const uint32_t *frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt, uint8_t *out, int64_t cap,
                        int64_t *offsets) {
  using namespace tmx;
  TM_TRY(jpo::jpeg_out_check("tm_jpeg_encode_host", frames, stride_px, frame_px, nframes, w, h, opt));
  TM_CHECK(offsets && (out || !cap) && cap >= 0, TM_E_INVAL, "tm_jpeg_encode_host: null argument");
  jpo::JpegGeometry g;
  jpo::jpeg_geometry(w, h, *opt, &g);
  std::vector<std::vector<uint8_t>> files((size_t)nframes);
  for (int f = 0; f < nframes; f++) TM_TRY(jpo::jpeg_encode_one_host(g, frames + (int64_t)f * frame_px, stride_px, files[(size_t)f]));
  return jpo::lay_out("tm_jpeg_encode_host", files, out, cap, offsets);
}

int tm_stage_jpeg_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_jpeg_options *opt, uint8_t *host_out,
                         int64_t cap, int64_t *offsets, void *stream) {
  using namespace tmx;
  TM_TRY(jpo::jpeg_out_check("tm_stage_jpeg_encode", dev_frames, stride_px, frame_px, nframes, w, h, opt));
  TM_CHECK(offsets && (host_out || !cap) && cap >= 0, TM_E_INVAL, "tm_stage_jpeg_encode: null argument");
  TM_TRY(require_device());
  std::vector<std::vector<uint8_t>> files;
  jpo::JpegDeviceEncoder encoder;
  TM_TRY(encoder.encode(dev_frames, stride_px, frame_px, nframes, w, h, *opt, stream, files));
  return jpo::lay_out("tm_stage_jpeg_encode", files, host_out, cap, offsets);
}

}  // extern "C"
