// tm_png_out.hip -- the PNG writer on the device.  The rule is tm_deflate.h's; the host twin is tm_deflate.hip, and the
// two write the same bytes.  A chunk of frames (at most 32, at most 256 MB of stream) goes through these stages, all on the caller's stream:
//
//   filter    k_png_filter, a workgroup per row: RGB32 frames of any row and frame stride to the stream of filtered rows (ADAPTIVE: the five
//             costs of the row are summed first, then the row is written with the cheapest type).
//   links     the positions of all frames of the chunk, keyed by (frame, three bytes), in one stable radix sort (rocPRIM): the entry below
//             a position's own is the nearest earlier position of its frame with the same three bytes -- k_png_links turns the order into
//             prev[], the chain best_match walks.
//   match     k_png_match, a lane per position: the rule's best match, len | dist << 16.
//   parse     k_png_parse, a workgroup per segment: the segment's lengths in LDS, one lane follows i -> i + max(1, len[i]) there and marks the
//             tokens, then the workgroup counts their symbols (LDS atomics) and writes the token bitmap.  k_png_adler: the segments' sums.
//   codes     the histograms come to the host, plan_segment (tm_deflate.hip) runs on up to min(TM_HOST_THREADS, 16) threads, and the tables,
//             header bits and byte offsets go back: one round trip per chunk.  Every segment's size follows from its histogram and its code
//             lengths, so the offsets are known before a bit is packed.
//   pack      k_png_pack, a workgroup per segment: per-token bit lengths, a workgroup scan for the offsets, the bits OR-ed together in
//             LDS, the segment written as whole words to its slot.  k_png_compact lays the slots behind one another.
//   host      the packed bytes come back; signature, IHDR, IDAT framing, Adler-32 (combined from the segments' sums), CRC-32 and IEND are
//             put around them (png_wrap).
//
// Every loop is bounded by the stream's length, kDepth or kMaxMatch; plain launches, nothing waits on another workgroup.  Device memory
// for a chunk of P stream bytes: P (stream) + 8 P (prev, matches) + 16 P (sort keys and values, in and out) + rocPRIM's temporary + about
// P (slots) + P / 8 (bitmaps) + 3 KB per segment.
#include <rocprim/device/device_radix_sort.hpp>

#include <thread>

#include "tm_common.h"
#include "tm_deflate.h"

namespace tmx {
namespace dfl {
namespace {

constexpr int kHistStride = 320;                // a segment's histograms: literal/length at 0, distance at 288
constexpr int kMapWords = kSeg / 32;            // a segment's token bitmap
constexpr int kSlotWords = kSlotBytes / 4;
constexpr size_t kParseLds = kSeg * 2 + kHistStride * 4;
constexpr uint64_t kChunkBytes = (uint64_t)256 << 20;

struct Streams {  // nf streams of n bytes each, stream f at base + f * ns
  const uint8_t *base;
  uint64_t ns;
  uint32_t n, segs;  // segs: segments per stream
};
struct Seg { uint64_t base; uint32_t count; };  // where a segment's bytes start (from Streams::base) and how many they are
__device__ inline Seg seg_of(const Streams &S, uint32_t seg) {
  const uint32_t f = seg / S.segs, first = (seg % S.segs) * kSeg;
  const uint32_t left = S.n - first;
  return Seg{(uint64_t)f * S.ns + first, left < kSeg ? left : kSeg};
}

// ---- filter
__global__ __launch_bounds__(256) void k_png_filter(const uint32_t *__restrict__ frames, int64_t stride_px, int64_t frame_px, int w, int adaptive,
                                                    uint8_t *__restrict__ stream, uint64_t ns) {
  __shared__ uint32_t cost[5][256];
  __shared__ int s_type;
  const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const uint32_t *row = frames + (int64_t)f * frame_px + (int64_t)y * stride_px, *up = row - stride_px;  // (up is read only when y > 0)
  const uint32_t rb = 3u * (uint32_t)w;
  uint8_t *out = stream + (uint64_t)f * ns + (uint64_t)y * (1 + rb);
  int type = 0;
  if (adaptive) {
    uint32_t c5[5] = {0, 0, 0, 0, 0};
    for (uint32_t k = tid; k < rb; k += 256) {
      const uint32_t x = row_byte(row, k), a = k >= 3 ? row_byte(row, k - 3) : 0, b = y ? row_byte(up, k) : 0, c = (y && k >= 3) ? row_byte(up, k - 3) : 0;
      for (int t = 0; t < 5; t++) c5[t] += filter_cost(filter_byte(t, x, a, b, c));
    }
    for (int t = 0; t < 5; t++) cost[t][tid] = c5[t];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if (tid < half) for (int t = 0; t < 5; t++) cost[t][tid] += cost[t][tid + half];
      __syncthreads();
    }
    if (tid == 0) {
      int best = 0;
      for (int t = 1; t < 5; t++) if (cost[t][0] < cost[best][0]) best = t;
      s_type = best;
    }
    __syncthreads();
    type = s_type;
  }
  if (tid == 0) out[0] = (uint8_t)type;
  for (uint32_t k = tid; k < rb; k += 256) {
    const uint32_t x = row_byte(row, k);
    uint8_t v = (uint8_t)x;
    if (type) v = filter_byte(type, x, k >= 3 ? row_byte(row, k - 3) : 0, y ? row_byte(up, k) : 0, (y && k >= 3) ? row_byte(up, k - 3) : 0);
    out[1 + k] = v;
  }
}

// ---- links
__global__ void k_png_keys(Streams S, uint32_t per, uint32_t total, uint32_t *__restrict__ keys, uint32_t *__restrict__ pos) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < total; r += gridDim.x * blockDim.x) {
    const uint32_t f = r / per, i = r % per;
    const uint64_t at = (uint64_t)f * S.ns + i;
    keys[r] = (f << 24) | key3(S.base + at);
    pos[r] = (uint32_t)at;
  }
}
// sorted by (frame, key, position): the entry below is the nearest earlier position of the frame with the same three bytes
__global__ void k_png_links(const uint32_t *__restrict__ keys_sorted, const uint32_t *__restrict__ ord, uint32_t total, uint32_t ns, int32_t *__restrict__ prev) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < total; r += gridDim.x * blockDim.x) {
    const uint32_t at = ord[r];
    prev[at] = (r > 0 && keys_sorted[r - 1] == keys_sorted[r]) ? (int32_t)(ord[r - 1] - (keys_sorted[r] >> 24) * ns) : -1;
  }
}

// ---- match
__global__ __launch_bounds__(256) void k_png_match(Streams S, uint64_t positions, const int32_t *__restrict__ prev, uint32_t *__restrict__ md) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < positions; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t base = (t / S.n) * S.ns;
    const uint32_t i = (uint32_t)(t % S.n);
    uint32_t dist = 0;
    const uint32_t len = best_match(S.base + base, S.n, prev + base, i, &dist);
    md[base + i] = len ? (len | (dist << 16)) : 0u;
  }
}

// ---- parse and histograms
__global__ __launch_bounds__(256) void k_png_parse(Streams S, const uint32_t *__restrict__ md, uint32_t *__restrict__ hist, uint32_t *__restrict__ tokmap) {
  extern __shared__ __align__(16) uint32_t parse_lds[];
  uint16_t *len16 = reinterpret_cast<uint16_t *>(parse_lds);  // the lengths; bit 15: the parse stops here (a token)
  uint32_t *h = parse_lds + kSeg / 2;
  const uint32_t seg = blockIdx.x, tid = threadIdx.x;
  const Seg g = seg_of(S, seg);
  for (uint32_t k = tid; k < g.count; k += 256) len16[k] = (uint16_t)(md[g.base + k] & 0xffffu);
  for (uint32_t k = tid; k < kHistStride; k += 256) h[k] = 0;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t k = 0; k < g.count;) {
      const uint32_t l = len16[k];
      len16[k] = (uint16_t)(l | 0x8000u);
      k += l ? l : 1;
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < g.count; k += 256) {
    const uint32_t v = len16[k];
    if (!(v & 0x8000u)) continue;
    const uint32_t len = v & 0x7fffu;
    if (len) {
      uint32_t sym, eb, ev;
      len_symbol(len, &sym, &eb, &ev);
      atomicAdd(&h[sym], 1u);
      dist_symbol(md[g.base + k] >> 16, &sym, &eb, &ev);
      atomicAdd(&h[288 + sym], 1u);
    } else {
      atomicAdd(&h[S.base[g.base + k]], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < kHistStride; k += 256) hist[(size_t)seg * kHistStride + k] = h[k];
  for (uint32_t wd = tid; wd < kMapWords; wd += 256) {
    uint32_t bits = 0;
    for (uint32_t b = 0; b < 32; b++) {
      const uint32_t k = wd * 32 + b;
      if (k < g.count && (len16[k] & 0x8000u)) bits |= 1u << b;
    }
    tokmap[(size_t)seg * kMapWords + wd] = bits;
  }
}

// a segment's Adler-32 sums: s1 = sum of the bytes, s2 = sum of (count - k) byte[k]
__global__ __launch_bounds__(256) void k_png_adler(Streams S, unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long r1[256], r2[256];
  const uint32_t seg = blockIdx.x, tid = threadIdx.x;
  const Seg g = seg_of(S, seg);
  unsigned long long s1 = 0, s2 = 0;
  for (uint32_t k = tid; k < g.count; k += 256) {
    const uint32_t b = S.base[g.base + k];
    s1 += b; s2 += (unsigned long long)(g.count - k) * b;
  }
  r1[tid] = s1; r2[tid] = s2;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)tid < half) { r1[tid] += r1[tid + half]; r2[tid] += r2[tid + half]; }
    __syncthreads();
  }
  if (tid == 0) { sums[(size_t)seg * 2] = r1[0]; sums[(size_t)seg * 2 + 1] = r2[0]; }
}

// ---- pack
__device__ inline void or_word(uint32_t *out, uint32_t word, uint32_t v) {
  if (v && word < (uint32_t)kSlotWords) atomicOr(&out[word], v);
}
__device__ inline void put_bits(uint32_t *out, uint32_t pos, uint64_t val, uint32_t nb) {  // nb <= 48 bits at bit pos, lowest first
  const uint32_t word = pos >> 5, sh = pos & 31u;
  const uint64_t lo = val << sh;
  or_word(out, word, (uint32_t)lo);
  or_word(out, word + 1, (uint32_t)(lo >> 32));
  if (sh + nb > 64) or_word(out, word + 2, (uint32_t)(val >> (64 - sh)));
}
__device__ inline void put_byte(uint32_t *out, uint32_t at, uint32_t v) { or_word(out, at >> 2, v << (8 * (at & 3u))); }

__global__ __launch_bounds__(256) void k_png_pack(Streams S, const uint32_t *__restrict__ md, const uint32_t *__restrict__ tokmap, const SegTables *__restrict__ tabs,
                                                  uint32_t *__restrict__ slots) {
  __shared__ uint32_t out[kSlotWords];
  __shared__ uint32_t lit[kLitSyms + 2], dst[kDistSyms + 2], wsum[4];
  const uint32_t seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const Seg g = seg_of(S, seg);
  const SegTables &T = tabs[seg];
  const uint32_t stored = T.stored, last = T.last, hdr_nbits = T.hdr_nbits, out_bytes = T.out_bytes;
  for (uint32_t k = tid; k < (uint32_t)kSlotWords; k += 256) out[k] = 0;
  for (uint32_t k = tid; k < (uint32_t)kLitSyms + 2; k += 256) lit[k] = T.lit[k];
  if (tid < (uint32_t)kDistSyms + 2) dst[tid] = T.dist[tid];
  __syncthreads();
  if (stored) {
    const uint32_t hdr[5] = {last, g.count & 0xffu, g.count >> 8, ~g.count & 0xffu, (~g.count >> 8) & 0xffu};
    for (uint32_t k = tid; k < 5 + g.count; k += 256) put_byte(out, k, k < 5 ? hdr[k] : (uint32_t)S.base[g.base + k - 5]);
    if (tid == 0 && !last) { put_byte(out, 5 + g.count + 3, 0xff); put_byte(out, 5 + g.count + 4, 0xff); }
  } else {
    for (uint32_t k = tid; k < (hdr_nbits + 31) / 32 && k < (uint32_t)kHdrWords; k += 256) out[k] = T.hdr[k];
    __syncthreads();
    uint32_t run = hdr_nbits;  // the bit the next token starts at; the same in every lane
    for (uint32_t k0 = 0; k0 < g.count; k0 += 256) {
      const uint32_t k = k0 + tid;
      uint64_t val = 0;
      uint32_t nb = 0;
      if (k < g.count && ((tokmap[(size_t)seg * kMapWords + (k >> 5)] >> (k & 31u)) & 1u)) {
        const uint32_t m = md[g.base + k];
        nb = m ? match_bits(lit, dst, m & 0xffffu, m >> 16, &val) : literal_bits(lit, S.base[g.base + k], &val);
      }
      uint32_t incl = nb;
      for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t below = __shfl_up(incl, off);
        if (lane >= off) incl += below;
      }
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      uint32_t before = 0, total = 0;
      for (uint32_t v = 0; v < 4; v++) { if (v < wave) before += wsum[v]; total += wsum[v]; }
      if (nb) put_bits(out, run + before + incl - nb, val, nb);
      run += total;
      __syncthreads();
    }
    if (tid == 0) {
      put_bits(out, run, lit[256] & 0xffffu, lit[256] >> 16);
      run += lit[256] >> 16;
      if (!last) { const uint32_t at = (run + 3 + 7) / 8; put_byte(out, at + 2, 0xff); put_byte(out, at + 3, 0xff); }
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < (out_bytes + 3) / 4 && k < (uint32_t)kSlotWords; k += 256) slots[(size_t)seg * kSlotWords + k] = out[k];
}

// the slots behind one another: segment seg's out_bytes at dst + offs[seg]
__global__ __launch_bounds__(256) void k_png_compact(const uint32_t *__restrict__ slots, const SegTables *__restrict__ tabs, const unsigned long long *__restrict__ offs,
                                                     uint8_t *__restrict__ dst) {
  const uint32_t seg = blockIdx.x;
  const uint8_t *src = reinterpret_cast<const uint8_t *>(slots + (size_t)seg * kSlotWords);
  const uint32_t nbytes = tabs[seg].out_bytes < kSlotBytes ? tabs[seg].out_bytes : kSlotBytes;
  uint8_t *to = dst + offs[seg];
  for (uint32_t k = threadIdx.x; k < nbytes; k += 256) to[k] = src[k];
}

inline dim3 grid_of(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192))); }

// The coder on nf streams of n bytes in device memory: bodies[f] = the deflate blocks of stream f, adlers[f] its Adler-32.
struct DeviceCoder {
  DevBuf prev, md, keys, pos, keys_sorted, ord, tmp, hist, tokmap, sums, tabs, slots, offs, packed;
  std::vector<uint32_t> h_hist;
  std::vector<unsigned long long> h_sums, h_offs;
  std::vector<SegTables> h_tabs;
  std::vector<uint8_t> h_packed;

  int run(const uint8_t *dev_streams, uint64_t ns, uint32_t n, int nf, hipStream_t stream, std::vector<std::vector<uint8_t>> &bodies, std::vector<uint32_t> &adlers) {
    bodies.assign((size_t)nf, {});
    adlers.assign((size_t)nf, 1u);
    if (nf == 0) return TM_OK;
    const uint32_t segs = seg_count(n), nseg = segs * (uint32_t)nf;
    const Streams S{dev_streams, ns, n, segs};
    const uint64_t span = (uint64_t)nf * ns;  // prev[] and md[] are indexed like the streams
    TM_TRY(prev.alloc(std::max<uint64_t>(span, 1) * 4)); TM_TRY(md.alloc(std::max<uint64_t>(span, 1) * 4));
    TM_TRY(hist.alloc((size_t)nseg * kHistStride * 4)); TM_TRY(tokmap.alloc((size_t)nseg * kMapWords * 4)); TM_TRY(sums.alloc((size_t)nseg * 16));
    TM_TRY(tabs.alloc((size_t)nseg * sizeof(SegTables))); TM_TRY(slots.alloc((size_t)nseg * kSlotBytes)); TM_TRY(offs.alloc((size_t)nseg * 8));
    if (span) TM_HIP(hipMemsetAsync(prev.p, 0xff, span * 4, stream));
    if (n >= 3) {
      const uint32_t per = n - 2;
      const uint64_t total64 = (uint64_t)per * nf;
      TM_CHECK(total64 < ((uint64_t)1 << 32) && span < ((uint64_t)1 << 32), TM_E_UNSUPPORTED, "png out: a chunk of %llu stream bytes", (unsigned long long)span);
      const uint32_t total = (uint32_t)total64;
      TM_TRY(keys.alloc((size_t)total * 4)); TM_TRY(pos.alloc((size_t)total * 4)); TM_TRY(keys_sorted.alloc((size_t)total * 4)); TM_TRY(ord.alloc((size_t)total * 4));
      hipLaunchKernelGGL(k_png_keys, grid_of(total), dim3(256), 0, stream, S, per, total, keys.as<uint32_t>(), pos.as<uint32_t>());
      int bits = 24;
      while ((1 << (bits - 24)) < nf) bits++;
      TM_TRY(with_temp(tmp, "png out: radix sort of the positions", [&](void *t, size_t &b) {
        return rocprim::radix_sort_pairs(t, b, keys.as<uint32_t>(), keys_sorted.as<uint32_t>(), pos.as<uint32_t>(), ord.as<uint32_t>(), (size_t)total, 0, bits, stream);
      }));
      hipLaunchKernelGGL(k_png_links, grid_of(total), dim3(256), 0, stream, keys_sorted.as<uint32_t>(), ord.as<uint32_t>(), total, (uint32_t)ns, prev.as<int32_t>());
    }
    if (n) hipLaunchKernelGGL(k_png_match, grid_of((uint64_t)nf * n), dim3(256), 0, stream, S, (uint64_t)nf * n, prev.as<int32_t>(), md.as<uint32_t>());
    TM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_png_parse), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kParseLds));  // (65 KB: above the default limit)
    hipLaunchKernelGGL(k_png_parse, dim3(nseg), dim3(256), kParseLds, stream, S, md.as<uint32_t>(), hist.as<uint32_t>(), tokmap.as<uint32_t>());
    hipLaunchKernelGGL(k_png_adler, dim3(nseg), dim3(256), 0, stream, S, sums.as<unsigned long long>());
    TM_HIP(hipGetLastError());
    h_hist.resize((size_t)nseg * kHistStride); h_sums.resize((size_t)nseg * 2);
    TM_HIP(hipMemcpyAsync(h_hist.data(), hist.p, h_hist.size() * 4, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipMemcpyAsync(h_sums.data(), sums.p, h_sums.size() * 8, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    // the code lengths, tables and sizes of every segment, on the host
    h_tabs.resize(nseg); h_offs.resize(nseg);
    auto plan = [&](uint32_t from, uint32_t to) {
      for (uint32_t seg = from; seg < to; seg++) {
        const uint32_t g = seg % segs, first = g * kSeg;
        plan_segment(&h_hist[(size_t)seg * kHistStride], &h_hist[(size_t)seg * kHistStride + 288], std::min(kSeg, n - first), g + 1 == segs, &h_tabs[seg]);
      }
    };
    const uint32_t nthreads = std::min<uint32_t>((uint32_t)host_threads(), std::max<uint32_t>(1, nseg / 16));
    if (nthreads <= 1) plan(0, nseg);
    else {
      std::vector<std::thread> helpers;
      for (uint32_t t = 1; t < nthreads; t++) helpers.emplace_back(plan, (uint32_t)((uint64_t)nseg * t / nthreads), (uint32_t)((uint64_t)nseg * (t + 1) / nthreads));
      plan(0, (uint32_t)((uint64_t)nseg / nthreads));
      for (auto &h : helpers) h.join();
    }
    uint64_t at = 0;
    for (uint32_t seg = 0; seg < nseg; seg++) { h_offs[seg] = at; at += h_tabs[seg].out_bytes; }
    TM_TRY(packed.alloc(at));
    TM_HIP(hipMemcpyAsync(tabs.p, h_tabs.data(), (size_t)nseg * sizeof(SegTables), hipMemcpyHostToDevice, stream));
    TM_HIP(hipMemcpyAsync(offs.p, h_offs.data(), (size_t)nseg * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_png_pack, dim3(nseg), dim3(256), 0, stream, S, md.as<uint32_t>(), tokmap.as<uint32_t>(), tabs.as<SegTables>(), slots.as<uint32_t>());
    hipLaunchKernelGGL(k_png_compact, dim3(nseg), dim3(256), 0, stream, slots.as<uint32_t>(), tabs.as<SegTables>(), offs.as<unsigned long long>(), packed.as<uint8_t>());
    TM_HIP(hipGetLastError());
    h_packed.resize(at);
    TM_HIP(hipMemcpyAsync(h_packed.data(), packed.p, at, hipMemcpyDeviceToHost, stream));
    TM_HIP(hipStreamSynchronize(stream));
    for (int f = 0; f < nf; f++) {
      const uint32_t s0 = (uint32_t)f * segs;
      const uint64_t from = h_offs[s0], to = f + 1 < nf ? h_offs[s0 + segs] : at;
      bodies[(size_t)f].assign(h_packed.begin() + (ptrdiff_t)from, h_packed.begin() + (ptrdiff_t)to);
      uint32_t a = 1, b = 0;
      for (uint32_t g = 0; g < segs; g++) adler_append(&a, &b, h_sums[(size_t)(s0 + g) * 2], h_sums[(size_t)(s0 + g) * 2 + 1], std::min(kSeg, n - g * kSeg));
      adlers[(size_t)f] = (b << 16) | a;
    }
    return TM_OK;
  }
};

}  // namespace

struct PngDeviceEncoder::State {
  DevBuf streams;
  DeviceCoder coder;
  std::vector<std::vector<uint8_t>> bodies;
  std::vector<uint32_t> adlers;
  std::vector<uint8_t> other;
};
PngDeviceEncoder::PngDeviceEncoder() : state_(new State) {}
PngDeviceEncoder::~PngDeviceEncoder() { delete state_; }

int PngDeviceEncoder::encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, int filter, void *hip_stream,
                             std::vector<std::vector<uint8_t>> &files) {
  hipStream_t stream = (hipStream_t)hip_stream;
  DevBuf &streams = state_->streams;
  DeviceCoder &coder = state_->coder;
  std::vector<std::vector<uint8_t>> &bodies = state_->bodies;
  std::vector<uint32_t> &adlers = state_->adlers;
  std::vector<uint8_t> &other = state_->other;
  files.assign((size_t)nframes, {});
  const uint32_t n = (uint32_t)((uint64_t)h * (1 + 3 * (uint64_t)w));
  const uint64_t ns = ((uint64_t)n + 3) & ~(uint64_t)3;
  const int chunk = (int)std::max<uint64_t>(1, std::min<uint64_t>(32, kChunkBytes / ns));
  TM_TRY(streams.alloc(ns * (uint64_t)std::min(chunk, std::max(nframes, 1))));
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const int nf = std::min(chunk, nframes - f0);
    for (int pass = 0; pass < (filter == kFilterSmaller ? 2 : 1); pass++) {
      const bool adaptive = filter == kFilterAdaptive || pass == 1;
      hipLaunchKernelGGL(k_png_filter, dim3((unsigned)h, (unsigned)nf), dim3(256), 0, stream, dev_frames + (int64_t)f0 * frame_px, stride_px, frame_px, w, adaptive ? 1 : 0,
                         streams.as<uint8_t>(), ns);
      TM_HIP(hipGetLastError());
      TM_TRY(coder.run(streams.as<uint8_t>(), ns, n, nf, stream, bodies, adlers));
      for (int f = 0; f < nf; f++) {
        std::vector<uint8_t> &file = files[(size_t)(f0 + f)];
        if (pass == 0) { png_wrap(w, h, bodies[(size_t)f].data(), bodies[(size_t)f].size(), adlers[(size_t)f], file); continue; }
        png_wrap(w, h, bodies[(size_t)f].data(), bodies[(size_t)f].size(), adlers[(size_t)f], other);
        if (other.size() < file.size()) file.swap(other);  // SMALLER: a tie stays with NONE
      }
    }
  }
  return TM_OK;
}

}  // namespace dfl
}  // namespace tmx

extern "C" {

int tm_stage_png_encode(const uint32_t *dev_frames, int64_t stride_px, int64_t frame_px, int nframes, int w, int h, const tm_png_options *opt, uint8_t *host_out,
                        int64_t cap, int64_t *offsets, void *stream) {
  using namespace tmx;
  TM_TRY(dfl::png_check("tm_stage_png_encode", dev_frames, stride_px, frame_px, nframes, w, h, opt));
  TM_CHECK(offsets && (host_out || !cap) && cap >= 0, TM_E_INVAL, "tm_stage_png_encode: null argument");
  TM_TRY(require_device());
  std::vector<std::vector<uint8_t>> files;
  if (opt->level == 0) {  // the stored writer on frames brought to the host, a chunk of rows at their stride at a time
    files.resize((size_t)nframes);
    const int64_t span = (int64_t)(h - 1) * stride_px + w;
    std::vector<uint32_t> px((size_t)span);
    for (int f = 0; f < nframes; f++) {
      TM_HIP(hipMemcpyAsync(px.data(), dev_frames + (int64_t)f * frame_px, (size_t)span * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
      TM_HIP(hipStreamSynchronize((hipStream_t)stream));
      dfl::png_stored(px.data(), stride_px, w, h, files[(size_t)f]);
    }
  } else {
    dfl::PngDeviceEncoder encoder;
    TM_TRY(encoder.encode(dev_frames, stride_px, frame_px, nframes, w, h, opt->filter == TM_PNG_FILTER_AUTO ? TM_PNG_FILTER_NONE : opt->filter, stream, files));
  }
  int64_t total = 0;
  for (const auto &f : files) total += (int64_t)f.size();
  if (total > cap) {
    offsets[nframes] = total;
    TM_CHECK(false, TM_E_INVAL, "tm_stage_png_encode: %lld bytes needed, %lld given", (long long)total, (long long)cap);
  }
  int64_t at = 0;
  for (int f = 0; f < nframes; f++) {
    offsets[f] = at;
    memcpy(host_out + at, files[(size_t)f].data(), files[(size_t)f].size());
    at += (int64_t)files[(size_t)f].size();
  }
  offsets[nframes] = at;
  return TM_OK;
}

int tm_stage_zlib_compress(const uint8_t *dev_src, int64_t n, uint8_t *host_out, int64_t cap, int64_t *out_n, void *stream) {
  using namespace tmx;
  TM_CHECK((dev_src || !n) && out_n && (host_out || !cap), TM_E_INVAL, "tm_stage_zlib_compress: null argument");
  TM_CHECK(n >= 0 && n < ((int64_t)1 << 31) && cap >= 0, TM_E_INVAL, "tm_stage_zlib_compress: a stream of %lld bytes (0 .. 2^31 - 1)", (long long)n);
  TM_TRY(require_device());
  dfl::DeviceCoder coder;
  std::vector<std::vector<uint8_t>> bodies;
  std::vector<uint32_t> adlers;
  TM_TRY(coder.run(dev_src, (uint64_t)n, (uint32_t)n, 1, (hipStream_t)stream, bodies, adlers));
  const int64_t need = 2 + (int64_t)bodies[0].size() + 4;
  *out_n = need;
  TM_CHECK(cap >= need, TM_E_INVAL, "tm_stage_zlib_compress: %lld bytes needed, %lld given", (long long)need, (long long)cap);
  host_out[0] = 0x78; host_out[1] = 0x9c;
  memcpy(host_out + 2, bodies[0].data(), bodies[0].size());
  const uint32_t ad = adlers[0];
  uint8_t *tail = host_out + 2 + bodies[0].size();
  tail[0] = ad >> 24; tail[1] = ad >> 16; tail[2] = ad >> 8; tail[3] = ad;
  return TM_OK;
}

}  // extern "C"
