// tm_lz_matches.hip -- the LZMA coder's match finder on the device, and the pipeline that feeds the host parser from it (DESIGN.md
// section 33).  The rule is tm_lz_matches.h's; the host twin is IncrementalFinder (tm_lzma.hip), and the two return the same pairs in the
// same order.
//
//   prepare   three stable radix sorts (rocPRIM) of the stream's positions, by the 2-byte value, by h3 and by h4.  In a stable sort by key
//             the entry just below a position's own is the nearest earlier position with that key: k_lz_links turns the first two orders
//             into prev2[] / prev3[] (-1: none).  The h4 order is kept whole -- ord4[] (positions by (h4, position)), key4s[] (their keys)
//             and rank4[] (a position's place in it): a position's hash chain, nearest first, is the stretch of ord4 just below its own
//             rank, read downwards while the key holds.  Contiguous reads, not a pointer chase.  Only positions with j + 2 / 3 / 4 <= n
//             are sorted: what the incremental finder inserts.
//   window    k_lz_window, one lane per position of [first, first + count): c2, c3, then at most kDepth steps down the stretch, keeping the
//             records of the running maximum.  It runs twice: a count pass (counts only), an exclusive scan of the counts, then the same
//             walk again storing each list at its offset -- the pair buffer is sized from the counts, no list is ever truncated.  Bytes are
//             compared a word at a time where the two positions are congruent mod 4.  Every loop is bounded by kDepth and kMaxLen; plain
//             launches, nothing waits on another workgroup.
//
// Device memory for a stream of n bytes: n (the bytes) + 20 n (prev2, prev3, ord4, key4s, rank4) held while its windows are found, plus
// 16 n of sort buffers and rocPRIM's temporary (about 8 n) during prepare; per window of w positions 13 w (counts, 64-bit offsets, 32-bit
// counts) + 8 bytes per pair.  Host memory: per stream in flight two windows of w + 8 bytes per pair.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include "tm_common.h"
#include "tm_lz_matches.h"

namespace tmx {
namespace {

using lzm::Pair;
constexpr size_t kDefaultWindow = (size_t)1 << 18;

// ---- prepare
template <int WHICH>  // 2, 3, 4: the key of the bytes at a position
__global__ void k_lz_keys(const uint8_t *__restrict__ src, uint32_t m, uint32_t *__restrict__ keys, uint32_t *__restrict__ pos) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) {
    keys[r] = WHICH == 2 ? lzm::key2(src + r) : WHICH == 3 ? lzm::h3(src + r) : lzm::h4(src + r);
    pos[r] = r;
  }
}
// sorted by (key, position): the entry below is the nearest earlier position with the same key
__global__ void k_lz_links(const uint32_t *__restrict__ keys_sorted, const uint32_t *__restrict__ ord, uint32_t m, int32_t *__restrict__ prev) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x)
    prev[ord[r]] = (r > 0 && keys_sorted[r - 1] == keys_sorted[r]) ? (int32_t)ord[r - 1] : -1;
}
__global__ void k_lz_ranks(const uint32_t *__restrict__ ord, uint32_t m, uint32_t *__restrict__ rank) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) rank[ord[r]] = r;
}

// ---- window
// equal bytes of src[a + l] and src[b + l] from l = from on, at most max_len (a > b, a + max_len <= n)
__device__ inline uint32_t match_len_dev(const uint8_t *__restrict__ src, uint32_t a, uint32_t b, uint32_t from, uint32_t max_len) {
  uint32_t l = from;
  if (((a - b) & 3u) == 0) {  // the two run through word boundaries together
    const uint8_t *pa = src + a, *pb = src + b;
    while (l < max_len && ((uintptr_t)(pa + l) & 3u)) {
      if (pa[l] != pb[l]) return l;
      l++;
    }
    while (l + 4 <= max_len) {
      const uint32_t x = *reinterpret_cast<const uint32_t *>(pa + l) ^ *reinterpret_cast<const uint32_t *>(pb + l);
      if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
      l += 4;
    }
  }
  while (l < max_len && src[a + l] == src[b + l]) l++;
  return l;
}

struct LzLinks {  // what prepare leaves for the windows
  const uint8_t *src;
  uint32_t n;
  const int32_t *prev2, *prev3;
  const uint32_t *ord4, *key4s, *rank4;
};

// WRITE = false: counts[t] and cnt32[t] of position first + t.  WRITE = true: the same walk, the pairs stored at pairs[offs[t]...].
template <bool WRITE>
__global__ __launch_bounds__(256) void k_lz_window(LzLinks L, uint32_t first, uint32_t count, uint8_t *__restrict__ counts, uint32_t *__restrict__ cnt32,
                                                   const unsigned long long *__restrict__ offs, Pair *__restrict__ pairs) {
  const uint8_t *__restrict__ src = L.src;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = first + t, max_len = lzm::max_len_at(L.n, i);
    Pair *out = WRITE ? pairs + offs[t] : nullptr;
    uint32_t np = 0, best = 1;
    auto record = [&](uint32_t len, uint32_t dist) {
      if (WRITE) out[np] = Pair{(uint16_t)len, 0, dist - 1};
      np++;
    };
    if (max_len >= 2) {
      const int32_t c2 = L.prev2[i];
      if (c2 >= 0 && i - (uint32_t)c2 <= lzm::kDict) {
        best = match_len_dev(src, i, (uint32_t)c2, 2, max_len);
        record(best, i - (uint32_t)c2);
      }
      if (max_len >= 3 && best < max_len) {
        const int32_t c3 = L.prev3[i];
        if (c3 >= 0 && c3 != c2 && i - (uint32_t)c3 <= lzm::kDict && src[c3] == src[i] && src[c3 + 1] == src[i + 1] && src[c3 + 2] == src[i + 2]) {
          const uint32_t l = match_len_dev(src, i, (uint32_t)c3, 3, max_len);
          if (l > best) { best = l; record(l, i - (uint32_t)c3); }
        }
      }
      if (max_len >= 4 && best < max_len) {
        const uint32_t r = L.rank4[i], key = L.key4s[r];
        for (uint32_t depth = 0; depth < (uint32_t)lzm::kDepth && depth < r; depth++) {
          const uint32_t q = r - 1 - depth;
          if (L.key4s[q] != key) break;
          const uint32_t c = L.ord4[q], dist = i - c;
          if (dist > lzm::kDict) break;
          if (src[c + best] != src[i + best] || src[c] != src[i]) continue;  // (best < max_len <= n - i, c < i: in bounds)
          const uint32_t l = match_len_dev(src, i, c, 0, max_len);
          if (l > best) {
            best = l;
            record(l, dist);
            if (l == max_len) break;
          }
        }
      }
    }
    if (!WRITE) { counts[t] = (uint8_t)np; cnt32[t] = np; }
  }
}

inline dim3 grid_of(size_t n) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096))); }

// The finder of one stream: prepare() once, then windows in any order.
class LzDeviceFinder {
 public:
  int prepare(const uint8_t *dev_src, size_t n, hipStream_t stream) {
    TM_CHECK(n < ((size_t)1 << 31), TM_E_UNSUPPORTED, "lz matches: streams of 2^31 bytes or more are not supported (%zu)", n);
    src_ = dev_src; n_ = n; stream_ = stream;
    if (n < 2) return TM_OK;  // no position has two bytes left: every list is empty
    const size_t words = n * 4;
    TM_TRY(prev2_.alloc(words)); TM_TRY(prev3_.alloc(words)); TM_TRY(ord4_.alloc(words)); TM_TRY(key4s_.alloc(words)); TM_TRY(rank4_.alloc(words));
    DevBuf keys, pos, keys_sorted, ord, tmp;
    TM_TRY(keys.alloc(words)); TM_TRY(pos.alloc(words)); TM_TRY(keys_sorted.alloc(words)); TM_TRY(ord.alloc(words));
    // (positions past a set are never asked for their link: a query there has fewer bytes left than the key is long)
    const uint32_t m2 = (uint32_t)(n - 1), m3 = n >= 3 ? (uint32_t)(n - 2) : 0, m4 = n >= 4 ? (uint32_t)(n - 3) : 0;
    hipLaunchKernelGGL(k_lz_keys<2>, grid_of(m2), dim3(256), 0, stream, src_, m2, keys.as<uint32_t>(), pos.as<uint32_t>());
    TM_TRY(sort(tmp, keys, keys_sorted.as<uint32_t>(), pos, ord.as<uint32_t>(), m2, lzm::kBits2));
    hipLaunchKernelGGL(k_lz_links, grid_of(m2), dim3(256), 0, stream, keys_sorted.as<uint32_t>(), ord.as<uint32_t>(), m2, prev2_.as<int32_t>());
    if (m3) {
      hipLaunchKernelGGL(k_lz_keys<3>, grid_of(m3), dim3(256), 0, stream, src_, m3, keys.as<uint32_t>(), pos.as<uint32_t>());
      TM_TRY(sort(tmp, keys, keys_sorted.as<uint32_t>(), pos, ord.as<uint32_t>(), m3, lzm::kBits3));
      hipLaunchKernelGGL(k_lz_links, grid_of(m3), dim3(256), 0, stream, keys_sorted.as<uint32_t>(), ord.as<uint32_t>(), m3, prev3_.as<int32_t>());
    }
    if (m4) {
      hipLaunchKernelGGL(k_lz_keys<4>, grid_of(m4), dim3(256), 0, stream, src_, m4, keys.as<uint32_t>(), pos.as<uint32_t>());
      TM_TRY(sort(tmp, keys, key4s_.as<uint32_t>(), pos, ord4_.as<uint32_t>(), m4, lzm::kBits4));
      hipLaunchKernelGGL(k_lz_ranks, grid_of(m4), dim3(256), 0, stream, ord4_.as<uint32_t>(), m4, rank4_.as<uint32_t>());
    }
    TM_HIP(hipGetLastError());
    TM_HIP(hipStreamSynchronize(stream));  // (the sort buffers are released on return)
    return TM_OK;
  }
  // counts of positions [first, first + count) into dev_counts; *total = their pairs.  Leaves the offsets for fill().
  int count(size_t first, size_t count, uint8_t *dev_counts, size_t *total) {
    *total = 0;
    counted_ = count;
    if (count == 0) return TM_OK;
    if (n_ < 2) { TM_HIP(hipMemsetAsync(dev_counts, 0, count, stream_)); TM_HIP(hipStreamSynchronize(stream_)); return TM_OK; }
    TM_TRY(cnt32_.alloc((count + 1) * 4)); TM_TRY(offs_.alloc((count + 1) * 8));
    TM_HIP(hipMemsetAsync(cnt32_.as<uint32_t>() + count, 0, 4, stream_));
    hipLaunchKernelGGL(k_lz_window<false>, grid_of(count), dim3(256), 0, stream_, links(), (uint32_t)first, (uint32_t)count, dev_counts, cnt32_.as<uint32_t>(),
                       (const unsigned long long *)nullptr, (Pair *)nullptr);
    TM_HIP(hipGetLastError());
    TM_TRY(with_temp(tmp_, "lz matches: scan of the counts", [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, cnt32_.as<uint32_t>(), offs_.as<unsigned long long>(), 0ull, count + 1, rocprim::plus<unsigned long long>(), stream_);
    }));
    unsigned long long tot = 0;
    TM_HIP(hipMemcpyAsync(&tot, offs_.as<unsigned long long>() + count, 8, hipMemcpyDeviceToHost, stream_));
    TM_HIP(hipStreamSynchronize(stream_));
    *total = (size_t)tot;
    first_ = first;
    return TM_OK;
  }
  // the pairs of the positions just counted into dev_pairs (room for *total of them)
  int fill(Pair *dev_pairs) {
    if (counted_ == 0 || n_ < 2) return TM_OK;
    hipLaunchKernelGGL(k_lz_window<true>, grid_of(counted_), dim3(256), 0, stream_, links(), (uint32_t)first_, (uint32_t)counted_, (uint8_t *)nullptr,
                       (uint32_t *)nullptr, offs_.as<unsigned long long>(), dev_pairs);
    TM_HIP(hipGetLastError());
    return TM_OK;
  }

 private:
  LzLinks links() const { return LzLinks{src_, (uint32_t)n_, prev2_.as<int32_t>(), prev3_.as<int32_t>(), ord4_.as<uint32_t>(), key4s_.as<uint32_t>(), rank4_.as<uint32_t>()}; }
  int sort(DevBuf &tmp, DevBuf &keys, uint32_t *keys_out, DevBuf &pos, uint32_t *pos_out, uint32_t m, int bits) {
    return with_temp(tmp, "lz matches: radix sort of the positions", [&](void *t, size_t &b) {
      return rocprim::radix_sort_pairs(t, b, keys.as<uint32_t>(), keys_out, pos.as<uint32_t>(), pos_out, (size_t)m, 0, bits, stream_);
    });
  }
  const uint8_t *src_ = nullptr;
  size_t n_ = 0, first_ = 0, counted_ = 0;
  hipStream_t stream_ = nullptr;
  DevBuf prev2_, prev3_, ord4_, key4s_, rank4_, cnt32_, offs_, tmp_;
};

size_t window_positions() {  // TM_LZ_WINDOW, read at each call
  const char *v = getenv("TM_LZ_WINDOW");
  const long long w = v ? atoll(v) : 0;
  return w > 0 ? (size_t)w : kDefaultWindow;
}

// ---- the pipeline: windows of lists from the calling thread to a stream's parser thread
struct LzWindow {
  size_t first = 0, count = 0;
  std::vector<uint8_t> counts;
  std::vector<Pair> pairs;
};
struct LzPipe {  // what the queues of all streams share
  std::mutex m;
  std::condition_variable cv_producer, cv_parsers;
  bool failed = false;  // the producer gave up: parsers run on without lists and their output is dropped
  int completed = 0;    // streams parsed to their end
};
class QueueSource : public lzm::MatchSource {
 public:
  static constexpr size_t kDeep = 2;
  explicit QueueSource(LzPipe *pipe) : pipe_(pipe) {}
  int find(size_t i, uint32_t *lens, uint32_t *dists) override {
    while (i >= cur_.first + cur_.count) {
      std::unique_lock<std::mutex> lk(pipe_->m);
      pipe_->cv_parsers.wait(lk, [&] { return !q_.empty() || pipe_->failed; });
      if (q_.empty()) return 0;
      cur_ = std::move(q_.front());
      q_.pop_front();
      at_ = cur_.first; off_ = 0;
      pipe_->cv_producer.notify_one();
    }
    while (at_ < i) off_ += cur_.counts[at_++ - cur_.first];
    const int np = cur_.counts[i - cur_.first];
    const Pair *p = cur_.pairs.data() + off_;
    for (int q = 0; q < np; q++) { lens[q] = p[q].len; dists[q] = p[q].dist; }
    return np;
  }
  bool has_room() const { return q_.size() < kDeep; }       // (under the pipe's lock)
  void push(LzWindow &&w) { q_.push_back(std::move(w)); }   // (under the pipe's lock)

 private:
  LzPipe *pipe_;
  std::deque<LzWindow> q_;
  LzWindow cur_;
  size_t at_ = 0, off_ = 0;
};

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

struct OpenStream {  // a stream whose windows are being found
  size_t job = 0, next = 0;
  DevBuf src;
  LzDeviceFinder finder;
};

int compress_jobs_host(std::vector<LzJob> &jobs, int threads, LzJobsReport *report) {
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t k = next.fetch_add(1); k < jobs.size(); k = next.fetch_add(1)) {
      const auto t0 = std::chrono::steady_clock::now();
      lz_compress_from(jobs[k].src, jobs[k].n, nullptr, jobs[k].out);
      jobs[k].parse_ms = ms_since(t0);
    }
  };
  std::vector<std::thread> helpers;
  for (int t = 1; t < threads; t++) helpers.emplace_back(work);
  work();
  for (auto &h : helpers) h.join();
  for (const LzJob &j : jobs) report->parse_ms += j.parse_ms;
  return TM_OK;
}

int compress_jobs_device(std::vector<LzJob> &jobs, int threads, hipStream_t stream, LzJobsReport *report) {
  for (const LzJob &j : jobs) TM_CHECK(j.n < ((size_t)1 << 31), TM_E_UNSUPPORTED, "lz matches: streams of 2^31 bytes or more are not supported (%zu)", j.n);
  const size_t window = window_positions(), njobs = jobs.size();
  LzPipe pipe;
  std::vector<std::unique_ptr<QueueSource>> sources;
  for (size_t k = 0; k < njobs; k++) sources.emplace_back(new QueueSource(&pipe));
  std::atomic<size_t> next{0};
  std::vector<std::thread> parsers;
  for (int t = 0; t < threads; t++)
    parsers.emplace_back([&] {
      for (size_t k = next.fetch_add(1); k < njobs; k = next.fetch_add(1)) {
        const auto t0 = std::chrono::steady_clock::now();
        lz_compress_from(jobs[k].src, jobs[k].n, sources[k].get(), jobs[k].out);
        jobs[k].parse_ms = ms_since(t0);
        { std::lock_guard<std::mutex> lk(pipe.m); pipe.completed++; }
        pipe.cv_producer.notify_one();
      }
    });
  // the producer: streams are opened in order, at most threads + 1 of them opened and not yet parsed to the end; an open stream gets its
  // next window whenever its queue has room
  std::vector<std::unique_ptr<OpenStream>> open;
  DevBuf d_counts, d_pairs;
  size_t opened = 0;
  auto produce = [&]() -> int {
    for (;;) {
      bool progressed = false;
      int completed;
      { std::lock_guard<std::mutex> lk(pipe.m); completed = pipe.completed; }
      if (opened < njobs && opened - (size_t)completed < (size_t)threads + 1) {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<OpenStream> s(new OpenStream);
        s->job = opened++;
        const LzJob &j = jobs[s->job];
        TM_TRY(s->src.alloc(j.n));
        if (j.n) TM_HIP(hipMemcpyAsync(s->src.p, j.src, j.n, hipMemcpyHostToDevice, stream));
        TM_TRY(s->finder.prepare(s->src.as<uint8_t>(), j.n, stream));
        report->finder_ms += ms_since(t0);
        if (j.n) open.push_back(std::move(s));
        progressed = true;
      }
      for (size_t o = 0; o < open.size();) {
        OpenStream &s = *open[o];
        bool room;
        { std::lock_guard<std::mutex> lk(pipe.m); room = sources[s.job]->has_room(); }
        if (!room) { o++; continue; }
        const auto t0 = std::chrono::steady_clock::now();
        LzWindow w;
        w.first = s.next; w.count = std::min(window, jobs[s.job].n - s.next);
        size_t total = 0;
        TM_TRY(d_counts.alloc(w.count));
        TM_TRY(s.finder.count(w.first, w.count, d_counts.as<uint8_t>(), &total));
        TM_TRY(d_pairs.alloc(std::max<size_t>(total, 1) * sizeof(Pair)));
        TM_TRY(s.finder.fill(d_pairs.as<Pair>()));
        w.counts.resize(w.count); w.pairs.resize(total);
        TM_HIP(hipMemcpyAsync(w.counts.data(), d_counts.p, w.count, hipMemcpyDeviceToHost, stream));
        if (total) TM_HIP(hipMemcpyAsync(w.pairs.data(), d_pairs.p, total * sizeof(Pair), hipMemcpyDeviceToHost, stream));
        TM_HIP(hipStreamSynchronize(stream));
        report->finder_ms += ms_since(t0);
        s.next += w.count;
        { std::lock_guard<std::mutex> lk(pipe.m); sources[s.job]->push(std::move(w)); }
        pipe.cv_parsers.notify_all();
        progressed = true;
        if (s.next >= jobs[s.job].n) open.erase(open.begin() + (long)o);  // (its device memory goes back to the pool)
        else o++;
      }
      if (opened == njobs && open.empty()) return TM_OK;
      if (!progressed) {  // every open queue is full and no stream may be opened: until a parser takes a window or ends a stream
        std::unique_lock<std::mutex> lk(pipe.m);
        pipe.cv_producer.wait(lk, [&] {
          if (pipe.completed != completed) return true;
          for (const auto &s : open) if (sources[s->job]->has_room()) return true;
          return false;
        });
      }
    }
  };
  const int rc = produce();
  if (rc != TM_OK) {
    { std::lock_guard<std::mutex> lk(pipe.m); pipe.failed = true; }
    pipe.cv_parsers.notify_all();
  }
  for (auto &p : parsers) p.join();
  for (const LzJob &j : jobs) report->parse_ms += j.parse_ms;
  return rc;
}

}  // namespace

int lz_compress_jobs(std::vector<LzJob> &jobs, int threads, bool device_finder, void *hip_stream, LzJobsReport *report) {
  threads = (int)std::max<size_t>(1, std::min<size_t>({(size_t)std::max(threads, 1), jobs.size(), (size_t)16}));
  *report = LzJobsReport{};
  report->threads = threads;
  if (jobs.empty()) return TM_OK;
  return device_finder ? compress_jobs_device(jobs, threads, (hipStream_t)hip_stream, report) : compress_jobs_host(jobs, threads, report);
}

}  // namespace tmx

extern "C" int tm_stage_lz_matches(const uint8_t *dev_src, size_t n, size_t first, size_t count, uint8_t *dev_counts_u8, tm_lz_pair *dev_pairs,
                                   size_t cap_pairs, size_t *host_npairs, void *stream) {
  using namespace tmx;
  TM_TRY(require_device());
  TM_CHECK((dev_src || !n) && host_npairs && (dev_counts_u8 || !count), TM_E_INVAL, "tm_stage_lz_matches: null argument");
  TM_CHECK(n < ((size_t)1 << 31), TM_E_UNSUPPORTED, "tm_stage_lz_matches: streams of 2^31 bytes or more are not supported (%zu)", n);
  TM_CHECK(first <= n && count <= n - first, TM_E_INVAL, "tm_stage_lz_matches: positions [%zu,+%zu) outside the %zu bytes", first, count, n);
  *host_npairs = 0;
  LzDeviceFinder finder;
  TM_TRY(finder.prepare(dev_src, n, (hipStream_t)stream));
  const size_t window = window_positions();
  // window by window: the counts of each, then its pairs behind those of the windows before
  size_t total = 0;
  std::vector<size_t> totals;
  for (size_t w0 = 0; w0 < count; w0 += window) {
    size_t t = 0;
    TM_TRY(finder.count(first + w0, std::min(window, count - w0), dev_counts_u8 + w0, &t));
    totals.push_back(t);
    total += t;
  }
  *host_npairs = total;
  TM_CHECK(total <= cap_pairs && (dev_pairs || !total), TM_E_INVAL, "tm_stage_lz_matches: %zu pairs needed, %zu given", total, cap_pairs);
  size_t at = 0, wi = 0;
  for (size_t w0 = 0; w0 < count; w0 += window, wi++) {
    size_t t = 0;
    if (totals.size() > 1) TM_TRY(finder.count(first + w0, std::min(window, count - w0), dev_counts_u8 + w0, &t));  // (the offsets of this window again)
    TM_TRY(finder.fill(reinterpret_cast<lzm::Pair *>(dev_pairs) + at));
    at += totals[wi];
  }
  TM_HIP(hipStreamSynchronize((hipStream_t)stream));
  return TM_OK;
}

extern "C" int tm_stage_lz_compress(const uint8_t *host_src, size_t n, uint8_t *dst, size_t cap, size_t *out_n) {
  using namespace tmx;
  TM_TRY(require_device());
  TM_CHECK((host_src || !n) && out_n, TM_E_INVAL, "tm_stage_lz_compress: null argument");
  std::vector<LzJob> jobs(1);
  jobs[0].src = host_src; jobs[0].n = n;
  LzJobsReport report;
  TM_TRY(lz_compress_jobs(jobs, 1, true, nullptr, &report));
  const std::vector<uint8_t> &out = jobs[0].out;
  *out_n = out.size();
  TM_CHECK(dst && cap >= out.size(), TM_E_INVAL, "tm_stage_lz_compress: %zu bytes needed, %zu given", out.size(), cap);
  memcpy(dst, out.data(), out.size());
  return TM_OK;
}
