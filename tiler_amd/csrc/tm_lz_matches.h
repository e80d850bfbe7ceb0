// tm_lz_matches.h -- what the LZMA coder's match finder is, stated once for its host form (tm_lzma.hip) and its device form
// (tm_lz_matches.hip): DESIGN.md section 33.
//
// The list of position i of a stream src[0, n) is a function of (src, n, i) alone.  Candidates, in this order:
//   c2     the nearest j < i with the same two bytes;
//   c3     the nearest j < i with j + 3 <= n and h3(j) == h3(i); taken only if it differs from c2 and its three bytes are equal;
//   chain  the j < i with j + 4 <= n and h4(j) == h4(i), nearest first, at most kDepth of them visited (rejects included);
// each within kDict of i (the chain walk ends at the first one beyond it).  The list holds the records of the running maximum of the
// match length over that order, starting from 1, capped at min(kMaxLen, n - i), ending once the cap is reached: lengths strictly increase.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TM_LZ_HD __host__ __device__
#else
#define TM_LZ_HD
#endif

namespace tmx {
namespace lzm {

constexpr uint32_t kDict = 1u << 22;  // the furthest a match may lie
constexpr int kDepth = 96;            // chain candidates visited per position
constexpr int kMaxLen = 273;          // the format's longest match
constexpr int kMaxPairs = 1 + 1 + kDepth;  // c2, c3 and a record per chain step
constexpr int kBits2 = 16, kBits3 = 16, kBits4 = 20;  // widths of the three keys

// One entry of a list; a table of lists is CSR: counts (uint8) per position, the pairs of all positions in a row.
struct Pair {
  uint16_t len;
  uint16_t zero;  // (padding, written as 0 so that tables compare as bytes)
  uint32_t dist;  // distance - 1, as the coder emits it
};
static_assert(sizeof(Pair) == 8, "tm_lz_pair of include/tilemotion.h");

TM_LZ_HD inline uint32_t key2(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
TM_LZ_HD inline uint32_t h3(const uint8_t *p) { return (uint32_t)(((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) * 2654435761u) >> 16; }
TM_LZ_HD inline uint32_t h4(const uint8_t *p) {
  return (uint32_t)(((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)) * 2654435761u) >> 12;
}
TM_LZ_HD inline uint32_t max_len_at(size_t n, size_t i) { return n - i < (size_t)kMaxLen ? (uint32_t)(n - i) : (uint32_t)kMaxLen; }

// Where a position's lists come from, as the parser sees it (tm_lzma.hip).  Positions are asked for in ascending order; the last one may be
// asked for again.
class MatchSource {
 public:
  virtual ~MatchSource() {}
  virtual int find(size_t i, uint32_t *lens, uint32_t *dists) = 0;  // fills (length, distance - 1) pairs, returns their number
};

// A precomputed table handed over whole: counts[n], pairs in position order.
class TableSource : public MatchSource {
 public:
  TableSource(const uint8_t *counts, const Pair *pairs) : counts_(counts), pairs_(pairs) {}
  int find(size_t i, uint32_t *lens, uint32_t *dists) override {
    while (at_ < i) off_ += counts_[at_++];  // (ascending: the offset is a running sum)
    const int np = counts_[i];
    const Pair *p = pairs_ + off_;
    for (int q = 0; q < np; q++) { lens[q] = p[q].len; dists[q] = p[q].dist; }
    return np;
  }

 private:
  const uint8_t *counts_;
  const Pair *pairs_;
  size_t at_ = 0, off_ = 0;  // off_ = pairs before position at_
};

}  // namespace lzm

// tm_lzma.hip: the coder on a source of lists (nullptr: its own incremental finder); appends the 13 header bytes and the stream to dst
void lz_compress_from(const uint8_t *src, size_t n, lzm::MatchSource *source, std::vector<uint8_t> &dst);
// tm_lzma.hip: the incremental finder's lists of positions [first, first + count); pairs appended, counts[count] filled
void lz_matches_host(const uint8_t *src, size_t n, size_t first, size_t count, uint8_t *counts, std::vector<lzm::Pair> &pairs);

// tm_lz_matches.hip: independent streams coded side by side (the key frames of a .gtm).  `threads` parser threads, at most 16 and at most
// one per job.  Host finder: every thread codes whole streams with the coder's own finder, the caller among them (one thread: the caller
// alone, no thread is made).  Device finder: the caller is the only thread that touches the device -- it uploads a stream, sorts, and
// finds window after window, handing each stream's windows to its parser thread through a queue two windows deep.
struct LzJob {
  const uint8_t *src = nullptr;
  size_t n = 0;
  std::vector<uint8_t> out;  // the 13 header bytes and the stream
  double parse_ms = 0;
};
struct LzJobsReport { int threads = 0; double finder_ms = 0, parse_ms = 0; };
int lz_compress_jobs(std::vector<LzJob> &jobs, int threads, bool device_finder, void *hip_stream, LzJobsReport *report);

}  // namespace tmx
