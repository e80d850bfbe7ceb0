// tm_kmodes_init.hip -- k-modes, what runs before the iterations: the check of the values, GetMinMatchingDissim over a range of points,
// the farthest-first initialisation and the initial assignment with its tables and modes.  See tm_kmodes.hip for the map.
#include "tm_kmodes.h"

namespace tmx {
namespace {

__global__ void k_kmodes_validate(const uint8_t *__restrict__ rows, int64_t nbytes, int nmod, int *__restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * blockDim.x)
    if (rows[i] >= nmod) atomicExch(bad, 1);
}

// clust[i], dis[i] for points [first, n): the LAST mode reaching the minimum wins (kmodes.pas:272, 414)
__global__ __launch_bounds__(256) void k_kmodes_argmin(const uint32_t *__restrict__ rows, int64_t first, int64_t n, const uint32_t *__restrict__ modes, int k,
                                                       int32_t *__restrict__ clust, unsigned *__restrict__ dis) {
  extern __shared__ uint32_t s_modes[];  // [k][20]
  for (int e = threadIdx.x; e < k * KM_WORDS; e += 256) s_modes[e] = modes[e];
  __syncthreads();
  for (int64_t i = first + blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t p[KM_WORDS];
    km_load_row(p, rows, i);
    unsigned best = 0xffffffffu;
    int res = -1;
    for (int c = 0; c < k; c++) {
      const unsigned d = km_dissim(s_modes + c * KM_WORDS, p);
      if (d <= best) { best = d; res = c; }
    }
    clust[i] = res;
    dis[i] = best;
  }
}

// farthest-first: mind[i] = min(mind[i], dissim(centre, row i)) for unused points, then this block's candidate for the next pick:
// the LAST index among the unused points with the largest mind (kmodes.pas:757-762) -> key = mind << 32 | index, maximum
__global__ __launch_bounds__(256) void k_kmodes_ff(const uint32_t *__restrict__ rows, int64_t n, int64_t centre, const uint8_t *__restrict__ used,
                                                   unsigned *__restrict__ mind, u64 *__restrict__ partial) {
  __shared__ u64 s_best[4];
  uint32_t c[KM_WORDS];
  km_load_row(c, rows, centre);
  u64 best = 0;
  bool any = false;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (used[i] || i == centre) continue;
    const unsigned d = km_dissim(rows + i * KM_WORDS, c);
    unsigned m = mind[i];
    if (d < m) { m = d; mind[i] = m; }
    const u64 key = ((u64)m << 32) | (u64)(uint32_t)i;
    if (!any || key >= best) { best = key; any = true; }
  }
  u64 enc = any ? best + 1 : 0;  // 0 = no candidate; keys shifted by one so that (mind 0, index 0) is still a candidate
  for (int o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(enc, o); enc = other > enc ? other : enc; }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = enc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) enc = s_best[w] > enc ? s_best[w] : enc;
    partial[blockIdx.x] = enc;
  }
}

__global__ void k_kmodes_take_rows(const uint8_t *__restrict__ rows, const int64_t *__restrict__ which, int k, uint8_t *__restrict__ cent) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < k * KM_ATTRS; e += gridDim.x * blockDim.x) cent[e] = rows[which[e / KM_ATTRS] * KM_ATTRS + e % KM_ATTRS];
}

// initial membership = the first scores; member counts and histograms by integer atomics (order-free) -- kmodes.pas:978-996
__global__ void k_kmodes_init_tables(const uint8_t *__restrict__ rows, int64_t n, int nmod, KmState st) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * KM_ATTRS; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / KM_ATTRS;
    const int a = (int)(e - i * KM_ATTRS), c = st.clust[i];
    if (a == 0) { st.memb[i] = c; atomicAdd(&st.members[c], 1); }
    atomicAdd(&st.freq[((int64_t)c * KM_ATTRS + a) * nmod + rows[e]], 1);
  }
}

// the modes after the initial assignment (997-1011): an empty cluster takes, attribute by attribute, the value of a row drawn with
// RandInt -- clusters in order, attributes in order, one draw each: a single thread walks the LCG; the others' modes come from their histograms
__global__ __launch_bounds__(64) void k_kmodes_init_modes(const uint8_t *__restrict__ rows, int64_t n, int k, int nmod, KmState st) {
  const int lane = threadIdx.x;
  if (blockIdx.x == 0) {
    if (lane == 0) {
      uint32_t seed = *st.seed;
      for (int c = 0; c < k; c++)
        if (st.members[c] == 0)
          for (int a = 0; a < KM_ATTRS; a++) st.cent[c * KM_ATTRS + a] = rows[(int64_t)rand_int((uint32_t)n, seed) * KM_ATTRS + a];
      *st.seed = seed;
    }
    return;
  }
  for (int pr = blockIdx.x - 1; pr < k * KM_ATTRS; pr += gridDim.x - 1) {
    const int c = pr / KM_ATTRS;
    if (st.members[c] == 0) continue;
    int t[4];
    km_hist_load(t, st.freq, pr, nmod, lane);
    const int m = km_first_largest(t, nmod, lane);
    if (lane == 0) st.cent[pr] = (uint8_t)m;
  }
}

}  // namespace

int validate_values(const KmBuffers &b) {
  hipLaunchKernelGGL(k_kmodes_validate, dim3((unsigned)std::min<int64_t>((b.n * KM_ATTRS + 255) / 256, 4096)), dim3(256), 0, b.stream, b.rows, b.n * KM_ATTRS, b.nmod, b.st.bad);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// k_kmodes_argmin keeps all k modes in LDS
int score_prepare(int k) {
  const size_t lds = (size_t)k * KM_ATTRS;
  TM_CHECK(lds <= 160 * 1024 - 1024, TM_E_INVAL, "kmodes: the modes of %d clusters do not fit LDS", k);
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_kmodes_argmin), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return TM_OK;
}
int score(const KmBuffers &b, int64_t first, int64_t last) {
  hipLaunchKernelGGL(k_kmodes_argmin, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((last - first + 255) / 256, 2048))), dim3(256), (size_t)b.k * KM_ATTRS, b.stream,
                     reinterpret_cast<const uint32_t *>(b.rows), first, last, b.cent.as<uint32_t>(), b.k, b.st.clust, b.st.dis);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- InitFarthestFirst (694-772): the picks settle on the host from every block's candidate
int farthest_first(KmBuffers &b, int64_t start) {
  std::vector<u64> &partial = b.ff_partial_host;
  std::vector<int64_t> &which = b.which_host;
  TM_HIP(hipMemsetAsync(b.mind.p, 0xff, (size_t)b.n * 4, b.stream));
  TM_HIP(hipMemsetAsync(b.used.p, 0, (size_t)b.n, b.stream));
  int64_t far = start;
  for (int c = 0; c < b.k; c++) {
    which[(size_t)c] = far;
    TM_HIP(hipMemsetAsync(b.used.as<uint8_t>() + far, 1, 1, b.stream));
    if (c == b.k - 1) break;
    hipLaunchKernelGGL(k_kmodes_ff, dim3(b.ff_blocks), dim3(256), 0, b.stream, reinterpret_cast<const uint32_t *>(b.rows), b.n, far, b.used.as<uint8_t>(), b.mind.as<unsigned>(),
                       b.ff_partial.as<u64>());
    TM_HIP(hipGetLastError());
    TM_HIP(hipMemcpyAsync(partial.data(), b.ff_partial.p, (size_t)b.ff_blocks * 8, hipMemcpyDeviceToHost, b.stream));
    TM_HIP(hipStreamSynchronize(b.stream));
    u64 best = 0;
    for (u64 v : partial) best = std::max(best, v);
    far = best ? (int64_t)(uint32_t)(best - 1) : start;  // no unused point left: ifarthest stays InitPoint (756)
  }
  TM_HIP(hipMemcpyAsync(b.which.p, which.data(), (size_t)b.k * 8, hipMemcpyHostToDevice, b.stream));
  hipLaunchKernelGGL(k_kmodes_take_rows, dim3((unsigned)((b.k * KM_ATTRS + 255) / 256)), dim3(256), 0, b.stream, b.rows, b.which.as<int64_t>(), b.k, b.st.cent);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- initial assignment and modes (978-1011)
int initial_assignment(const KmBuffers &b) {
  TM_HIP(hipMemsetAsync(b.freq.p, 0, (size_t)b.k * KM_ATTRS * b.nmod * 4, b.stream));
  TM_HIP(hipMemsetAsync(b.members.p, 0, (size_t)b.k * 4, b.stream));
  TM_TRY(score(b, 0, b.n));
  hipLaunchKernelGGL(k_kmodes_init_tables, dim3((unsigned)std::min<int64_t>((b.n * KM_ATTRS + 255) / 256, 8192)), dim3(256), 0, b.stream, b.rows, b.n, b.nmod, b.st);
  hipLaunchKernelGGL(k_kmodes_init_modes, dim3((unsigned)std::min(b.k * KM_ATTRS, 2048) + 1), dim3(64), 0, b.stream, b.rows, b.n, b.k, b.nmod, b.st);
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(b.stream));  // b.which_host is host memory farthest_first's copy reads
  return TM_OK;
}

}  // namespace tmx
