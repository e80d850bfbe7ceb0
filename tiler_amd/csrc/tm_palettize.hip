// tm_palettize.hip -- PreparePalettes on top of the build's k-means (tm_kmeans.hip): the D^2 seeding of the tile -> palette clustering,
// DoPalettization on one process (run_palettize) and over several (run_palettize_dist), QuantizeUsingYakmo + DoQuantization
// (run_quantize_palettes).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "tm_kmeans.h"

namespace tmx {

struct FfCandOut { long long *dist, *gidx; int32_t *row; };  // where a process writes its candidate (FfCand's fields)

// ---- the build's seeding of the tile -> palette clustering: D^2 sampling, deterministic ---------------------------------------
// k-means++-style seeding measured 0.1-0.7 dB (mean 0.5) above farthest-first on the bench clip with as many or fewer final tiles
// (profiles/r02_seeding_experiment*.json); the build makes it reproducible: a 64-bit LCG (Knuth's MMIX constants) from PP_SEED, pick t draws
// r = floor(x_t * total / 2^64) over the exact integer masses q_i = weight_i * (squared distance of point i to its nearest centre so
// far) (q_i = weight_i for the first pick) in 128-bit sums, and takes the first point whose running sum exceeds r; a total of 0 (no
// point apart from the centres) ends the seeding.  The oracle states the same rule (tmo_kmeans_pp_seeds).
// (Measured in round 3 and dropped: skipping the rows the triangle inequality rules out -- D(own centre, new centre)^2 >= 4 md, exact in
// integers -- took 0.07 ms off the sixteen passes: the pass is not bound by the rows' bytes.)
// Per pick: k_pp_mass (distances to the newest centre folded into the running minimum, masses, one 128-bit sum per 512 points) and
// k_pp_pick (the block holding r, then the point inside it).
typedef unsigned __int128 u128;
constexpr u64 PP_SEED = 0x42381337ull, PP_MUL = 6364136223846793005ull, PP_INC = 1442695040888963407ull;
constexpr int PP_BLOCK = 512;   // points per workgroup of k_pp_mass = per partial sum
struct PpState { u64 rng; int kk, done; long long pick; u64 tot_lo, tot_hi; };
struct PpSum { u64 lo, hi; };
__device__ __forceinline__ u128 pp_mass(const uint32_t *w, const long long *mind, int64_t i, int first) {
  return (u128)(w ? w[i] : 1u) * (u128)(first ? 1ull : (u64)mind[i]);
}
__device__ __forceinline__ u128 pp_draw(u64 x, u128 total) {  // floor(x * total / 2^64) < total
  return (u128)x * (u64)(total >> 64) + (((u128)x * (u64)total) >> 64);
}
// A point over 16 lanes (three 16-byte pieces each: a wave's load covers four whole rows); the squared distance is a sum of integers
// mod 2^64, so the lanes' partial sums add up to the value the in-order loop gives.  A thread per point, each striding through its own
// 768-byte row, measured 74 us per launch at 64 k points (192 us with smaller workgroups: every line fetched eight times over).
constexpr int PP_NT = PP_BLOCK;  // (1024 / 1024 and 256 / 256 measured 0.3 and 0.1 ms per clip slower)
__global__ __launch_bounds__(PP_NT) void k_pp_mass(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, int64_t n, const int32_t *__restrict__ cur_row,
                                                   const PpState *__restrict__ st, int first, long long *__restrict__ mind, PpSum *__restrict__ bsum) {
  __shared__ PpSum s_part[PP_NT / 64];
  const int tid = threadIdx.x, l = tid & 15, grp = tid >> 4;
  const bool update = !first && !st->done;
  u128 mine = 0;
  if (update) {
    int4 c[3];
#pragma unroll
    for (int q = 0; q < 3; q++) c[q] = reinterpret_cast<const int4 *>(cur_row)[l + 16 * q];
#pragma unroll 4
    for (int m = 0; m < PP_BLOCK / (PP_NT / 16); m++) {
      const int64_t i = (int64_t)blockIdx.x * PP_BLOCK + m * (PP_NT / 16) + grp;
      const bool valid = i < n;
      const int4 *p = reinterpret_cast<const int4 *>(pts + (valid ? i : 0) * 192);
      u64 dd = 0;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int4 v = p[l + 16 * q];
        const long long t0 = (long long)v.x - c[q].x, t1 = (long long)v.y - c[q].y, t2 = (long long)v.z - c[q].z, t3 = (long long)v.w - c[q].w;
        dd += (u64)(t0 * t0) + (u64)(t1 * t1) + (u64)(t2 * t2) + (u64)(t3 * t3);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) dd += __shfl_xor(dd, o);
      if (valid && l == 0) {
        long long md = mind[i];
        if ((long long)dd < md) { md = (long long)dd; mind[i] = md; }
        mine += (u128)(w ? w[i] : 1u) * (u128)(u64)md;
      }
    }
  } else {
    for (int m = 0; m < PP_BLOCK / PP_NT; m++) {
      const int64_t i = (int64_t)blockIdx.x * PP_BLOCK + m * PP_NT + tid;
      if (i < n) mine += pp_mass(w, mind, i, first);
    }
  }
  u64 lo = (u64)mine, hi = (u64)(mine >> 64);
  for (int o = 32; o > 0; o >>= 1) {
    const u128 other = ((u128)__shfl_xor(hi, o) << 64) | __shfl_xor(lo, o);
    const u128 sum = (((u128)hi << 64) | lo) + other;
    lo = (u64)sum; hi = (u64)(sum >> 64);
  }
  if ((tid & 63) == 0) s_part[tid >> 6] = PpSum{lo, hi};
  __syncthreads();
  if (tid == 0) {
    u128 t = 0;
    for (int wv = 0; wv < PP_NT / 64; wv++) t += ((u128)s_part[wv].hi << 64) | s_part[wv].lo;
    bsum[blockIdx.x] = PpSum{(u64)t, (u64)(t >> 64)};
  }
}
// inclusive prefix (128-bit) of one value per thread over a workgroup of 256, in thread order: shuffles inside the waves, the four wave
// totals through LDS; *total = the sum of all.  Every thread of the workgroup calls it.
__device__ __forceinline__ u128 pp_scan256(u128 v, PpSum *s_w, u128 *total) {
  u64 lo = (u64)v, hi = (u64)(v >> 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 olo = __shfl_up(lo, o), ohi = __shfl_up(hi, o);
    if (lane >= o) {
      const u128 s = (((u128)hi << 64) | lo) + (((u128)ohi << 64) | olo);
      lo = (u64)s; hi = (u64)(s >> 64);
    }
  }
  if (lane == 63) s_w[wave] = PpSum{lo, hi};
  __syncthreads();
  u128 before = 0, tot = 0;
#pragma unroll
  for (int wv = 0; wv < 4; wv++) {
    const u128 t = ((u128)s_w[wv].hi << 64) | s_w[wv].lo;
    if (wv < wave) before += t;
    tot += t;
  }
  *total = tot;
  __syncthreads();  // (s_w may be written again)
  return before + (((u128)hi << 64) | lo);
}
// the first thread (in thread order) whose flag is set, 256 if none: a ballot per wave, the four answers through LDS
__device__ __forceinline__ int pp_first256(bool flag, int *s_f) {
  const unsigned long long b = __builtin_amdgcn_ballot_w64(flag);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = b ? (int)(threadIdx.x & ~63u) + __builtin_ctzll(b) : 256;
  __syncthreads();
  const int f = min(min(s_f[0], s_f[1]), min(s_f[2], s_f[3]));
  __syncthreads();
  return f;
}

// One workgroup.  mode 0: the whole pick (single process): total, draw, block, point -> st->pick, cur_row, cent, seeds.
// mode 1 (several processes): only this process's total -> st->tot_*.  mode 2: the draw against the totals of all processes (rank
// order = global point order); the owner of r finds the point, everybody else reports no candidate.
// "The first point whose running sum exceeds r" is found with prefix sums over the workgroup instead of one thread walking 2 x 256
// partial sums (24 -> 9 us per pick: sixteen picks wait for it one after the other).
__global__ __launch_bounds__(256) void k_pp_pick(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, int64_t n, const long long *__restrict__ mind,
                                                 const PpSum *__restrict__ bsum, int nb, int first, int k, PpState *__restrict__ st, int mode,
                                                 const PpSum *__restrict__ totals, int rank, int world, long long global_begin,
                                                 int32_t *__restrict__ cur_row, double *__restrict__ cent, long long *__restrict__ seeds, FfCandOut cand) {
  __shared__ PpSum s_w[4];
  __shared__ int s_f[4];
  __shared__ long long s_pick;
  __shared__ u64 s_r[2];
  const int tid = threadIdx.x;
  if (st->done || st->kk >= k) {
    if (mode == 2 && cand.dist && tid == 0) { *cand.dist = -1; *cand.gidx = 0x7fffffffffffffffll; }
    return;
  }
  // the blocks' sums: thread t adds its share (consecutive blocks); their prefix over the workgroup
  const int per = (nb + 255) / 256;
  u128 part = 0;
  for (int b = tid * per; b < min(nb, (tid + 1) * per); b++) part += ((u128)bsum[b].hi << 64) | bsum[b].lo;
  u128 local = 0;
  const u128 incl = pp_scan256(part, s_w, &local);
  if (tid == 0) {
    s_pick = -1;  // -1: the point is another process's, -2: nothing left to pick, -3: ours
    if (mode == 1) { st->tot_lo = (u64)local; st->tot_hi = (u64)(local >> 64); }
    else {
      u128 total = local, before = 0;
      if (mode == 2) {
        total = 0;
        for (int r = 0; r < world; r++) {
          const u128 t = ((u128)totals[r].hi << 64) | totals[r].lo;
          if (r < rank) before += t;
          total += t;
        }
      }
      if (total == 0) { st->done = 1; s_pick = -2; }
      else {
        const u64 x = st->rng * PP_MUL + PP_INC;
        st->rng = x;
        const u128 r = pp_draw(x, total);
        if (r >= before && r < before + local) {  // the point is one of ours
          const u128 rl = r - before;
          s_r[0] = (u64)rl; s_r[1] = (u64)(rl >> 64);
          s_pick = -3;
        }
      }
    }
  }
  __syncthreads();
  if (mode == 1) return;
  long long blk = s_pick;
  if (blk == -2) {
    if (mode == 2 && cand.dist && tid == 0) { *cand.dist = -1; *cand.gidx = 0x7fffffffffffffffll; }
    return;
  }
  if (blk == -3) {  // (uniform) which thread's share of blocks, which block of it, which point of the block
    const u128 rl = ((u128)s_r[1] << 64) | s_r[0];
    const int ts = pp_first256(incl > rl, s_f);  // rl < local: there is one
    if (tid == ts) {
      u128 run = incl - part;
      int b = tid * per;
      for (; b < min(nb, (tid + 1) * per) - 1; b++) {
        const u128 v = ((u128)bsum[b].hi << 64) | bsum[b].lo;
        if (run + v > rl) break;
        run += v;
      }
      s_pick = b;
      const u128 rest = rl - run;
      s_r[0] = (u64)rest; s_r[1] = (u64)(rest >> 64);
    }
    __syncthreads();
    blk = s_pick;
    const u128 rest = ((u128)s_r[1] << 64) | s_r[0];
    // masses of the block's points in index order: thread t holds PP_BLOCK / 256 consecutive ones
    constexpr int E = PP_BLOCK / 256;
    u128 q[E], qs = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int64_t i = blk * PP_BLOCK + tid * E + e;
      q[e] = i < n ? pp_mass(w, mind, i, first) : (u128)0;
      qs += q[e];
    }
    u128 unused;
    const u128 qincl = pp_scan256(qs, s_w, &unused);
    const int tq = pp_first256(qincl > rest, s_f);
    if (tid == tq) {
      u128 run = qincl - qs;
      long long pick = -1;
#pragma unroll
      for (int e = 0; e < E; e++) {
        run += q[e];
        if (pick < 0 && run > rest) pick = blk * PP_BLOCK + tid * E + e;
      }
      s_pick = pick;
    }
    if (tq >= 256 && tid == 0) s_pick = -1;  // (cannot happen: rest < the block's sum)
    __syncthreads();
  }
  const long long pick = blk >= 0 ? s_pick : -1;  // (blk = -1: another process's)
  if (mode == 0) {
    if (pick >= 0) {
      const int kk = st->kk;
      for (int j = tid; j < 192; j += 256) { const int32_t v = pts[pick * 192 + j]; cur_row[j] = v; cent[(int64_t)kk * 192 + j] = (double)v; }
      __syncthreads();
      if (tid == 0) { seeds[kk] = pick; st->pick = pick; st->kk = kk + 1; }
    }
  } else {  // this process's candidate for the all-gather: the row of the picked point, or none
    if (tid == 0) { *cand.dist = pick >= 0 ? 1 : -1; *cand.gidx = pick >= 0 ? global_begin + pick : 0x7fffffffffffffffll; }
    if (tid < 192) cand.row[tid] = pick >= 0 ? pts[pick * 192 + tid] : 0;
  }
}

// ---- DoPalettization -------------------------------------------------------------------------------------------
__global__ void k_count_assign(const int32_t *__restrict__ assign, int64_t n, int k, u64 *__restrict__ cnt) {
  extern __shared__ unsigned int s_cnt[];  // per-workgroup histogram when k fits (a handful of hot global counters would serialise)
  const bool use_lds = k <= 8192;
  if (use_lds) {
    for (int e = threadIdx.x; e < k; e += blockDim.x) s_cnt[e] = 0;
    __syncthreads();
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (use_lds) atomicAdd(&s_cnt[assign[i]], 1u);
    else atomicAdd(&cnt[assign[i]], 1ull);
  }
  if (use_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < k; e += blockDim.x)
      if (s_cnt[e]) atomicAdd(&cnt[e], (u64)s_cnt[e]);
  }
}
__global__ void k_apply_lut(const int32_t *__restrict__ assign, int64_t n, const int32_t *__restrict__ lut, int32_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = lut[assign[i]];
}

// the ranking of up to RANK_DEV_MAX counts by one workgroup: lut[i] = the number of j with cnt[j] > cnt[i], or cnt[j] == cnt[i] and j < i --
// descending, ties in the initial order, which is the position a stable sort gives i
constexpr int RANK_DEV_MAX = 1024;
__global__ __launch_bounds__(RANK_DEV_MAX) void k_rank_counts(const u64 *__restrict__ cnt, int npal, int32_t *__restrict__ lut) {
  __shared__ u64 s_c[RANK_DEV_MAX];
  const int i = threadIdx.x;
  if (i < npal) s_c[i] = cnt[i];
  __syncthreads();
  if (i >= npal) return;
  const u64 c = s_c[i];
  int before = 0;
  for (int j = 0; j < npal; j++) {
    const u64 o = s_c[j];
    before += (o > c || (o == c && j < i)) ? 1 : 0;
  }
  lut[i] = before;
}

// palettes ranked by number of tiles (over all processes when `co` is given), descending (tilingencoder.pas:4229-4234); ties keep the initial order
static int rank_palettes(const int32_t *assign, int64_t n, int npal, const Collectives *co, int32_t *out_pal_idx, hipStream_t stream) {
  DevBuf cnt, lut;
  TM_TRY(cnt.alloc((size_t)npal * 8)); TM_TRY(lut.alloc((size_t)npal * 4));
  TM_HIP(hipMemsetAsync(cnt.p, 0, (size_t)npal * 8, stream));
  if (n > 0)
    hipLaunchKernelGGL(k_count_assign, dim3((int)std::min<int64_t>((n + 255) / 256, 512)), dim3(256), npal <= 8192 ? (size_t)npal * 4 : 0, stream, assign, n, npal, cnt.as<u64>());
  if (!co && npal <= RANK_DEV_MAX) {  // the host is not asked: no read, no upload, nothing to wait for (cnt and lut go back to the pool, stream-ordered)
    hipLaunchKernelGGL(k_rank_counts, dim3(1), dim3(RANK_DEV_MAX), 0, stream, cnt.as<u64>(), npal, lut.as<int32_t>());
    if (n > 0) hipLaunchKernelGGL(k_apply_lut, dim3((int)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, stream, assign, n, lut.as<int32_t>(), out_pal_idx);
    TM_HIP(hipGetLastError());
    return TM_OK;
  }
  if (co) {
    TM_HIP(hipGetLastError());
    TM_TRY(co->allreduce_sum_i64(cnt.p, npal));
  }
  std::vector<u64> hc(npal);
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(hc.data(), cnt.p, (size_t)npal * 8));
    TM_TRY(hr_.wait());
  }
  std::vector<int> ord(npal), hl(npal);
  for (int i = 0; i < npal; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return hc[a] > hc[b]; });
  for (int i = 0; i < npal; i++) hl[ord[i]] = i;
  TM_HIP(hipMemcpyAsync(lut.p, hl.data(), (size_t)npal * 4, hipMemcpyHostToDevice, stream));
  if (n > 0) hipLaunchKernelGGL(k_apply_lut, dim3((int)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, stream, assign, n, lut.as<int32_t>(), out_pal_idx);
  TM_HIP(hipGetLastError());
  TM_HIP(host_sync(stream));  // hl, the upload's source, is on this frame: the copy must have read it before the frame goes
  return TM_OK;
}

// the k seed points of one process's whole point set (indices, -1 beyond the centres found)
// out (host) and / or dev_out (the device buffer itself: k indices, -1 beyond the centres found); nothing is read back unless `out` is asked for
static int pp_seeds(const int32_t *pts, const uint32_t *w, int64_t n, int k, std::vector<int64_t> *out, hipStream_t stream, DevBuf *dev_out = nullptr) {
  DevBuf mind, bsum, state, cur_row, cent, seeds;
  const int nb = (int)((n + PP_BLOCK - 1) / PP_BLOCK);
  TM_TRY(mind.alloc((size_t)n * 8)); TM_TRY(bsum.alloc(sizeof(PpSum) * (size_t)nb)); TM_TRY(state.alloc(sizeof(PpState)));
  TM_TRY(cur_row.alloc(192 * 4)); TM_TRY(cent.alloc((size_t)k * 192 * 8)); TM_TRY(seeds.alloc((size_t)k * 8));
  TM_HIP(hipMemsetAsync(mind.p, 0x7f, (size_t)n * 8, stream));
  TM_HIP(hipMemsetAsync(seeds.p, 0xff, (size_t)k * 8, stream));
  PpState h0;
  memset(&h0, 0, sizeof(h0));
  h0.rng = PP_SEED;
  TM_HIP(hipMemcpyAsync(state.p, &h0, sizeof(h0), hipMemcpyHostToDevice, stream));
  for (int c = 0; c < k; c++) {
    hipLaunchKernelGGL(k_pp_mass, dim3(nb), dim3(PP_NT), 0, stream, pts, w, n, cur_row.as<int32_t>(), state.as<PpState>(), c == 0 ? 1 : 0, mind.as<long long>(), bsum.as<PpSum>());
    hipLaunchKernelGGL(k_pp_pick, dim3(1), dim3(256), 0, stream, pts, w, n, mind.as<long long>(), bsum.as<PpSum>(), nb, c == 0 ? 1 : 0, k, state.as<PpState>(), 0,
                       (const PpSum *)nullptr, 0, 1, 0ll, cur_row.as<int32_t>(), cent.as<double>(), seeds.as<long long>(), FfCandOut{nullptr, nullptr, nullptr});
  }
  TM_HIP(hipGetLastError());
  if (out) {
    out->assign((size_t)k, -1);
    HostRead hr_(stream);
    TM_TRY(hr_.get(out->data(), seeds.p, (size_t)k * 8));
    TM_TRY(hr_.wait());
  }
  if (dev_out) *dev_out = std::move(seeds);  // (the other buffers go back to the pool: what is queued on this stream after them is ordered behind their last use)
  return TM_OK;
}

int run_pp_seeds(const void *feat, const void *use, int64_t n, int k, int64_t *out_seeds_host, int *out_kk, hipStream_t stream) {
  TM_TRY(require_device());
  TM_CHECK(k >= 1 && k <= 65536, TM_E_INVAL, "PaletteCount %d outside 1..65536 (tilingencoder.pas:2959)", k);
  std::vector<int64_t> seeds((size_t)k, -1);
  if (n > 0) TM_TRY(pp_seeds((const int32_t *)feat, (const uint32_t *)use, n, k, &seeds, stream));
  int kk = 0;
  while (kk < k && seeds[kk] >= 0) kk++;
  std::copy(seeds.begin(), seeds.end(), out_seeds_host);
  *out_kk = kk;
  return TM_OK;
}

// would run_palettize put the clustering through the resident launch?  (one process per GPU: then every process clusters ALL global tiles
// itself -- 6 ms, no collective -- instead of a share of them with an all-reduce per Lloyd iteration)
bool palettize_resident(int64_t n, int npal) { return !knobs().km_launches && resident_plan(n, npal, cu_count()).rounds != 0; }

int run_palettize(const void *feat, const void *use, int64_t n, int npal, int max_iter, void *out_pal_idx, hipStream_t stream) {
  TM_TRY(require_device());
  TM_CHECK(npal >= 1 && npal <= 65536, TM_E_INVAL, "PaletteCount %d outside 1..65536 (tilingencoder.pas:2959)", npal);
  if (n <= 0) return TM_OK;
  DevBuf assign, cent;
  TM_TRY(assign.alloc(n * 4));
  TM_TRY(cent.alloc((size_t)npal * 192 * 8));
  int iters = 0;
  {
    DevBuf dseeds;  // the seeds never leave the device: no read-back, no drain of the stream, no upload between the seeding and the iterations
    TM_TRY(pp_seeds((const int32_t *)feat, (const uint32_t *)use, n, npal, nullptr, stream, &dseeds));
    std::vector<int64_t> b{0}, c{n};
    std::vector<int> kks;
    TM_TRY(kmeans_batched((const int32_t *)feat, (const uint32_t *)use, 192, b, c, npal, max_iter, assign.as<int32_t>(), cent.as<double>(), &kks, &iters, stream, nullptr,
                          dseeds.as<long long>()));
  }
  kmeans_run_stats().tile_iters = iters;
  kmeans_run_stats().tile_points = n;
  return rank_palettes(assign.as<int32_t>(), n, npal, nullptr, (int32_t *)out_pal_idx, stream);
}

// ---- DoPalettization over several processes ---------------------------------------------------------------------
struct FfCand { long long dist, gidx; int32_t row[192]; };  // one farthest-first candidate per process: largest min-distance, then lowest global index
struct FfState { int kk, done; };

// every process makes the same choice among the gathered candidates
__global__ __launch_bounds__(256) void k_ffd_pick(const FfCand *__restrict__ cands, int world, int k, FfState *__restrict__ st, int32_t *__restrict__ cur_row,
                                                  double *__restrict__ cent) {
  __shared__ int s_win;
  if (threadIdx.x == 0) {
    int win = -1;
    if (!st->done && st->kk < k)
      for (int r = 0; r < world; r++)
        if (cands[r].dist > 0 && (win < 0 || cands[r].dist > cands[win].dist || (cands[r].dist == cands[win].dist && cands[r].gidx < cands[win].gidx))) win = r;
    s_win = win;
    if (win < 0) st->done = 1;
  }
  __syncthreads();
  const int win = s_win;
  if (win < 0) return;
  const int kk = st->kk;
  if (threadIdx.x < 192) {
    cur_row[threadIdx.x] = cands[win].row[threadIdx.x];
    cent[(int64_t)kk * 192 + threadIdx.x] = (double)cands[win].row[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) st->kk = kk + 1;
}
__global__ void k_kmd_pack(const u64 *__restrict__ sums, const u64 *__restrict__ cnts, const Seg *__restrict__ segs, int k, u64 *__restrict__ red) {
  const int total = k * 192 + k + 1;  // sums | counts | number of points that changed cluster
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x)
    red[e] = e < k * 192 ? sums[e] : e < k * 192 + k ? cnts[e - k * 192] : (u64)(long long)segs[0].changed;
}
__global__ __launch_bounds__(1024) void k_kmd_update(const u64 *__restrict__ red, Seg *__restrict__ segs, int k, double *__restrict__ cent) {
  const bool changed = red[k * 192 + k] != 0;
  if (changed)
    for (int e = threadIdx.x; e < k * 192; e += 1024) {
      const u64 cn = red[k * 192 + e / 192];
      if (cn > 0) cent[e] = __ddiv_rn((double)(long long)red[e], (double)(long long)cn);
    }
  if (threadIdx.x == 0) segs[0].changed = 0;
}

int run_palettize_dist(const void *feat_local, const void *use_local, int64_t n, int64_t global_begin, int npal, int max_iter, void *out_pal_idx_local,
                       const Collectives &co, hipStream_t stream) {
  TM_TRY(require_device());
  TM_CHECK(npal >= 1 && npal <= 65536, TM_E_INVAL, "PaletteCount %d outside 1..65536 (tilingencoder.pas:2959)", npal);
  TM_CHECK(co.world >= 1 && co.call, TM_E_INVAL, "palettize: collectives missing");
  const int k = npal, d = 192;
  const int32_t *pts = (const int32_t *)feat_local;
  const uint32_t *w = (const uint32_t *)use_local;
  const int64_t n1 = std::max<int64_t>(n, 1);
  DevBuf dsegs, mind, partial, sums, cnts, cent, assign, cur_row, cand, cands, state, red, ptsc, quiet;
  Seg hs;
  memset(&hs, 0, sizeof(hs));
  hs.begin = 0; hs.count = n; hs.nseg = 1; hs.blk_first = 0; hs.blk_count = 1;
  const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
  TM_TRY(dsegs.alloc(sizeof(Seg))); TM_TRY(mind.alloc((size_t)n1 * 8)); TM_TRY(partial.alloc(sizeof(BestKey) * (size_t)nblk));
  TM_TRY(sums.alloc((size_t)k * d * 8)); TM_TRY(cnts.alloc((size_t)k * 8)); TM_TRY(cent.alloc((size_t)k * d * 8)); TM_TRY(assign.alloc((size_t)n1 * 4));
  TM_TRY(cur_row.alloc(192 * 4)); TM_TRY(cand.alloc(sizeof(FfCand))); TM_TRY(cands.alloc(sizeof(FfCand) * (size_t)co.world)); TM_TRY(state.alloc(sizeof(FfState)));
  TM_TRY(red.alloc((size_t)(k * d + k + 1) * 8)); TM_TRY(quiet.alloc(4));
  TM_HIP(hipMemsetAsync(mind.p, 0x7f, (size_t)n1 * 8, stream));
  TM_HIP(hipMemsetAsync(sums.p, 0, (size_t)k * d * 8, stream));
  TM_HIP(hipMemsetAsync(cnts.p, 0, (size_t)k * 8, stream));
  TM_HIP(hipMemsetAsync(cent.p, 0, (size_t)k * d * 8, stream));
  TM_HIP(hipMemsetAsync(assign.p, 0xff, (size_t)n1 * 4, stream));
  TM_HIP(hipMemsetAsync(state.p, 0, sizeof(FfState), stream));
  TM_HIP(hipMemsetAsync(quiet.p, 0xff, 4, stream));
  // D^2 seeding over all processes (k_pp_mass / k_pp_pick): every process keeps the same generator state; per pick the processes'
  // total masses are all-gathered (rank order = global point order), the owner of the draw finds the point, and the candidates
  // (one real, the others empty) are all-gathered like the farthest-first ones were
  FfState hst{0, 0};
  DevBuf ppstate, bsum, totals, mytot, ppseeds;
  const int nb = (int)std::max<int64_t>(1, (n + PP_BLOCK - 1) / PP_BLOCK);
  TM_TRY(ppstate.alloc(sizeof(PpState))); TM_TRY(bsum.alloc(sizeof(PpSum) * (size_t)nb)); TM_TRY(totals.alloc(sizeof(PpSum) * (size_t)co.world));
  TM_TRY(mytot.alloc(sizeof(PpSum))); TM_TRY(ppseeds.alloc((size_t)k * 8));
  {
    PpState h0;
    memset(&h0, 0, sizeof(h0));
    h0.rng = PP_SEED;
    TM_HIP(hipMemcpyAsync(ppstate.p, &h0, sizeof(h0), hipMemcpyHostToDevice, stream));
    TM_HIP(hipMemsetAsync(bsum.p, 0, sizeof(PpSum) * (size_t)nb, stream));
    TM_HIP(host_sync(stream));  // h0 is on the stack
  }
  FfCand *cd = cand.as<FfCand>();
  for (int c = 0; c < k; c++) {
    {
      const int first = c == 0 ? 1 : 0;
      if (n > 0)
        hipLaunchKernelGGL(k_pp_mass, dim3(nb), dim3(PP_NT), 0, stream, pts, w, n, cur_row.as<int32_t>(), ppstate.as<PpState>(), first, mind.as<long long>(), bsum.as<PpSum>());
      hipLaunchKernelGGL(k_pp_pick, dim3(1), dim3(256), 0, stream, pts, w, n, mind.as<long long>(), bsum.as<PpSum>(), n > 0 ? nb : 0, first, k, ppstate.as<PpState>(), 1,
                         (const PpSum *)nullptr, co.rank, co.world, (long long)global_begin, cur_row.as<int32_t>(), cent.as<double>(), ppseeds.as<long long>(),
                         FfCandOut{nullptr, nullptr, nullptr});
      TM_HIP(hipGetLastError());
      // tot_lo, tot_hi sit side by side in PpState: 16 bytes per process
      TM_TRY(co.allgather(reinterpret_cast<uint8_t *>(ppstate.p) + offsetof(PpState, tot_lo), totals.p, (int64_t)sizeof(PpSum)));
      hipLaunchKernelGGL(k_pp_pick, dim3(1), dim3(256), 0, stream, pts, w, n, mind.as<long long>(), bsum.as<PpSum>(), n > 0 ? nb : 0, first, k, ppstate.as<PpState>(), 2,
                         totals.as<PpSum>(), co.rank, co.world, (long long)global_begin, cur_row.as<int32_t>(), cent.as<double>(), ppseeds.as<long long>(),
                         FfCandOut{&cd->dist, &cd->gidx, cd->row});
    }
    TM_HIP(hipGetLastError());
    TM_TRY(co.allgather(cand.p, cands.p, (int64_t)sizeof(FfCand)));
    hipLaunchKernelGGL(k_ffd_pick, dim3(1), dim3(256), 0, stream, cands.as<FfCand>(), co.world, k, state.as<FfState>(), cur_row.as<int32_t>(), cent.as<double>());
    TM_HIP(hipGetLastError());
    if ((c & 3) == 3 || c == k - 1) {  // "no distinct point left" ends the picks early; looked at every few picks
      {
        HostRead hr_(stream);
        TM_TRY(hr_.get(&hst, state.p, sizeof(FfState)));
        TM_TRY(hr_.wait());
      }
      if (hst.done) break;
    }
  }
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(&hst, state.p, sizeof(FfState)));
    TM_TRY(hr_.wait());
  }
  hs.kk = hst.kk;
  hs.init_done = 1;
  TM_CHECK(hs.kk >= 1, TM_E_INVAL, "palettize: no point anywhere");
  TM_HIP(hipMemcpyAsync(dsegs.p, &hs, sizeof(Seg), hipMemcpyHostToDevice, stream));
  // Lloyd: local assignment (the sums of this process's points are carried with +/- deltas), all-reduce, identical update everywhere
  TM_TRY(ptsc.alloc((size_t)n1 * 192 * 4));
  if (n > 0) launch_chunk_major(pts, n, ptsc.as<int32_t>(), stream);
  const Assign192Shape a192 = assign192_shape(n1, 1, k, cu_count());
  for (int it = 0; it < max_iter; it++) {
    if (n > 0)
      launch_assign192(a192, 1, stream, {pts, ptsc.as<int32_t>(), n, w, dsegs.as<Seg>(), k, cent.as<double>(), assign.as<int32_t>(), sums.as<u64>(), cnts.as<u64>(), quiet.as<int>()});
    hipLaunchKernelGGL(k_kmd_pack, dim3(32), dim3(256), 0, stream, sums.as<u64>(), cnts.as<u64>(), dsegs.as<Seg>(), k, red.as<u64>());
    TM_HIP(hipGetLastError());
    TM_TRY(co.allreduce_sum_i64(red.p, (int64_t)k * d + k + 1));
    hipLaunchKernelGGL(k_kmd_update, dim3(1), dim3(1024), 0, stream, red.as<u64>(), dsegs.as<Seg>(), k, cent.as<double>());
    u64 changed = 0;
    {
      HostRead hr_(stream);
      TM_TRY(hr_.get(&changed, red.as<u64>() + (size_t)k * d + k, 8));
      TM_TRY(hr_.wait());
    }
    if (changed == 0) break;
  }
  return rank_palettes(assign.as<int32_t>(), n, npal, &co, (int32_t *)out_pal_idx_local, stream);
}

// ---- QuantizeUsingYakmo + DoQuantization -----------------------------------------------------------------------
// pixel key = palette << 24 | G << 16 | R << 8 | B  (CompareDSPixel: G, then R, then B; tilingencoder.pas:1046-1056)
#ifndef TM_PP_WIDE_KEYS
#define TM_PP_WIDE_KEYS 0  // 1 (tools/build_variant.sh NAME -DTM_PP_WIDE_KEYS=1): 64-bit keys at every PaletteCount, to measure the key width alone
#endif
// Key: uint32_t while the palette number fits the 8 bits above the colour (PaletteCount <= 256), else u64.  Every pass over the keys -- this
// kernel's writes, the sort's histogram and passes, the run lengths -- is bound by their bytes.  A palette number outside 0..npal-1 (negative
// ones included) raises *bad: a 32-bit key would carry it modulo 256.
template <class Key>
__global__ void k_pixel_keys(const uint32_t *__restrict__ tiles, const int32_t *__restrict__ pal_idx, int64_t n, int npal, Key *__restrict__ keys, int *__restrict__ bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n * 64; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t c = tiles[i];
    const uint32_t p = (uint32_t)pal_idx[i >> 6];
    if (p >= (uint32_t)npal) *bad = 1;
    keys[i] = (Key)((Key)p << 24) | (Key)(((c >> 8) & 0xff) << 16 | (c & 0xff) << 8 | ((c >> 16) & 0xff));
  }
}
// head[p] = first unique key whose palette field is >= p, for p = 0..npal (head[npal]: first >= npal); the number of unique keys is read
// from the device (the low word of head[npal + 1], where the run-length pass left it)
template <class Key>
__global__ void k_palette_bounds(const Key *__restrict__ ukeys, int npal, long long *__restrict__ head) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > npal) return;
  int64_t lo = 0, hi = (int64_t)*reinterpret_cast<const unsigned int *>(head + npal + 1);
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((long long)(ukeys[mid] >> 24) < (long long)p) lo = mid + 1; else hi = mid;
  }
  head[p] = lo;
}
// the unique keys as points (R, G, B) and, where Dither is to have them (wide != null), as the u64 list palette << 24 | colour it reads
template <class Key>
__global__ void k_unpack_colours(const Key *__restrict__ ukeys, int64_t nu, int32_t *__restrict__ pts, u64 *__restrict__ wide) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nu; i += (int64_t)gridDim.x * blockDim.x) {
    const Key kx = ukeys[i];
    pts[i * 3 + 0] = (int32_t)((kx >> 8) & 0xff);   // R
    pts[i * 3 + 1] = (int32_t)((kx >> 16) & 0xff);  // G
    pts[i * 3 + 2] = (int32_t)(kx & 0xff);          // B
    if (wide) wide[i] = (u64)kx;
  }
}

// The colour keys of all pixels, sorted and run-length-encoded, and the palettes' bounds in them: everything in front of the one read.
// head (device): lb[0..npal], then the number of unique keys and the bad-palette flag, a long long each.
struct ColourRuns { DevBuf ukeys, ucnt, head; };
template <class Key>
static int colour_runs(const uint32_t *tiles, const int32_t *pal_idx, int64_t n, int npal, int key_bits, hipStream_t stream, ColourRuns &r) {
  const int64_t npx = n * 64;
  DevBuf keys, keys2, tmp;  // (back to the pool at the return: what is queued on this stream after them is ordered behind their last use)
  TM_TRY(keys.alloc(npx * sizeof(Key))); TM_TRY(keys2.alloc(npx * sizeof(Key))); TM_TRY(r.ukeys.alloc(npx * sizeof(Key))); TM_TRY(r.ucnt.alloc(npx * 4));
  TM_TRY(r.head.alloc((size_t)(npal + 3) * 8));
  long long *head = r.head.as<long long>();
  TM_HIP(hipMemsetAsync(head + npal + 1, 0, 16, stream));
  hipLaunchKernelGGL(k_pixel_keys<Key>, dim3((int)std::min<int64_t>((npx + 255) / 256, 4096)), dim3(256), 0, stream, tiles, pal_idx, n, npal, keys.as<Key>(),
                     reinterpret_cast<int *>(head + npal + 2));
  TM_TRY(with_temp(tmp, "palettes: radix sort of the pixel keys", [&](void *t, size_t &b) {
    return rocprim::radix_sort_keys(t, b, keys.as<Key>(), keys2.as<Key>(), (size_t)npx, 0, key_bits, stream);
  }));
  TM_TRY(with_temp(tmp, "palettes: run lengths of the pixel keys", [&](void *t, size_t &b) {
    return rocprim::run_length_encode(t, b, keys2.as<Key>(), (unsigned int)npx, r.ukeys.as<Key>(), r.ucnt.as<uint32_t>(), reinterpret_cast<unsigned int *>(head + npal + 1), stream);
  }));
  hipLaunchKernelGGL(k_palette_bounds<Key>, dim3((npal + 1 + 63) / 64), dim3(64), 0, stream, r.ukeys.as<Key>(), npal, head);
  TM_HIP(hipGetLastError());
  return TM_OK;
}
template <class Key>
static void unpack_colours(const ColourRuns &r, int64_t nu, int32_t *pts, u64 *wide, hipStream_t stream) {
  hipLaunchKernelGGL(k_unpack_colours<Key>, dim3((int)std::min<int64_t>((nu + 255) / 256, 4096)), dim3(256), 0, stream, r.ukeys.as<Key>(), nu, pts, wide);
}

static int muldiv_win(int a, int b, int c) {  // Windows MulDiv: round half away from zero
  long long p = (long long)a * b, q = p >= 0 ? p : -p, cc = c >= 0 ? c : -c;
  long long r = (q + cc / 2) / cc;
  return (int)(((p < 0) != (c < 0)) ? -r : r);
}
static void rgb_to_hsv_bytes(int rr, int gg, int bb, int &h, int &s, int &v) {  // RGBToHSV, utils.pas:278-325
  int mx = std::max(rr, std::max(gg, bb)), mn = std::min(rr, std::min(gg, bb));
  int hh = 0, ss = 0, ll = mx;
  if (ll != mn) {
    const int delta = ll - mn;
    ss = muldiv_win(delta, 255, ll);
    if (rr == ll) hh = muldiv_win(42, gg - bb, delta);
    else if (gg == ll) hh = muldiv_win(42, bb - rr, delta) + 84;
    else if (bb == ll) hh = muldiv_win(42, rr - gg, delta) + 168;
    hh = hh % 252;
  }
  h = hh & 0xff; s = ss & 0xff; v = ll & 0xff;
}

int run_quantize_palettes(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter, void *out_palettes,
                          hipStream_t stream, DevBuf *keep_keys, int64_t *keep_n, int32_t *host_palettes) {
  return run_quantize_palettes_part(tiles, pal_idx, n, npal, pal_size, max_iter, out_palettes, 0, 1, stream, keep_keys, keep_n, host_palettes);
}

int run_quantize_palettes_part(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter, void *out_palettes,
                               int pal_rank, int pal_world, hipStream_t stream, DevBuf *keep_keys, int64_t *keep_n, int32_t *host_palettes) {
  TM_TRY(require_device());
  TM_CHECK(out_palettes || host_palettes, TM_E_INVAL, "quantize: no destination for the palettes");
  if (keep_n) *keep_n = 0;
  TM_CHECK(pal_world >= 1 && pal_rank >= 0 && pal_rank < pal_world, TM_E_INVAL, "quantize: bad palette share %d of %d", pal_rank, pal_world);
  TM_CHECK(npal >= 1 && npal <= 65536, TM_E_INVAL, "PaletteCount %d outside 1..65536", npal);
  TM_CHECK(pal_size >= 2 && pal_size <= 64, TM_E_INVAL, "PaletteSize %d outside 2..64 (tilingencoder.pas:2965)", pal_size);
  std::vector<int32_t> hpal((size_t)npal * pal_size, TM_NULL_COLOR);  // unused slots: cDitheringNullColor (4557-4558)
  if (n > 0) {
    const bool dbg = knobs().pp_debug;
    if (dbg) (void)hipStreamSynchronize(stream);
    const auto t_km = std::chrono::steady_clock::now();
    int key_bits = 25;  // 24 bits of colour + the palette number's: every 8 bits less is a pass over all pixels less
    while (key_bits < 41 && (1ll << (key_bits - 24)) < npal) key_bits++;
    const bool narrow = key_bits <= 32 && !TM_PP_WIDE_KEYS;  // PaletteCount <= 256: 32-bit keys
    ColourRuns runs;
    DevBuf pts, assign, cent, wide;
    TM_TRY(narrow ? colour_runs<uint32_t>((const uint32_t *)tiles, (const int32_t *)pal_idx, n, npal, key_bits, stream, runs)
                  : colour_runs<u64>((const uint32_t *)tiles, (const int32_t *)pal_idx, n, npal, key_bits, stream, runs));
    // the one read: the palettes' bounds in the unique keys, their number, and the flag of a palette number out of range
    std::vector<long long> lb((size_t)npal + 3);
    {
      HostRead hr_(stream);
      TM_TRY(hr_.get(lb.data(), runs.head.p, lb.size() * 8));
      TM_TRY(hr_.wait());
    }
    const unsigned int nu = (unsigned int)lb[(size_t)npal + 1];
    TM_CHECK(lb[(size_t)npal + 2] == 0 && lb[npal] == (long long)nu, TM_E_INVAL, "quantize: a tile names palette >= PaletteCount");
    std::vector<int64_t> sb(npal, 0), sc(npal, 0);
    for (int p = 0; p < npal; p++) { sb[p] = lb[p]; sc[p] = p % pal_world == pal_rank ? lb[p + 1] - lb[p] : 0; }  // other processes' palettes: empty segments
    TM_TRY(pts.alloc((size_t)std::max<unsigned>(nu, 1) * 12));
    TM_TRY(assign.alloc((size_t)std::max<unsigned>(nu, 1) * 4));
    TM_TRY(cent.alloc((size_t)npal * pal_size * 3 * 8));
    const bool keep = keep_keys && keep_n;
    if (narrow) {  // Dither reads u64 keys: the unpacking pass, which reads every unique key anyway, writes them out as such
      if (keep) TM_TRY(wide.alloc((size_t)std::max<unsigned>(nu, 1) * 8));
      unpack_colours<uint32_t>(runs, (int64_t)nu, pts.as<int32_t>(), keep ? wide.as<u64>() : nullptr, stream);
    } else {
      unpack_colours<u64>(runs, (int64_t)nu, pts.as<int32_t>(), nullptr, stream);
    }
    std::vector<int> kk;
    int iters = 0;
    const auto t_km0 = std::chrono::steady_clock::now();
    kmeans_run_stats().pixel_colour_iters = 0;
    std::vector<double> hc((size_t)npal * pal_size * 3);  // the centroids come to the host with the clustering's own read and stay here
    TM_TRY(kmeans_batched(pts.as<int32_t>(), runs.ucnt.as<uint32_t>(), 3, sb, sc, pal_size, max_iter, assign.as<int32_t>(), cent.as<double>(),
                          &kk, &iters, stream, nullptr, nullptr, hc.data()));
    kmeans_run_stats().pixel_iters = iters;  // (pixel_colour_iters: summed by the persistent launch, reset before it below)
    kmeans_run_stats().pixel_colours = (int64_t)nu;
    kmeans_run_stats().pixels = n * 64;
    if (dbg) fprintf(stderr, "[tm_pp]   colour keys + sort + runs %7.3f ms, k-means of %u colours %7.3f ms (%d iterations)\n",
                     std::chrono::duration<double, std::milli>(t_km0 - t_km).count() , nu,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_km0).count(), iters);
    // host tail (P x PaletteSize colours): Round, clamp, Posterize(.,255) = identity, sort by (Val, Sat, Hue)
    // -- tilingencoder.pas:4513-4558, utils.pas:526-534, 741-748
    struct Item { int v, s, h, r, g, b, idx; };
    for (int p = 0; p < npal; p++) {
      std::vector<Item> items;
      for (int i = 0; i < kk[p]; i++) {
        const double *c = &hc[((size_t)p * pal_size + i) * 3];
        Item it;
        it.r = (int)std::min<long long>(255, std::max<long long>(0, llrint(c[0])));
        it.g = (int)std::min<long long>(255, std::max<long long>(0, llrint(c[1])));
        it.b = (int)std::min<long long>(255, std::max<long long>(0, llrint(c[2])));
        it.idx = i;
        rgb_to_hsv_bytes(it.r, it.g, it.b, it.h, it.s, it.v);
        items.push_back(it);
      }
      std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) {
        if (a.v != b.v) return a.v < b.v;
        if (a.s != b.s) return a.s < b.s;
        if (a.h != b.h) return a.h < b.h;
        if (a.r != b.r) return a.r < b.r;
        if (a.g != b.g) return a.g < b.g;
        if (a.b != b.b) return a.b < b.b;
        return a.idx < b.idx;
      });
      for (size_t i = 0; i < items.size(); i++) hpal[(size_t)p * pal_size + i] = (items[i].b << 16) | (items[i].g << 8) | items[i].r;
    }
    if (keep) { *keep_keys = std::move(narrow ? wide : runs.ukeys); *keep_n = (int64_t)nu; }
  }
  if (pal_world > 1)
    for (int p = 0; p < npal; p++)
      if (p % pal_world != pal_rank)
        for (int i = 0; i < pal_size; i++) hpal[(size_t)p * pal_size + i] = 0;
  if (host_palettes) {  // the caller goes on with the palettes on the host: nothing to upload, nothing to wait for
    memcpy(host_palettes, hpal.data(), hpal.size() * 4);
    return TM_OK;
  }
  TM_HIP(hipMemcpyAsync(out_palettes, hpal.data(), hpal.size() * 4, hipMemcpyHostToDevice, stream));
  TM_HIP(host_sync(stream));  // hpal, the upload's source, is on this frame: the copy must have read it before the frame goes
  return TM_OK;
}

}  // namespace tmx
