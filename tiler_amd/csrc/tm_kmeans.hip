// tm_kmeans.hip -- the build's deterministic k-means, A9/A10 (replaces BICO.dll + ANN.dll + yakmo.dll; the DLLs'
// RNG/tie behaviour is not recoverable, SURVEY.md section 8c, so the algorithm below IS the specification and the
// oracle (oracle/tm_oracle.c: tmo_kmeans_i32) states the same thing for the CPU):
//   * points are int32 vectors with uint32 weights, grouped in contiguous segments (one independent problem each);
//   * init = farthest-first from the segment's first point, exact int64 distances, ties -> lowest index
//     (cf. TKModes.InitFarthestFirst, kmodes.pas:694); stops early when no distinct point is left;
//   * Lloyd: distance = sum over dimensions in order of (p - c)^2 in IEEE double (no FMA), ties -> lowest centroid;
//     centroid = exact integer weighted sum / weight (one IEEE division); empty clusters keep their centroid;
//     stop when no assignment changes or after max_iter (cYakmoMaxIterations = 300, utils.pas:17).
// Integer sums are order independent, so the parallel reduction is bit-reproducible.
//
// Callers: tm_stage_kmeans (one segment), run_palettize (DoPalettization, tilingencoder.pas:4105-4245, D = 192) and
// run_quantize_palettes (QuantizeUsingYakmo + DoQuantization, 4434-4564, D = 3, one segment per palette, run on the
// (G,R,B)-sorted colour histogram of each palette's pixels).
// The D = 192 kernels are in tm_kmeans_assign192.hip, tm_kmeans_skip.hip and tm_kmeans_resident.hip (their own rules: tm_kmeans_tile.h), the resident
// D = 3 clustering in tm_kmeans_pixel.hip, PreparePalettes' use of all of it in tm_palettize.hip; tm_kmeans.h is what all of them share.
#include <type_traits>
#include <chrono>
#include <cstdlib>

#include "tm_kmeans.h"

namespace tmx {

// One resident launch at a time per process: the resident kernels (k_h_resident, k_kmeans3_persistent) need all their workgroups on the chip
// together, and two of them started from two host threads could each be dealt part of the CUs and wait for the rest for ever (until their
// barriers give up).  Held from the launch to the read-back that ends it.  (Two PROCESSES on one device are not covered: there the barrier's
// time limit and the launches-per-iteration path are the answer -- a development set-up, one process per device is the deployment.)
// Keyed by device: a device group's shards on different devices run their replicated clusterings at the same time, shards on one device
// take turns.
static std::mutex g_resident_launch_dev[64];
std::mutex &resident_launch_lock() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return g_resident_launch_dev[dev & 63];
}

// ---- farthest-first ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_ff_update(const int32_t *__restrict__ pts, Seg *__restrict__ segs, int k,
                                                   long long *__restrict__ mind, BestKey *__restrict__ partial) {
  __shared__ BestKey s_best[4];
  int bx, nbx;
  const int seg = find_seg(segs, bx, nbx);
  if (nbx <= 0) return;  // only when every segment is empty
  const Seg sg = segs[seg];
  BestKey mine{0, LLONG_MIN};
  if (!sg.init_done && sg.kk <= k) {
    int32_t c[D];
#pragma unroll
    for (int j = 0; j < D; j++) c[j] = pts[sg.cur * D + j];  // wave-uniform: scalar loads
    for (int64_t i = bx * 256 + threadIdx.x; i < sg.count; i += (int64_t)nbx * 256) {
      const int32_t *p = pts + (sg.begin + i) * D;
      long long d = 0;
#pragma unroll
      for (int j = 0; j < D; j++) { const long long t = (long long)p[j] - c[j]; d += t * t; }
      long long m = mind[sg.begin + i];
      if (d < m) { m = d; mind[sg.begin + i] = m; }
      const BestKey cand{m, -(long long)i};
      if (better(cand, mine)) mine = cand;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    BestKey other{__shfl_xor(mine.dist, o), __shfl_xor(mine.negidx, o)};
    if (better(other, mine)) mine = other;
  }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++)
      if (better(s_best[w], mine)) mine = s_best[w];
    partial[blockIdx.x] = mine;
  }
}

// D=192 variant: the centre row does not fit registers as scalars cheaply; read it through LDS.
__global__ __launch_bounds__(256) void k_ff_update_wide(const int32_t *__restrict__ pts, int d, Seg *__restrict__ segs, int k,
                                                        long long *__restrict__ mind, BestKey *__restrict__ partial) {
  __shared__ BestKey s_best[4];
  __shared__ int32_t s_c[256];
  int bx, nbx;
  const int seg = find_seg(segs, bx, nbx);
  if (nbx <= 0) return;  // only when every segment is empty
  const Seg sg = segs[seg];
  BestKey mine{0, LLONG_MIN};
  const bool active = !sg.init_done && sg.kk <= k;
  if (active)
    for (int j = threadIdx.x; j < d; j += 256) s_c[j] = pts[sg.cur * d + j];
  __syncthreads();
  if (active) {
    for (int64_t i = bx * 256 + threadIdx.x; i < sg.count; i += (int64_t)nbx * 256) {
      const int4 *p = reinterpret_cast<const int4 *>(pts + (sg.begin + i) * d);
      long long dd = 0;
      for (int j = 0; j < d / 4; j++) {
        const int4 v = p[j];
        const long long t0 = (long long)v.x - s_c[4 * j], t1 = (long long)v.y - s_c[4 * j + 1];
        const long long t2 = (long long)v.z - s_c[4 * j + 2], t3 = (long long)v.w - s_c[4 * j + 3];
        dd += t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3;
      }
      long long m = mind[sg.begin + i];
      if (dd < m) { m = dd; mind[sg.begin + i] = m; }
      const BestKey cand{m, -(long long)i};
      if (better(cand, mine)) mine = cand;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    BestKey other{__shfl_xor(mine.dist, o), __shfl_xor(mine.negidx, o)};
    if (better(other, mine)) mine = other;
  }
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++)
      if (better(s_best[w], mine)) mine = s_best[w];
    partial[blockIdx.x] = mine;
  }
}

// one thread per segment: fold block partials, append the next centre (or finish)
// one workgroup per segment: the blocks' partial bests are reduced by 256 threads (`better` is a total order, so the reduction tree
// gives the same winner as a serial scan), then the picked point becomes the next centre
__global__ __launch_bounds__(256) void k_ff_pick(Seg *__restrict__ segs, int nseg, int k, const BestKey *__restrict__ partial, int nblk,
                                                 const int32_t *__restrict__ pts, int d, double *__restrict__ cent) {
  __shared__ BestKey s_best[256];
  __shared__ int64_t s_cur;
  const int seg = blockIdx.x, tid = threadIdx.x;
  if (seg >= nseg) return;
  Seg sg = segs[seg];
  if (sg.init_done) return;  // uniform over the workgroup
  BestKey best{0, LLONG_MIN};
  for (int b = sg.blk_first + tid; b < sg.blk_first + sg.blk_count; b += 256) {
    const BestKey c = partial[b];
    if (better(c, best)) best = c;
  }
  s_best[tid] = best;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o && better(s_best[tid + o], s_best[tid])) s_best[tid] = s_best[tid + o];
    __syncthreads();
  }
  best = s_best[0];
  const bool done = sg.kk >= k || best.dist <= 0;  // enough centres, or no distinct point left
  if (tid == 0) s_cur = done ? -1 : sg.begin + (-best.negidx);
  __syncthreads();
  if (!done) {
    const int64_t cur = s_cur;
    for (int j = tid; j < d; j += 256) cent[((int64_t)seg * k + sg.kk) * d + j] = (double)pts[cur * d + j];
  }
  if (tid == 0) {
    if (done) sg.init_done = 1;
    else { sg.cur = s_cur; sg.kk++; }
    segs[seg] = sg;
  }
}

__global__ void k_ff_first(Seg *__restrict__ segs, int nseg, int k, const int32_t *__restrict__ pts, int d, double *__restrict__ cent) {
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= nseg) return;
  Seg sg = segs[seg];
  sg.kk = 0;
  sg.init_done = 0;
  sg.changed = 0;
  if (sg.count <= 0 || k <= 0) {
    sg.init_done = 1;
  } else {
    sg.cur = sg.begin;
    for (int j = 0; j < d; j++) cent[((int64_t)seg * k) * d + j] = (double)pts[sg.cur * d + j];
    sg.kk = 1;
  }
  segs[seg] = sg;
}




// Assignment step for D = 3 (pixel colours; D = 192 has its own kernel, k_assign192): points are read directly and, with
// FUSE_ACC, the exact integer sums of the new assignment are accumulated in LDS in the same pass.
template <int D, bool FUSE_ACC>
__global__ __launch_bounds__(256) void k_assign(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w, Seg *__restrict__ segs,
                                                int k, const double *__restrict__ cent, int32_t *__restrict__ assign,
                                                u64 *__restrict__ sums, u64 *__restrict__ cnts, const int *__restrict__ quiet) {
  if (*quiet >= 0) return;  // converged earlier in this batch of launches (the host polls every few iterations)
  extern __shared__ double s_dyn[];
  // [KCH][3] centroid chunk (double) | [NCOPY][kk][4] u64 partial sums (FUSE_ACC)
  static_assert(D == 3, "k_assign is the pixel kernel");
  double *s_cent = s_dyn;
  u64 *s_acc = reinterpret_cast<u64 *>(s_dyn + KCH * D);
  int bx, nbx;
  const int seg = find_seg(segs, bx, nbx);
  if (nbx <= 0) return;  // only when every segment is empty
  const Seg sg = segs[seg];
  const int kk = sg.kk;
  int changed = 0;
  constexpr int NCOPY = 16;  // private copies of the LDS sums (lane & 15): same-cluster lanes no longer serialise on one word
  if (FUSE_ACC) {
    for (int e = threadIdx.x; e < NCOPY * kk * (D + 1); e += 256) s_acc[e] = 0;
  }
  const int64_t iters = (sg.count + (int64_t)nbx * 256 - 1) / ((int64_t)nbx * 256);
  const bool cent_resident = D == 3 && kk <= KCH;  // the usual palette size: the centroids are staged once, not once per 256 points
  if (cent_resident) {
    for (int e = threadIdx.x; e < kk * D; e += 256) s_cent[e] = cent[((int64_t)seg * k) * D + e];
    __syncthreads();
  }
  // the next point's loads are issued before the current one is scored (each thread walks ~9 points; without this every step
  // waits out a full memory round trip)
  int32_t n3[3] = {0, 0, 0};
  long long nwi = 1;
  int nold = -1;
  bool nvalid = false;
  auto fetch = [&](int64_t it) {
    const int64_t i = (it * nbx + bx) * 256 + threadIdx.x;
    nvalid = it < iters && i < sg.count;
    if (nvalid) {
      n3[0] = pts[(sg.begin + i) * 3]; n3[1] = pts[(sg.begin + i) * 3 + 1]; n3[2] = pts[(sg.begin + i) * 3 + 2];
      nwi = w ? (long long)w[sg.begin + i] : 1;
      nold = assign[sg.begin + i];
    }
  };
  fetch(0);
  for (int64_t it = 0; it < iters; it++) {
    const int64_t base = (it * nbx + bx) * 256;
    const int64_t i = base + threadIdx.x;
    const bool valid = nvalid;
    const int32_t p3[3] = {n3[0], n3[1], n3[2]};
    const long long cur_w = nwi;
    const int cur_old = nold;
    fetch(it + 1);
    double bd = 0.0;
    int bc = -1;
    for (int c0 = 0; c0 < kk; c0 += KCH) {
      const int nc = min(KCH, kk - c0);
      double s[KCH];
#pragma unroll
      for (int c = 0; c < KCH; c++) s[c] = 0.0;
      if (D == 3) {
        if (!cent_resident) {
          __syncthreads();
          for (int e = threadIdx.x; e < nc * D; e += 256) s_cent[e] = cent[((int64_t)seg * k + c0) * D + e];
          __syncthreads();
        }
        if (valid) {
          if (nc == KCH) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
              const double pj = (double)p3[j];
#pragma unroll
              for (int c = 0; c < KCH; c++) { const double t = __dsub_rn(pj, s_cent[c * 3 + j]); s[c] = __fma_rn(t, t, s[c]); }
            }
          } else {
            for (int j = 0; j < 3; j++) {
              const double pj = (double)p3[j];
              for (int c = 0; c < nc; c++) { const double t = __dsub_rn(pj, s_cent[c * 3 + j]); s[c] = __fma_rn(t, t, s[c]); }
            }
          }
        }
      }
      if (valid) {
        if (nc == KCH) {
#pragma unroll
          for (int c = 0; c < KCH; c++)
            if (bc < 0 || s[c] < bd) { bd = s[c]; bc = c0 + c; }
        } else {
          for (int c = 0; c < nc; c++)
            if (bc < 0 || s[c] < bd) { bd = s[c]; bc = c0 + c; }
        }
      }
    }
    if (valid) {
      if (cur_old != bc) { assign[sg.begin + i] = bc; changed++; }
      if (FUSE_ACC && cur_old != bc) {
        // The exact integer sums are carried from iteration to iteration, as in k_assign192: only a point that changes cluster touches
        // them -- its weighted row is added to the new cluster and subtracted from the old one (u64 arithmetic: exact, order-free).
        // After the first few iterations almost no point moves, and the LDS atomics, which bounded this kernel, are gone.
        const long long wi = cur_w;
        u64 *acc = s_acc + ((threadIdx.x & (NCOPY - 1)) * kk + bc) * (D + 1);
        atomicAdd(&acc[D], (u64)wi);
#pragma unroll
        for (int j = 0; j < 3; j++) atomicAdd(&acc[j], (u64)(wi * p3[j]));
        if (cur_old >= 0) {
          u64 *old = s_acc + ((threadIdx.x & (NCOPY - 1)) * kk + cur_old) * (D + 1);
          atomicAdd(&old[D], (u64)0 - (u64)wi);
#pragma unroll
          for (int j = 0; j < 3; j++) atomicAdd(&old[j], (u64)0 - (u64)(wi * p3[j]));
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o);
  if ((threadIdx.x & 63) == 0 && changed) atomicAdd(&segs[seg].changed, changed);
  if (FUSE_ACC) {
    __syncthreads();
    for (int e = threadIdx.x; e < kk * (D + 1); e += 256) {
      u64 v = 0;
#pragma unroll
      for (int cp = 0; cp < NCOPY; cp++) v += s_acc[cp * kk * (D + 1) + e];
      if (v == 0) continue;
      const int c = e / (D + 1), j = e - c * (D + 1);
      if (j == D) atomicAdd(&cnts[(int64_t)seg * k + c], v);
      else atomicAdd(&sums[((int64_t)seg * k + c) * D + j], v);
    }
  }
}

// exact integer weighted sums: LDS partials per workgroup for up to KCH_ACC clusters x D, flushed with global atomics
template <int D>
__global__ __launch_bounds__(256) void k_accumulate(const int32_t *__restrict__ pts, const uint32_t *__restrict__ w,
                                                    const Seg *__restrict__ segs, int k, const int32_t *__restrict__ assign,
                                                    u64 *__restrict__ sums, u64 *__restrict__ cnts, const int *__restrict__ quiet) {
  if (*quiet >= 0) return;
  extern __shared__ u64 s_acc[];  // [kk][D+1] when it fits, else straight to global
  int bx, nbx;
  const int seg = find_seg(segs, bx, nbx);
  if (nbx <= 0) return;  // only when every segment is empty
  const Seg sg = segs[seg];
  const int kk = sg.kk;
  const bool use_lds = (size_t)kk * (D + 1) * 8 <= 64 * 1024;
  if (use_lds) {
    for (int e = threadIdx.x; e < kk * (D + 1); e += 256) s_acc[e] = 0;
    __syncthreads();
  }
  for (int64_t i = bx * 256 + threadIdx.x; i < sg.count; i += (int64_t)nbx * 256) {
    const int c = assign[sg.begin + i];
    const long long wi = w ? (long long)w[sg.begin + i] : 1;
    const int32_t *p = pts + (sg.begin + i) * D;
    if (use_lds) {
      atomicAdd(&s_acc[c * (D + 1) + D], (u64)wi);
      for (int j = 0; j < D; j++) atomicAdd(&s_acc[c * (D + 1) + j], (u64)(wi * p[j]));
    } else {
      atomicAdd(&cnts[(int64_t)seg * k + c], (u64)wi);
      for (int j = 0; j < D; j++) atomicAdd(&sums[((int64_t)seg * k + c) * D + j], (u64)(wi * p[j]));
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int e = threadIdx.x; e < kk * (D + 1); e += 256) {
      const u64 v = s_acc[e];
      if (v == 0) continue;
      const int c = e / (D + 1), j = e - c * (D + 1);
      if (j == D) atomicAdd(&cnts[(int64_t)seg * k + c], v);
      else atomicAdd(&sums[((int64_t)seg * k + c) * D + j], v);
    }
  }
}

// One block: centroid = sum / weight where weight > 0 (segments that changed), reset sums/counts/changed, and latch the
// first iteration in which nothing changed anywhere (so the host can poll rarely).
__global__ __launch_bounds__(1024) void k_update_all(Seg *__restrict__ segs, int nseg, int k, int d, int carry, u64 *__restrict__ sums,
                                                     u64 *__restrict__ cnts, double *__restrict__ cent, int it,
                                                     int *__restrict__ quiet_iter, int *host_quiet = nullptr /* page-locked host word that gets the flag too */) {
  if (*quiet_iter >= 0) return;
  __shared__ int s_any;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  // carry: the assignment kernels (k_assign192, fused k_assign<3>) keep the sums current with +/- deltas; the unfused D = 3 path rebuilds them
  const int64_t total = (int64_t)nseg * k * d;
  for (int64_t e = threadIdx.x; e < total; e += 1024) {
    const int64_t sc = e / d;
    const int seg = (int)(sc / k);
    const u64 cn = cnts[sc];
    if (segs[seg].changed && cn > 0) cent[e] = __ddiv_rn((double)(long long)sums[e], (double)(long long)cn);
    if (!carry) sums[e] = 0;
  }
  __syncthreads();
  for (int seg = threadIdx.x; seg < nseg; seg += 1024) {
    if (segs[seg].changed) s_any = 1;
    segs[seg].changed = 0;
  }
  if (!carry)
    for (int64_t sc = threadIdx.x; sc < (int64_t)nseg * k; sc += 1024) cnts[sc] = 0;
  __syncthreads();
  if (threadIdx.x == 0 && s_any == 0 && *quiet_iter < 0) {
    *quiet_iter = it;
    if (host_quiet) __hip_atomic_store(host_quiet, it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- driver ----------------------------------------------------------------------------------------------------
// kmeans_batched (tm_kmeans.h) as a sequence of steps over one KmRun.
// the caller's own initial centres instead of the farthest-first picks: point indices (relative to the segment), -1 = none
__global__ void k_seed_centres(Seg *__restrict__ segs, int nseg, int k, const int32_t *__restrict__ pts, int d, const long long *__restrict__ idx, double *__restrict__ cent) {
  const int seg = blockIdx.x;
  if (seg >= nseg) return;
  Seg sg = segs[seg];
  int kk = 0;
  for (int c = 0; c < k; c++) {
    const long long i = idx[(int64_t)seg * k + c];
    if (i < 0 || i >= sg.count) continue;  // uniform over the workgroup
    for (int j = threadIdx.x; j < d; j += blockDim.x) cent[((int64_t)seg * k + kk) * d + j] = (double)pts[(sg.begin + i) * d + j];
    kk++;
  }
  __syncthreads();
  if (threadIdx.x == 0) { sg.kk = kk; sg.init_done = 1; sg.changed = 0; segs[seg] = sg; }
}

struct KmRun {  // one clustering from its seeds: what the steps below share
  TileRun t;    // the points, the outputs and the device state every launcher sees (the skipping iterations' own when `skipping`)
  int d, nseg;
  std::vector<Seg> hs;
  int nblk;     // workgroups of the 1-D grids over all segments
  bool skipping;
  DevBuf dsegs, mind, partial, sums, cnts, ptsc, quiet, look;
};

// the segments' table, zeroed sums, the initial centres (the caller's or farthest-first picks) and, for D = 192, what the tile kernels need
static int km_setup(KmRun &r, const std::vector<int64_t> &seg_begin, const std::vector<int64_t> &seg_count, const int64_t *init_idx, const long long *dev_init_idx) {
  TileRun &t = r.t;
  const int nseg = r.nseg, d = r.d, k = t.k;
  hipStream_t stream = t.stream;
  const bool seeded = init_idx != nullptr || dev_init_idx != nullptr;
  int64_t n = 0, maxcount = 0;
  for (int s = 0; s < nseg; s++) { n = std::max(n, seg_begin[s] + seg_count[s]); maxcount = std::max(maxcount, seg_count[s]); }
  t.n = n;
  std::vector<Seg> &hs = r.hs;
  hs.resize(nseg);
  for (int s = 0; s < nseg; s++) { memset(&hs[s], 0, sizeof(Seg)); hs[s].begin = seg_begin[s]; hs[s].count = seg_count[s]; }
  // workgroups are shared out in proportion to segment size (about 4 per CU in total), so a large palette does not
  // leave most of the chip idle while its few workgroups loop
  int64_t total_pts = 0;
  for (int s = 0; s < nseg; s++) total_pts += seg_count[s];
  constexpr int blk_target = 768;
  const int64_t rows_per_blk = std::max<int64_t>(256, (total_pts / blk_target + 255) / 256 * 256);
  int nblk = 0;
  for (int s = 0; s < nseg; s++) {
    hs[s].blk_first = nblk;
    hs[s].blk_count = (int)((seg_count[s] + rows_per_blk - 1) / rows_per_blk);
    nblk += hs[s].blk_count;
  }
  hs[0].nseg = nseg;
  r.nblk = nblk = std::max(nblk, 1);
  TM_TRY(r.dsegs.alloc(sizeof(Seg) * nseg));
  TM_TRY(r.mind.alloc(std::max<int64_t>(n, 1) * 8));
  TM_TRY(r.partial.alloc(sizeof(BestKey) * (size_t)nblk));
  TM_TRY(r.sums.alloc((size_t)nseg * k * d * 8));
  TM_TRY(r.cnts.alloc((size_t)nseg * k * 8));
  TM_HIP(hipMemcpyAsync(r.dsegs.p, hs.data(), sizeof(Seg) * nseg, hipMemcpyHostToDevice, stream));
  if (!seeded) TM_HIP(hipMemsetAsync(r.mind.p, 0x7f, std::max<int64_t>(n, 1) * 8, stream));  // 0x7f7f... ~ 9.2e18 > any distance (the farthest-first picks' running minima)
  TM_HIP(hipMemsetAsync(r.sums.p, 0, (size_t)nseg * k * d * 8, stream));
  TM_HIP(hipMemsetAsync(r.cnts.p, 0, (size_t)nseg * k * 8, stream));
  TM_HIP(hipMemsetAsync(t.assign, 0xff, std::max<int64_t>(n, 1) * 4, stream));
  TM_HIP(hipMemsetAsync(t.cent, 0, (size_t)nseg * k * d * 8, stream));
  Seg *ds = t.ds = r.dsegs.as<Seg>();
  t.sums = r.sums.as<u64>();
  t.cnts = r.cnts.as<u64>();
  const int32_t *pts = t.pts;
  DevBuf didx;
  if (dev_init_idx) {
    hipLaunchKernelGGL(k_seed_centres, dim3(nseg), dim3(64), 0, stream, ds, nseg, k, pts, d, dev_init_idx, t.cent);
  } else if (init_idx) {
    TM_TRY(didx.alloc((size_t)nseg * k * 8));
    TM_HIP(hipMemcpyAsync(didx.p, init_idx, (size_t)nseg * k * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_seed_centres, dim3(nseg), dim3(64), 0, stream, ds, nseg, k, pts, d, didx.as<long long>(), t.cent);
  } else
  hipLaunchKernelGGL(k_ff_first, dim3((nseg + 63) / 64), dim3(64), 0, stream, ds, nseg, k, pts, d, t.cent);
  for (int c = 1; c < k && !seeded; c++) {  // k-1 further picks (segments with no distinct point left latch init_done)
    if (d == 3)
      hipLaunchKernelGGL(k_ff_update<3>, dim3(nblk), dim3(256), 0, stream, pts, ds, k, r.mind.as<long long>(), r.partial.as<BestKey>());
    else
      hipLaunchKernelGGL(k_ff_update_wide, dim3(nblk), dim3(256), 0, stream, pts, d, ds, k, r.mind.as<long long>(), r.partial.as<BestKey>());
    hipLaunchKernelGGL(k_ff_pick, dim3(nseg), dim3(256), 0, stream, ds, nseg, k, r.partial.as<BestKey>(), nblk, pts, d, t.cent);
  }
  TM_HIP(hipGetLastError());
  if (d == 192) {
    TM_TRY(r.ptsc.alloc((size_t)std::max<int64_t>(n, 1) * 192 * 4));
    launch_chunk_major(pts, n, r.ptsc.as<int32_t>(), stream);
    t.ptsc = r.ptsc.as<int32_t>();
    t.a192 = assign192_shape(maxcount, nseg, k, cu_count());
  }
  TM_TRY(r.quiet.alloc(4));
  TM_HIP(hipMemsetAsync(r.quiet.p, 0xff, 4, stream));
  t.quiet = r.quiet.as<int>();
  TM_TRY(r.look.alloc(16));
  TM_HIP(hipMemsetAsync(r.look.p, 0, 16, stream));
  t.look = r.look.as<u64>();
  r.skipping = d == 192 && nseg == 1 && k <= H_MAXK;
  if (r.skipping) TM_TRY(tile_skip_setup(t));
  return TM_OK;
}

// One iteration per group of launches until the device's convergence flag is up or max_iter is reached.
// Convergence is a flag on the device; the launches after it return at once.  The host queues the iterations in batches and reads the
// flag of a batch while the NEXT batch runs (a copy into page-locked memory and an event behind every batch): the device never waits
// for the host to look, and at most two short batches of launches are wasted at the end.  (Batches of 16 with the stream drained at
// every poll left the device idle ~30 us six times per clustering and, on the bench clip, 42 no-op launches -- 0.45 ms -- behind the
// 87th iteration.)
// (the flag reaches the host in a page-locked word the update kernel itself writes: a 4-byte copy behind every batch was a launch of its own
// -- 75 of them per clustering on the literal bench clip)
static int km_launches(KmRun &r, int *iters) {
  TileRun &t = r.t;
  const int d = r.d, nseg = r.nseg, k = t.k, max_iter = t.max_iter, nblk = r.nblk;
  hipStream_t stream = t.stream;
  const size_t lds_assign = (size_t)KCH * 3 * 8 + (size_t)16 * k * 4 * 8;
  const size_t lds_acc = std::min<size_t>((size_t)k * (d + 1) * 8, 64 * 1024);
  const bool fuse3 = d == 3 && (size_t)16 * k * 4 * 8 <= 48 * 1024;
  int *pin = pinned_words();
  int *pin_dev = nullptr;
  if (pin && hipHostGetDevicePointer(reinterpret_cast<void **>(&pin_dev), pin, 0) != hipSuccess) { (void)hipGetLastError(); pin = nullptr; pin_dev = nullptr; }
  if (pin) __atomic_store_n(&pin[0], -1, __ATOMIC_RELEASE);
  const int poll_every = pin ? 4 : 16;
  hipEvent_t pev[2] = {nullptr, nullptr};
  struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_guard{pev};
  if (pin) {
    TM_HIP(hipEventCreateWithFlags(&pev[0], hipEventDisableTiming));
    TM_HIP(hipEventCreateWithFlags(&pev[1], hipEventDisableTiming));
  }
  int it = 0, issued = 0, nbatch = 0, qflag = -1;
  while (issued < max_iter) {
    const int batch = std::min(poll_every, max_iter - issued);
    for (int b = 0; b < batch; b++, issued++) {
      if (r.skipping) {
        tile_skip_iteration(t, issued, pin_dev);
        continue;
      }
      if (d == 3) {
        if (fuse3) {
          hipLaunchKernelGGL((k_assign<3, true>), dim3(nblk), dim3(256), lds_assign, stream, t.pts, t.w, t.ds, k, t.cent, t.assign, t.sums, t.cnts, t.quiet);
        } else {
          hipLaunchKernelGGL((k_assign<3, false>), dim3(nblk), dim3(256), lds_assign, stream, t.pts, t.w, t.ds, k, t.cent, t.assign, t.sums, t.cnts, t.quiet);
          hipLaunchKernelGGL(k_accumulate<3>, dim3(nblk), dim3(256), lds_acc, stream, t.pts, t.w, t.ds, k, t.assign, t.sums, t.cnts, t.quiet);
        }
      } else {
        launch_assign192(t.a192, nseg, stream, t.assign192_args());
      }
      hipLaunchKernelGGL(k_update_all, dim3(1), dim3(1024), 0, stream, t.ds, nseg, k, d, (d == 192 || fuse3) ? 1 : 0, t.sums, t.cnts, t.cent, issued, t.quiet, pin_dev);
    }
    if (!pin) {
      int q = -1;
      {
        HostRead hr_(stream);
        TM_TRY(hr_.get(&q, t.quiet, 4));
        TM_TRY(hr_.wait());
      }
      if (q >= 0) { it = q; qflag = q; break; }
      it = issued;
      continue;
    }
    TM_HIP(hipEventRecord(pev[nbatch & 1], stream));
    nbatch++;
    it = issued;
    if (nbatch >= 2) {  // the batch before the one just queued
      TM_HIP(hipEventSynchronize(pev[nbatch & 1]));
      qflag = __atomic_load_n(&pin[0], __ATOMIC_ACQUIRE);  // (written once: -1 until an update finds the clustering quiet)
      if (qflag >= 0) { it = qflag; break; }
    }
  }
  if (pin && qflag < 0 && nbatch >= 1) {  // the last batch queued
    TM_HIP(hipEventSynchronize(pev[(nbatch - 1) & 1]));
    qflag = __atomic_load_n(&pin[0], __ATOMIC_ACQUIRE);
    if (qflag >= 0) it = qflag;
  }
  *iters = it;
  return TM_OK;
}

int kmeans_batched(const int32_t *pts, const uint32_t *w, int d, const std::vector<int64_t> &seg_begin, const std::vector<int64_t> &seg_count, int k,
                   int max_iter, int32_t *assign, double *cent, std::vector<int> *host_kk, int *host_iters, hipStream_t stream, const int64_t *init_idx,
                   const long long *dev_init_idx, double *host_cent) {
  TM_CHECK(d == 3 || d == 192, TM_E_INVAL, "kmeans: only d = 3 (pixels) or 192 (tile features) are built");
  TM_CHECK(k >= 1 && k <= 65536, TM_E_INVAL, "kmeans: k out of range");
  const int nseg = (int)seg_begin.size();
  if (host_iters) *host_iters = 0;
  kmeans_run_stats().resident = 0;
  if (d == 192) kmeans_run_stats().look_scored = kmeans_run_stats().look_exact = 0;
  if (nseg == 0) return TM_OK;
  if (d == 3 && !init_idx && !dev_init_idx) {  // the whole clustering in one launch when its workgroups fit the chip together
    int used = 0;
    TM_TRY(kmeans3_persistent(pts, w, seg_begin, seg_count, k, max_iter, assign, cent, host_kk, host_iters, stream, &used, host_cent));
    if (used) { kmeans_run_stats().resident = 1; return TM_OK; }
  }
  for (bool allow_resident = true;; allow_resident = false) {  // a resident launch that gave up: once more, from the seeds, without it
    KmRun r;
    r.d = d; r.nseg = nseg;
    r.t.pts = pts; r.t.ptsc = nullptr; r.t.w = w; r.t.k = k; r.t.max_iter = max_iter; r.t.assign = assign; r.t.cent = cent; r.t.stream = stream;
    TM_TRY(km_setup(r, seg_begin, seg_count, init_idx, dev_init_idx));
    int it = 0;
    u64 look[2] = {0, 0};
    Resident leg = Resident::not_applicable;
    if (r.skipping && allow_resident && !knobs().km_launches && max_iter > H_WARM) {
      const ResidentPlan plan = resident_plan(r.t.n, k, cu_count());
      if (plan.rounds) TM_TRY(tile_resident(r.t, plan, &leg, &it, r.hs.data(), look));  // (r.skipping: one segment)
    }
    if (leg == Resident::gave_up) {
      fprintf(stderr, "[tm_kmeans] the resident tile k-means gave up at its barrier; repeating the clustering with one launch per step\n");
      continue;
    }
    if (leg == Resident::not_applicable) TM_TRY(km_launches(r, &it));
    else kmeans_run_stats().resident = 1;
    TM_HIP(hipGetLastError());
    if (host_iters) *host_iters = it;
    const bool have_state = leg == Resident::done;  // the resident leg's read-back brought the segment and the look's counters along
    if (!have_state || host_cent) {
      HostRead hr_(stream);
      if (!have_state) {
        TM_TRY(hr_.get(r.hs.data(), r.dsegs.p, sizeof(Seg) * nseg));
        TM_TRY(hr_.get(look, r.look.p, 16));
      }
      if (host_cent) TM_TRY(hr_.get(host_cent, cent, sizeof(double) * (size_t)nseg * k * d));
      TM_TRY(hr_.wait());
    }
    if (d == 192) {
      kmeans_run_stats().look_scored = (int64_t)look[0];
      kmeans_run_stats().look_exact = (int64_t)look[1];
    }
    if (host_kk) {
      host_kk->resize(nseg);
      for (int s = 0; s < nseg; s++) (*host_kk)[s] = r.hs[s].kk;
    }
    return TM_OK;
  }
}

int run_kmeans(const void *pts, const void *weights, int64_t n, int d, int k, int max_iter, void *assign, void *centroids, int *host_k,
               int *host_iters, hipStream_t stream) {
  return run_kmeans_seeded(pts, weights, n, d, k, nullptr, max_iter, assign, centroids, host_k, host_iters, stream);
}

int run_kmeans_seeded(const void *pts, const void *weights, int64_t n, int d, int k, const int64_t *host_init_idx, int max_iter, void *assign, void *centroids,
                      int *host_k, int *host_iters, hipStream_t stream) {
  TM_TRY(require_device());
  TM_CHECK(n >= 0, TM_E_INVAL, "kmeans: negative point count");
  if (host_k) *host_k = 0;
  if (host_iters) *host_iters = 0;
  if (n == 0) return TM_OK;
  std::vector<int64_t> b{0}, c{n};
  std::vector<int> kk;
  TM_TRY(kmeans_batched((const int32_t *)pts, (const uint32_t *)weights, d, b, c, k, max_iter, (int32_t *)assign, (double *)centroids,
                        &kk, host_iters, stream, host_init_idx));
  if (host_k) *host_k = kk[0];
  return TM_OK;
}

KmeansRunStats &kmeans_run_stats() {
  static thread_local KmeansRunStats st;
  return st;
}

}  // namespace tmx
