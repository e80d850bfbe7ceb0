// tm_knn3_seed.h -- the first kernel of the third scan shape (tm_knn3.h): every query sub-tile against its group's seed window.
#pragma once
#include "tm_knn3_block.h"

namespace tmx {

// One workgroup (8 waves) per query group: wave w holds seed tile w in registers; the group's sub-tiles pass through LDS three at a time
// (double buffered, LDS-DMA), every wave scoring each against its tile.  Bests meet in LDS (64-bit atomic minimum per query) and leave as
// gbest / gsmax.  A wave keeps its tile's 32 original indices in LDS of its own for its whole life (s_tidx: plain stores before the first
// barrier).  ~61 KB of LDS: two workgroups per CU, 100 registers per wave.
constexpr int K3_SEED_SLICE = 3;
template <int HT, int HQ, bool TD, bool UNUSED>
__global__ __launch_bounds__(K3_SEEDS * 64, 4) void k_knn_seed(const Knn3Args a) {
  constexpr int KT = 6 + HT, KQ = 6 + HQ;
  constexpr int T_BYTES = knn_pack_bytes(KT, 1), Q_BYTES = knn_pack_bytes(KQ, 0);
  constexpr int SL = (2 * K3_SEED_SLICE * KQ * 1024 + 10 * 1024 > 80 * 1024) ? K3_SEED_SLICE - 1 : K3_SEED_SLICE, NW = K3_SEEDS;  // two workgroups per CU
  __shared__ __attribute__((aligned(16))) uint8_t s_q[2][SL * KQ * 1024];
  __shared__ unsigned long long s_best[16 * 32];
  __shared__ unsigned s_tidx[NW * 32];
  __shared__ int s_qn[16 * 32];
  __shared__ unsigned s_qm[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), half = lane >> 5;
  const int NS = a.ns;
  const int64_t g = blockIdx.x, st0 = g * NS;
  const int nvalid = (int)min((int64_t)NS, a.n_qtiles - st0);
  const K3SeedWindow seeds = k3_seed_window(a.qmeta[qmeta_at(st0, QMETA_HOME)], a.n_ttiles);
  const int r0a = seeds.first, n_seed = seeds.count;
  auto stage = [&](int slice, int buf) {  // the slice's query operands, SL * KQ pieces of 1 KB over the waves
    for (int piece = wave; piece < SL * KQ; piece += NW) {
      const int s = piece / KQ, kc = piece - s * KQ;
      const int64_t st = min(st0 + slice * SL + s, a.n_qtiles - 1);
      const uint8_t *src = a.qpack + st * (int64_t)Q_BYTES + kc * 1024 + lane * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                       (__attribute__((address_space(3))) void *)(&s_q[buf][piece * 1024]), 16, 0, 0);
    }
  };
#if TM_KNN3_STAMPS
  unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_last = __builtin_amdgcn_s_memtime();
  const unsigned long long st_begin = st_last;
#endif
  stage(0, 0);
  for (int i = tid; i < NS * 32; i += NW * 64) {
    const int64_t st = min(st0 + (i >> 5), a.n_qtiles - 1);
    s_qn[i] = reinterpret_cast<const int *>(a.qpack + st * (int64_t)Q_BYTES + knn_pack_row_terms(KQ))[i & 31] & ~1;
    s_best[i] = ~0ull;
  }
  if (tid < 16) s_qm[tid] = tid < nvalid ? (unsigned)a.qmeta[qmeta_at(st0 + tid, QMETA_HMASK)] : 0u;
  const bool active = wave < n_seed;
  const int tile = r0a + (active ? wave : 0);
  const unsigned tm = (unsigned)__builtin_amdgcn_readfirstlane((int)a.thmask[tile]);
  v4i T[KT];
  v16i cin;
  unsigned pwh;
  k3_load_tile<KT>(a.tpack + (int64_t)tile * T_BYTES, lane, half, T, cin, pwh);
  if (lane < 32) s_tidx[wave * 32 + lane] = reinterpret_cast<const unsigned *>(a.tpack + (int64_t)tile * T_BYTES + knn_pack_indices(KT))[lane];
  const int n_slices = (nvalid + SL - 1) / SL;
  long long nblocks = 0, npairs = 0;
  const int vt = (int)min((int64_t)32, a.nt_rows - (int64_t)tile * 32);
  K3_STAMP(0);  // set-up: addresses, the tile's loads issued
  for (int sl = 0; sl < n_slices; sl++) {
    __syncthreads();  // slice sl has landed (the barrier waits for the LDS-DMA pieces); buffer (sl + 1) & 1 is no longer read
    K3_STAMP(sl == 0 ? 1 : 2);  // waiting for the first slice (and the tile) / for a later slice and the other waves
    if (sl + 1 < n_slices) stage(sl + 1, (sl + 1) & 1);
    if (active) {
      for (int j = 0; j < SL && sl * SL + j < nvalid; j++) {
        const int s = sl * SL + j;
        const int qi = s * 32 + (lane & 31);
        const unsigned cur_hi = k3_peek(reinterpret_cast<unsigned *>(&s_best[qi]) + 1), qn = (unsigned)s_qn[qi];  // (asked for before the chain: they arrive under it)
        const v16i acc = k3_chain<HT, HQ, TD>(T, cin, &s_q[sl & 1][j * KQ * 1024] + lane * 16, tm, (unsigned)__builtin_amdgcn_readfirstlane((int)s_qm[s]));
        k3_epilogue<TD, false>(acc, pwh, &s_tidx[wave * 32], half, qn, &s_best[qi], 0u, cur_hi);
        nblocks++;
        npairs += (long long)vt * (int)min((int64_t)32, a.nq - (st0 + s) * 32);
      }
    }
    K3_STAMP(3);  // the slice's blocks (behind the wait for the NEXT slice's pieces the compiler puts before the first LDS read)
  }
  __syncthreads();
  K3_STAMP(4);
  for (int i = tid; i < nvalid * 32; i += NW * 64) a.gbest[st0 * 32 + i] = s_best[i];
  for (int s = wave; s < nvalid; s += NW) {
    const unsigned mx = k3_wave_umax((unsigned)(s_best[s * 32 + (lane & 31)] >> 32));
    if (lane == 0) a.gsmax[st0 + s] = k3_bound_of(mx);
  }
#if TM_KNN3_STAMPS
  K3_STAMP(5);  // results
  if (a.stats && lane == 0) {
    for (int i = 0; i < 6; i++) atomicAdd(a.stats + K3S_SEED_STAMPS + i, st_acc[i]);
    atomicAdd(a.stats + K3S_SEED_STAMPS + 6, __builtin_amdgcn_s_memtime() - st_begin);
  }
#endif
  // The seeds' own counters (blocks, tiles read, pairs), one set of atomics per WORKGROUP into one of 64 striped slots: 90 000 waves adding to
  // three words of one cache line took their turns at the L2 and held every other request of the kernel up behind them (2.5 of its 3.3 ms).
  if (a.seed_stats) {
    __shared__ unsigned long long s_sum[2];  // blocks, pairs
    if (tid < 2) s_sum[tid] = 0;
    __syncthreads();
    if (lane == 0 && active) { atomicAdd(&s_sum[0], (unsigned long long)nblocks); atomicAdd(&s_sum[1], (unsigned long long)npairs); }
    __syncthreads();
    if (tid == 0) {
      unsigned long long *slot = a.seed_stats + (blockIdx.x & 63) * K3SEED_WORDS;
      atomicAdd(slot + K3SEED_BLOCKS, s_sum[0]);
      atomicAdd(slot + K3SEED_TILES, (unsigned long long)n_seed);
      atomicAdd(slot + K3SEED_PAIRS, s_sum[1]);
    }
  }
}

}  // namespace tmx
