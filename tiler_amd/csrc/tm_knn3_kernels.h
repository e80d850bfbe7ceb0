// tm_knn3_kernels.h -- what a tm_knn3_k<HT>.hip includes: the seed and consume kernels of the third scan shape (tm_knn3.h) and the launches
// of one database digit plan's instantiations, one per query plan (knn3_launch_*_ht, declared in tm_knn3.h and called by tm_knn.hip).
#pragma once
#include "tm_knn3_seed.h"
#include "tm_knn3_consume.h"

// FLAG: the kernels' fourth template argument (k_knn_consume's TOPK; the seed kernel ignores its own)
#define TM_KNN3_LAUNCH(KERNEL, HT, HQ, FLAG)                                                            \
  do {                                                                                                 \
    if (a.tdouble) hipLaunchKernelGGL((KERNEL<HT, HQ, true, FLAG>), grid, block, 0, stream, a);        \
    else hipLaunchKernelGGL((KERNEL<HT, HQ, false, FLAG>), grid, block, 0, stream, a);                 \
  } while (0)
#define TM_KNN3_CASE(KERNEL, HT, HQ, FLAG) \
  case HQ: TM_KNN3_LAUNCH(KERNEL, HT, HQ, FLAG); break;
#define TM_KNN3_SWITCH(KERNEL, HT, FLAG)                                                                                      \
  switch (hq) {                                                                                                               \
    TM_KNN3_CASE(KERNEL, HT, 0, FLAG) TM_KNN3_CASE(KERNEL, HT, 1, FLAG) TM_KNN3_CASE(KERNEL, HT, 2, FLAG)                     \
    TM_KNN3_CASE(KERNEL, HT, 3, FLAG) TM_KNN3_CASE(KERNEL, HT, 4, FLAG) TM_KNN3_CASE(KERNEL, HT, 5, FLAG)                     \
    default: TM_KNN3_LAUNCH(KERNEL, HT, 6, FLAG);                                                                             \
  }

#define TM_KNN3_DEFINE_HT(HT)                                                                         \
  template <> void knn3_launch_seed_ht<HT>(int hq, const Knn3Args &a, hipStream_t stream) {          \
    const dim3 grid((unsigned)a.n_groups), block(K3_SEEDS * 64);                                      \
    TM_KNN3_SWITCH(k_knn_seed, HT, false)                                                             \
  }                                                                                                   \
  template <> void knn3_launch_consume_ht<HT>(int hq, const Knn3Args &a, hipStream_t stream) {       \
    const dim3 grid((unsigned)a.grid_blocks), block(K3_NT);                                           \
    TM_KNN3_SWITCH(k_knn_consume, HT, false)                                                          \
  }                                                                                                   \
  template <> void knn3_launch_collect_ht<HT>(int hq, const Knn3Args &a, hipStream_t stream) {       \
    const dim3 grid((unsigned)a.grid_blocks), block(K3_NT);                                           \
    TM_KNN3_SWITCH(k_knn_consume, HT, true)                                                           \
  }
