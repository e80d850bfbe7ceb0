// tm_lists.hip -- index lists by a scan or a sort: the flagged items of an array (compact_kept), the members of every group (build_groups).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

namespace {
__global__ void k_scatter_kept(const int32_t *__restrict__ keep, const uint32_t *__restrict__ pos, int64_t n, int32_t *__restrict__ out_idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (keep[i]) out_idx[pos[i]] = (int32_t)i;
}
}  // namespace

// indices of the flagged items in ascending order (TransferTiles' gather, tilingencoder.pas:4048-4103, made deterministic);
// pos[i] = rank of item i among the kept ones (valid where keep[i] != 0)
int compact_kept(const void *keep, int64_t n, void *out_idx, void *pos, int64_t *host_count, hipStream_t stream) {
  TM_CHECK(n >= 0 && n < (int64_t)1 << 31, TM_E_INVAL, "compact: count out of range");
  *host_count = 0;
  if (n == 0) return TM_OK;
  DevBuf tmp;
  TM_TRY(with_temp(tmp, "compact: scan of the flags", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, (const uint32_t *)keep, (uint32_t *)pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream);
  }));
  hipLaunchKernelGGL(k_scatter_kept, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, (const int32_t *)keep,
                     (const uint32_t *)pos, n, (int32_t *)out_idx);
  TM_HIP(hipGetLastError());
  uint32_t last_pos = 0;
  int32_t last_keep = 0;
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(&last_pos, (const uint32_t *)pos + (n - 1), 4));
    TM_TRY(hr_.get(&last_keep, (const int32_t *)keep + (n - 1), 4));
    TM_TRY(hr_.wait());
  }
  *host_count = (int64_t)last_pos + (last_keep ? 1 : 0);
  return TM_OK;
}

namespace {
__global__ void k_iota_u32(uint32_t *__restrict__ v, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = (uint32_t)i;
}
}  // namespace

// member lists of a dedup: off[g] .. off[g+1] index `members`, which holds the rows of group g in ascending row order
// (remap = row -> group, counts = rows per group, as run_dedup_ex(by_index = 1) returns them)
int build_groups(const void *remap, int64_t n, const void *counts, int64_t ngroups, void *off, void *members, hipStream_t stream) {
  TM_CHECK(n >= 0 && n < (int64_t)1 << 31 && ngroups >= 0, TM_E_INVAL, "groups: count out of range");
  if (n == 0) return TM_OK;
  DevBuf tmp, keys_out, iota;
  TM_TRY(with_temp(tmp, "groups: scan of the counts", [&](void *t, size_t &b) {
    return rocprim::exclusive_scan(t, b, (const uint32_t *)counts, (uint32_t *)off, 0u, (size_t)ngroups, rocprim::plus<uint32_t>(), stream);
  }));
  const uint32_t total = (uint32_t)n;
  TM_HIP(hipMemcpyAsync((uint32_t *)off + ngroups, &total, 4, hipMemcpyHostToDevice, stream));
  TM_TRY(keys_out.alloc((size_t)n * 4)); TM_TRY(iota.alloc((size_t)n * 4));
  hipLaunchKernelGGL(k_iota_u32, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, iota.as<uint32_t>(), n);
  TM_TRY(with_temp(tmp, "groups: radix sort of the rows by group", [&](void *t, size_t &b) {
    return rocprim::radix_sort_pairs(t, b, (const uint32_t *)remap, keys_out.as<uint32_t>(), iota.as<uint32_t>(), (uint32_t *)members, (size_t)n, 0, 32, stream);
  }));
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(stream));  // `total` is on the stack; temporaries are released on return
  return TM_OK;
}

}  // namespace tmx
