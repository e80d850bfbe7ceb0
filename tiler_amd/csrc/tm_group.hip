// tm_group.hip -- the in-process communicator of a device group (tm_set_devices, include/tilemotion.h): the four collective kinds of
// Collectives between the shards of ONE process, each shard a host thread with its own device and stream.
//
// No kernel stores to another device's memory and no kernel waits for another shard's kernel: every cross-shard wait is a host
// barrier, and data crosses devices only as copies a shard pulls into its own memory (hipMemcpyPeerAsync; a plain device copy when
// both shards sit on one device).  An all-reduce is a reduce-scatter fused with an all-gather:
//   1. drain the stream, publish (device, pointer, bytes), barrier;
//   2. shard r pulls slice r of every peer's buffer into local staging, and k_group_reduce folds the N slices into slice r of its
//      own buffer; drain, barrier;
//   3. shard r pulls every other reduced slice from its owner; drain, barrier (nobody reuses its buffer while a peer still reads it).
// Every barrier gives up after TM_COMM_TIMEOUT_S and wakes at once when a shard has marked the group broken.
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "tm_common.h"
#include "tm_internal.h"

namespace tmx {

// ---- the reduce kernel ---------------------------------------------------------------------------------------------
// dst[i] = op over the N sources of element i; int32 sums wrap around as RCCL's do (two's complement), max is signed.  One 16-byte
// vector per thread and source: N slice reads and one write, nothing else touches memory.
struct GroupSrcs { const void *p[GROUP_MAX]; };

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void k_group_reduce(GroupSrcs src, int nsrc, int64_t n_elem, void *dst) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (KIND == TM_COLL_ALLREDUCE_SUM_I64) {
    if (VEC) {
      const int64_t nv = n_elem / 2;
      for (int64_t v = tid; v < nv; v += stride) {
        ulonglong2 a = reinterpret_cast<const ulonglong2 *>(src.p[0])[v];
        for (int s = 1; s < nsrc; s++) {
          const ulonglong2 b = reinterpret_cast<const ulonglong2 *>(src.p[s])[v];
          a.x += b.x; a.y += b.y;
        }
        reinterpret_cast<ulonglong2 *>(dst)[v] = a;
      }
    }
    for (int64_t i = (VEC ? n_elem / 2 * 2 : 0) + tid; i < n_elem; i += stride) {
      unsigned long long a = reinterpret_cast<const unsigned long long *>(src.p[0])[i];
      for (int s = 1; s < nsrc; s++) a += reinterpret_cast<const unsigned long long *>(src.p[s])[i];
      reinterpret_cast<unsigned long long *>(dst)[i] = a;
    }
  } else {
    auto op = [](uint32_t a, uint32_t b) -> uint32_t {
      if (KIND == TM_COLL_ALLREDUCE_MAX_I32) return (int32_t)a > (int32_t)b ? a : b;
      return a + b;
    };
    if (VEC) {
      const int64_t nv = n_elem / 4;
      for (int64_t v = tid; v < nv; v += stride) {
        uint4 a = reinterpret_cast<const uint4 *>(src.p[0])[v];
        for (int s = 1; s < nsrc; s++) {
          const uint4 b = reinterpret_cast<const uint4 *>(src.p[s])[v];
          a.x = op(a.x, b.x); a.y = op(a.y, b.y); a.z = op(a.z, b.z); a.w = op(a.w, b.w);
        }
        reinterpret_cast<uint4 *>(dst)[v] = a;
      }
    }
    for (int64_t i = (VEC ? n_elem / 4 * 4 : 0) + tid; i < n_elem; i += stride) {
      uint32_t a = reinterpret_cast<const uint32_t *>(src.p[0])[i];
      for (int s = 1; s < nsrc; s++) a = op(a, reinterpret_cast<const uint32_t *>(src.p[s])[i]);
      reinterpret_cast<uint32_t *>(dst)[i] = a;
    }
  }
}

template <int KIND> static void launch_reduce_kind(const GroupSrcs &s, int nsrc, int64_t n, void *dst, bool vec, hipStream_t stream) {
  const int64_t per_thread = vec ? (KIND == TM_COLL_ALLREDUCE_SUM_I64 ? 2 : 4) : 1;
  const int64_t threads = (n + per_thread - 1) / per_thread;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, 256 * 8));
  if (vec) hipLaunchKernelGGL((k_group_reduce<KIND, true>), dim3(grid), dim3(256), 0, stream, s, nsrc, n, dst);
  else hipLaunchKernelGGL((k_group_reduce<KIND, false>), dim3(grid), dim3(256), 0, stream, s, nsrc, n, dst);
}

int launch_group_reduce(int kind, const void *const *srcs, int nsrc, int64_t n_elem, void *dst, hipStream_t stream) {
  TM_CHECK(nsrc >= 1 && nsrc <= GROUP_MAX && n_elem >= 0 && kind >= 0 && kind <= TM_COLL_ALLREDUCE_SUM_I64, TM_E_INVAL, "group reduce: bad arguments");
  if (n_elem == 0) return TM_OK;
  GroupSrcs s{};
  uintptr_t align = (uintptr_t)dst;
  for (int i = 0; i < nsrc; i++) { s.p[i] = srcs[i]; align |= (uintptr_t)srcs[i]; }
  const bool vec = (align & 15) == 0;  // 16-byte loads where every pointer allows them (pool blocks and slice starts do)
  switch (kind) {
    case TM_COLL_ALLREDUCE_SUM_I32: launch_reduce_kind<TM_COLL_ALLREDUCE_SUM_I32>(s, nsrc, n_elem, dst, vec, stream); break;
    case TM_COLL_ALLREDUCE_MAX_I32: launch_reduce_kind<TM_COLL_ALLREDUCE_MAX_I32>(s, nsrc, n_elem, dst, vec, stream); break;
    default: launch_reduce_kind<TM_COLL_ALLREDUCE_SUM_I64>(s, nsrc, n_elem, dst, vec, stream); break;
  }
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// ---- the communicator ---------------------------------------------------------------------------------------------
struct GroupComm {
  int n = 0;
  std::vector<int> dev;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool broken = false;
  int broken_by = -1;
  struct Slot { const void *a = nullptr; void *b = nullptr; int64_t bytes = 0; };
  std::vector<Slot> slot;
};

GroupComm *group_comm_create(const std::vector<int> &devices) {
  GroupComm *g = new GroupComm();
  g->n = (int)devices.size();
  g->dev = devices;
  g->slot.resize(devices.size());
  return g;
}
void group_comm_destroy(GroupComm *g) { delete g; }

void group_comm_reset(GroupComm *g) {
  std::lock_guard<std::mutex> lk(g->mu);
  g->arrived = 0;
  g->broken = false;
  g->broken_by = -1;
}

void group_comm_abort(GroupComm *g, int rank) {
  std::lock_guard<std::mutex> lk(g->mu);
  if (!g->broken) { g->broken = true; g->broken_by = rank; }
  g->cv.notify_all();
}

int group_comm_broken_by(GroupComm *g) {
  std::lock_guard<std::mutex> lk(g->mu);
  return g->broken ? g->broken_by : -1;
}

// all shards arrive, or the group is broken (by a shard's failure or by this wait's time limit)
static int barrier(GroupComm *g, int rank) {
  std::unique_lock<std::mutex> lk(g->mu);
  TM_CHECK(!g->broken, TM_E_HIP, "device group: shard %d failed, the collective is abandoned", g->broken_by);
  const uint64_t my = g->gen;
  if (++g->arrived == g->n) {
    g->arrived = 0;
    g->gen++;
    g->cv.notify_all();
    return TM_OK;
  }
  const double limit = knobs().comm_timeout_s;
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(limit));
  while (g->gen == my && !g->broken) {
    if (g->cv.wait_until(lk, deadline) == std::cv_status::timeout && g->gen == my && !g->broken) {
      g->broken = true;
      g->broken_by = rank;
      g->cv.notify_all();
      set_error("device group: shard %d waited %.0f s for the other shards (TM_COMM_TIMEOUT_S)", rank, limit);
      return TM_E_HIP;
    }
  }
  TM_CHECK(g->gen != my, TM_E_HIP, "device group: shard %d failed, the collective is abandoned", g->broken_by);
  return TM_OK;
}

static int pull(GroupComm *g, int rank, void *dst, int peer, const void *src, size_t bytes, hipStream_t stream) {
  if (bytes == 0) return TM_OK;
  if (g->dev[peer] == g->dev[rank]) TM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
  else TM_HIP(hipMemcpyPeerAsync(dst, g->dev[rank], src, g->dev[peer], bytes, stream));
  return TM_OK;
}

// slice r of a buffer of `bytes`: [lo, hi), in 16-byte units so that every slice starts on a vector
static void slice_of(int64_t bytes, int r, int n, int64_t *lo, int64_t *hi) {
  const int64_t units = (bytes + 15) / 16, base = units / n, rem = units % n;
  const int64_t u0 = r * base + std::min<int64_t>(r, rem), u1 = u0 + base + (r < rem ? 1 : 0);
  *lo = std::min(bytes, u0 * 16);
  *hi = std::min(bytes, u1 * 16);
}

int group_allreduce(GroupComm *g, int rank, int kind, void *buf, int64_t count, hipStream_t stream) {
  const int n = g->n;
  const int64_t es = kind == TM_COLL_ALLREDUCE_SUM_I64 ? 8 : 4, bytes = count * es;
  TM_HIP(hipStreamSynchronize(stream));
  g->slot[rank] = GroupComm::Slot{buf, buf, bytes};
  TM_TRY(barrier(g, rank));
  int64_t lo, hi;
  slice_of(bytes, rank, n, &lo, &hi);
  const int64_t len = hi - lo;
  const size_t pitch = ((size_t)std::max<int64_t>(len, 0) + 15) & ~(size_t)15;  // staging rows start on 16 bytes
  DevBuf stage;
  if (len > 0) {
    TM_TRY(stage.alloc(pitch * n));
    const void *srcs[GROUP_MAX];
    for (int p = 0; p < n; p++) {
      if (p == rank) { srcs[p] = (const uint8_t *)buf + lo; continue; }
      srcs[p] = stage.as<uint8_t>() + pitch * p;
      TM_TRY(pull(g, rank, stage.as<uint8_t>() + pitch * p, p, (const uint8_t *)g->slot[p].a + lo, (size_t)len, stream));
    }
    TM_TRY(launch_group_reduce(kind, srcs, n, len / es, (uint8_t *)buf + lo, stream));
  }
  TM_HIP(hipStreamSynchronize(stream));
  TM_TRY(barrier(g, rank));
  for (int p = 0; p < n; p++) {
    if (p == rank) continue;
    int64_t plo, phi;
    slice_of(bytes, p, n, &plo, &phi);
    if (phi > plo) TM_TRY(pull(g, rank, (uint8_t *)buf + plo, p, (const uint8_t *)g->slot[p].a + plo, (size_t)(phi - plo), stream));
  }
  TM_HIP(hipStreamSynchronize(stream));
  return barrier(g, rank);
}

int group_allgather(GroupComm *g, int rank, const void *send, void *recv, int64_t bytes, hipStream_t stream) {
  const int n = g->n;
  TM_HIP(hipStreamSynchronize(stream));
  g->slot[rank] = GroupComm::Slot{send, recv, bytes};
  TM_TRY(barrier(g, rank));
  for (int p = 0; p < n; p++) {
    uint8_t *dst = (uint8_t *)recv + (size_t)bytes * p;
    if (p == rank) {
      if (dst != send && bytes > 0) TM_HIP(hipMemcpyAsync(dst, send, (size_t)bytes, hipMemcpyDeviceToDevice, stream));  // (in place: already there)
    } else TM_TRY(pull(g, rank, dst, p, g->slot[p].a, (size_t)bytes, stream));
  }
  TM_HIP(hipStreamSynchronize(stream));
  return barrier(g, rank);
}

}  // namespace tmx

// tm_probe_group_allreduce: `iters` int32 sum all-reduces of `bytes` over a throw-away group of n shards, one thread each (tools/group_bench.py)
extern "C" int tm_probe_group_allreduce(const int *devices, int n, int64_t bytes, int iters, double *us_per_call) {
  using namespace tmx;
  TM_TRY(require_device());
  TM_CHECK(devices && n >= 1 && n <= GROUP_MAX && bytes >= 4 && iters >= 1 && us_per_call, TM_E_INVAL, "group probe: bad arguments");
  GroupComm *g = group_comm_create(std::vector<int>(devices, devices + n));
  const Knobs kn = knobs();
  std::vector<int> rcs((size_t)n, TM_OK);
  std::vector<std::string> errs((size_t)n);
  double us = 0;
  auto shard = [&](int r) {
    knobs_set(kn);
    int rc = TM_OK;
    {
      DevBuf buf;
      hipStream_t st = nullptr;
      rc = hipSetDevice(devices[r]) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess ? TM_OK : TM_E_HIP;
      if (rc == TM_OK) rc = buf.alloc((size_t)bytes);
      if (rc == TM_OK && hipMemsetAsync(buf.p, r + 1, (size_t)bytes, st) != hipSuccess) rc = TM_E_HIP;
      for (int i = 0; rc == TM_OK && i < 3; i++) rc = group_allreduce(g, r, TM_COLL_ALLREDUCE_SUM_I32, buf.p, bytes / 4, st);  // warm-up
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; rc == TM_OK && i < iters; i++) rc = group_allreduce(g, r, TM_COLL_ALLREDUCE_SUM_I32, buf.p, bytes / 4, st);
      if (rc == TM_OK && r == 0) us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / iters;
      if (rc != TM_OK) { errs[(size_t)r] = get_error(); group_comm_abort(g, r); }
      if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    }
    pool_trim();
    rcs[(size_t)r] = rc;
  };
  std::vector<std::thread> th;
  for (int r = 1; r < n; r++) th.emplace_back(shard, r);
  shard(0);
  for (auto &t : th) t.join();
  group_comm_destroy(g);
  for (int r = 0; r < n; r++)
    if (rcs[(size_t)r] != TM_OK) { set_error("group probe, shard %d: %s", r, errs[(size_t)r].c_str()); return rcs[(size_t)r]; }
  *us_per_call = us;
  return TM_OK;
}
