// tm_shard.hip -- the encoder's multi-GPU side: the collectives and their three transports (the host's callback, the linked RCCL
// communicator, a device group's in-process communicator), the shares of work, and the device group of one process (tm_set_devices).
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include <rccl/rccl.h>

#include "tm_encoder.h"

// ---- the encoder's collectives (Collectives, tm_internal.h): every call is counted here, then handed to one of three transports -------
// The host's callback (tm_set_collective): everything queued so far is done before the host's collective touches the buffers (unless the
// callback enqueues on e->stream itself, tm_set_collective_mode), and the callback returns with the result in place.
static int coll_callback(tm_encoder *e, int kind, const void *send, void *recv, int64_t count) {
  if (!e->coll_stream_ordered) TM_HIP(hipStreamSynchronize(e->stream));
  const int rc = e->coll_cb(e->coll_user, kind, const_cast<void *>(send), recv, count);
  TM_CHECK(rc == 0, TM_E_HIP, "the host's collective callback failed (kind %d, code %d)", kind, rc);
  return TM_OK;
}
#define TM_NCCL(call)                                                                                         \
  do {                                                                                                        \
    const ncclResult_t r_ = (call);                                                                           \
    if (r_ != ncclSuccess) { set_error("%s failed: %s", #call, ncclGetErrorString(r_)); return TM_E_HIP; }  \
  } while (0)
// The library's communicator is non-blocking (tm_comm_init), so a call on it may answer ncclInProgress: the state is then polled until
// it settles, for at most TM_COMM_TIMEOUT_S seconds (default 120).
static ncclResult_t nccl_settle(ncclComm_t comm, ncclResult_t r) {
  if (r != ncclInProgress) return r;
  const double limit = knobs().comm_timeout_s;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    ncclResult_t st = ncclSuccess;
    const ncclResult_t q = ncclCommGetAsyncError(comm, &st);
    if (q != ncclSuccess) return q;
    if (st != ncclInProgress) return st;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) return ncclSystemError;
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}
#define TM_NCCLC(comm, call)                                                                                  \
  do {                                                                                                        \
    const ncclResult_t r_ = nccl_settle((comm), (call));                                                      \
    if (r_ != ncclSuccess) { set_error("%s failed: %s", #call, ncclGetErrorString(r_)); return TM_E_HIP; }  \
  } while (0)

// The library's own communicator (tm_comm_init), on the encoder's stream: nothing drains the stream before and nothing waits after --
// the RCCL kernel is ordered between what the step queued before and what it queues next.  The all-reduces work in place.
static int coll_native(tm_encoder *e, int kind, const void *send, void *recv, int64_t count) {
  void *b = const_cast<void *>(send);
  switch (kind) {
    case TM_COLL_ALLREDUCE_SUM_I32: TM_NCCLC(e->comm, ncclAllReduce(b, b, (size_t)count, ncclInt32, ncclSum, e->comm, e->stream)); break;
    case TM_COLL_ALLREDUCE_MAX_I32: TM_NCCLC(e->comm, ncclAllReduce(b, b, (size_t)count, ncclInt32, ncclMax, e->comm, e->stream)); break;
    case TM_COLL_ALLREDUCE_SUM_I64: TM_NCCLC(e->comm, ncclAllReduce(b, b, (size_t)count, ncclInt64, ncclSum, e->comm, e->stream)); break;
    default: TM_NCCLC(e->comm, ncclAllGather(send, recv, (size_t)count, ncclInt8, e->comm, e->stream));
  }
  return TM_OK;
}

// A device group's in-process communicator (tm_group.hip): it drains the stream, meets the other shards at host barriers and returns with
// the result in place.
static int coll_group(tm_encoder *e, int kind, const void *send, void *recv, int64_t count) {
  if (kind == TM_COLL_ALLGATHER_BYTES) return group_allgather(e->gcomm, e->co.rank, send, recv, count, e->stream);
  return group_allreduce(e->gcomm, e->co.rank, kind, const_cast<void *>(send), count, e->stream);
}

// the encoder becomes process `rank` of `world` on `transport`: the steps and Dither shard over them, the query features prefetched are void
static void join(tm_encoder *e, int rank, int world, int (*transport)(tm_encoder *, int, const void *, void *, int64_t)) {
  e->co.rank = rank;
  e->co.world = world;
  e->co.call = [e, transport](int kind, const void *send, void *recv, int64_t count) {
    e->coll_calls[kind]++;
    e->coll_bytes += kind == TM_COLL_ALLGATHER_BYTES ? count * e->co.world : count * (kind == TM_COLL_ALLREDUCE_SUM_I64 ? 8 : 4);
    return transport(e, kind, send, recv, count);
  };
  e->dither_rank = rank;
  e->dither_world = world;
  e->qf_valid = false;
}

void comm_abort(tm_encoder *e) {  // (abort = destroy without the collective handshake: no peer is waited for)
  if (e->comm) { (void)hipStreamSynchronize(e->stream); (void)ncclCommAbort(e->comm); }
}

// this process's share [lo, hi) of n items, contiguous, earlier processes take the remainder (the same rule as tiler_amd.distributed.frame_shard)
void share_of(int64_t n, int rank, int world, int64_t *lo, int64_t *hi) {
  const int64_t base = n / world, rem = n % world;
  *lo = rank * base + std::min<int64_t>(rank, rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}
// all-gather of per-process pieces of different sizes: send `count` items of `item` bytes, receive everyone's into `out` (in rank
// order, contiguous); counts[r] comes back on the host
int gather_var(tm_encoder *e, const void *send, int64_t count, int item, DevBuf &out, std::vector<int64_t> *counts) {
  const int W = e->co.world;
  DevBuf dcnt, dall, pad, recv;
  TM_TRY(dcnt.alloc(8)); TM_TRY(dall.alloc((size_t)W * 8));
  TM_HIP(hipMemcpyAsync(dcnt.p, &count, 8, hipMemcpyHostToDevice, e->stream));
  TM_TRY(e->co.allgather(dcnt.p, dall.p, 8));
  counts->assign((size_t)W, 0);
  {
    HostRead hr_(e->stream);
    TM_TRY(hr_.get(counts->data(), dall.p, (size_t)W * 8));
    TM_TRY(hr_.wait());
  }
  int64_t mx = 0, total = 0;
  for (int64_t c : *counts) { mx = std::max(mx, c); total += c; }
  TM_TRY(out.alloc((size_t)std::max<int64_t>(total, 1) * item));
  if (mx == 0) return TM_OK;
  const size_t chunk = (((size_t)mx * item + 15) / 16) * 16;
  TM_TRY(pad.alloc(chunk)); TM_TRY(recv.alloc(chunk * W));
  if (count > 0) TM_HIP(hipMemcpyAsync(pad.p, send, (size_t)count * item, hipMemcpyDeviceToDevice, e->stream));
  TM_TRY(e->co.allgather(pad.p, recv.p, (int64_t)chunk));
  int64_t off = 0;
  for (int r = 0; r < W; r++) {
    if ((*counts)[r] > 0)
      TM_HIP(hipMemcpyAsync(out.as<uint8_t>() + (size_t)off * item, recv.as<uint8_t>() + chunk * r, (size_t)(*counts)[r] * item, hipMemcpyDeviceToDevice, e->stream));
    off += (*counts)[r];
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

static void set_query_shard(tm_encoder *e, int first_frame, int frame_count) {
  if (first_frame != e->shard_first || frame_count != e->shard_count) e->qf_valid = false;  // prefetched for the old range (freed with the next Load / Reconstruct)
  e->shard_first = first_frame;
  e->shard_count = frame_count;
}

// ---- one process, several devices (tm_set_devices) ---------------------------------------------------------------------------
// Shard 0 is the front encoder, driven on the caller's thread; shards 1 .. N-1 are encoders that live on persistent worker threads, one
// each: a thread's device pool, page-locked area, knobs and error text are its own (tm_tables.hip), so a shard's memory is allocated and
// freed on its thread from its creation to tm_destroy.  A call reaches every shard at once and returns the first error.
struct ShardWorker {
  int rank = 0, device = 0;
  tm_encoder *enc = nullptr;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int(tm_encoder *)> job;
  Knobs kn;                // the caller's sampled switches, taken with the job
  bool pending = true, quit = false;
  int rc = TM_OK;
  std::string err;
};

struct Group {
  std::vector<int> devices;
  std::vector<std::unique_ptr<ShardWorker>> workers;  // shards 1 .. N-1
  GroupComm *comm = nullptr;
};

static void shard_main(ShardWorker *w, Settings s, bool auto_tile_count) {
  std::unique_lock<std::mutex> lk(w->mu);
  if (hipSetDevice(w->device) != hipSuccess) {
    w->rc = TM_E_HIP;
    w->err = std::string("hipSetDevice failed: ") + hipGetErrorString(hipGetLastError());
  } else {
    w->enc = new tm_encoder();
    w->enc->device = w->device;
    w->enc->s = s;  // settings made before the group was formed carry over
    w->enc->auto_tile_count = auto_tile_count;
  }
  w->pending = false;
  w->cv.notify_all();
  for (;;) {
    w->cv.wait(lk, [w] { return (bool)w->job || w->quit; });
    if (!w->job) break;
    std::function<int(tm_encoder *)> job = std::move(w->job);
    w->job = nullptr;
    knobs_set(w->kn);
    lk.unlock();
    const int rc = w->enc ? job(w->enc) : TM_E_INVAL;
    const std::string err = rc == TM_OK ? std::string() : w->enc ? std::string(get_error()) : std::string("shard not created");
    if (rc != TM_OK && w->enc && w->enc->gcomm) group_comm_abort(w->enc->gcomm, w->rank);  // the other shards stop waiting for this one
    lk.lock();
    w->rc = rc;
    w->err = err;
    w->pending = false;
    w->cv.notify_all();
  }
  lk.unlock();
  if (w->enc) {
    delete w->enc;
    pool_trim();  // the shard's device blocks go back to the driver from the thread that holds them
  }
}

void group_teardown(tm_encoder *e) {
  Group *g = e->grp;
  for (auto &w : g->workers) {
    { std::lock_guard<std::mutex> lk(w->mu); w->quit = true; }
    w->cv.notify_all();
    if (w->th.joinable()) w->th.join();
  }
  if (g->comm) group_comm_destroy(g->comm);
  delete g;
  e->grp = nullptr;
  e->gcomm = nullptr;
}

// fn on every shard at once (shard 0 on the caller's thread); the error of the shard that broke the group first, else of the lowest failing shard
int group_each(tm_encoder *e, const std::function<int(tm_encoder *)> &fn) {
  Group *g = e->grp;
  const Knobs kn = knobs();
  for (auto &w : g->workers) {
    { std::lock_guard<std::mutex> lk(w->mu); w->job = fn; w->kn = kn; w->pending = true; }
    w->cv.notify_all();
  }
  e->grp = nullptr;  // shard 0 is the front encoder itself: while its share runs it is a plain encoder
  const int rc0 = fn(e);
  e->grp = g;
  const std::string err0 = rc0 == TM_OK ? std::string() : std::string(get_error());
  if (rc0 != TM_OK && e->gcomm) group_comm_abort(e->gcomm, 0);
  const int n = (int)g->devices.size();
  std::vector<int> rcs((size_t)n, TM_OK);
  std::vector<std::string> errs((size_t)n);
  rcs[0] = rc0;
  errs[0] = err0;
  for (auto &w : g->workers) {
    std::unique_lock<std::mutex> lk(w->mu);
    w->cv.wait(lk, [&] { return !w->pending; });
    rcs[(size_t)w->rank] = w->rc;
    errs[(size_t)w->rank] = w->err;
  }
  int pick = e->gcomm ? group_comm_broken_by(e->gcomm) : -1;
  if (pick < 0 || rcs[(size_t)pick] == TM_OK) {
    pick = -1;
    for (int r = 0; r < n && pick < 0; r++)
      if (rcs[(size_t)r] != TM_OK) pick = r;
  }
  if (pick < 0) return TM_OK;
  if (pick == 0) set_error("%s", err0.c_str());
  else set_error("shard %d (device %d): %s", pick, g->devices[(size_t)pick], errs[(size_t)pick].c_str());
  return rcs[(size_t)pick];
}

// tiler_amd.distributed.keyframe_shard: the frame shares' borders snapped to the nearest key-frame start (ties: the earlier one)
static void keyframe_shard(const std::vector<int32_t> &kf, int nframes, int rank, int world, int *first, int *count) {
  std::vector<int64_t> cuts{0};
  for (int r = 1; r < world; r++) {
    int64_t ideal, hi;
    share_of(nframes, r, world, &ideal, &hi);
    int64_t snap = kf.empty() ? 0 : kf[0];
    for (int32_t k : kf)
      if (std::llabs(k - ideal) < std::llabs(snap - ideal) || (std::llabs(k - ideal) == std::llabs(snap - ideal) && k < snap)) snap = k;
    cuts.push_back(std::max(snap, cuts.back()));
  }
  cuts.push_back(nframes);
  *first = (int)cuts[(size_t)rank];
  *count = (int)(cuts[(size_t)rank + 1] - cuts[(size_t)rank]);
}

// one step on every shard, with the query frames tiler_amd.distributed.run_all would give each: the Load share (motion prediction off: what
// Reconstruct requires of a sharded Load), the key-frame-snapped share for Reconstruct with motion prediction
int group_run_step(tm_encoder *e, int step) {
  Group *g = e->grp;
  const int n = (int)g->devices.size();
  group_comm_reset(g->comm);
  std::vector<int> qf((size_t)n), qc((size_t)n);
  for (int r = 0; r < n; r++) {
    int64_t lo, hi;
    share_of(e->nframes, r, n, &lo, &hi);
    qf[(size_t)r] = (int)lo;
    qc[(size_t)r] = (int)(hi - lo);
  }
  TM_HIP(hipSetDevice(e->device));
  if (step == TM_STEP_RECONSTRUCT && e->s.MotionPredictRadius > 0) {
    TM_TRY(load_tail(e));
    for (int r = 0; r < n; r++) keyframe_shard(e->kf_start, e->nframes, r, n, &qf[(size_t)r], &qc[(size_t)r]);
  }
  // PreparePalettes' branch is taken once for the group, from shard 0's state, so that the shards cannot disagree
  const int whole = step == TM_STEP_PREPARE_PALETTES ? (!knobs().pp_sharded && palettize_resident(e->t, e->s.PaletteCount) ? 1 : 0) : -1;
  return group_each(e, [&](tm_encoder *s) {
    set_query_shard(s, qf[(size_t)s->co.rank], qc[(size_t)s->co.rank]);
    s->pp_whole = whole;
    return run_step(s, step);
  });
}

static int group_form(tm_encoder *e, const std::vector<int> &devices) {
  const int n = (int)devices.size();
  for (int a : devices)  // every pair of distinct devices must reach each other's memory (the shards pull across)
    for (int b : devices) {
      if (a == b) continue;
      int can = 0;
      TM_HIP(hipDeviceCanAccessPeer(&can, a, b));
      TM_CHECK(can, TM_E_UNSUPPORTED, "device group: device %d cannot reach the memory of device %d", a, b);
      TM_HIP(hipSetDevice(a));
      const hipError_t pe = hipDeviceEnablePeerAccess(b, 0);
      if (pe == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
      else TM_HIP(pe);
    }
  e->device = devices[0];
  TM_HIP(hipSetDevice(e->device));
  Group *g = new Group();
  g->devices = devices;
  g->comm = group_comm_create(devices);
  e->grp = g;
  e->gcomm = g->comm;
  int rc = TM_OK;
  std::string err;
  for (int r = 1; r < n; r++) {
    g->workers.emplace_back(new ShardWorker());
    ShardWorker *w = g->workers.back().get();
    w->rank = r;
    w->device = devices[(size_t)r];
    w->th = std::thread(shard_main, w, e->s, e->auto_tile_count);
    std::unique_lock<std::mutex> lk(w->mu);
    w->cv.wait(lk, [w] { return !w->pending; });
    if (w->rc != TM_OK && rc == TM_OK) { rc = w->rc; err = w->err; }
  }
  if (rc != TM_OK) {
    group_teardown(e);
    set_error("device group: shard on device %s", err.c_str());
    return rc;
  }
  std::vector<tm_encoder *> shards{e};
  for (auto &w : g->workers) shards.push_back(w->enc);  // (the workers are idle: the next job's hand-over publishes these fields)
  for (int r = 0; r < n; r++) {
    tm_encoder *s = shards[(size_t)r];
    s->gcomm = g->comm;
    join(s, r, n, coll_group);
  }
  return TM_OK;
}

// tm_get_frame_quality / tm_render_frames(input) of a group whose Load was sharded: each shard holds the source frames of its own Load range, so
// the range is cut at those borders and every piece is computed on its shard
std::vector<Piece> group_pieces(tm_encoder *e, int first, int count) {
  std::vector<Piece> out(e->grp->devices.size());
  for (size_t r = 0; r < out.size(); r++) {
    int64_t lo, hi;
    share_of(e->nframes, (int)r, (int)out.size(), &lo, &hi);
    const int64_t a = std::max<int64_t>(lo, first), b = std::min<int64_t>(hi, (int64_t)first + count);
    if (b > a) out[r] = Piece{(int)a, (int)(b - a)};
  }
  return out;
}

extern "C" {

int tm_set_query_shard(tm_encoder *e, int first_frame, int frame_count) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_set_query_shard: a device group shards by itself");
  TM_CHECK(first_frame >= 0, TM_E_INVAL, "bad shard");
  set_query_shard(e, first_frame, frame_count);
  return TM_OK;
}

int tm_set_collective_mode(tm_encoder *e, int stream_ordered) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  e->coll_stream_ordered = stream_ordered != 0;
  return TM_OK;
}

int tm_comm_unique_id(uint8_t id[TM_COMM_ID_BYTES]) {
  TM_CHECK(id, TM_E_INVAL, "null argument");
  static_assert(sizeof(ncclUniqueId) == TM_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  TM_NCCL(ncclGetUniqueId(&u));
  memcpy(id, &u, sizeof(u));
  return TM_OK;
}

int tm_comm_init(tm_encoder *e, const uint8_t id[TM_COMM_ID_BYTES], int rank, int world) {
  TM_CHECK(e && id, TM_E_INVAL, "null argument");
  TM_CHECK(world >= 1 && rank >= 0 && rank < world, TM_E_INVAL, "bad process %d of %d", rank, world);
  TM_CHECK(e->comm == nullptr, TM_E_INVAL, "tm_comm_init: this encoder already has a communicator (tm_comm_destroy first)");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_comm_init: the encoder is a device group (tm_set_devices), which carries its own collectives");
  knobs_reload();
  TM_HIP(hipSetDevice(e->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  {
    // Non-blocking: a rank that never arrives (it failed before this call) must end in an error here, not in a wait without end
    // (TM_COMM_TIMEOUT_S seconds, default 120).  Later calls on the communicator go through TM_NCCL, which waits out ncclInProgress.
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclResult_t r = ncclCommInitRankConfig(&e->comm, world, u, rank, &cfg);
    const double limit = knobs().comm_timeout_s;
    const auto t0 = std::chrono::steady_clock::now();
    while (r == ncclInProgress || (r == ncclSuccess && e->comm)) {
      ncclResult_t st = ncclSuccess;
      const ncclResult_t q = ncclCommGetAsyncError(e->comm, &st);
      if (q != ncclSuccess) { r = q; break; }
      if (st != ncclInProgress) { r = st; break; }
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) { r = ncclSystemError; set_error("tm_comm_init: not every one of the %d processes arrived within %.0f s", world, limit); break; }
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (r != ncclSuccess) {
      const std::string why = std::string(get_error());
      if (e->comm) { (void)ncclCommAbort(e->comm); e->comm = nullptr; }
      if (why.find("tm_comm_init: not every") == std::string::npos) set_error("ncclCommInitRankConfig failed: %s", ncclGetErrorString(r));
      return TM_E_HIP;
    }
  }
  e->coll_cb = nullptr;
  e->coll_user = nullptr;
  e->coll_stream_ordered = true;
  e->force_dist = knobs().comm_force_dist;
  join(e, rank, world, coll_native);
  return TM_OK;
}

int tm_get_collective_stats(tm_encoder *e, int64_t calls[4], int64_t *bytes, int reset) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (calls) memcpy(calls, e->coll_calls, sizeof(e->coll_calls));
  if (bytes) *bytes = e->coll_bytes;
  if (reset) { memset(e->coll_calls, 0, sizeof(e->coll_calls)); e->coll_bytes = 0; }
  return TM_OK;
}

int tm_comm_destroy(tm_encoder *e) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  if (!e->comm) return TM_OK;
  TM_HIP(hipStreamSynchronize(e->stream));
  TM_NCCLC(e->comm, ncclCommFinalize(e->comm));  // (non-blocking communicator: flush what it still holds, then free it)
  TM_NCCL(ncclCommDestroy(e->comm));
  e->comm = nullptr;
  e->coll_stream_ordered = false;  // a callback installed afterwards gets the default contract: stream drained before, result in place after
  e->force_dist = false;
  e->co = Collectives();
  e->dither_rank = 0;
  e->dither_world = 1;
  e->qf_valid = false;
  return TM_OK;
}

int tm_set_collective(tm_encoder *e, int rank, int world, tm_collective_cb cb, void *user) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(world >= 1 && rank >= 0 && rank < world && (cb != nullptr || world == 1), TM_E_INVAL, "bad process %d of %d", rank, world);
  TM_CHECK(e->comm == nullptr, TM_E_INVAL, "tm_set_collective: the encoder has a native communicator (tm_comm_destroy first)");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_set_collective: the encoder is a device group (tm_set_devices), which carries its own collectives");
  e->coll_stream_ordered = false;  // mode 0 until tm_set_collective_mode says otherwise
  e->coll_cb = world > 1 ? cb : nullptr;
  e->coll_user = user;
  join(e, rank, world, coll_callback);
  return TM_OK;
}

int tm_set_dither_shard(tm_encoder *e, int rank, int world) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_set_dither_shard: a device group shards by itself");
  TM_CHECK(world >= 1 && rank >= 0 && rank < world, TM_E_INVAL, "bad dither shard %d of %d", rank, world);
  e->dither_rank = rank;
  e->dither_world = world;
  return TM_OK;
}

int tm_set_devices(tm_encoder *e, const int *devices, int n) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(devices && n >= 1 && n <= GROUP_MAX, TM_E_INVAL, "tm_set_devices: %d devices (1 .. %d)", n, GROUP_MAX);
  const int nd = tm_device_count();
  for (int i = 0; i < n; i++) TM_CHECK(devices[i] >= 0 && devices[i] < nd, TM_E_INVAL, "tm_set_devices: device %d outside 0 .. %d", devices[i], nd - 1);
  TM_CHECK(e->nframes == 0, TM_E_INVAL, "tm_set_devices: call it before tm_set_video");
  TM_CHECK(!e->grp, TM_E_INVAL, "tm_set_devices: the encoder is already a device group");
  TM_CHECK(e->coll_cb == nullptr && e->comm == nullptr, TM_E_INVAL, "tm_set_devices: the encoder has a communicator (tm_set_collective / tm_comm_init)");
  if (n == 1) return tm_set_device(e, devices[0]);
  return group_form(e, std::vector<int>(devices, devices + n));
}

int tm_set_device_mask(tm_encoder *e, uint32_t mask) {
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_CHECK(mask != 0, TM_E_INVAL, "tm_set_device_mask: empty mask");
  std::vector<int> devs;
  for (int d = 0; d < 32; d++)
    if (mask & (1u << d)) devs.push_back(d);
  return tm_set_devices(e, devs.data(), (int)devs.size());
}

}  // extern "C"
