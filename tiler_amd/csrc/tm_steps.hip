// tm_steps.hip -- run_step and the steps of Run (tilingencoder.pas:5529-5554) without a file of their own: Load, PredictMotion, PreparePalettes,
// Dither and Reindex (Reduce: tm_reduce.hip, Reconstruct: tm_reconstruct.hip), and what the steps share (tm_steps.h): the small kernels
// behind their host wrappers, the merge of the tile-map arrays, the motion search's scratch.
//
// Every step reads and writes the encoder's device state (tm_encoder.h).  With one process per GPU or a device group (tm_shard.hip) a step
// works on its share and merges through the encoder's collectives (co); the sharded branches sit beside the single-process code they mirror.
#include <chrono>

#include "tm_steps.h"

namespace tmx {

// ---- small device helpers ------------------------------------------------------------------------------------
__global__ void k_gather_rows16(const uint4 *__restrict__ src, const int32_t *__restrict__ idx, int64_t n, int vec_per_row,
                                uint4 *__restrict__ dst) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * vec_per_row; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / vec_per_row;
    const int v = (int)(e - r * vec_per_row);
    dst[e] = src[(int64_t)idx[r] * vec_per_row + v];
  }
}
template <class T> __global__ void k_gather(const T *__restrict__ src, const int32_t *__restrict__ idx, int64_t n, T *__restrict__ dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}
// use counts.  Neighbouring items often name the same tile (flat areas: one tile can own a tenth of the clip, and its counter then
// serialises every atomic of the launch), so a wave adds a RUN of equal indices with one atomic: heads of runs by comparing with the lane
// before, run lengths off the ballot of heads.  The counts go into one copy of the histogram PER XCD: a workgroup adds to the copy of the
// XCD it runs on (the id is read from the hardware; placement only decides which copy, any copy is right) and k_hist_fold adds the eight
// copies up.  Every XCD has its own L2: an atomic on a word that all eight keep adding to travels between them every time, while a word
// only one XCD touches stays in that XCD's L2 --
// 0.49 -> 0.2 ms for the 4.3 M tile-map items of the bench clip (memset of the copies and the fold included); agent scope or workgroup
// scope measured the same, so the scope stays the one the memory model asks for.
__global__ __launch_bounds__(256) void k_histogram_xcd(const int32_t *__restrict__ idx, int64_t n, uint32_t *__restrict__ hist8, int64_t bins) {
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  uint32_t *hist = hist8 + (int64_t)(xcc & 7u) * bins;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x; i0 < n; i0 += stride) {
    const int64_t i = i0 + threadIdx.x;
    const int v = i < n ? idx[i] : -1;
    const int prev = __shfl_up(v, 1);
    const bool head = lane == 0 || v != prev;
    const unsigned long long heads = __ballot(head);
    if (head && v >= 0) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;
      atomicAdd(&hist[v], (uint32_t)len);
    }
  }
}
__global__ void k_hist_fold(const uint32_t *__restrict__ hist8, int64_t bins, uint32_t *__restrict__ hist) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < bins; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t s = 0;
#pragma unroll
    for (int x = 0; x < 8; x++) s += hist8[x * bins + i];
    hist[i] = s;
  }
}
__global__ void k_lookup(const int32_t *__restrict__ idx, int64_t n, const int32_t *__restrict__ table, int32_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = idx[i] >= 0 ? table[idx[i]] : -1;
}
__global__ void k_lookup_inplace(int32_t *__restrict__ idx, int64_t n, const int32_t *__restrict__ table) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (idx[i] >= 0) idx[i] = table[idx[i]];
}

}  // namespace tmx

// ---- their host wrappers (tm_steps.h) --------------------------------------------------------------------------
static int launched() { TM_HIP(hipGetLastError()); return TM_OK; }
int gather_rows(tm_encoder *e, const void *src, const void *idx, int64_t n, int bytes_per_row, void *dst) {
  const int vec = bytes_per_row / 16;
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(n * vec)), dim3(256), 0, e->stream, (const uint4 *)src, (const int32_t *)idx, n, vec, (uint4 *)dst);
  return launched();
}
template <class T> int gather(tm_encoder *e, const void *src, const void *idx, int64_t n, void *dst) {
  hipLaunchKernelGGL(k_gather<T>, dim3(gridn(n)), dim3(256), 0, e->stream, (const T *)src, (const int32_t *)idx, n, (T *)dst);
  return launched();
}
template int gather<uint8_t>(tm_encoder *, const void *, const void *, int64_t, void *);
template int gather<int32_t>(tm_encoder *, const void *, const void *, int64_t, void *);
template int gather<uint32_t>(tm_encoder *, const void *, const void *, int64_t, void *);
int lookup(tm_encoder *e, const void *idx, int64_t n, const void *table, void *out) {
  hipLaunchKernelGGL(k_lookup, dim3(gridn(n)), dim3(256), 0, e->stream, (const int32_t *)idx, n, (const int32_t *)table, (int32_t *)out);
  return launched();
}
int lookup_inplace(tm_encoder *e, void *idx, int64_t n, const void *table) {
  hipLaunchKernelGGL(k_lookup_inplace, dim3(gridn(n)), dim3(256), 0, e->stream, (int32_t *)idx, n, (const int32_t *)table);
  return launched();
}
int pal_from_tile(tm_encoder *e) { return lookup(e, e->tm_tile.p, e->q, e->gpal_idx.p, e->tm_pal.p); }

// Steps that read the frame tiles / the global tiles' RGB pixels: ReloadGTM brings neither (the stream holds palette indices
// only, HasRGBPixels = False at tilingencoder.pas:4937), so after a reload these steps need Load (and Reduce) to have run again.
int need_frame_tiles(tm_encoder *e, const char *step) {
  TM_CHECK(e->ftiles.p != nullptr && e->fflags.p != nullptr && e->flab.p != nullptr && e->q > 0, TM_E_INVAL,
           "step order: %s needs the frame tiles, which are not in memory (run Load first; ReloadGTM does not bring them)", step);
  return TM_OK;
}
int need_global_rgb(tm_encoder *e, const char *step) {
  TM_CHECK(e->gtiles_have_rgb && e->gtiles.p != nullptr, TM_E_INVAL,
           "step order: %s needs the global tiles' RGB pixels (run Reduce first; a reloaded .gtm holds palette indices only)", step);
  return TM_OK;
}
bool query_range(const tm_encoder *e, int *sf, int *sn) {
  *sf = std::max(0, std::min(e->shard_first, e->nframes));
  *sn = e->shard_count < 0 ? e->nframes - *sf : std::max(0, std::min(e->shard_count, e->nframes - *sf));
  return *sf > 0 || *sn < e->nframes;
}

// ---- the tile-map arrays over several processes (tm_steps.h) ----------------------------------------------------
// TileIdx and PalIdx: others hold -1, merged with MAX; the errors (any 32-bit pattern) and the motion results: others hold 0, merged with
// SUM -- the byte arrays as 32-bit words (they are allocated with 4 bytes to spare)
static const struct TmArray { int bit; DevBuf tm_encoder::*buf; int item, identity; bool by_max; } kTmArrays[] = {
    {TMA_TILE, &tm_encoder::tm_tile, 4, 0xff, true}, {TMA_ERR, &tm_encoder::tm_err, 4, 0, false},   {TMA_PAL, &tm_encoder::tm_pal, 4, 0xff, true},
    {TMA_PM_ERR, &tm_encoder::pm_err, 4, 0, false},  {TMA_PRED, &tm_encoder::tm_pred, 1, 0, false}, {TMA_PX, &tm_encoder::tm_px, 1, 0, false},
    {TMA_PY, &tm_encoder::tm_py, 1, 0, false}};

int clear_items(tm_encoder *e, int which, int keep_f0, int keep_nf) {
  const int64_t a = keep_nf > 0 ? keep_f0 * e->tm_size() : e->q, b = keep_nf > 0 ? a + keep_nf * e->tm_size() : e->q;  // the items [a, b) stay
  for (const TmArray &t : kTmArrays) {
    if (!(which & t.bit)) continue;
    uint8_t *p = (e->*t.buf).as<uint8_t>();
    if (a > 0) TM_HIP(hipMemsetAsync(p, t.identity, (size_t)(a * t.item), e->stream));
    if (b < e->q) TM_HIP(hipMemsetAsync(p + b * t.item, t.identity, (size_t)((e->q - b) * t.item), e->stream));
  }
  return TM_OK;
}

int merge_items(tm_encoder *e, int which) {
  for (const TmArray &t : kTmArrays) {
    if (!(which & t.bit)) continue;
    const int64_t words = t.item == 4 ? e->q : (e->q + 3) / 4;
    TM_TRY(t.by_max ? e->co.allreduce_max_i32((e->*t.buf).p, words) : e->co.allreduce_sum_i32((e->*t.buf).p, words));
  }
  return TM_OK;
}

// ---- motion search -----------------------------------------------------------------------------------------------
int MotionScratch::alloc(const tm_encoder *e, int nscreens) {
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  const int64_t nwin = (int64_t)(sw - 7) * (sh - 7);
  screen_bytes = (size_t)sw * sh * 4;
  for (int i = 0; i < nscreens; i++) TM_TRY(screen[i].alloc(screen_bytes));
  TM_TRY(win.alloc((size_t)nwin * 384));
  TM_TRY(cur.alloc((size_t)e->tm_size() * 384));
  return TM_OK;
}

std::vector<uint8_t> key_frame_mask(const tm_encoder *e) {
  std::vector<uint8_t> mask((size_t)e->nframes, 0);
  for (int32_t k : e->kf_start) mask[(size_t)k] = 1;
  return mask;
}

// ---- steps ---------------------------------------------------------------------------------------------------
// the host tail of Load -- PearsonCorrelation's last lines (2221-2227) and FindKeyFrames (3373-3411) -- once the sums are there
int load_tail(tm_encoder *e, hipStream_t st) {  // st: the stream the sums sit behind (null: the correlation's own)
  if (!e->load_tail_pending) return TM_OK;
  std::vector<float> sums((size_t)e->nframes * 3);
  if (!st) st = e->stream_aux ? e->stream_aux : e->stream;
  {
    HostRead hr_(st);
    TM_TRY(hr_.get(sums.data(), e->dcorrel.p, sums.size() * 4));
    TM_TRY(hr_.wait());
  }
  e->load_tail_pending = false;  // only now: a failed read-back leaves the tail to the next caller instead of stale key frames
  e->correl.assign(e->nframes, 0.0f);
  TM_TRY(tm_pearson_finish_host(sums.data(), e->nframes, e->correl.data()));  // tail of PearsonCorrelation (2221-2227) in host IEEE arithmetic
  e->kf_start.clear();
  if (e->kf_manual) {  // FindKeyFrames, manual mode (3380-3384): the thresholds and the spacing play no part
    e->kf_start = e->kf_manual_list;
    return TM_OK;
  }
  // FindKeyFrames, automatic mode (3373-3411)
  int64_t last = INT32_MIN;
  for (int f = 0; f < e->nframes; f++) {
    bool kf = f == 0;
    // (the settings as they stood when Load ran: the reference finds its key frames inside Load, 1741-1840)
    if (!kf && (double)e->correl[f] < e->kf_lo_thres) kf = true;
    if (!kf && (double)(f - last) >= e->kf_max_s * e->kf_fps) kf = true;
    if ((double)(f - last) < e->kf_min_s * e->kf_fps) kf = false;
    if (kf) { e->kf_start.push_back(f); last = f; }
  }
  return TM_OK;
}

// the chunked upload of a host clip into device buffer `slot`, queued on the copy stream with one event per chunk
int queue_host_clip(tm_encoder *e, int slot, const void *host) {
  tm_encoder::HostClip &hc = e->hclip[slot];
  const size_t fbytes = (size_t)e->width * e->height * 4;
  TM_TRY(hc.buf.alloc(fbytes * e->nframes));
  if (!e->copy_stream) TM_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  constexpr size_t chunk_mb = 48;  // (4-48 MB measured alike)
  hc.chunk = (int)std::max<size_t>(1, (chunk_mb << 20) / fbytes);
  hc.nchunks = (e->nframes + hc.chunk - 1) / hc.chunk;
  while ((int)hc.events.size() < hc.nchunks) {
    hipEvent_t ev;
    TM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hc.events.push_back(ev);
  }
  for (int c = 0; c < hc.nchunks; c++) {
    const int f0 = c * hc.chunk, nf = std::min(hc.chunk, e->nframes - f0);
    TM_HIP(hipMemcpyAsync(hc.buf.as<uint8_t>() + fbytes * f0, (const uint8_t *)host + fbytes * f0, fbytes * nf, hipMemcpyHostToDevice, e->copy_stream));
    TM_HIP(hipEventRecord(hc.events[c], e->copy_stream));
  }
  hc.host = host;
  hc.pending = true;
  hc.seq = ++e->hclip_seq;
  return TM_OK;
}

static int step_load(tm_encoder *e) {  // Load, tilingencoder.pas:1741-1841 (frames are pushed in, or decoded from InputFileName: load_from_input, tm_input.hip)
  TM_TRY(load_tail(e));  // (a correlation still running reads the Lab means this Load is about to replace)
  e->drop_prefetch();  // features of the previous frame tiles
  e->q_groups = 0;
  e->load_sharded = false;
  TM_CHECK(e->nframes > 0 && e->width > 0, TM_E_INVAL, "tm_set_video has not been called");
  const size_t fbytes = (size_t)e->width * e->height * 4;  // a frame
  const int64_t per = e->tm_size();                        // its tiles
  const bool own_frames_only = e->dist() && e->s.MotionPredictRadius <= 0;
  if (e->input.kind) TM_TRY(load_from_input(e));  // the source "file": from here on as if the clip had been set with tm_set_frames_device / _host
  if (e->frames_peer) {
    // a device group's clip on another device (tm_set_frames_device): this shard pulls the frames its Load reads into its own memory
    int64_t a = 0, b = e->nframes;
    if (own_frames_only) {
      share_of(e->nframes, e->co.rank, e->co.world, &a, &b);
      a = std::max<int64_t>(a - 1, 0);
    }
    TM_TRY(e->frames_owned.alloc(fbytes * e->nframes));
    if (b > a)
      TM_HIP(hipMemcpyPeerAsync(e->frames_owned.as<uint8_t>() + fbytes * a, e->device, (const uint8_t *)e->frames_peer + fbytes * a, e->frames_peer_dev,
                                fbytes * (b - a), e->stream));
    e->frames = e->frames_owned.p;
  }
  TM_CHECK(e->frames != nullptr || e->frames_host != nullptr, TM_E_INVAL, "no frames: call tm_push_frame_rgb32 / tm_set_frames_device / tm_set_frames_host first");
  e->q = (int64_t)e->nframes * per;
  TM_CHECK(e->q < (1ll << 31), TM_E_UNSUPPORTED, "%lld tile-map items: the index arrays are 32-bit (TileIdx is an Integer, tilingencoder.pas:179)", (long long)e->q);
  TM_TRY(e->ftiles.alloc((size_t)e->q * 256));
  TM_TRY(e->fflags.alloc((size_t)e->q + 4));  // (+4: merged as 32-bit words)
  TM_TRY(e->flab.alloc((size_t)e->q * 12));
  // frames f0 .. f0 + nf of the clip at src_base into their places in the frame tiles, mirror flags and Lab means
  auto load_frames = [&](const void *src_base, int64_t f0, int64_t nf) {
    return launch_load((const uint8_t *)src_base + fbytes * f0, (int)nf, e->width, e->height, e->tm_w, e->tm_h, e->ftiles.as<uint8_t>() + f0 * per * 256,
                       e->fflags.as<uint8_t>() + f0 * per, e->flab.as<uint8_t>() + f0 * per * 12, e->stream);
  };
  if (e->frames_host) {
    // The clip sits in host memory: chunks of frames cross PCIe on a copy stream while the Load kernel works on the chunk before
    // (pinned memory makes the copies asynchronous; pageable memory still works, serialised by the runtime).  A clip that
    // tm_prefetch_frames_host already queued is adopted instead: its copies ran beside the previous clip's steps.
    int slot = -1;
    for (int i = 0; i < 2; i++)
      if (e->hclip[i].pending && e->hclip[i].host == e->frames_host && (slot < 0 || e->hclip[i].seq < e->hclip[slot].seq)) slot = i;
    if (slot < 0) {
      // no prefetch of this clip: any buffer that holds no waiting clip will do (the last Load's own included: its clip is being
      // replaced); with two other clips waiting the older one is dropped (the copy stream orders the new copies behind its own)
      for (int i = 0; i < 2; i++)
        if (!e->hclip[i].pending && (slot < 0 || i != e->hclip_cur)) slot = i;
      if (slot < 0) slot = e->hclip[0].seq < e->hclip[1].seq ? 0 : 1;
      TM_HIP(host_sync(e->stream));       // the destination may have been handed out by the pool a moment ago
      TM_TRY(queue_host_clip(e, slot, e->frames_host));
    }
    tm_encoder::HostClip &hc = e->hclip[slot];
    // chunks that have already arrived (a prefetched clip: all of them, as a rule) go through ONE launch; the rest follow chunk by chunk
    int arrived = 0;
    while (arrived < hc.nchunks && hipEventQuery(hc.events[arrived]) == hipSuccess) arrived++;
    (void)hipGetLastError();  // (hipErrorNotReady of the first chunk still in flight is not an error)
    if (arrived > 0) {
      TM_HIP(hipStreamWaitEvent(e->stream, hc.events[arrived - 1], 0));
      TM_TRY(load_frames(hc.buf.p, 0, std::min(arrived * hc.chunk, e->nframes)));
    }
    for (int c = arrived; c < hc.nchunks; c++) {
      const int f0 = c * hc.chunk;
      TM_HIP(hipStreamWaitEvent(e->stream, hc.events[c], 0));
      TM_TRY(load_frames(hc.buf.p, f0, std::min(hc.chunk, e->nframes - f0)));
    }
    // From here on the encoder reads its own device copy: the host clip is no longer borrowed once this Load has returned (it
    // synchronises below), and a later Run(esLoad) without new frames reads the copy again.
    hc.pending = false;
    e->hclip_cur = slot;
    e->frames = hc.buf.p;
    e->frames_host = nullptr;
  } else if (own_frames_only) {
    // One process per GPU, motion prediction off: every process loads its own frames (frames are independent, 1293-1411) plus the
    // one before them, whose Lab means the first correlation needs.  The mirror flags (read back with every tile map) and the
    // correlation sums are merged; the frame tiles stay where they are -- Reduce and Reconstruct only need a process's own.
    int64_t f0, f1;
    share_of(e->nframes, e->co.rank, e->co.world, &f0, &f1);
    const int64_t lo = std::max<int64_t>(f0 - 1, 0);
    TM_HIP(hipMemsetAsync(e->fflags.p, 0, (size_t)e->q, e->stream));
    if (f1 > f0) TM_TRY(load_frames(e->frames, lo, f1 - lo));
    if (lo < f0) TM_HIP(hipMemsetAsync(e->fflags.as<uint8_t>() + lo * per, 0, (size_t)per, e->stream));  // the neighbour's flags are its owner's to report
    e->load_sharded = true; e->load_first = (int)f0; e->load_count = (int)(f1 - f0);
  } else {
    TM_TRY(load_frames(e->frames, 0, e->nframes));
  }
  progress(e, TM_STEP_LOAD, 1, 3);
  e->src_tiles = true;
  // inter-frame correlation: one GPU thread per frame runs the reference's sequential Single sums (order matters)
  const int lab_per = (int)per * 3;  // Lab means of a frame
  DevBuf &dcorrel = e->dcorrel;
  TM_TRY(dcorrel.alloc((size_t)e->nframes * 12));
  e->h_fflags.clear();  // fetched lazily by tm_get_tilemap
  e->kf_lo_thres = e->s.ShotTransCorrelLoThres; e->kf_min_s = e->s.ShotTransMinSecondsPerKF; e->kf_max_s = e->s.ShotTransMaxSecondsPerKF; e->kf_fps = e->fps;
  e->kf_manual = e->input.kind == TM_INPUT_PNGS || e->input.kind == TM_INPUT_JPEGS;
  e->kf_manual_list = e->kf_manual ? e->input.manual_kf : std::vector<int32_t>();
  if (e->load_sharded) {
    const int64_t f0 = e->load_first, f1 = f0 + e->load_count, lo = std::max<int64_t>(f0 - 1, 0);
    TM_HIP(hipMemsetAsync(dcorrel.p, 0, (size_t)e->nframes * 12, e->stream));
    // block b of the launch correlates frame lo + b with the one before it (block 0 has none): frames f0 .. f1-1 (frame 0 has no sum)
    if (f1 > f0) TM_TRY(launch_pearson(e->flab.as<uint8_t>() + lo * lab_per * 4, (int)(f1 - lo), lab_per, dcorrel.as<uint8_t>() + lo * 12, e->stream));
    if (lo < f0) TM_HIP(hipMemsetAsync(dcorrel.as<uint8_t>() + lo * 12, 0, 12, e->stream));
    TM_TRY(e->co.allreduce_sum_i32(dcorrel.p, (int64_t)e->nframes * 3));  // owner holds the float, everyone else +0.0: exact
    TM_TRY(e->co.allreduce_sum_i32(e->fflags.p, (e->q + 3) / 4));
    TM_HIP(host_sync(e->stream));
    e->load_tail_pending = true;
    TM_TRY(load_tail(e, e->stream));  // (the sums sit behind the encoder's own stream here)
  } else {
    if (!e->stream_aux) TM_HIP(hipStreamCreateWithFlags(&e->stream_aux, hipStreamNonBlocking));
    if (!e->ev_tiles) TM_HIP(hipEventCreateWithFlags(&e->ev_tiles, hipEventDisableTiming));
    TM_HIP(hipEventRecord(e->ev_tiles, e->stream));
    TM_HIP(hipStreamWaitEvent(e->stream_aux, e->ev_tiles, 0));
    TM_TRY(launch_pearson(e->flab.p, e->nframes, lab_per, dcorrel.p, e->stream_aux));
    e->load_tail_pending = true;
  }
  progress(e, TM_STEP_LOAD, 2, 3);
  if (e->auto_tile_count || e->s.GlobalTilingTileCount <= 0) recompute_auto_tile_count(e);
  // tile map starts empty (InitFrames, 2661-2686)
  TM_TRY(e->tm_tile.alloc((size_t)e->q * 4));
  TM_TRY(e->tm_pal.alloc((size_t)e->q * 4));
  TM_TRY(e->tm_err.alloc((size_t)e->q * 4));
  TM_HIP(hipMemsetAsync(e->tm_tile.p, 0xff, (size_t)e->q * 4, e->stream));
  TM_HIP(hipMemsetAsync(e->tm_pal.p, 0xff, (size_t)e->q * 4, e->stream));
  TM_HIP(hipMemsetAsync(e->tm_err.p, 0xff, (size_t)e->q * 4, e->stream));
  e->t = 0;
  e->has_pal_px = e->reconstructed = e->has_pm = false;
  TM_HIP(host_sync(e->stream));  // Run(esLoad) is blocking for everything but the correlation above (and the stage times stay the stages')
  std::vector<uint32_t>().swap(e->input_clip);  // (a PNG sequence's host copy: the device holds it now)
  progress(e, TM_STEP_LOAD, 3, 3);
  return TM_OK;
}

static int step_predict_motion(tm_encoder *e) {
  // PredictMotion, tilingencoder.pas:1964-1991: frame 0 is searched in frame 1, frame f >= 1 in the SOURCE pixels of
  // frame f-1 (the front buffer is drawn from the un-mirrored frame tiles, 1255-1260), so frames are independent.
  TM_TRY(need(e, TM_STEP_LOAD, "Load"));
  e->has_pm = false;
  if (e->s.MotionPredictRadius <= 0) return TM_OK;  // 1972
  TM_TRY(need_frame_tiles(e, "PredictMotion"));
  TM_CHECK(!e->load_sharded, TM_E_INVAL, "PredictMotion: Load ran with motion prediction off and only brought this process's frames; run Load again");
  const int64_t per = e->tm_size();
  TM_TRY(e->pm_err.alloc((size_t)e->q * 4));
  TM_TRY(e->tm_px.alloc((size_t)e->q + 4));  // (+4: merged as 32-bit words)
  TM_TRY(e->tm_py.alloc((size_t)e->q + 4));
  TM_TRY(e->tm_pred.alloc((size_t)e->q + 4));
  TM_TRY(clear_items(e, TMA_PRED));  // nothing is predicted before Reduce
  int sf, sn;
  if (query_range(e, &sf, &sn)) TM_TRY(clear_items(e, TMA_PM_ERR | TMA_PX | TMA_PY));  // frames of other shards
  MotionScratch ms;
  TM_TRY(ms.alloc(e, 1));
  for (int f = sf; f < sf + sn; f++) {
    const int src = f >= 1 ? f - 1 : (e->nframes > 1 ? 1 : -1);
    if (src >= 0)
      TM_TRY(launch_tiles_to_screen(e->ftiles.as<uint8_t>() + (int64_t)src * per * 256, e->fflags.as<uint8_t>() + (int64_t)src * per, e->tm_w, e->tm_h, ms.screen[0].p, e->stream));
    else
      TM_HIP(hipMemsetAsync(ms.screen[0].p, 0, ms.screen_bytes, e->stream));  // a single frame is searched in a black buffer
    const int64_t off = (int64_t)f * per;
    TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + off * 256, per, e->fflags.as<uint8_t>() + off, TM_PVS_WEIGHTED_DCT, 0, ms.cur.p, e->stream));
    TM_TRY(launch_motion_search_fb(ms.cur.p, e->tm_w, e->tm_h, ms.screen[0].p, ms.win.p, e->s.MotionPredictRadius, e->pm_err.as<uint32_t>() + off,
                                   e->tm_px.as<int8_t>() + off, e->tm_py.as<int8_t>() + off, e->stream));
    if ((f & 15) == 15) progress(e, TM_STEP_PREDICT_MOTION, f, e->nframes);
  }
  if (e->gcomm && sf == 0)  // a device group reports from shard 0 only: the other shards' frames too, so that the sequence is the single run's
    for (int f = sn; f < e->nframes; f++)
      if ((f & 15) == 15) progress(e, TM_STEP_PREDICT_MOTION, f, e->nframes);
  if (e->dist()) TM_TRY(merge_items(e, TMA_PM_ERR | TMA_PX | TMA_PY));
  TM_HIP(host_sync(e->stream));
  e->has_pm = true;
  e->reconstructed = false;
  progress(e, TM_STEP_PREDICT_MOTION, e->nframes, e->nframes);
  return TM_OK;
}

static int step_prepare_palettes(tm_encoder *e) {  // PreparePalettes, tilingencoder.pas:1843-1871
  TM_TRY(need(e, TM_STEP_REDUCE, "Reduce"));
  TM_TRY(need_global_rgb(e, "PreparePalettes"));
  TM_CHECK(e->t > 0, TM_E_INVAL, "no global tiles");
  const bool dbg = knobs().pp_debug;  // wall time of the sub-steps (adds stream synchronisations)
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!dbg) return;
    (void)hipStreamSynchronize(e->stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[tm_pp] %-28s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  DevBuf feat;
  e->pair_keys_n = 0;
  TM_TRY(e->gpal_idx.alloc((size_t)e->t * 4));
  TM_TRY(e->palettes_dev.alloc((size_t)e->s.PaletteCount * e->s.PaletteSize * 4));
  // One process per GPU.  Tile -> palette: every process holds the clustering features of its own share of the global tiles; the
  // farthest-first picks are settled by an all-gather of one candidate per process and the Lloyd iterations by an all-reduce
  // of the exact integer sums (run_palettize_dist), then the palette indices of all shares are all-gathered.  Palette colours:
  // the palettes are independent tasks (one thread per palette in the reference, 1864): process r quantises the palettes
  // p = r (mod world), an all-reduce(SUM) assembles the set.
  // Up to 16 palettes and half a million tiles, though, the single-GPU clustering is ONE resident launch of a few milliseconds (k_h_resident),
  // and every process holds all the global tiles: each runs it whole.  Sharded, a Lloyd iteration is an all-reduce of 25 KB -- 300 latency-bound
  // collectives on the bench clip, more than the whole clustering takes here -- plus two all-gathers per seeding pick; replicated there is none.
  // Integer sums and a fixed seed: every process ends with the same palettes.  (TM_PP_SHARDED=1 keeps the data-parallel form for A/B and tests.)
  const bool whole = !e->dist() || (e->pp_whole >= 0 ? e->pp_whole != 0 : !knobs().pp_sharded && palettize_resident(e->t, e->s.PaletteCount));
  if (whole) {
    TM_TRY(feat.alloc((size_t)e->t * 192 * 4));
    TM_TRY(launch_features_cluster(e->gtiles.p, e->t, e->s.DitheringMode, feat.p, e->stream));
    lap("cluster features (all tiles)");
    TM_TRY(run_palettize(feat.p, e->guse.p, e->t, e->s.PaletteCount, 300, e->gpal_idx.p, e->stream));
    lap("tile -> palette (192-D)");
  } else {
    int64_t t0, t1;
    share_of(e->t, e->co.rank, e->co.world, &t0, &t1);
    const int64_t nl = t1 - t0;
    TM_TRY(alloc_rows(feat, nl, 192 * 4));
    if (nl > 0) TM_TRY(launch_features_cluster(e->gtiles.as<uint8_t>() + t0 * 256, nl, e->s.DitheringMode, feat.p, e->stream));
    lap("cluster features (own share)");
    DevBuf lidx, all;
    TM_TRY(alloc_rows(lidx, nl, 4));
    TM_TRY(run_palettize_dist(feat.p, e->guse.as<uint8_t>() + t0 * 4, nl, t0, e->s.PaletteCount, 300, lidx.p, e->co, e->stream));
    std::vector<int64_t> counts;
    TM_TRY(gather_var(e, lidx.p, nl, 4, all, &counts));
    TM_HIP(hipMemcpyAsync(e->gpal_idx.p, all.p, (size_t)e->t * 4, hipMemcpyDeviceToDevice, e->stream));
    lap("tile -> palette (192-D, data-parallel)");
  }
  progress(e, TM_STEP_PREPARE_PALETTES, 1, 3);
  e->palettes_host.resize((size_t)e->s.PaletteCount * e->s.PaletteSize);
  if (e->dist()) {
    TM_TRY(run_quantize_palettes_part(e->gtiles.p, e->gpal_idx.p, e->t, e->s.PaletteCount, e->s.PaletteSize, 300, e->palettes_dev.p, e->co.rank, e->co.world, e->stream));
    TM_TRY(e->co.allreduce_sum_i32(e->palettes_dev.p, (int64_t)e->s.PaletteCount * e->s.PaletteSize));
    lap("palette colours (3-D, own palettes)");
    HostRead hr_(e->stream);
    TM_TRY(hr_.get(e->palettes_host.data(), e->palettes_dev.p, e->palettes_host.size() * 4));
    TM_TRY(hr_.wait());
  } else {
    // the quantisation ends on the host and OptimizePalettes goes on there: the palettes stay in palettes_host, and palettes_dev is written
    // once, below
    TM_TRY(run_quantize_palettes(e->gtiles.p, e->gpal_idx.p, e->t, e->s.PaletteCount, e->s.PaletteSize, 300, nullptr, e->stream, &e->pair_keys, &e->pair_keys_n,
                                 e->palettes_host.data()));
    e->km_stats = kmeans_run_stats();
    lap("palette colours (3-D)");
  }
  progress(e, TM_STEP_PREPARE_PALETTES, 2, 3);
  TM_TRY(prefetch_query_features(e));  // the GPU has nothing to do while the host searches: Reconstruct's query features run now
  lap("prefetch launch");
  // OptimizePalettes (4309-4432): slot permutation by Powell on the host (P x PaletteSize colours)
  TM_TRY(optimize_palettes_host(e->palettes_host, e->s.PaletteCount, e->s.PaletteSize, nullptr));
  lap("OptimizePalettes (host)");
  // (the source is an encoder member and outlives the copy; the wait ends the step: Run(esPreparePalettes) is blocking like the other steps)
  TM_HIP(hipMemcpyAsync(e->palettes_dev.p, e->palettes_host.data(), e->palettes_host.size() * 4, hipMemcpyHostToDevice, e->stream));
  TM_HIP(host_sync(e->stream));
  progress(e, TM_STEP_PREPARE_PALETTES, 3, 3);
  return TM_OK;
}

static int step_dither(tm_encoder *e) {  // Dither, tilingencoder.pas:1873-1907
  TM_TRY(need(e, TM_STEP_PREPARE_PALETTES, "PreparePalettes"));
  TM_TRY(need_global_rgb(e, "Dither"));
  TM_TRY(e->gpal_px.alloc((size_t)e->t * 64));
  const int64_t t0 = e->t * e->dither_rank / e->dither_world, t1 = e->t * (e->dither_rank + 1) / e->dither_world;
  if (e->dither_world > 1) TM_HIP(hipMemsetAsync(e->gpal_px.p, 0, (size_t)e->t * 64, e->stream));  // other shards' tiles: 0, merged with SUM
  e->dither_pairs = 0;
  if (t1 > t0)
    TM_TRY(launch_dither(e->gtiles.as<uint8_t>() + t0 * 256, e->gflags.as<uint8_t>() + t0, e->gpal_idx.as<uint8_t>() + t0 * 4, t1 - t0, e->palettes_dev.p,
                         e->s.PaletteCount, e->s.PaletteSize, e->s.DitheringUseThomasKnoll ? 1 : 0, e->s.DitheringYliluoma2MixedColors,
                         e->gpal_px.as<uint8_t>() + t0 * 64, e->stream, &e->dither_pairs, e->pair_keys_n > 0 && !knobs().dither_own_keys ? e->pair_keys.p : nullptr,
                         e->pair_keys_n));
  if (e->dist() && e->dither_world > 1) TM_TRY(e->co.allreduce_sum_i32(e->gpal_px.p, e->t * 16));  // 64 bytes per tile = 16 words; other shares hold 0
  TM_HIP(host_sync(e->stream));
  e->has_pal_px = true;
  progress(e, TM_STEP_DITHER, 2, 2);
  return TM_OK;
}

static int step_reindex(tm_encoder *e) {  // Reindex, tilingencoder.pas:1993-2038
  TM_TRY(need(e, TM_STEP_RECONSTRUCT, "Reconstruct"));
  DevBuf hist, remap, order, use;
  TM_TRY(hist.alloc((size_t)e->t * 4)); TM_TRY(remap.alloc((size_t)e->t * 4)); TM_TRY(order.alloc((size_t)e->t * 4)); TM_TRY(use.alloc((size_t)e->t * 4));
  // UseCount recount from the tile maps (2018-2031); MakeTilesUnique(False) merges by palette-index content and
  // sums the counts of merged tiles -- same totals as counting after the merge remap
  {  // one histogram copy per XCD, folded afterwards ("Atomics across XCDs")
    DevBuf h8;
    TM_TRY(h8.alloc((size_t)e->t * 4 * 8));
    TM_HIP(hipMemsetAsync(h8.p, 0, (size_t)e->t * 4 * 8, e->stream));
    hipLaunchKernelGGL(k_histogram_xcd, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, h8.as<uint32_t>(), (int64_t)e->t);
    hipLaunchKernelGGL(k_hist_fold, dim3(gridn(e->t)), dim3(256), 0, e->stream, h8.as<uint32_t>(), (int64_t)e->t, hist.as<uint32_t>());
    TM_TRY(launched());
    // (h8 goes back to the pool with this scope; what takes it next is queued on this stream behind the fold)
  }
  int64_t nu = 0;
  TM_TRY(run_dedup(e->gpal_px.p, e->t, 64, hist.p, remap.p, order.p, use.p, &nu, e->stream));
  progress(e, TM_STEP_REINDEX, 2, 3);
  DevBuf ntiles, nflags, npal_idx, npal_px, ntm;
  TM_TRY(ntiles.alloc((size_t)nu * 256)); TM_TRY(alloc_rows(nflags, nu, 1)); TM_TRY(npal_idx.alloc((size_t)nu * 4));
  TM_TRY(npal_px.alloc((size_t)nu * 64)); TM_TRY(ntm.alloc((size_t)e->q * 4));
  TM_TRY(gather_rows(e, e->gtiles.p, order.p, nu, 256, ntiles.p));
  TM_TRY(gather_rows(e, e->gpal_px.p, order.p, nu, 64, npal_px.p));
  TM_TRY(gather<uint8_t>(e, e->gflags.p, order.p, nu, nflags.p));
  TM_TRY(gather<int32_t>(e, e->gpal_idx.p, order.p, nu, npal_idx.p));
  TM_TRY(lookup(e, e->tm_tile.p, e->q, remap.p, ntm.p));
  TM_HIP(host_sync(e->stream));
  e->pair_keys_n = 0;
  e->gtiles = std::move(ntiles); e->gflags = std::move(nflags); e->gpal_idx = std::move(npal_idx); e->gpal_px = std::move(npal_px);
  e->tm_tile = std::move(ntm);
  e->guse = std::move(use);
  e->t = nu;
  progress(e, TM_STEP_REINDEX, 3, 3);
  return TM_OK;
}

int run_step(tm_encoder *e, int step) {
  TM_CHECK(!(e->gcomm && knobs().group_fail_shard == e->co.rank), TM_E_INVAL, "forced failure of shard %d (TM_GROUP_FAIL_SHARD)", e->co.rank);
  TM_HIP(hipSetDevice(e->device));
  const auto t0 = std::chrono::steady_clock::now();
  int rc = TM_OK;
  switch (step) {
    case TM_STEP_LOAD: rc = step_load(e); break;
    case TM_STEP_PREDICT_MOTION: rc = step_predict_motion(e); break;
    case TM_STEP_REDUCE: rc = step_reduce(e); break;
    case TM_STEP_PREPARE_PALETTES: rc = step_prepare_palettes(e); break;
    case TM_STEP_DITHER: rc = step_dither(e); break;
    case TM_STEP_RECONSTRUCT: rc = step_reconstruct(e); break;
    case TM_STEP_REINDEX: rc = step_reindex(e); break;
    case TM_STEP_SAVE: rc = save_to(e, e->s.OutputFileName.c_str()); break;
    default: set_error("bad step %d", step); rc = TM_E_INVAL;
  }
  if (rc == TM_OK) {
    e->stage_ms[step] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    e->steps_done |= 1 << step;
    for (int later = step + 1; later < 8; later++) e->steps_done &= ~(1 << later);  // later state is stale now
  }
  return rc;
}

extern "C" {

int tm_sync_tilemap(tm_encoder *e) {  // after shards were merged: TMI^.PalIdx := FTiles[TileIdx]^.PalIdx_Initial for every item
  TM_CHECK(e, TM_E_INVAL, "null encoder");
  TM_TRY(need(e, TM_STEP_RECONSTRUCT, "Reconstruct"));
  if (e->s.FrameTilingExtendedPaletteUsage) return TM_OK;  // the item's palette is the re-rank's choice: merged like TileIdx (array 2)
  TM_HIP(hipSetDevice(e->device));
  TM_TRY(pal_from_tile(e));
  TM_HIP(host_sync(e->stream));
  return TM_OK;
}

}  // extern "C"
