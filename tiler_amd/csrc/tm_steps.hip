// tm_steps.hip -- the steps of Run (tilingencoder.pas:5529-5554), Load .. Reindex, and the small kernels they launch.
//
// Every step reads and writes the encoder's device state (tm_encoder.h).  With one process per GPU or a device group (tm_shard.hip) a step
// works on its share and merges through the encoder's collectives (co); the sharded branches sit beside the single-process code they mirror.
#include <chrono>

#include "tm_encoder.h"

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
__global__ void k_clip_index(int32_t *__restrict__ idx, int64_t n, int32_t limit) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (idx[i] >= limit) idx[i] = -1;
}
__global__ void k_tilemap_from_subset(const int32_t *__restrict__ keep, const int32_t *__restrict__ pos, const int32_t *__restrict__ sub_remap,
                                      int64_t n, int32_t *__restrict__ tm_tile) {  // TransferTiles: TMI^.TileIdx := tIdx / -1 (4079-4083), then the remaps
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    tm_tile[i] = keep[i] ? sub_remap[pos[i]] : -1;
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
// sharded Reduce: one record per locally distinct tile = 64 pixel dwords + use count + mirror flags
__global__ void k_pack_unique(const uint32_t *__restrict__ tiles, const uint8_t *__restrict__ flags, const int32_t *__restrict__ order,
                              const uint32_t *__restrict__ use, int64_t n, uint32_t *__restrict__ rec) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * 66; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / 66;
    const int v = (int)(e - r * 66);
    rec[e] = v < 64 ? tiles[(int64_t)order[r] * 64 + v] : v == 64 ? use[r] : (uint32_t)flags[order[r]];
  }
}
__global__ void k_unpack_unique(const uint32_t *__restrict__ rec, int64_t n, uint32_t *__restrict__ tiles, uint32_t *__restrict__ use, uint8_t *__restrict__ flags) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n * 66; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / 66;
    const int v = (int)(e - r * 66);
    if (v < 64) tiles[r * 64 + v] = rec[e]; else if (v == 64) use[r] = rec[e]; else flags[r] = (uint8_t)rec[e];
  }
}

// a frame tile's global index through the candidates: its local distinct tile travelled (in_s) as candidate number cand_pos[.] of this
// process, which the exact dedup of all candidates mapped to cand_remap[.]; anything else is beyond the tile budget
__global__ void k_compose_remap_cand(const int32_t *__restrict__ local_remap, int64_t n, const uint32_t *__restrict__ in_s, const int32_t *__restrict__ cand_pos,
                                     const int32_t *__restrict__ cand_remap, int32_t cand_off, int32_t limit, int32_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = local_remap[i];
    int32_t g = -1;
    if (in_s[l]) g = cand_remap[cand_off + cand_pos[l]];
    out[i] = g >= 0 && g < limit ? g : -1;
  }
}

}  // namespace tmx

// ---- steps ---------------------------------------------------------------------------------------------------
// Steps that read the frame tiles / the global tiles' RGB pixels: ReloadGTM brings neither (the stream holds palette indices
// only, HasRGBPixels = False at tilingencoder.pas:4937), so after a reload these steps need Load (and Reduce) to have run again.
static int need_frame_tiles(tm_encoder *e, const char *step) {
  TM_CHECK(e->ftiles.p != nullptr && e->fflags.p != nullptr && e->flab.p != nullptr && e->q > 0, TM_E_INVAL,
           "step order: %s needs the frame tiles, which are not in memory (run Load first; ReloadGTM does not bring them)", step);
  return TM_OK;
}
static int need_global_rgb(tm_encoder *e, const char *step) {
  TM_CHECK(e->gtiles_have_rgb && e->gtiles.p != nullptr, TM_E_INVAL,
           "step order: %s needs the global tiles' RGB pixels (run Reduce first; a reloaded .gtm holds palette indices only)", step);
  return TM_OK;
}

// the query frames [sf, sf + sn) of this process (tm_set_query_shard), inside the clip
static void query_range(const tm_encoder *e, int *sf, int *sn) {
  *sf = std::max(0, std::min(e->shard_first, e->nframes));
  *sn = e->shard_count < 0 ? e->nframes - *sf : std::max(0, std::min(e->shard_count, e->nframes - *sf));
}

// the host tail of Load -- PearsonCorrelation's last lines (2221-2227) and FindKeyFrames (3373-3411) -- once the sums are there
int load_tail(tm_encoder *e) {
  if (!e->load_tail_pending) return TM_OK;
  std::vector<float> sums((size_t)e->nframes * 3);
  hipStream_t st = e->stream_aux ? e->stream_aux : e->stream;
  {
    HostRead hr_(st);
    TM_TRY(hr_.get(sums.data(), e->dcorrel.p, sums.size() * 4));
    TM_TRY(hr_.wait());
  }
  e->load_tail_pending = false;  // only now: a failed read-back leaves the tail to the next caller instead of stale key frames
  e->correl.assign(e->nframes, 0.0f);
  for (int f = 1; f < e->nframes; f++) {  // tail of PearsonCorrelation (2221-2227) in host IEEE arithmetic
    const float denx = std::sqrt(sums[f * 3 + 1]), deny = std::sqrt(sums[f * 3 + 2]);
    const float den = denx * deny;
    e->correl[f] = den != 0.0f ? sums[f * 3] / den : 1.0f;
  }
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

static int step_load(tm_encoder *e) {  // Load, tilingencoder.pas:1741-1841 (frames are pushed in, or decoded from InputFileName: tm_input.hip)
  TM_TRY(load_tail(e));  // (a correlation still running reads the Lab means this Load is about to replace)
  e->drop_prefetch();  // features of the previous frame tiles
  e->q_groups = 0;
  e->load_sharded = false;
  TM_CHECK(e->nframes > 0 && e->width > 0, TM_E_INVAL, "tm_set_video has not been called");
  if (e->input.kind) TM_TRY(load_from_input(e));  // the source "file": from here on as if the clip had been set with tm_set_frames_device / _host
  if (e->frames_peer) {
    // a device group's clip on another device (tm_set_frames_device): this shard pulls the frames its Load reads into its own memory
    const size_t fbytes = (size_t)e->width * e->height * 4;
    int64_t a = 0, b = e->nframes;
    if (e->dist() && e->s.MotionPredictRadius <= 0) {
      share_of(e->nframes, e->co.rank, e->co.world, &a, &b);
      a = std::max<int64_t>(a - 1, 0);
    }
    TM_TRY(e->frames_owned.alloc(fbytes * e->nframes));
    if (b > a) TM_HIP(hipMemcpyPeerAsync(e->frames_owned.as<uint8_t>() + fbytes * a, e->device, (const uint8_t *)e->frames_peer + fbytes * a, e->frames_peer_dev,
                                         fbytes * (b - a), e->stream));
    e->frames = e->frames_owned.p;
  }
  TM_CHECK(e->frames != nullptr || e->frames_host != nullptr, TM_E_INVAL, "no frames: call tm_push_frame_rgb32 / tm_set_frames_device / tm_set_frames_host first");
  e->q = (int64_t)e->nframes * e->tm_size();
  TM_CHECK(e->q < (1ll << 31), TM_E_UNSUPPORTED, "%lld tile-map items: the index arrays are 32-bit (TileIdx is an Integer, tilingencoder.pas:179)", (long long)e->q);
  TM_TRY(e->ftiles.alloc((size_t)e->q * 256));
  TM_TRY(e->fflags.alloc((size_t)e->q + 4));  // (+4: merged as 32-bit words)
  TM_TRY(e->flab.alloc((size_t)e->q * 12));
  if (e->frames_host) {
    // The clip sits in host memory: chunks of frames cross PCIe on a copy stream while the Load kernel works on the chunk before
    // (pinned memory makes the copies asynchronous; pageable memory still works, serialised by the runtime).  A clip that
    // tm_prefetch_frames_host already queued is adopted instead: its copies ran beside the previous clip's steps.
    const size_t fbytes = (size_t)e->width * e->height * 4;
    const int64_t per = e->tm_size();
    int slot = -1;
    for (int i = 0; i < 2; i++)
      if (e->hclip[i].pending && e->hclip[i].host == e->frames_host && (slot < 0 || e->hclip[i].seq < e->hclip[slot].seq)) slot = i;
    if (slot < 0) {
      // no prefetch of this clip: any buffer that holds no waiting clip will do (the last Load's own included: its clip is being
      // replaced); with two other clips waiting the older one is dropped (the copy stream orders the new copies behind its own)
      for (int i = 0; i < 2; i++)
        if (!e->hclip[i].pending && (slot < 0 || i != e->hclip_cur)) slot = i;
      if (slot < 0) slot = e->hclip[0].seq < e->hclip[1].seq ? 0 : 1;
      TM_HIP(hipStreamSynchronize(e->stream));       // the destination may have been handed out by the pool a moment ago
      TM_TRY(queue_host_clip(e, slot, e->frames_host));
    }
    tm_encoder::HostClip &hc = e->hclip[slot];
    // chunks that have already arrived (a prefetched clip: all of them, as a rule) go through ONE launch; the rest follow chunk by chunk
    int arrived = 0;
    while (arrived < hc.nchunks && hipEventQuery(hc.events[arrived]) == hipSuccess) arrived++;
    (void)hipGetLastError();  // (hipErrorNotReady of the first chunk still in flight is not an error)
    if (arrived > 0) {
      const int nf = std::min(arrived * hc.chunk, e->nframes);
      TM_HIP(hipStreamWaitEvent(e->stream, hc.events[arrived - 1], 0));
      TM_TRY(launch_load(hc.buf.p, nf, e->width, e->height, e->tm_w, e->tm_h, e->ftiles.p, e->fflags.p, e->flab.p, e->stream));
    }
    for (int c = arrived; c < hc.nchunks; c++) {
      const int f0 = c * hc.chunk, nf = std::min(hc.chunk, e->nframes - f0);
      TM_HIP(hipStreamWaitEvent(e->stream, hc.events[c], 0));
      TM_TRY(launch_load(hc.buf.as<uint8_t>() + fbytes * f0, nf, e->width, e->height, e->tm_w, e->tm_h, e->ftiles.as<uint8_t>() + (int64_t)f0 * per * 256,
                         e->fflags.as<uint8_t>() + (int64_t)f0 * per, e->flab.as<uint8_t>() + (int64_t)f0 * per * 12, e->stream));
    }
    // From here on the encoder reads its own device copy: the host clip is no longer borrowed once this Load has returned (it
    // synchronises below), and a later Run(esLoad) without new frames reads the copy again.
    hc.pending = false;
    e->hclip_cur = slot;
    e->frames = hc.buf.p;
    e->frames_host = nullptr;
  } else if (e->dist() && e->s.MotionPredictRadius <= 0) {
    // One process per GPU, motion prediction off: every process loads its own frames (frames are independent, 1293-1411) plus the
    // one before them, whose Lab means the first correlation needs.  The mirror flags (read back with every tile map) and the
    // correlation sums are merged; the frame tiles stay where they are -- Reduce and Reconstruct only need a process's own.
    const size_t fbytes = (size_t)e->width * e->height * 4;
    const int64_t per1 = e->tm_size();
    int64_t f0, f1;
    share_of(e->nframes, e->co.rank, e->co.world, &f0, &f1);
    const int64_t lo = std::max<int64_t>(f0 - 1, 0);
    TM_HIP(hipMemsetAsync(e->fflags.p, 0, (size_t)e->q, e->stream));
    if (f1 > f0)
      TM_TRY(launch_load((const uint8_t *)e->frames + fbytes * lo, (int)(f1 - lo), e->width, e->height, e->tm_w, e->tm_h, e->ftiles.as<uint8_t>() + lo * per1 * 256,
                         e->fflags.as<uint8_t>() + lo * per1, e->flab.as<uint8_t>() + lo * per1 * 12, e->stream));
    if (lo < f0) TM_HIP(hipMemsetAsync(e->fflags.as<uint8_t>() + lo * per1, 0, (size_t)per1, e->stream));  // the neighbour's flags are its owner's to report
    e->load_sharded = true; e->load_first = (int)f0; e->load_count = (int)(f1 - f0);
  } else
  TM_TRY(launch_load(e->frames, e->nframes, e->width, e->height, e->tm_w, e->tm_h, e->ftiles.p, e->fflags.p, e->flab.p, e->stream));
  progress(e, TM_STEP_LOAD, 1, 3);
  e->src_tiles = true;
  // inter-frame correlation: one GPU thread per frame runs the reference's sequential Single sums (order matters)
  const int per = (int)e->tm_size() * 3;
  DevBuf &dcorrel = e->dcorrel;
  TM_TRY(dcorrel.alloc((size_t)e->nframes * 12));
  e->h_fflags.clear();  // fetched lazily by tm_get_tilemap
  e->kf_lo_thres = e->s.ShotTransCorrelLoThres; e->kf_min_s = e->s.ShotTransMinSecondsPerKF; e->kf_max_s = e->s.ShotTransMaxSecondsPerKF; e->kf_fps = e->fps;
  e->kf_manual = e->input.kind == TM_INPUT_PNGS;
  e->kf_manual_list = e->kf_manual ? e->input.manual_kf : std::vector<int32_t>();
  if (e->load_sharded) {
    const int64_t f0 = e->load_first, f1 = f0 + e->load_count, lo = std::max<int64_t>(f0 - 1, 0);
    TM_HIP(hipMemsetAsync(dcorrel.p, 0, (size_t)e->nframes * 12, e->stream));
    // block b of the launch correlates frame lo + b with the one before it (block 0 has none): frames f0 .. f1-1 (frame 0 has no sum)
    if (f1 > f0) TM_TRY(launch_pearson(e->flab.as<uint8_t>() + lo * per * 4, (int)(f1 - lo), per, dcorrel.as<uint8_t>() + lo * 12, e->stream));
    if (lo < f0) TM_HIP(hipMemsetAsync(dcorrel.as<uint8_t>() + lo * 12, 0, 12, e->stream));
    TM_TRY(e->co.allreduce_sum_i32(dcorrel.p, (int64_t)e->nframes * 3));  // owner holds the float, everyone else +0.0: exact
    TM_TRY(e->co.allreduce_sum_i32(e->fflags.p, (e->q + 3) / 4));
    TM_HIP(hipStreamSynchronize(e->stream));
    hipStream_t keep = e->stream_aux;
    e->stream_aux = nullptr;  // (the sums sit behind the encoder's own stream here)
    e->load_tail_pending = true;
    const int rc = load_tail(e);
    e->stream_aux = keep;
    TM_TRY(rc);
  } else {
    if (!e->stream_aux) TM_HIP(hipStreamCreateWithFlags(&e->stream_aux, hipStreamNonBlocking));
    if (!e->ev_tiles) TM_HIP(hipEventCreateWithFlags(&e->ev_tiles, hipEventDisableTiming));
    TM_HIP(hipEventRecord(e->ev_tiles, e->stream));
    TM_HIP(hipStreamWaitEvent(e->stream_aux, e->ev_tiles, 0));
    TM_TRY(launch_pearson(e->flab.p, e->nframes, per, dcorrel.p, e->stream_aux));
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
  TM_HIP(hipStreamSynchronize(e->stream));  // Run(esLoad) is blocking for everything but the correlation above (and the stage times stay the stages')
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
  const int sw = e->tm_w * 8, sh = e->tm_h * 8;
  const int64_t nwin = (int64_t)(sw - 7) * (sh - 7);
  TM_TRY(e->pm_err.alloc((size_t)e->q * 4));
  TM_TRY(e->tm_px.alloc((size_t)e->q + 4));  // (+4: merged as 32-bit words)
  TM_TRY(e->tm_py.alloc((size_t)e->q + 4));
  TM_TRY(e->tm_pred.alloc((size_t)e->q + 4));
  TM_HIP(hipMemsetAsync(e->tm_pred.p, 0, (size_t)e->q, e->stream));
  int sf, sn;
  query_range(e, &sf, &sn);
  if (sf > 0 || sn < e->nframes) {  // frames of other shards stay 0: the host merges shards with all-reduce(SUM)
    TM_HIP(hipMemsetAsync(e->pm_err.p, 0, (size_t)e->q * 4, e->stream));
    TM_HIP(hipMemsetAsync(e->tm_px.p, 0, (size_t)e->q, e->stream));
    TM_HIP(hipMemsetAsync(e->tm_py.p, 0, (size_t)e->q, e->stream));
  }
  DevBuf screen, win, cur;
  TM_TRY(screen.alloc((size_t)sw * sh * 4));
  TM_TRY(win.alloc((size_t)nwin * 384));
  TM_TRY(cur.alloc((size_t)per * 384));
  for (int f = sf; f < sf + sn; f++) {
    const int src = f >= 1 ? f - 1 : (e->nframes > 1 ? 1 : -1);
    if (src >= 0) TM_TRY(launch_tiles_to_screen(e->ftiles.as<uint8_t>() + (int64_t)src * per * 256, e->fflags.as<uint8_t>() + (int64_t)src * per, e->tm_w, e->tm_h, screen.p, e->stream));
    else TM_HIP(hipMemsetAsync(screen.p, 0, (size_t)sw * sh * 4, e->stream));  // a single frame is searched in a black buffer
    const int64_t off = (int64_t)f * per;
    TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + off * 256, per, e->fflags.as<uint8_t>() + off, TM_PVS_WEIGHTED_DCT, 0, cur.p, e->stream));
    TM_TRY(launch_motion_search_fb(cur.p, e->tm_w, e->tm_h, screen.p, win.p, e->s.MotionPredictRadius, e->pm_err.as<uint32_t>() + off,
                                   e->tm_px.as<int8_t>() + off, e->tm_py.as<int8_t>() + off, e->stream));
    if ((f & 15) == 15) progress(e, TM_STEP_PREDICT_MOTION, f, e->nframes);
  }
  if (e->gcomm && sf == 0)  // a device group reports from shard 0 only: the other shards' frames too, so that the sequence is the single run's
    for (int f = sn; f < e->nframes; f++)
      if ((f & 15) == 15) progress(e, TM_STEP_PREDICT_MOTION, f, e->nframes);
  if (e->dist()) {  // owner holds the value, everyone else 0
    TM_TRY(e->co.allreduce_sum_i32(e->pm_err.p, e->q));
    TM_TRY(e->co.allreduce_sum_i32(e->tm_px.p, (e->q + 3) / 4));
    TM_TRY(e->co.allreduce_sum_i32(e->tm_py.p, (e->q + 3) / 4));
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  e->has_pm = true;
  e->reconstructed = false;
  progress(e, TM_STEP_PREDICT_MOTION, e->nframes, e->nframes);
  return TM_OK;
}

// Reduce's last move on every path: rows order[0 .. t) of (tiles, flags) become the global tiles, use[0 .. t) their use counts
static int adopt_global_tiles(tm_encoder *e, const void *tiles, const void *flags, const void *order, const void *use) {
  e->pair_keys_n = 0;
  TM_TRY(e->gtiles.alloc((size_t)e->t * 256));
  TM_TRY(e->gflags.alloc((size_t)std::max<int64_t>(e->t, 1)));
  TM_TRY(e->guse.alloc((size_t)e->t * 4));
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(e->t * 16)), dim3(256), 0, e->stream, (const uint4 *)tiles, (const int32_t *)order, e->t, 16,
                     e->gtiles.as<uint4>());
  hipLaunchKernelGGL(k_gather<uint8_t>, dim3(gridn(e->t)), dim3(256), 0, e->stream, (const uint8_t *)flags, (const int32_t *)order, e->t,
                     e->gflags.as<uint8_t>());
  TM_HIP(hipMemcpyAsync(e->guse.p, use, (size_t)e->t * 4, hipMemcpyDeviceToDevice, e->stream));
  return TM_OK;
}

static int step_reduce_motion(tm_encoder *e) {
  TM_TRY(load_tail(e));
  // Reduce with motion prediction (1909-1926): SolveTileCount searches the PSNR threshold above which a tile-map item
  // stays predicted (4014-4046); the items below it are transferred (4048-4103), made unique and ordered (4038, 1923).
  // The search runs on per-group maxima of the prediction error (a group = one distinct tile content): PSNR is a
  // non-increasing function of the error, so "some member has PSNR <= x" is "the group's largest error exceeds the
  // largest error still predicted at x".  The state kept is the last probe's, as in the reference.
  // GlobalTilingUseTargetPSNR (1916-1919): no search, one STCGREval probe at GlobalTilingTargetPSNR; the tile count is what it leaves.
  const int64_t per = e->tm_size();
  DevBuf kfmask, keep, sel, pos;
  std::vector<uint8_t> hk((size_t)e->nframes, 0);
  for (int32_t k : e->kf_start) hk[(size_t)k] = 1;
  TM_TRY(kfmask.alloc(hk.size()));
  TM_HIP(hipMemcpyAsync(kfmask.p, hk.data(), hk.size(), hipMemcpyHostToDevice, e->stream));
  TM_TRY(keep.alloc((size_t)e->q * 4)); TM_TRY(sel.alloc((size_t)e->q * 4)); TM_TRY(pos.alloc((size_t)e->q * 4));
  if (e->s.GlobalTilingUseTargetPSNR) {
    e->reduce_threshold = e->s.GlobalTilingTargetPSNR;
    e->reduce_probes = 1;
    TM_TRY(mark_at_threshold(e->pm_err.p, kfmask.p, (int)per, e->q, e->reduce_threshold, e->tm_pred.p, keep.p, e->stream));
  } else {
    DevBuf remap, order, use;
    TM_TRY(remap.alloc((size_t)e->q * 4)); TM_TRY(order.alloc((size_t)e->q * 4)); TM_TRY(use.alloc((size_t)e->q * 4));
    int64_t ngroups = 0;
    TM_TRY(run_dedup(e->ftiles.p, e->q, 256, nullptr, remap.p, order.p, use.p, &ngroups, e->stream));
    const double target = e->s.GlobalTilingTileCount > 0 ? (double)e->s.GlobalTilingTileCount : (double)ngroups;
    TM_TRY(solve_tile_count(remap.p, ngroups, e->pm_err.p, kfmask.p, (int)per, e->q, target, e->tm_pred.p, keep.p, &e->reduce_threshold,
                            &e->reduce_probes, e->stream));
  }
  progress(e, TM_STEP_REDUCE, 1, 2);
  int64_t nkeep = 0;
  TM_TRY(compact_kept(keep.p, e->q, sel.p, pos.p, &nkeep, e->stream));
  TM_CHECK(nkeep > 0, TM_E_INVAL, "Reduce: every tile is predicted, no global tile left");
  DevBuf sub, sremap, sorder, suse;
  TM_TRY(sub.alloc((size_t)nkeep * 256)); TM_TRY(sremap.alloc((size_t)nkeep * 4)); TM_TRY(sorder.alloc((size_t)nkeep * 4)); TM_TRY(suse.alloc((size_t)nkeep * 4));
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(nkeep * 16)), dim3(256), 0, e->stream, e->ftiles.as<uint4>(), sel.as<int32_t>(), nkeep, 16, sub.as<uint4>());
  int64_t nu = 0;
  TM_TRY(run_dedup(sub.p, nkeep, 256, nullptr, sremap.p, sorder.p, suse.p, &nu, e->stream));
  e->t = nu;
  DevBuf gsrc;  // global tile -> frame tile index
  TM_TRY(gsrc.alloc((size_t)e->t * 4));
  hipLaunchKernelGGL(k_gather<int32_t>, dim3(gridn(e->t)), dim3(256), 0, e->stream, sel.as<int32_t>(), sorder.as<int32_t>(), e->t, gsrc.as<int32_t>());
  TM_TRY(adopt_global_tiles(e, e->ftiles.p, e->fflags.p, gsrc.p, suse.p));
  hipLaunchKernelGGL(k_tilemap_from_subset, dim3(gridn(e->q)), dim3(256), 0, e->stream, keep.as<int32_t>(), pos.as<int32_t>(), sremap.as<int32_t>(),
                     e->q, e->tm_tile.as<int32_t>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  e->has_pal_px = e->reconstructed = false;
  progress(e, TM_STEP_REDUCE, 2, 2);
  return TM_OK;
}

// the Reduce tile budget without motion prediction, 0 = none.  With GlobalTilingUseTargetPSNR no item has a motion PSNR to exceed the
// target, so STCGREval predicts nothing and every distinct tile stays (GlobalTilingTileCount plays no part, 1916-1919).
static int64_t tile_budget(const tm_encoder *e) {
  if (e->s.GlobalTilingUseTargetPSNR) return 0;
  return e->s.GlobalTilingTileCount > 0 ? (int64_t)e->s.GlobalTilingTileCount : 0;
}

static int step_reduce(tm_encoder *e) {
  // Reduce, tilingencoder.pas:1909-1926 = SolveTileCount (4043) + ReindexTiles(True).  After PredictMotion the threshold
  // search of step_reduce_motion runs.  With motion prediction switched off (MotionPredictRadius = 0, the benchmark's headline
  // configuration) no tile-map item is predicted, so TransferTiles (4048) moves every frame tile; MakeTilesUnique(True) +
  // ReindexTiles(True) are exact; the tile budget is then met by keeping the first GlobalTilingTileCount tiles of
  // that order (most used first), see DESIGN.md "Scope".
  TM_TRY(need(e, TM_STEP_LOAD, "Load"));
  TM_TRY(need_frame_tiles(e, "Reduce"));
  e->gtiles_have_rgb = true;
  e->q_groups = 0;
  e->drop_prefetch();
  if (e->has_pm) return step_reduce_motion(e);
  if (e->load_sharded) {
    // One process per GPU: exact dedup of this process's own frame tiles first, then of the union of every process's distinct
    // tiles (all-gathered: tile, use count, mirror flags of its first occurrence).  Processes own increasing frame ranges and the
    // union is laid out in process order, so "first occurrence" and the final order (use count descending, content ascending)
    // are those of the single-process run.
    const int64_t per = e->tm_size(), f0 = e->load_first, nloc = (int64_t)e->load_count * per;
    DevBuf lremap, lorder, luse, rec, urec, utiles, uuse, uflags, gremap, gorder, guse2;
    int64_t lnu = 0;
    TM_TRY(lremap.alloc((size_t)std::max<int64_t>(nloc, 1) * 4)); TM_TRY(lorder.alloc((size_t)std::max<int64_t>(nloc, 1) * 4)); TM_TRY(luse.alloc((size_t)std::max<int64_t>(nloc, 1) * 4));
    if (nloc > 0) TM_TRY(run_dedup(e->ftiles.as<uint8_t>() + f0 * per * 256, nloc, 256, nullptr, lremap.p, lorder.p, luse.p, &lnu, e->stream));
    // What travels: only the tiles that can be among the first GlobalTilingTileCount of the merged order, chosen on 16-byte keys every
    // process exchanges first (tm_dedup.hip, "Reduce over several processes"; gathering every distinct tile of every process, as the
    // first two rounds did, moved 857 MB on the bench clip).
    const int64_t budget = tile_budget(e);  // 0: no budget, everything stays
    DevBuf lkeys, allkeys, in_s, sel, spos, sidx, suse;
    int64_t nsel = lnu, key_off = 0;
    {
      TM_TRY(lkeys.alloc((size_t)std::max<int64_t>(lnu, 1) * 16));
      TM_TRY(reduce_make_keys(e->ftiles.as<uint8_t>() + f0 * per * 256, lorder.p, luse.p, lnu, 256, lkeys.p, e->stream));
      std::vector<int64_t> kcounts;
      TM_TRY(gather_var(e, lkeys.p, lnu, 16, allkeys, &kcounts));
      int64_t ntot = 0;
      for (int r = 0; r < e->co.world; r++) { if (r < e->co.rank) key_off += kcounts[r]; ntot += kcounts[r]; }
      TM_CHECK(ntot > 0 && ntot < (1ll << 31), TM_E_INVAL, "Reduce: %lld distinct tiles over all processes", (long long)ntot);
      TM_TRY(in_s.alloc((size_t)ntot * 4));
      TM_TRY(reduce_select_candidates(allkeys.p, ntot, budget, in_s.p, e->stream));
      TM_TRY(sel.alloc((size_t)std::max<int64_t>(lnu, 1) * 4)); TM_TRY(spos.alloc((size_t)std::max<int64_t>(lnu, 1) * 4));
      nsel = 0;
      if (lnu > 0) TM_TRY(compact_kept(in_s.as<uint32_t>() + key_off, lnu, sel.p, spos.p, &nsel, e->stream));
      TM_TRY(sidx.alloc((size_t)std::max<int64_t>(nsel, 1) * 4)); TM_TRY(suse.alloc((size_t)std::max<int64_t>(nsel, 1) * 4));
      if (nsel > 0) {
        hipLaunchKernelGGL(k_gather<int32_t>, dim3(gridn(nsel)), dim3(256), 0, e->stream, lorder.as<int32_t>(), sel.as<int32_t>(), nsel, sidx.as<int32_t>());
        hipLaunchKernelGGL(k_gather<uint32_t>, dim3(gridn(nsel)), dim3(256), 0, e->stream, luse.as<uint32_t>(), sel.as<int32_t>(), nsel, suse.as<uint32_t>());
      }
    }
    TM_TRY(rec.alloc((size_t)std::max<int64_t>(nsel, 1) * 264));
    if (nsel > 0)
      hipLaunchKernelGGL(k_pack_unique, dim3(gridn(nsel * 66)), dim3(256), 0, e->stream, e->ftiles.as<uint32_t>() + f0 * per * 64, e->fflags.as<uint8_t>() + f0 * per,
                         sidx.as<int32_t>(), suse.as<uint32_t>(), nsel, rec.as<uint32_t>());
    TM_HIP(hipGetLastError());
    std::vector<int64_t> counts;
    TM_TRY(gather_var(e, rec.p, nsel, 264, urec, &counts));
    int64_t nun = 0, my_off = 0;
    for (int r = 0; r < e->co.world; r++) { if (r < e->co.rank) my_off += counts[r]; nun += counts[r]; }
    TM_CHECK(nun > 0 && nun < (1ll << 31), TM_E_INVAL, "Reduce: %lld distinct tiles over all processes", (long long)nun);
    TM_TRY(utiles.alloc((size_t)nun * 256)); TM_TRY(uuse.alloc((size_t)nun * 4)); TM_TRY(uflags.alloc((size_t)nun));
    hipLaunchKernelGGL(k_unpack_unique, dim3(gridn(nun * 66)), dim3(256), 0, e->stream, urec.as<uint32_t>(), nun, utiles.as<uint32_t>(), uuse.as<uint32_t>(), uflags.as<uint8_t>());
    TM_HIP(hipGetLastError());
    TM_TRY(gremap.alloc((size_t)nun * 4)); TM_TRY(gorder.alloc((size_t)nun * 4)); TM_TRY(guse2.alloc((size_t)nun * 4));
    int64_t nu = 0;
    TM_TRY(run_dedup(utiles.p, nun, 256, uuse.p, gremap.p, gorder.p, guse2.p, &nu, e->stream));
    progress(e, TM_STEP_REDUCE, 1, 2);
    const int64_t target = tile_budget(e) > 0 ? tile_budget(e) : nu;
    e->t = std::min<int64_t>(nu, target);
    TM_TRY(adopt_global_tiles(e, utiles.p, uflags.p, gorder.p, guse2.p));
    // tile map of this process's frames (TransferTiles: TileIdx := the tile's index, 4079-4083); the other frames' items are their owners'
    TM_HIP(hipMemsetAsync(e->tm_tile.p, 0xff, (size_t)e->q * 4, e->stream));
    if (nloc > 0)
      hipLaunchKernelGGL(k_compose_remap_cand, dim3(gridn(nloc)), dim3(256), 0, e->stream, lremap.as<int32_t>(), nloc, in_s.as<uint32_t>() + key_off, spos.as<int32_t>(),
                         gremap.as<int32_t>(), (int32_t)my_off, (int32_t)e->t, e->tm_tile.as<int32_t>() + f0 * per);
    TM_HIP(hipGetLastError());
    TM_HIP(hipStreamSynchronize(e->stream));
    e->has_pal_px = e->reconstructed = false;
    progress(e, TM_STEP_REDUCE, 2, 2);
    return TM_OK;
  }
  DevBuf remap, order, use;
  TM_TRY(remap.alloc((size_t)e->q * 4));
  TM_TRY(order.alloc((size_t)e->q * 4));
  TM_TRY(use.alloc((size_t)e->q * 4));
  int64_t nu = 0;
  // (only the first GlobalTilingTileCount tiles of the order stay: the rows behind them are counted and numbered, not ordered)
  TM_TRY(run_dedup(e->ftiles.p, e->q, 256, nullptr, remap.p, order.p, use.p, &nu, e->stream, tile_budget(e)));
  progress(e, TM_STEP_REDUCE, 1, 2);
  int64_t target = tile_budget(e) > 0 ? tile_budget(e) : nu;
  e->t = std::min<int64_t>(nu, target);
  TM_TRY(adopt_global_tiles(e, e->ftiles.p, e->fflags.p, order.p, use.p));
  TM_HIP(hipMemcpyAsync(e->tm_tile.p, remap.p, (size_t)e->q * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(k_clip_index, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, (int32_t)e->t);
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  if (!knobs().no_query_groups) {  // kept for Reconstruct: one search per distinct frame tile
    e->q_group = std::move(remap);
    e->q_rep = std::move(order);
    e->q_groups = nu;
  }
  e->has_pal_px = e->reconstructed = false;
  progress(e, TM_STEP_REDUCE, 2, 2);
  return TM_OK;
}

// frames per chunk of Reconstruct's query features (bounded scratch for long / 4K clips: streaming through HBM)
static int recon_chunk_frames(const tm_encoder *e, int sn, bool epu) {
  const int64_t per = e->tm_size(), budget = epu ? ((int64_t)2 << 30) : ((int64_t)8 << 30);
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::max(sn, 1), budget / (per * 384)));
}

// may Reconstruct search once per distinct frame tile?  (the k = 1 search of the whole clip in one process, rows within one chunk)
static bool query_groups_usable(const tm_encoder *e, int sf, int sn, bool epu) {
  // (the extended-palette search keeps 64 candidates per query: 512 more bytes a row)
  return e->q_groups > 0 && !e->dist() && sf == 0 && sn == e->nframes && e->q_groups * (epu ? 384 + 512 : 384) <= ((int64_t)8 << 30);
}

static int prefetch_query_features(tm_encoder *e) {
  int sf, sn;
  query_range(e, &sf, &sn);
  if (sn <= 0) return TM_OK;
  const bool epu = e->s.FrameTilingExtendedPaletteUsage;
  const int nf = std::min(recon_chunk_frames(e, sn, epu), sn);
  const int64_t per = e->tm_size();
  e->drop_prefetch();
  const bool distinct = query_groups_usable(e, sf, sn, epu);
  if (!e->stream2) {  // lowest priority: the small dependent kernels of PreparePalettes must not queue behind this one's workgroups
    int lo = 0, hi = 0;
    TM_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    TM_HIP(hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, lo));
  }
  if (!e->ev_qf) TM_HIP(hipEventCreateWithFlags(&e->ev_qf, hipEventDisableTiming));
  TM_TRY(e->qf_pre.alloc((size_t)(distinct ? e->q_groups : (int64_t)nf * per) * 384));
  TM_HIP(hipStreamSynchronize(e->stream));  // the pool handed out memory that work on the main stream may just have released
  if (distinct) {
    TM_TRY(e->qf_colmm.alloc(384 * 4));
    TM_HIP(hipMemsetAsync(e->qf_colmm.p, 0x7f, 192 * 4, e->stream2));                           // 0x7f7f7f7f: above any int16
    TM_HIP(hipMemsetAsync(e->qf_colmm.as<uint8_t>() + 192 * 4, 0x80, 192 * 4, e->stream2));     // 0x80808080: below any int16
    TM_TRY(launch_features_rgb_rows(e->ftiles.p, e->q_rep.p, e->q_groups, TM_PVS_WEIGHTED_DCT, 0, e->qf_pre.p, e->stream2, e->qf_colmm.p));
  }
  else
    TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + (int64_t)sf * per * 256, (int64_t)nf * per, nullptr, TM_PVS_WEIGHTED_DCT, 0, e->qf_pre.p, e->stream2));
  TM_HIP(hipEventRecord(e->ev_qf, e->stream2));
  e->qf_f0 = sf; e->qf_nf = nf; e->qf_epu = epu ? 1 : 0;
  e->qf_distinct = distinct;
  e->qf_valid = true;
  return TM_OK;
}

// the chunk [f0, f0 + nf) of query features: the prefetched buffer when it is that chunk (the main stream then waits for it), else computed now
static int query_features(tm_encoder *e, int f0, int nf, bool epu, DevBuf &qf, void **out) {
  const int64_t per = e->tm_size();
  if (e->qf_valid && !e->qf_distinct && e->qf_f0 == f0 && e->qf_nf == nf && e->qf_epu == (epu ? 1 : 0)) {
    TM_HIP(hipStreamWaitEvent(e->stream, e->ev_qf, 0));
    *out = e->qf_pre.p;
    return TM_OK;
  }
  TM_TRY(qf.alloc((size_t)nf * per * 384));
  *out = qf.p;
  return launch_features_rgb(e->ftiles.as<uint8_t>() + (int64_t)f0 * per * 256, (int64_t)nf * per, nullptr, TM_PVS_WEIGHTED_DCT, 0, qf.p, e->stream);
}

// the features of Reduce's distinct frame tiles: the prefetched ones when they are these (the main stream then waits for them), else
// computed now.  colmm (optional): their column ranges, which only the prefetch keeps (null otherwise)
static int distinct_query_features(tm_encoder *e, DevBuf &qf, void **out, const void **colmm) {
  if (e->qf_valid && e->qf_distinct) {
    TM_HIP(hipStreamWaitEvent(e->stream, e->ev_qf, 0));
    *out = e->qf_pre.p;
    if (colmm) *colmm = e->qf_colmm.p;
    return TM_OK;
  }
  TM_TRY(qf.alloc((size_t)e->q_groups * 384));
  *out = qf.p;
  return launch_features_rgb_rows(e->ftiles.p, e->q_rep.p, e->q_groups, TM_PVS_WEIGHTED_DCT, 0, qf.p, e->stream);
}

// one search's kernel time and pairs into the last Reconstruct's totals (tm_get_knn_stats, tm_get_knn_kernel_split)
static void add_knn_stats(tm_encoder *e, tm_knn_index_impl *ix) {
  double ms = 0, sm[3];
  int kb = 0;
  int64_t pairs = 0, sp[3];
  knn_index_stats(ix, &ms, &kb, &pairs);
  e->knn_ms += ms; e->knn_pairs += pairs; e->knn_launches++; e->knn_kbytes = kb;
  knn_index_kernel_split(ix, sm, sp);
  for (int i = 0; i < 3; i++) { e->knn_split_ms[i] += sm[i]; e->knn_split_pairs[i] += sp[i]; }
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
    TM_TRY(feat.alloc((size_t)std::max<int64_t>(nl, 1) * 192 * 4));
    if (nl > 0) TM_TRY(launch_features_cluster(e->gtiles.as<uint8_t>() + t0 * 256, nl, e->s.DitheringMode, feat.p, e->stream));
    lap("cluster features (own share)");
    DevBuf lidx, all;
    TM_TRY(lidx.alloc((size_t)std::max<int64_t>(nl, 1) * 4));
    TM_TRY(run_palettize_dist(feat.p, e->guse.as<uint8_t>() + t0 * 4, nl, t0, e->s.PaletteCount, 300, lidx.p, e->co, e->stream));
    std::vector<int64_t> counts;
    TM_TRY(gather_var(e, lidx.p, nl, 4, all, &counts));
    TM_HIP(hipMemcpyAsync(e->gpal_idx.p, all.p, (size_t)e->t * 4, hipMemcpyDeviceToDevice, e->stream));
    lap("tile -> palette (192-D, data-parallel)");
  }
  progress(e, TM_STEP_PREPARE_PALETTES, 1, 3);
  if (e->dist()) {
    TM_TRY(run_quantize_palettes_part(e->gtiles.p, e->gpal_idx.p, e->t, e->s.PaletteCount, e->s.PaletteSize, 300, e->palettes_dev.p, e->co.rank, e->co.world, e->stream));
    TM_TRY(e->co.allreduce_sum_i32(e->palettes_dev.p, (int64_t)e->s.PaletteCount * e->s.PaletteSize));
    lap("palette colours (3-D, own palettes)");
  } else {
    TM_TRY(run_quantize_palettes(e->gtiles.p, e->gpal_idx.p, e->t, e->s.PaletteCount, e->s.PaletteSize, 300, e->palettes_dev.p, e->stream, &e->pair_keys, &e->pair_keys_n));
    e->km_stats = kmeans_run_stats();
    lap("palette colours (3-D)");
  }
  e->palettes_host.resize((size_t)e->s.PaletteCount * e->s.PaletteSize);
  {
    HostRead hr_(e->stream);
    TM_TRY(hr_.get(e->palettes_host.data(), e->palettes_dev.p, e->palettes_host.size() * 4));
    TM_TRY(hr_.wait());
  }
  progress(e, TM_STEP_PREPARE_PALETTES, 2, 3);
  TM_TRY(prefetch_query_features(e));  // the GPU has nothing to do while the host searches: Reconstruct's query features run now
  lap("prefetch launch");
  // OptimizePalettes (4309-4432): slot permutation by Powell on the host (P x PaletteSize colours)
  TM_TRY(optimize_palettes_host(e->palettes_host, e->s.PaletteCount, e->s.PaletteSize, nullptr));
  lap("OptimizePalettes (host)");
  TM_HIP(hipMemcpyAsync(e->palettes_dev.p, e->palettes_host.data(), e->palettes_host.size() * 4, hipMemcpyHostToDevice, e->stream));
  TM_HIP(hipStreamSynchronize(e->stream));
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
  TM_HIP(hipStreamSynchronize(e->stream));
  e->has_pal_px = true;
  progress(e, TM_STEP_DITHER, 2, 2);
  return TM_OK;
}

static int step_reconstruct(tm_encoder *e) {
  // Reconstruct, tilingencoder.pas:1928-1962: PrepareReconstruct (4566) builds the int16 database of all global
  // tiles; TFrame.Reconstruct.DoXY (1464-1659) matches every frame tile.  The nearest-neighbour part does not depend on the
  // previous reconstructed frame, so all frames go in one batch; the motion branch (below) then walks the frames in order.
  TM_TRY(need(e, TM_STEP_DITHER, "Dither"));
  TM_TRY(need_frame_tiles(e, "Reconstruct"));
  TM_TRY(load_tail(e));
  DevBuf db, qf;
  TM_TRY(db.alloc((size_t)e->t * 384));
  if (e->dist()) {  // PrepareReconstruct (4566-4613) per share of the global tiles, then the all-gather of the int16 rows (T x 384 bytes in all)
    int64_t t0, t1;
    share_of(e->t, e->co.rank, e->co.world, &t0, &t1);
    DevBuf part, all;
    TM_TRY(part.alloc((size_t)std::max<int64_t>(t1 - t0, 1) * 384));
    if (t1 > t0)
      TM_TRY(launch_features_pal(e->gpal_px.as<uint8_t>() + t0 * 64, e->gpal_idx.as<uint8_t>() + t0 * 4, t1 - t0, e->palettes_dev.p, e->s.PaletteSize, TM_PVS_WEIGHTED_DCT, part.p, e->stream));
    std::vector<int64_t> counts;
    TM_TRY(gather_var(e, part.p, t1 - t0, 384, all, &counts));
    TM_HIP(hipMemcpyAsync(db.p, all.p, (size_t)e->t * 384, hipMemcpyDeviceToDevice, e->stream));
  } else
  TM_TRY(launch_features_pal(e->gpal_px.p, e->gpal_idx.p, e->t, e->palettes_dev.p, e->s.PaletteSize, TM_PVS_WEIGHTED_DCT, db.p, e->stream));
  // Many dithered tiles are byte-identical (Reindex merges them later, MakeTilesUnique(False) at 2014).  Under the
  // lowest-index tie rule the nearest neighbour among ALL rows is the nearest among the DISTINCT rows taken in order of
  // their first occurrence, so only those are searched; indices are mapped back afterwards.
  const int64_t per = e->tm_size();
  int sf, sn;
  query_range(e, &sf, &sn);
  TM_CHECK(!e->load_sharded || (sf >= e->load_first && sf + sn <= e->load_first + e->load_count), TM_E_INVAL,
           "Reconstruct: frames [%d, %d) are not the ones this process loaded ([%d, %d))", sf, sf + sn, e->load_first, e->load_first + e->load_count);
  if (sf > 0 || sn < e->nframes) {  // frames of other shards: TileIdx / PalIdx -1 (merged with MAX), error 0 (merged with SUM: an error is any 32-bit pattern)
    TM_HIP(hipMemsetAsync(e->tm_tile.p, 0xff, (size_t)e->q * 4, e->stream));
    TM_HIP(hipMemsetAsync(e->tm_err.p, 0, (size_t)e->q * 4, e->stream));
    TM_HIP(hipMemsetAsync(e->tm_pal.p, 0xff, (size_t)e->q * 4, e->stream));
  }
  e->knn_ms = 0; e->knn_pairs = 0; e->knn_launches = 0; e->knn_db_rows = 0; e->knn_queries = 0;
  for (double &v : e->knn_split_ms) v = 0;
  e->knn_split_pairs[0] = e->knn_split_pairs[1] = e->knn_split_pairs[2] = 0;
  const bool epu = e->s.FrameTilingExtendedPaletteUsage;
  if (epu) {
    // FrameTilingExtendedPaletteUsage (1559-1610): the 64 nearest rows of the whole database (duplicates included, as
    // ann_kdtree_short_search_multi sees them), then every unique tile x every unique palette of that list, scored against a
    // table of all (tile, palette) feature vectors
    DevBuf table, idx64, err64;
    const int npal = e->s.PaletteCount;
    // the table of every tile under every palette while it fits (T x P x 384 bytes: 2 GB at 16 palettes); with the reference's default
    // of 1024 palettes it would be tens of terabytes, and the re-rank builds just the rows its queries name instead
    const double table_gib = knobs().epu_table_gib;
    const bool use_table = (double)e->t * npal * 384.0 <= table_gib * 1073741824.0;
    if (use_table) {
      TM_TRY(table.alloc((size_t)e->t * npal * 384));
      TM_TRY(launch_features_table(e->gpal_px.p, e->t, e->palettes_dev.p, npal, e->s.PaletteSize, table.p, e->stream));
    }
    progress(e, TM_STEP_RECONSTRUCT, 1, 2);
    const int chunk_frames = recon_chunk_frames(e, sn, true);
    const bool groups = query_groups_usable(e, sf, sn, true);
    TM_TRY(idx64.alloc((size_t)(groups ? e->q_groups : chunk_frames * per) * 64 * 4));
    TM_TRY(err64.alloc((size_t)(groups ? e->q_groups : chunk_frames * per) * 64 * 4));
    // the scan runs over the DISTINCT rows; every result is expanded to all its duplicates (they count, as
    // ann_kdtree_short_search_multi sees them) from member lists
    DevBuf d_remap, d_order, d_use, ddb, g_off, g_members;
    TM_TRY(d_remap.alloc((size_t)e->t * 4)); TM_TRY(d_order.alloc((size_t)e->t * 4)); TM_TRY(d_use.alloc((size_t)(e->t + 1) * 4));
    int64_t nd = 0;
    TM_TRY(run_dedup_ex(db.p, e->t, 384, nullptr, d_remap.p, d_order.p, d_use.p, &nd, 1, e->stream));
    TM_TRY(ddb.alloc((size_t)nd * 384));
    hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(nd * 24)), dim3(256), 0, e->stream, db.as<uint4>(), d_order.as<int32_t>(), nd, 24, ddb.as<uint4>());
    TM_HIP(hipGetLastError());
    TM_TRY(g_off.alloc((size_t)(nd + 1) * 4)); TM_TRY(g_members.alloc((size_t)e->t * 4));
    TM_TRY(build_groups(d_remap.p, e->t, d_use.p, nd, g_off.p, g_members.p, e->stream));
    e->knn_db_rows = nd;
    tm_knn_index_impl *ix = nullptr;
    TM_TRY(knn_index_create(ddb.p, nd, e->stream, &ix));
    int rc = TM_OK;
    if (groups) {
      // one query per DISTINCT frame tile (Reduce's groups): the 64 candidates and the re-rank are functions of the query's features alone
      const int64_t ng = e->q_groups;
      DevBuf gt, gp, ge;
      TM_TRY(gt.alloc((size_t)ng * 4)); TM_TRY(gp.alloc((size_t)ng * 4)); TM_TRY(ge.alloc((size_t)ng * 4));
      void *qfp = nullptr;
      TM_TRY(distinct_query_features(e, qf, &qfp, nullptr));
      e->knn_queries += ng;
      rc = knobs().topk_brute ? launch_knn_topk(qfp, ng, db.p, e->t, 64, idx64.p, err64.p, e->stream)
                                   : knn_index_search_topk(ix, qfp, ng, 64, idx64.p, err64.p, e->stream, g_off.p, g_members.p, db.p, e->t);
      if (rc == TM_OK)
        rc = use_table ? launch_epu_rerank(qfp, ng, idx64.p, 64, e->gpal_idx.p, e->t, npal, table.p, gt.as<int32_t>(), gp.as<int32_t>(), ge.as<uint32_t>(), e->stream)
                       : launch_epu_rerank_ondemand(qfp, ng, idx64.p, 64, e->gpal_idx.p, e->t, e->gpal_px.p, e->palettes_dev.p, npal, e->s.PaletteSize,
                                                    gt.as<int32_t>(), gp.as<int32_t>(), ge.as<uint32_t>(), e->stream);
      if (rc == TM_OK) {
        hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->q_group.as<int32_t>(), e->q, gt.as<int32_t>(), e->tm_tile.as<int32_t>());
        hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->q_group.as<int32_t>(), e->q, gp.as<int32_t>(), e->tm_pal.as<int32_t>());
        hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->q_group.as<int32_t>(), e->q, ge.as<int32_t>(), e->tm_err.as<int32_t>());
        TM_HIP(hipGetLastError());
        TM_HIP(hipStreamSynchronize(e->stream));  // gt / gp / ge die with this scope
      }
    } else
    for (int f0 = sf; rc == TM_OK && f0 < sf + sn; f0 += chunk_frames) {
      const int nf = std::min(chunk_frames, sf + sn - f0);
      const int64_t n = (int64_t)nf * per, off = (int64_t)f0 * per;
      void *qfp = nullptr;
      rc = query_features(e, f0, nf, true, qf, &qfp);
      e->knn_queries += n;
      if (rc == TM_OK)
        rc = knobs().topk_brute ? launch_knn_topk(qfp, n, db.p, e->t, 64, idx64.p, err64.p, e->stream)  // debugging aid: VALU brute force over all rows
                                     : knn_index_search_topk(ix, qfp, n, 64, idx64.p, err64.p, e->stream, g_off.p, g_members.p, db.p, e->t);
      if (rc == TM_OK)
        rc = use_table ? launch_epu_rerank(qfp, n, idx64.p, 64, e->gpal_idx.p, e->t, npal, table.p, e->tm_tile.as<int32_t>() + off,
                                           e->tm_pal.as<int32_t>() + off, e->tm_err.as<uint32_t>() + off, e->stream)
                       : launch_epu_rerank_ondemand(qfp, n, idx64.p, 64, e->gpal_idx.p, e->t, e->gpal_px.p, e->palettes_dev.p, npal, e->s.PaletteSize,
                                                    e->tm_tile.as<int32_t>() + off, e->tm_pal.as<int32_t>() + off, e->tm_err.as<uint32_t>() + off, e->stream);
    }
    knn_index_destroy(ix);
    TM_TRY(rc);
    TM_HIP(hipStreamSynchronize(e->stream));
  } else {
  DevBuf u_remap, u_order, u_use, udb;
  TM_TRY(u_remap.alloc((size_t)e->t * 4)); TM_TRY(u_order.alloc((size_t)e->t * 4)); TM_TRY(u_use.alloc((size_t)e->t * 4));
  int64_t nu = 0;
  TM_TRY(run_dedup_ex(db.p, e->t, 384, nullptr, u_remap.p, u_order.p, u_use.p, &nu, 1, e->stream));
  TM_TRY(udb.alloc((size_t)nu * 384));
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(nu * 24)), dim3(256), 0, e->stream, db.as<uint4>(), u_order.as<int32_t>(), nu, 24,
                     udb.as<uint4>());
  TM_HIP(hipGetLastError());
  e->knn_db_rows = nu;
  tm_knn_index_impl *ix = nullptr;
  TM_TRY(knn_index_create(udb.p, nu, e->stream, &ix));
  progress(e, TM_STEP_RECONSTRUCT, 1, 2);
  int rc = TM_OK;
  if (query_groups_usable(e, sf, sn, false)) {
    // one query per DISTINCT frame tile (Reduce's groups); the items of a group take its answer
    const int64_t ng = e->q_groups;
    DevBuf gt, ge;
    TM_TRY(gt.alloc((size_t)ng * 4)); TM_TRY(ge.alloc((size_t)ng * 4));
    void *qfp = nullptr;
    const void *qmm = nullptr;
    TM_TRY(distinct_query_features(e, qf, &qfp, &qmm));
    rc = knn_index_search(ix, qfp, ng, gt.p, ge.p, e->stream, qmm);
    e->knn_queries += ng;
    if (rc == TM_OK) {
      add_knn_stats(e, ix);
      hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->q_group.as<int32_t>(), e->q, gt.as<int32_t>(), e->tm_tile.as<int32_t>());
      hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->q_group.as<int32_t>(), e->q, ge.as<int32_t>(), e->tm_err.as<int32_t>());
      TM_HIP(hipGetLastError());
      TM_HIP(hipStreamSynchronize(e->stream));  // gt / ge die with this scope
    }
  } else {
  // query features in frame chunks (bounded scratch for long / 4K clips: streaming through HBM)
  const int chunk_frames = recon_chunk_frames(e, sn, false);
  for (int f0 = sf; rc == TM_OK && f0 < sf + sn; f0 += chunk_frames) {
    const int nf = std::min(chunk_frames, sf + sn - f0);
    const int64_t n = (int64_t)nf * per, off = (int64_t)f0 * per;
    void *qfp = nullptr;
    rc = query_features(e, f0, nf, false, qf, &qfp);
    if (rc == TM_OK) rc = knn_index_search(ix, qfp, n, e->tm_tile.as<int32_t>() + off, e->tm_err.as<uint32_t>() + off, e->stream);
    e->knn_queries += n;
    if (rc == TM_OK) add_knn_stats(e, ix);
  }
  }
  knn_index_destroy(ix);
  TM_TRY(rc);
  hipLaunchKernelGGL(k_lookup_inplace, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, u_order.as<int32_t>());
  hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, e->gpal_idx.as<int32_t>(),
                     e->tm_pal.as<int32_t>());  // TMI^.PalIdx := FTiles[TileIdx]^.PalIdx_Initial (1551)
  TM_HIP(hipGetLastError());
  }
  if (e->has_pm) {
    // motion branch (1496-1532, 1612-1654): frames in order, each searched in the previous RECONSTRUCTED frame; a key
    // frame's first frame has no motion candidate, so key-frame groups are independent chains.
    const int sw = e->tm_w * 8, sh = e->tm_h * 8;
    const int64_t nwin = (int64_t)(sw - 7) * (sh - 7);
    DevBuf fb[2], win, cur, mp;
    TM_TRY(fb[0].alloc((size_t)sw * sh * 4)); TM_TRY(fb[1].alloc((size_t)sw * sh * 4));
    TM_TRY(win.alloc((size_t)nwin * 384)); TM_TRY(cur.alloc((size_t)per * 384)); TM_TRY(mp.alloc((size_t)per * 4));
    TM_HIP(hipMemsetAsync(fb[0].p, 0, (size_t)sw * sh * 4, e->stream));
    TM_HIP(hipMemsetAsync(fb[1].p, 0, (size_t)sw * sh * 4, e->stream));
    std::vector<uint8_t> is_kf((size_t)e->nframes, 0);
    for (int32_t k : e->kf_start) is_kf[(size_t)k] = 1;
    TM_CHECK(sn == 0 || is_kf[(size_t)sf], TM_E_INVAL, "Reconstruct with motion prediction: a shard must start on a key frame (frame %d does not)", sf);
    if (sf > 0 || sn < e->nframes) {  // other shards' frames: zeros, so the host merges shards with all-reduce(SUM) on these arrays
      const int64_t a = (int64_t)sf * per, b = (int64_t)(sf + sn) * per;
      TM_HIP(hipMemsetAsync(e->tm_px.p, 0, (size_t)a, e->stream)); TM_HIP(hipMemsetAsync(e->tm_py.p, 0, (size_t)a, e->stream));
      TM_HIP(hipMemsetAsync(e->tm_px.as<uint8_t>() + b, 0, (size_t)(e->q - b), e->stream));
      TM_HIP(hipMemsetAsync(e->tm_py.as<uint8_t>() + b, 0, (size_t)(e->q - b), e->stream));
      TM_HIP(hipMemsetAsync(e->tm_pred.p, 0, (size_t)e->q, e->stream));
    }
    int cb = 0;
    for (int f = sf; f < sf + sn; f++) {
      const int64_t off = (int64_t)f * per;
      const bool search = !is_kf[(size_t)f];  // (Index <> PKeyFrame.StartFrame) and (ARadius >= 0), 1496
      if (search) {
        TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + off * 256, per, e->fflags.as<uint8_t>() + off, TM_PVS_WEIGHTED_DCT, 0, cur.p, e->stream));
        TM_TRY(launch_motion_search_fb(cur.p, e->tm_w, e->tm_h, fb[cb].p, win.p, e->s.MotionPredictRadius, mp.p, e->tm_px.as<int8_t>() + off,
                                       e->tm_py.as<int8_t>() + off, e->stream));
      }
      TM_TRY(launch_recon_decide(e->tm_w, (int)per, epu ? 1 : 0, search ? mp.p : nullptr, e->fflags.as<uint8_t>() + off, e->gpal_idx.p, e->gpal_px.p,
                                 e->palettes_dev.p, e->s.PaletteSize, fb[cb].p, fb[cb ^ 1].p, e->tm_tile.as<int32_t>() + off,
                                 e->tm_pal.as<int32_t>() + off, e->tm_err.as<uint32_t>() + off, e->tm_px.as<int8_t>() + off,
                                 e->tm_py.as<int8_t>() + off, e->tm_pred.as<uint8_t>() + off, e->stream));
      cb ^= 1;
    }
  }
  if (e->dist()) {  // merge the shards' items: TileIdx (and the re-rank's PalIdx) by MAX (others hold -1), the error and the motion results by SUM (others hold 0)
    TM_TRY(e->co.allreduce_max_i32(e->tm_tile.p, e->q));
    TM_TRY(e->co.allreduce_sum_i32(e->tm_err.p, e->q));
    if (epu) TM_TRY(e->co.allreduce_max_i32(e->tm_pal.p, e->q));
    if (e->has_pm) {
      TM_TRY(e->co.allreduce_sum_i32(e->tm_pred.p, (e->q + 3) / 4));
      TM_TRY(e->co.allreduce_sum_i32(e->tm_px.p, (e->q + 3) / 4));
      TM_TRY(e->co.allreduce_sum_i32(e->tm_py.p, (e->q + 3) / 4));
    }
    if (!epu) {  // TMI^.PalIdx := FTiles[TileIdx]^.PalIdx_Initial for every item (1551)
      hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, e->gpal_idx.as<int32_t>(), e->tm_pal.as<int32_t>());
      TM_HIP(hipGetLastError());
    }
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  e->drop_prefetch();  // consumed (or not this chunk's): the buffer goes back to the pool now that both streams are idle
  e->reconstructed = true;
  progress(e, TM_STEP_RECONSTRUCT, 2, 2);
  return TM_OK;
}

static int step_reindex(tm_encoder *e) {  // Reindex, tilingencoder.pas:1993-2038
  TM_TRY(need(e, TM_STEP_RECONSTRUCT, "Reconstruct"));
  DevBuf hist, remap, order, use;
  TM_TRY(hist.alloc((size_t)e->t * 4));
  TM_TRY(remap.alloc((size_t)e->t * 4));
  TM_TRY(order.alloc((size_t)e->t * 4));
  TM_TRY(use.alloc((size_t)e->t * 4));
  // UseCount recount from the tile maps (2018-2031); MakeTilesUnique(False) merges by palette-index content and
  // sums the counts of merged tiles -- same totals as counting after the merge remap
  {  // one histogram copy per XCD, folded afterwards ("Atomics across XCDs")
    DevBuf h8;
    TM_TRY(h8.alloc((size_t)e->t * 4 * 8));
    TM_HIP(hipMemsetAsync(h8.p, 0, (size_t)e->t * 4 * 8, e->stream));
    hipLaunchKernelGGL(k_histogram_xcd, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, h8.as<uint32_t>(), (int64_t)e->t);
    hipLaunchKernelGGL(k_hist_fold, dim3(gridn(e->t)), dim3(256), 0, e->stream, h8.as<uint32_t>(), (int64_t)e->t, hist.as<uint32_t>());
    // (h8 goes back to the pool with this scope; what takes it next is queued on this stream behind the fold)
  }
  int64_t nu = 0;
  TM_TRY(run_dedup(e->gpal_px.p, e->t, 64, hist.p, remap.p, order.p, use.p, &nu, e->stream));
  progress(e, TM_STEP_REINDEX, 2, 3);
  DevBuf ntiles, nflags, npal_idx, npal_px, ntm;
  TM_TRY(ntiles.alloc((size_t)nu * 256)); TM_TRY(nflags.alloc((size_t)std::max<int64_t>(nu, 1))); TM_TRY(npal_idx.alloc((size_t)nu * 4));
  TM_TRY(npal_px.alloc((size_t)nu * 64)); TM_TRY(ntm.alloc((size_t)e->q * 4));
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(nu * 16)), dim3(256), 0, e->stream, e->gtiles.as<uint4>(), order.as<int32_t>(), nu, 16, ntiles.as<uint4>());
  hipLaunchKernelGGL(k_gather_rows16, dim3(gridn(nu * 4)), dim3(256), 0, e->stream, e->gpal_px.as<uint4>(), order.as<int32_t>(), nu, 4, npal_px.as<uint4>());
  hipLaunchKernelGGL(k_gather<uint8_t>, dim3(gridn(nu)), dim3(256), 0, e->stream, e->gflags.as<uint8_t>(), order.as<int32_t>(), nu, nflags.as<uint8_t>());
  hipLaunchKernelGGL(k_gather<int32_t>, dim3(gridn(nu)), dim3(256), 0, e->stream, e->gpal_idx.as<int32_t>(), order.as<int32_t>(), nu, npal_idx.as<int32_t>());
  hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, remap.as<int32_t>(), ntm.as<int32_t>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
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
  hipLaunchKernelGGL(k_lookup, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, e->gpal_idx.as<int32_t>(),
                     e->tm_pal.as<int32_t>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  return TM_OK;
}

}  // extern "C"
