// tm_reduce.hip -- Reduce (tilingencoder.pas:1909-1926 = SolveTileCount (4043) + ReindexTiles(True)): step_reduce picks one of three forms --
// after PredictMotion the PSNR threshold search, with one process per GPU and motion prediction off the dedup over all processes, else the
// plain dedup of every frame tile -- and the kernels only they launch.
#include <numeric>

#include "tm_steps.h"

namespace tmx {

__global__ void k_clip_index(int32_t *__restrict__ idx, int64_t n, int32_t limit) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (idx[i] >= limit) idx[i] = -1;
}
__global__ void k_tilemap_from_subset(const int32_t *__restrict__ keep, const int32_t *__restrict__ pos, const int32_t *__restrict__ sub_remap,
                                      int64_t n, int32_t *__restrict__ tm_tile) {  // TransferTiles: TMI^.TileIdx := tIdx / -1 (4079-4083), then the remaps
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    tm_tile[i] = keep[i] ? sub_remap[pos[i]] : -1;
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

// the Reduce tile budget without motion prediction, 0 = none.  With GlobalTilingUseTargetPSNR no item has a motion PSNR to exceed the
// target, so STCGREval predicts nothing and every distinct tile stays (GlobalTilingTileCount plays no part, 1916-1919).
static int64_t tile_budget(const tm_encoder *e) {
  if (e->s.GlobalTilingUseTargetPSNR) return 0;
  return e->s.GlobalTilingTileCount > 0 ? (int64_t)e->s.GlobalTilingTileCount : 0;
}

// Reduce's last move on every path: the first t of nu distinct tiles -- rows order[0 .. t) of (tiles, flags) -- become the global tiles,
// use[0 .. t) their use counts
static int adopt_global_tiles(tm_encoder *e, int64_t nu, int64_t budget, const void *tiles, const void *flags, const void *order, const void *use) {
  e->t = budget > 0 ? std::min(nu, budget) : nu;
  e->pair_keys_n = 0;
  TM_TRY(e->gtiles.alloc((size_t)e->t * 256));
  TM_TRY(alloc_rows(e->gflags, e->t, 1));
  TM_TRY(e->guse.alloc((size_t)e->t * 4));
  TM_TRY(gather_rows(e, tiles, order, e->t, 256, e->gtiles.p));
  TM_TRY(gather<uint8_t>(e, flags, order, e->t, e->gflags.p));
  TM_HIP(hipMemcpyAsync(e->guse.p, use, (size_t)e->t * 4, hipMemcpyDeviceToDevice, e->stream));
  return TM_OK;
}

static int finish_reduce(tm_encoder *e) {
  e->has_pal_px = e->reconstructed = false;
  progress(e, TM_STEP_REDUCE, 2, 2);
  return TM_OK;
}

static int reduce_motion(tm_encoder *e) {
  TM_TRY(load_tail(e));
  // Reduce with motion prediction (1909-1926): SolveTileCount searches the PSNR threshold above which a tile-map item
  // stays predicted (4014-4046); the items below it are transferred (4048-4103), made unique and ordered (4038, 1923).
  // The search runs on per-group maxima of the prediction error (a group = one distinct tile content): PSNR is a
  // non-increasing function of the error, so "some member has PSNR <= x" is "the group's largest error exceeds the
  // largest error still predicted at x".  The state kept is the last probe's, as in the reference.
  // GlobalTilingUseTargetPSNR (1916-1919): no search, one STCGREval probe at GlobalTilingTargetPSNR; the tile count is what it leaves.
  const int64_t per = e->tm_size();
  DevBuf kfmask, keep, sel, pos;
  const std::vector<uint8_t> hk = key_frame_mask(e);
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
  TM_TRY(gather_rows(e, e->ftiles.p, sel.p, nkeep, 256, sub.p));
  int64_t nu = 0;
  TM_TRY(run_dedup(sub.p, nkeep, 256, nullptr, sremap.p, sorder.p, suse.p, &nu, e->stream));
  DevBuf gsrc;  // global tile -> frame tile index
  TM_TRY(gsrc.alloc((size_t)nu * 4));
  TM_TRY(gather<int32_t>(e, sel.p, sorder.p, nu, gsrc.p));
  TM_TRY(adopt_global_tiles(e, nu, 0, e->ftiles.p, e->fflags.p, gsrc.p, suse.p));
  hipLaunchKernelGGL(k_tilemap_from_subset, dim3(gridn(e->q)), dim3(256), 0, e->stream, keep.as<int32_t>(), pos.as<int32_t>(), sremap.as<int32_t>(),
                     e->q, e->tm_tile.as<int32_t>());
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  return finish_reduce(e);
}

// a rank's offset into the concatenation of every rank's items, and their total
static int64_t rank_offset(const std::vector<int64_t> &counts, int rank, int64_t *total) {
  *total = std::accumulate(counts.begin(), counts.end(), (int64_t)0);
  return std::accumulate(counts.begin(), counts.begin() + rank, (int64_t)0);
}

// What travels in sharded Reduce: only the tiles that can be among the first GlobalTilingTileCount of the merged order, chosen on 16-byte
// keys every process exchanges first (tm_reduce_keys.hip; gathering every distinct tile of every process, as
// the first two rounds did, moved 857 MB on the bench clip).
struct Selection {
  DevBuf in_s, spos;  // a flag per key of every process (this process's start at key_off); a local distinct tile's number among the selected
  DevBuf sidx, suse;  // the nsel selected tiles: row among this process's frame tiles, use count
  int64_t nsel = 0, key_off = 0;
};
static int select_candidates(tm_encoder *e, const void *tiles, const DevBuf &lorder, const DevBuf &luse, int64_t lnu, int64_t budget, Selection *s) {
  DevBuf lkeys, allkeys, sel;
  TM_TRY(alloc_rows(lkeys, lnu, 16));
  TM_TRY(reduce_make_keys(tiles, lorder.p, luse.p, lnu, 256, lkeys.p, e->stream));
  std::vector<int64_t> kcounts;
  TM_TRY(gather_var(e, lkeys.p, lnu, 16, allkeys, &kcounts));
  int64_t ntot = 0;
  s->key_off = rank_offset(kcounts, e->co.rank, &ntot);
  TM_CHECK(ntot > 0 && ntot < (1ll << 31), TM_E_INVAL, "Reduce: %lld distinct tiles over all processes", (long long)ntot);
  TM_TRY(s->in_s.alloc((size_t)ntot * 4));
  TM_TRY(reduce_select_candidates(allkeys.p, ntot, budget, s->in_s.p, e->stream));
  TM_TRY(alloc_rows(sel, lnu, 4)); TM_TRY(alloc_rows(s->spos, lnu, 4));
  s->nsel = 0;
  if (lnu > 0) TM_TRY(compact_kept(s->in_s.as<uint32_t>() + s->key_off, lnu, sel.p, s->spos.p, &s->nsel, e->stream));
  TM_TRY(alloc_rows(s->sidx, s->nsel, 4)); TM_TRY(alloc_rows(s->suse, s->nsel, 4));
  if (s->nsel > 0) {
    TM_TRY(gather<int32_t>(e, lorder.p, sel.p, s->nsel, s->sidx.p));
    TM_TRY(gather<uint32_t>(e, luse.p, sel.p, s->nsel, s->suse.p));
  }
  return TM_OK;
}

static int reduce_sharded(tm_encoder *e, int64_t budget) {
  // One process per GPU: exact dedup of this process's own frame tiles first, then of the union of every process's distinct
  // tiles (all-gathered: tile, use count, mirror flags of its first occurrence).  Processes own increasing frame ranges and the
  // union is laid out in process order, so "first occurrence" and the final order (use count descending, content ascending)
  // are those of the single-process run.
  const int64_t per = e->tm_size(), f0 = e->load_first, nloc = (int64_t)e->load_count * per;
  const uint8_t *tiles = e->ftiles.as<uint8_t>() + f0 * per * 256, *flags = e->fflags.as<uint8_t>() + f0 * per;  // this process's own
  DevBuf lremap, lorder, luse, rec, urec, utiles, uuse, uflags, gremap, gorder, guse2;
  int64_t lnu = 0;
  TM_TRY(alloc_rows(lremap, nloc, 4)); TM_TRY(alloc_rows(lorder, nloc, 4)); TM_TRY(alloc_rows(luse, nloc, 4));
  if (nloc > 0) TM_TRY(run_dedup(tiles, nloc, 256, nullptr, lremap.p, lorder.p, luse.p, &lnu, e->stream));
  Selection s;
  TM_TRY(select_candidates(e, tiles, lorder, luse, lnu, budget, &s));
  TM_TRY(alloc_rows(rec, s.nsel, 264));
  if (s.nsel > 0)
    hipLaunchKernelGGL(k_pack_unique, dim3(gridn(s.nsel * 66)), dim3(256), 0, e->stream, (const uint32_t *)tiles, flags, s.sidx.as<int32_t>(), s.suse.as<uint32_t>(),
                       s.nsel, rec.as<uint32_t>());
  TM_HIP(hipGetLastError());
  std::vector<int64_t> counts;
  TM_TRY(gather_var(e, rec.p, s.nsel, 264, urec, &counts));
  int64_t nun = 0;
  const int64_t my_off = rank_offset(counts, e->co.rank, &nun);
  TM_CHECK(nun > 0 && nun < (1ll << 31), TM_E_INVAL, "Reduce: %lld distinct tiles over all processes", (long long)nun);
  TM_TRY(utiles.alloc((size_t)nun * 256)); TM_TRY(uuse.alloc((size_t)nun * 4)); TM_TRY(uflags.alloc((size_t)nun));
  hipLaunchKernelGGL(k_unpack_unique, dim3(gridn(nun * 66)), dim3(256), 0, e->stream, urec.as<uint32_t>(), nun, utiles.as<uint32_t>(), uuse.as<uint32_t>(), uflags.as<uint8_t>());
  TM_HIP(hipGetLastError());
  TM_TRY(gremap.alloc((size_t)nun * 4)); TM_TRY(gorder.alloc((size_t)nun * 4)); TM_TRY(guse2.alloc((size_t)nun * 4));
  int64_t nu = 0;
  TM_TRY(run_dedup(utiles.p, nun, 256, uuse.p, gremap.p, gorder.p, guse2.p, &nu, e->stream));
  progress(e, TM_STEP_REDUCE, 1, 2);
  TM_TRY(adopt_global_tiles(e, nu, budget, utiles.p, uflags.p, gorder.p, guse2.p));
  // tile map of this process's frames (TransferTiles: TileIdx := the tile's index, 4079-4083); the other frames' items are their owners'
  TM_TRY(clear_items(e, TMA_TILE));
  if (nloc > 0)
    hipLaunchKernelGGL(k_compose_remap_cand, dim3(gridn(nloc)), dim3(256), 0, e->stream, lremap.as<int32_t>(), nloc, s.in_s.as<uint32_t>() + s.key_off, s.spos.as<int32_t>(),
                       gremap.as<int32_t>(), (int32_t)my_off, (int32_t)e->t, e->tm_tile.as<int32_t>() + f0 * per);
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  return finish_reduce(e);
}

static int reduce_plain(tm_encoder *e, int64_t budget) {
  // Motion prediction switched off (MotionPredictRadius = 0, the benchmark's headline configuration): no tile-map item is predicted, so
  // TransferTiles (4048) moves every frame tile; MakeTilesUnique(True) + ReindexTiles(True) are exact; the tile budget is then met by
  // keeping the first GlobalTilingTileCount tiles of that order (most used first), see DESIGN.md "Scope".
  DevBuf remap, order, use;
  TM_TRY(remap.alloc((size_t)e->q * 4)); TM_TRY(order.alloc((size_t)e->q * 4)); TM_TRY(use.alloc((size_t)e->q * 4));
  int64_t nu = 0;
  // (only the first GlobalTilingTileCount tiles of the order stay: the rows behind them are counted and numbered, not ordered)
  TM_TRY(run_dedup(e->ftiles.p, e->q, 256, nullptr, remap.p, order.p, use.p, &nu, e->stream, budget));
  progress(e, TM_STEP_REDUCE, 1, 2);
  TM_TRY(adopt_global_tiles(e, nu, budget, e->ftiles.p, e->fflags.p, order.p, use.p));
  TM_HIP(hipMemcpyAsync(e->tm_tile.p, remap.p, (size_t)e->q * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(k_clip_index, dim3(gridn(e->q)), dim3(256), 0, e->stream, e->tm_tile.as<int32_t>(), e->q, (int32_t)e->t);
  TM_HIP(hipGetLastError());
  TM_HIP(hipStreamSynchronize(e->stream));
  if (!knobs().no_query_groups) {  // kept for Reconstruct: one search per distinct frame tile
    e->q_group = std::move(remap);
    e->q_rep = std::move(order);
    e->q_groups = nu;
  }
  return finish_reduce(e);
}

int step_reduce(tm_encoder *e) {
  TM_TRY(need(e, TM_STEP_LOAD, "Load"));
  TM_TRY(need_frame_tiles(e, "Reduce"));
  e->gtiles_have_rgb = true;
  e->q_groups = 0;
  e->drop_prefetch();
  if (e->has_pm) return reduce_motion(e);
  const int64_t budget = tile_budget(e);  // 0: no budget, everything stays
  return e->load_sharded ? reduce_sharded(e, budget) : reduce_plain(e, budget);
}
