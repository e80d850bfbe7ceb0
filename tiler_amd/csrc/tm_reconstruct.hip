// tm_reconstruct.hip -- Reconstruct (tilingencoder.pas:1928-1962) and the query features PreparePalettes computes ahead for it: the database of
// dithered tiles, the query batches (one per distinct frame tile, or frame chunks), the k = 1 search and the extended-palette one, the
// motion chain, the merge over several processes.
#include "tm_steps.h"

// frames per chunk of Reconstruct's query features (bounded scratch for long / 4K clips: streaming through HBM)
static int recon_chunk_frames(const tm_encoder *e, int sn, bool epu) {
  if (knobs().recon_chunk_frames > 0) return std::min(knobs().recon_chunk_frames, sn);  // (tests: several chunks on a small clip)
  const int64_t per = e->tm_size(), budget = epu ? ((int64_t)2 << 30) : ((int64_t)8 << 30);
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::max(sn, 1), budget / (per * 384)));
}

// may Reconstruct search once per distinct frame tile?  (the k = 1 search of the whole clip in one process, rows within one chunk)
static bool query_groups_usable(const tm_encoder *e, int sf, int sn, bool epu) {
  // (the extended-palette search keeps 64 candidates per query: 512 more bytes a row)
  return e->q_groups > 0 && !e->dist() && sf == 0 && sn == e->nframes && e->q_groups * (epu ? 384 + 512 : 384) <= ((int64_t)8 << 30);
}

int prefetch_query_features(tm_encoder *e) {
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
  } else {
    TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + (int64_t)sf * per * 256, (int64_t)nf * per, nullptr, TM_PVS_WEIGHTED_DCT, 0, e->qf_pre.p, e->stream2));
  }
  TM_HIP(hipEventRecord(e->ev_qf, e->stream2));
  e->qf_f0 = sf; e->qf_nf = nf; e->qf_epu = epu ? 1 : 0;
  e->qf_distinct = distinct;
  e->qf_valid = true;
  return TM_OK;
}

// ---- the database ------------------------------------------------------------------------------------------------
// PrepareReconstruct (4566): the int16 rows of all global tiles.  Many dithered tiles are byte-identical (Reindex merges them later,
// MakeTilesUnique(False) at 2014).  Under the lowest-index tie rule the nearest neighbour among ALL rows is the nearest among the DISTINCT
// rows taken in order of their first occurrence, so only those are indexed; results are mapped back through `order`.
struct ReconDb {
  DevBuf rows, distinct;     // [t] and [n] rows of 384 bytes
  DevBuf remap, order, use;  // row -> distinct row, distinct row -> its first row, rows per distinct row
  int64_t n = 0;
  tm_knn_index_impl *ix = nullptr;  // over `distinct`
  ~ReconDb() { knn_index_destroy(ix); }
};

static int database_rows(tm_encoder *e, DevBuf &rows) {
  // PrepareReconstruct (4566-4613); with several processes per share of the global tiles, then the all-gather of the int16 rows (T x 384 bytes in all)
  int64_t t0 = 0, t1 = e->t;
  if (e->dist()) share_of(e->t, e->co.rank, e->co.world, &t0, &t1);
  DevBuf part, all;
  TM_TRY(rows.alloc((size_t)e->t * 384));
  if (e->dist()) TM_TRY(alloc_rows(part, t1 - t0, 384));
  if (t1 > t0)
    TM_TRY(launch_features_pal(e->gpal_px.as<uint8_t>() + t0 * 64, e->gpal_idx.as<uint8_t>() + t0 * 4, t1 - t0, e->palettes_dev.p, e->s.PaletteSize, TM_PVS_WEIGHTED_DCT,
                               e->dist() ? part.p : rows.p, e->stream));
  if (!e->dist()) return TM_OK;
  std::vector<int64_t> counts;
  TM_TRY(gather_var(e, part.p, t1 - t0, 384, all, &counts));
  TM_HIP(hipMemcpyAsync(rows.p, all.p, (size_t)e->t * 384, hipMemcpyDeviceToDevice, e->stream));
  return TM_OK;
}

static int build_database(tm_encoder *e, ReconDb *db) {
  TM_TRY(database_rows(e, db->rows));
  TM_TRY(db->remap.alloc((size_t)e->t * 4)); TM_TRY(db->order.alloc((size_t)e->t * 4)); TM_TRY(db->use.alloc((size_t)e->t * 4));
  TM_TRY(run_dedup_ex(db->rows.p, e->t, 384, nullptr, db->remap.p, db->order.p, db->use.p, &db->n, 1, e->stream));
  TM_TRY(db->distinct.alloc((size_t)db->n * 384));
  TM_TRY(gather_rows(e, db->rows.p, db->order.p, db->n, 384, db->distinct.p));
  e->knn_db_rows = db->n;
  return knn_index_create(db->distinct.p, db->n, e->stream, &db->ix);
}

// ---- the query batches -------------------------------------------------------------------------------------------
// One search's queries and where its answers go.  Reconstruct either asks once per distinct frame tile (Reduce's groups: one batch into
// scratch arrays, expanded to the groups' items afterwards) or walks its frames in chunks (the answers go straight into the tile-map arrays).
struct QueryBatch {
  const void *qf, *colmm;  // [n] features of 384 bytes; their column ranges where the prefetch kept them (else null)
  int64_t n;
  int32_t *tile, *pal;
  uint32_t *err;
};

// a batch's features -- of Reduce's distinct frame tiles, or of the frames [f0, f0 + nf): the prefetched buffer when it holds these (the main
// stream then waits for it), else computed now into qf
static int query_features(tm_encoder *e, bool distinct, int f0, int nf, bool epu, DevBuf &qf, QueryBatch *b) {
  const int64_t per = e->tm_size();
  b->n = distinct ? e->q_groups : nf * per;
  b->colmm = nullptr;
  if (e->qf_valid && e->qf_distinct == distinct && (distinct || (e->qf_f0 == f0 && e->qf_nf == nf && e->qf_epu == (epu ? 1 : 0)))) {
    TM_HIP(hipStreamWaitEvent(e->stream, e->ev_qf, 0));
    b->qf = e->qf_pre.p;
    if (distinct) b->colmm = e->qf_colmm.p;  // (only the prefetch keeps them)
    return TM_OK;
  }
  TM_TRY(qf.alloc((size_t)b->n * 384));
  b->qf = qf.p;
  if (distinct) return launch_features_rgb_rows(e->ftiles.p, e->q_rep.p, b->n, TM_PVS_WEIGHTED_DCT, 0, qf.p, e->stream);
  return launch_features_rgb(e->ftiles.as<uint8_t>() + f0 * per * 256, b->n, nullptr, TM_PVS_WEIGHTED_DCT, 0, qf.p, e->stream);
}

// search(batch) for every batch: the one place that decides between groups and frame chunks
template <class Search> static int for_each_batch(tm_encoder *e, int sf, int sn, bool epu, Search search) {
  DevBuf qf;
  QueryBatch b;
  if (query_groups_usable(e, sf, sn, epu)) {  // the answer is a function of the query's features alone: the items of a group take it
    DevBuf gt, gp, ge;
    TM_TRY(gt.alloc((size_t)e->q_groups * 4));
    if (epu) TM_TRY(gp.alloc((size_t)e->q_groups * 4));
    TM_TRY(ge.alloc((size_t)e->q_groups * 4));
    TM_TRY(query_features(e, true, 0, 0, epu, qf, &b));
    b.tile = gt.as<int32_t>(); b.pal = gp.as<int32_t>(); b.err = ge.as<uint32_t>();
    TM_TRY(search(b));
    TM_TRY(lookup(e, e->q_group.p, e->q, gt.p, e->tm_tile.p));
    if (epu) TM_TRY(lookup(e, e->q_group.p, e->q, gp.p, e->tm_pal.p));
    TM_TRY(lookup(e, e->q_group.p, e->q, ge.p, e->tm_err.p));
    TM_HIP(hipStreamSynchronize(e->stream));  // gt / gp / ge die with this scope
    return TM_OK;
  }
  const int chunk_frames = recon_chunk_frames(e, sn, epu);
  for (int f0 = sf; f0 < sf + sn; f0 += chunk_frames) {
    const int64_t off = (int64_t)f0 * e->tm_size();
    TM_TRY(query_features(e, false, f0, std::min(chunk_frames, sf + sn - f0), epu, qf, &b));
    b.tile = e->tm_tile.as<int32_t>() + off; b.pal = e->tm_pal.as<int32_t>() + off; b.err = e->tm_err.as<uint32_t>() + off;
    TM_TRY(search(b));
  }
  return TM_OK;
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

// ---- the two searches --------------------------------------------------------------------------------------------
// k = 1: every query's nearest distinct row, then back to that row's first occurrence among all rows
static int search_nearest(tm_encoder *e, const ReconDb &db, int sf, int sn) {
  TM_TRY(for_each_batch(e, sf, sn, false, [&](const QueryBatch &b) -> int {
    e->knn_queries += b.n;
    TM_TRY(knn_index_search(db.ix, b.qf, b.n, b.tile, b.err, e->stream, b.colmm));
    add_knn_stats(e, db.ix);
    return TM_OK;
  }));
  return lookup_inplace(e, e->tm_tile.p, e->q, db.order.p);
}

// FrameTilingExtendedPaletteUsage (1559-1610): the 64 nearest rows of the whole database (duplicates included, as
// ann_kdtree_short_search_multi sees them), then every unique tile x every unique palette of that list, scored against a
// table of all (tile, palette) feature vectors
static int search_extended(tm_encoder *e, const ReconDb &db, int sf, int sn) {
  DevBuf table, idx64, err64, g_off, g_members;
  const int npal = e->s.PaletteCount;
  // the table of every tile under every palette while it fits (T x P x 384 bytes: 2 GB at 16 palettes); with the reference's default
  // of 1024 palettes it would be tens of terabytes, and the re-rank builds just the rows its queries name instead
  const bool use_table = (double)e->t * npal * 384.0 <= knobs().epu_table_gib * 1073741824.0;
  if (use_table) {
    TM_TRY(table.alloc((size_t)e->t * npal * 384));
    TM_TRY(launch_features_table(e->gpal_px.p, e->t, e->palettes_dev.p, npal, e->s.PaletteSize, table.p, e->stream));
  }
  // the scan runs over the DISTINCT rows; every result is expanded to all its duplicates (they count) from member lists
  TM_TRY(g_off.alloc((size_t)(db.n + 1) * 4)); TM_TRY(g_members.alloc((size_t)e->t * 4));
  TM_TRY(build_groups(db.remap.p, e->t, db.use.p, db.n, g_off.p, g_members.p, e->stream));
  TM_TRY(for_each_batch(e, sf, sn, true, [&](const QueryBatch &b) -> int {
    e->knn_queries += b.n;
    TM_TRY(idx64.alloc((size_t)b.n * 64 * 4)); TM_TRY(err64.alloc((size_t)b.n * 64 * 4));  // 64 candidates a query (the first batch is the largest)
    if (knobs().topk_brute)  // debugging aid: VALU brute force over all rows
      TM_TRY(launch_knn_topk(b.qf, b.n, db.rows.p, e->t, 64, idx64.p, err64.p, e->stream));
    else
      TM_TRY(knn_index_search_topk(db.ix, b.qf, b.n, 64, idx64.p, err64.p, e->stream, g_off.p, g_members.p, db.rows.p, e->t));
    if (use_table) return launch_epu_rerank(b.qf, b.n, idx64.p, 64, e->gpal_idx.p, e->t, npal, table.p, b.tile, b.pal, b.err, e->stream);
    return launch_epu_rerank_ondemand(b.qf, b.n, idx64.p, 64, e->gpal_idx.p, e->t, e->gpal_px.p, e->palettes_dev.p, npal, e->s.PaletteSize, b.tile, b.pal, b.err,
                                      e->stream);
  }));
  TM_HIP(hipStreamSynchronize(e->stream));  // the table and the candidate lists die with this scope
  return TM_OK;
}

// ---- the motion chain --------------------------------------------------------------------------------------------
// motion branch (1496-1532, 1612-1654): frames in order, each searched in the previous RECONSTRUCTED frame; a key
// frame's first frame has no motion candidate, so key-frame groups are independent chains.
static int motion_chain(tm_encoder *e, int sf, int sn, bool epu, bool shard) {
  const int64_t per = e->tm_size();
  MotionScratch ms;
  DevBuf mp;
  TM_TRY(ms.alloc(e, 2)); TM_TRY(mp.alloc((size_t)per * 4));
  TM_HIP(hipMemsetAsync(ms.screen[0].p, 0, ms.screen_bytes, e->stream));
  TM_HIP(hipMemsetAsync(ms.screen[1].p, 0, ms.screen_bytes, e->stream));
  const std::vector<uint8_t> is_kf = key_frame_mask(e);
  TM_CHECK(sn == 0 || is_kf[(size_t)sf], TM_E_INVAL, "Reconstruct with motion prediction: a shard must start on a key frame (frame %d does not)", sf);
  if (shard) {  // (this shard's PredictedX / Y of PredictMotion stay until its frames are decided)
    TM_TRY(clear_items(e, TMA_PX | TMA_PY, sf, sn));
    TM_TRY(clear_items(e, TMA_PRED));
  }
  int cb = 0;
  for (int f = sf; f < sf + sn; f++) {
    const int64_t off = (int64_t)f * per;
    const bool search = !is_kf[(size_t)f];  // (Index <> PKeyFrame.StartFrame) and (ARadius >= 0), 1496
    if (search) {
      TM_TRY(launch_features_rgb(e->ftiles.as<uint8_t>() + off * 256, per, e->fflags.as<uint8_t>() + off, TM_PVS_WEIGHTED_DCT, 0, ms.cur.p, e->stream));
      TM_TRY(launch_motion_search_fb(ms.cur.p, e->tm_w, e->tm_h, ms.screen[cb].p, ms.win.p, e->s.MotionPredictRadius, mp.p, e->tm_px.as<int8_t>() + off,
                                     e->tm_py.as<int8_t>() + off, e->stream));
    }
    TM_TRY(launch_recon_decide(e->tm_w, (int)per, epu ? 1 : 0, search ? mp.p : nullptr, e->fflags.as<uint8_t>() + off, e->gpal_idx.p, e->gpal_px.p,
                               e->palettes_dev.p, e->s.PaletteSize, ms.screen[cb].p, ms.screen[cb ^ 1].p, e->tm_tile.as<int32_t>() + off,
                               e->tm_pal.as<int32_t>() + off, e->tm_err.as<uint32_t>() + off, e->tm_px.as<int8_t>() + off,
                               e->tm_py.as<int8_t>() + off, e->tm_pred.as<uint8_t>() + off, e->stream));
    cb ^= 1;
  }
  return TM_OK;
}

int step_reconstruct(tm_encoder *e) {
  // Reconstruct, tilingencoder.pas:1928-1962: PrepareReconstruct (4566) builds the int16 database of all global
  // tiles; TFrame.Reconstruct.DoXY (1464-1659) matches every frame tile.  The nearest-neighbour part does not depend on the
  // previous reconstructed frame, so all frames go in one batch; the motion chain then walks the frames in order.
  TM_TRY(need(e, TM_STEP_DITHER, "Dither"));
  TM_TRY(need_frame_tiles(e, "Reconstruct"));
  TM_TRY(load_tail(e));
  int sf, sn;
  const bool shard = query_range(e, &sf, &sn), epu = e->s.FrameTilingExtendedPaletteUsage;
  TM_CHECK(!e->load_sharded || (sf >= e->load_first && sf + sn <= e->load_first + e->load_count), TM_E_INVAL,
           "Reconstruct: frames [%d, %d) are not the ones this process loaded ([%d, %d))", sf, sf + sn, e->load_first, e->load_first + e->load_count);
  e->knn_ms = 0; e->knn_pairs = 0; e->knn_launches = 0; e->knn_queries = 0;
  for (double &v : e->knn_split_ms) v = 0;
  e->knn_split_pairs[0] = e->knn_split_pairs[1] = e->knn_split_pairs[2] = 0;
  {
    ReconDb db;
    TM_TRY(build_database(e, &db));
    progress(e, TM_STEP_RECONSTRUCT, 1, 2);
    if (shard) TM_TRY(clear_items(e, TMA_TILE | TMA_ERR | TMA_PAL));  // frames of other shards
    TM_TRY(epu ? search_extended(e, db, sf, sn) : search_nearest(e, db, sf, sn));
  }
  if (!epu) TM_TRY(pal_from_tile(e));  // (the extended search chose the palettes itself)
  if (e->has_pm) TM_TRY(motion_chain(e, sf, sn, epu, shard));
  if (e->dist()) {
    TM_TRY(merge_items(e, TMA_TILE | TMA_ERR | (epu ? TMA_PAL : 0) | (e->has_pm ? TMA_PRED | TMA_PX | TMA_PY : 0)));
    if (!epu) TM_TRY(pal_from_tile(e));  // now for every shard's items
  }
  TM_HIP(hipStreamSynchronize(e->stream));
  e->drop_prefetch();  // consumed (or not this chunk's): the buffer goes back to the pool now that both streams are idle
  e->reconstructed = true;
  progress(e, TM_STEP_RECONSTRUCT, 2, 2);
  return TM_OK;
}
