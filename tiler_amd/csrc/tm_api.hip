// tm_api.hip -- extern "C" surface of libtilemotion.so: stage seam + KNN index + misc (include/tilemotion.h).
#include <cmath>
#include <cstdlib>
#include <vector>

#include "tm_common.h"
#include "tm_internal.h"

using namespace tmx;

extern "C" {

int tm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// the trailing token names the build of the KNN scan kernel: PMC passes under profiles/ are keyed by it (bench.py reads `traffic` from them)
const char *tm_version(void) { return "tilemotion-mi355x 0.3 (gfx950) knn-scan3-r18"; }

int tm_stage_load(const void *frames, int nframes, int img_w, int img_h, int tm_w, int tm_h, void *tiles, void *flags,
                  void *lab_means, void *stream) {
  knobs_reload();
  return launch_load(frames, nframes, img_w, img_h, tm_w, tm_h, tiles, flags, lab_means, (hipStream_t)stream);
}

// the tail of PearsonCorrelation (tilingencoder.pas:2221-2227) in host IEEE arithmetic: the device's square root is not correctly rounded
int tm_pearson_finish_host(const float *sums, int n, float *correl) {
  TM_CHECK(n >= 0 && (n == 0 || (sums && correl)), TM_E_INVAL, "tm_pearson_finish_host: bad arguments");
  for (int f = 0; f < n; f++) {
    if (f == 0) { correl[0] = 0.0f; continue; }
    const float denx = std::sqrt(sums[f * 3 + 1]), deny = std::sqrt(sums[f * 3 + 2]);
    const float den = denx * deny;
    correl[f] = den != 0.0f ? sums[f * 3] / den : 1.0f;
  }
  return TM_OK;
}

int tm_stage_pearson(const void *lab_f32, int nframes, int per, void *correl_f32_host, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(nframes >= 0 && per >= 1 && (nframes == 0 || (lab_f32 && correl_f32_host)), TM_E_INVAL, "tm_stage_pearson: bad arguments");
  if (nframes == 0) return TM_OK;
  DevBuf dsums;
  TM_TRY(dsums.alloc((size_t)nframes * 12));
  TM_TRY(launch_pearson(lab_f32, nframes, per, dsums.p, (hipStream_t)stream));
  std::vector<float> sums((size_t)nframes * 3);
  {
    HostRead hr_((hipStream_t)stream);
    TM_TRY(hr_.get(sums.data(), dsums.p, sums.size() * 4));
    TM_TRY(hr_.wait());
  }
  return tm_pearson_finish_host(sums.data(), nframes, (float *)correl_f32_host);
}

int tm_stage_rgb_to_lab(const void *rgb, int64_t n, void *out_lab, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  return launch_rgb_to_lab(rgb, n, out_lab, (hipStream_t)stream);
}

int tm_stage_features_rgb(const void *tiles, int64_t n, const void *mirror_flags, int mode, int use_lab, void *out_i16,
                          void *stream) {
  knobs_reload();
  return launch_features_rgb(tiles, n, mirror_flags, mode, use_lab, out_i16, (hipStream_t)stream);
}

int tm_stage_features_rgb_rows(const void *tiles, const void *rows, int64_t n, int mode, int use_lab, void *out_i16, void *colmm_or_null,
                               void *stream) {
  knobs_reload();
  return launch_features_rgb_rows(tiles, rows, n, mode, use_lab, out_i16, (hipStream_t)stream, colmm_or_null);
}

int tm_stage_features_pal(const void *pal_px, const void *pal_idx, int64_t n, const void *palettes, int pal_size, int mode,
                          void *out_i16, void *stream) {
  knobs_reload();
  return launch_features_pal(pal_px, pal_idx, n, palettes, pal_size, mode, out_i16, (hipStream_t)stream);
}

int tm_stage_features_cluster(const void *tiles, int64_t n, int mode, void *out_i32, void *stream) {
  knobs_reload();
  return launch_features_cluster(tiles, n, mode, out_i32, (hipStream_t)stream);
}

int tm_stage_window_dcts(const void *frame_buffer, int width, int height, void *out_i16, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  return launch_window_dcts(frame_buffer, width, height, out_i16, (hipStream_t)stream);
}

int tm_stage_motion_search(const void *cur_i16, int tm_w, int tm_h, const void *window_dcts, int radius, void *out_err, void *out_px,
                           void *out_py, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  return launch_motion_search(cur_i16, tm_w, tm_h, window_dcts, radius, out_err, out_px, out_py, (hipStream_t)stream);
}

int tm_stage_motion_search_fb(const void *cur_i16, int tm_w, int tm_h, const void *fb_rgb32, int radius, void *out_err, void *out_px,
                              void *out_py, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(tm_w > 0 && tm_h > 0 && cur_i16 && fb_rgb32 && out_err && out_px && out_py, TM_E_INVAL, "tm_stage_motion_search_fb: bad arguments");
  DevBuf win;  // the int16 rows of the fallback
  TM_TRY(win.alloc((size_t)(tm_w * 8 - 7) * (size_t)(tm_h * 8 - 7) * 384));
  TM_TRY(launch_motion_search_fb(cur_i16, tm_w, tm_h, fb_rgb32, win.p, radius, out_err, out_px, out_py, (hipStream_t)stream));
  TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the rows are freed on return
  return TM_OK;
}

int tm_stage_knn_topk(const void *queries_i16, int64_t nq, const void *db_i16, int64_t nt, int k, void *out_idx, void *out_err, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  if (knobs().topk_brute) return launch_knn_topk(queries_i16, nq, db_i16, nt, k, out_idx, out_err, (hipStream_t)stream);  // the VALU brute force
  tm_knn_index_impl *ix = nullptr;
  TM_TRY(knn_index_create(db_i16, nt, (hipStream_t)stream, &ix));
  const int rc = knn_index_search_topk(ix, queries_i16, nq, k, out_idx, out_err, (hipStream_t)stream);
  knn_index_destroy(ix);
  return rc;
}

int tm_stage_epu_rerank(const void *queries_i16, int64_t nq, const void *knn_idx, int k, const void *pal_px, const void *tile_pal_idx,
                        int64_t ntiles, const void *palettes, int npal, int pal_size, void *out_tile, void *out_pal, void *out_err,
                        void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  const double table_gib = knobs().epu_table_gib;
  if ((double)ntiles * npal * 384.0 > table_gib * 1073741824.0)  // no room for every tile under every palette: only the rows the queries name
    return launch_epu_rerank_ondemand(queries_i16, nq, knn_idx, k, tile_pal_idx, ntiles, pal_px, palettes, npal, pal_size, out_tile, out_pal, out_err, (hipStream_t)stream);
  DevBuf table;
  TM_TRY(table.alloc((size_t)std::max<int64_t>(ntiles, 1) * npal * 384));
  TM_TRY(launch_features_table(pal_px, ntiles, palettes, npal, pal_size, table.p, (hipStream_t)stream));
  TM_TRY(launch_epu_rerank(queries_i16, nq, knn_idx, k, tile_pal_idx, ntiles, npal, table.p, out_tile, out_pal, out_err, (hipStream_t)stream));
  TM_HIP(hipStreamSynchronize((hipStream_t)stream));  // the table is freed on return
  return TM_OK;
}

tm_knn_index *tm_knn_index_create(const void *db_i16, int64_t nt, void *stream) {
  knobs_reload();
  tm_knn_index_impl *ix = nullptr;
  if (knn_index_create(db_i16, nt, (hipStream_t)stream, &ix) != TM_OK) return nullptr;
  return reinterpret_cast<tm_knn_index *>(ix);
}

void tm_knn_index_destroy(tm_knn_index *ix) { knn_index_destroy(reinterpret_cast<tm_knn_index_impl *>(ix)); }

int tm_knn_index_search(tm_knn_index *ix, const void *queries_i16, int64_t nq, void *out_idx, void *out_err, void *stream) {
  knobs_reload();
  return knn_index_search(reinterpret_cast<tm_knn_index_impl *>(ix), queries_i16, nq, out_idx, out_err, (hipStream_t)stream);
}

int tm_knn_index_last_stats(tm_knn_index *ix, double *kernel_ms, int *k_bytes, int64_t *pairs) {
  knobs_reload();
  TM_CHECK(ix != nullptr, TM_E_INVAL, "null index");
  knn_index_stats(reinterpret_cast<tm_knn_index_impl *>(ix), kernel_ms, k_bytes, pairs);
  return TM_OK;
}

int tm_knn_index_last_list_counts(tm_knn_index *ix, int64_t *listed, int64_t *popped) {
  TM_CHECK(ix != nullptr, TM_E_INVAL, "null index");
  knn_index_list_counts(reinterpret_cast<tm_knn_index_impl *>(ix), listed, popped);
  return TM_OK;
}

int tm_knn_index_last_chunk_counts(tm_knn_index *ix, int64_t *looked, int64_t *stopped) {
  TM_CHECK(ix != nullptr, TM_E_INVAL, "null index");
  knn_index_chunk_counts(reinterpret_cast<tm_knn_index_impl *>(ix), looked, stopped);
  return TM_OK;
}

int tm_knn_index_last_survivor_counts(tm_knn_index *ix, int64_t *tiles, int64_t *no_survivor, int64_t *pushed, int64_t *ring_full, int64_t *whole, int64_t *completed) {
  TM_CHECK(ix != nullptr, TM_E_INVAL, "null index");
  knn_index_survivor_counts(reinterpret_cast<tm_knn_index_impl *>(ix), tiles, no_survivor, pushed, ring_full, whole, completed);
  return TM_OK;
}

int tm_knn_index_row_order(tm_knn_index *ix, void *out_rows_u32, void *stream) {
  TM_CHECK(ix != nullptr && out_rows_u32 != nullptr, TM_E_INVAL, "null index or output");
  return knn_index_row_order(reinterpret_cast<tm_knn_index_impl *>(ix), out_rows_u32, (hipStream_t)stream);
}

int tm_stage_knn_tile_order(void *perm_u32, int64_t n, void *stream) {
  TM_TRY(require_device());
  TM_CHECK(perm_u32 != nullptr && n >= 0, TM_E_INVAL, "knn tile order: null rows or a negative count");
  return launch_tile_order((uint32_t *)perm_u32, n, (hipStream_t)stream);
}

int tm_stage_curve_keys(const void *coords_u32, int64_t n, const int *bits, int kind, void *keys_u32, void *stream) {
  TM_TRY(require_device());
  TM_CHECK(n >= 0 && bits != nullptr && (n == 0 || (coords_u32 != nullptr && keys_u32 != nullptr)), TM_E_INVAL, "curve keys: null argument or a negative count");
  TM_CHECK(kind == 0 || kind == 1, TM_E_INVAL, "curve keys: kind %d is neither 0 (Morton) nor 1 (Hilbert)", kind);
  int sum = 0, most = 0;
  for (int d = 0; d < 4; d++) {
    TM_CHECK(bits[d] >= 1 && bits[d] <= 16, TM_E_INVAL, "curve keys: %d bits for dimension %d (1..16)", bits[d], d);
    sum += bits[d];
    most = std::max(most, bits[d]);
  }
  TM_CHECK(kind == 0 ? sum <= 32 : most <= 8, TM_E_UNSUPPORTED, "curve keys: bits %d %d %d %d do not fit a 32-bit key (Morton: their sum, Hilbert: four times the largest)",
           bits[0], bits[1], bits[2], bits[3]);
  return launch_curve_keys((const uint32_t *)coords_u32, n, bits, kind, (uint32_t *)keys_u32, (hipStream_t)stream);
}

int tm_knn_last_plan(int *ht, int *hq, int *topk, int64_t *arena_retries) {
  long long r = 0;
  knn_last_plan(ht, hq, topk, &r);
  if (arena_retries) *arena_retries = (int64_t)r;
  return TM_OK;
}

int tm_stage_knn(const void *queries_i16, int64_t nq, const void *db_i16, int64_t nt, void *out_idx, void *out_err, void *stream) {
  knobs_reload();
  tm_knn_index_impl *ix = nullptr;
  TM_TRY(knn_index_create(db_i16, nt, (hipStream_t)stream, &ix));
  int rc = knn_index_search(ix, queries_i16, nq, out_idx, out_err, (hipStream_t)stream);
  knn_index_destroy(ix);
  return rc;
}

int tm_stage_dither(const void *tiles, const void *flags, const void *pal_idx, int64_t n, const void *palettes, int npal,
                    int pal_size, int use_thomas_knoll, int y2_mixed_colors, void *out_pal_px, void *stream) {
  knobs_reload();
  return launch_dither(tiles, flags, pal_idx, n, palettes, npal, pal_size, use_thomas_knoll, y2_mixed_colors, out_pal_px,
                       (hipStream_t)stream);
}

int tm_stage_dedup(const void *rows, int64_t n, int row_bytes, const void *use_in, void *remap, void *order, void *use_out,
                   int64_t *host_n_unique, void *stream) {
  knobs_reload();
  return run_dedup(rows, n, row_bytes, use_in, remap, order, use_out, host_n_unique, (hipStream_t)stream);
}

int tm_stage_dedup_by_index(const void *rows, int64_t n, int row_bytes, void *remap, void *order, void *use_out, int64_t *host_n_unique, void *stream) {
  knobs_reload();
  return run_dedup_ex(rows, n, row_bytes, nullptr, remap, order, use_out, host_n_unique, 1, (hipStream_t)stream);
}

long long tm_host_waits(void) { return host_waits(); }

int tm_stage_kmeans(const void *pts_i32, const void *weights, int64_t n, int d, int k, int max_iter, void *assign, void *centroids,
                    int *host_k, int *host_iters, void *stream) {
  knobs_reload();
  return run_kmeans(pts_i32, weights, n, d, k, max_iter, assign, centroids, host_k, host_iters, (hipStream_t)stream);
}

int tm_stage_kmeans_seeded(const void *pts_i32, const void *weights, int64_t n, int d, int k, const int64_t *host_init_idx, int max_iter, void *assign,
                           void *centroids, int *host_k, int *host_iters, void *stream) {
  knobs_reload();
  TM_CHECK(host_init_idx != nullptr, TM_E_INVAL, "kmeans: null initial centres");
  return run_kmeans_seeded(pts_i32, weights, n, d, k, host_init_idx, max_iter, assign, centroids, host_k, host_iters, (hipStream_t)stream);
}

int tm_stage_quantize_palettes(const void *tiles, const void *pal_idx, int64_t n, int npal, int pal_size, int max_iter,
                               void *out_palettes, void *stream) {
  knobs_reload();
  return run_quantize_palettes(tiles, pal_idx, n, npal, pal_size, max_iter, out_palettes, (hipStream_t)stream);
}

int tm_stage_palettize(const void *feat_i32, const void *use, int64_t n, int npal, int max_iter, void *out_pal_idx, void *stream) {
  knobs_reload();
  return run_palettize(feat_i32, use, n, npal, max_iter, out_pal_idx, (hipStream_t)stream);
}

int tm_kmeans_last_resident(void) { return kmeans_run_stats().resident; }
void tm_kmeans_last_first_look(int64_t *looked, int64_t *exact) {
  if (looked) *looked = kmeans_run_stats().look_scored;
  if (exact) *exact = kmeans_run_stats().look_exact;
}

int tm_stage_pp_seeds(const void *feat_i32, const void *use, int64_t n, int k, int64_t *out_seeds_host, int *out_kk, void *stream) {
  knobs_reload();
  TM_CHECK(feat_i32 && out_seeds_host && out_kk, TM_E_INVAL, "pp_seeds: null argument");
  return run_pp_seeds(feat_i32, use, n, k, out_seeds_host, out_kk, (hipStream_t)stream);
}

int tm_stage_render(const void *tile_idx, const void *pal_idx, const void *item_flags, const void *px, const void *py, int tm_w, int tm_h,
                    int nframes, const void *pal_px, int64_t ntiles, const void *palettes, int npal, int pal_size, void *out, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  TM_CHECK(tile_idx && pal_idx && item_flags && px && py && out && tm_w > 0 && tm_h > 0 && nframes >= 0 && ntiles >= 0 && npal >= 0 && pal_size > 0 &&
               (pal_px || ntiles == 0) && (palettes || npal == 0), TM_E_INVAL, "render: bad arguments");
  const RenderMap m{(const int32_t *)tile_idx, (const int32_t *)pal_idx, (const uint8_t *)item_flags, (const uint8_t *)item_flags, 4,
                    (const int8_t *)px, (const int8_t *)py, (const uint8_t *)pal_px, ntiles, (const int32_t *)palettes, npal, pal_size, tm_w, tm_h};
  return launch_render_output(m, 0, nframes, out, (hipStream_t)stream);
}

int tm_stage_frame_quality(const void *a, const void *b, int nframes, int w, int h, int64_t stride_px, void *sse_u64, void *ssim_f64, void *stream) {
  knobs_reload();
  TM_TRY(require_device());
  return launch_quality_frames(a, b, nframes, w, h, stride_px, sse_u64, ssim_f64, (hipStream_t)stream);
}

}  // extern "C"
