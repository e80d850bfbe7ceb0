// tm_knn_plan.hip -- the KNN stage's digit plan: the per-column ranges of both sides, which columns get a second int8 digit on which
// side, the centres and the column permutation (see tm_knn.hip for the scheme).
#include "tm_knn.h"

namespace tmx {

// ---------------------------------------------------------------------------------------------------------------
// per-column min/max over n rows.  192 threads: thread = (row slot 0..7, 16-byte vector 0..23).
__global__ __launch_bounds__(192) void k_col_minmax(const int16_t *__restrict__ feat, int64_t n, int *__restrict__ mn,
                                                    int *__restrict__ mx) {
  __shared__ int s_mn[8][192], s_mx[8][192];
  const int vec = threadIdx.x % 24, slot = threadIdx.x / 24;
  int lmn[8], lmx[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { lmn[i] = INT_MAX; lmx[i] = INT_MIN; }
  for (int64_t row = (int64_t)blockIdx.x * 8 + slot; row < n; row += (int64_t)gridDim.x * 8) {
    const v4i v = *reinterpret_cast<const v4i *>(feat + row * 192 + vec * 8);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int lo = (int)(int16_t)(v[i] & 0xffff), hi = v[i] >> 16;
      lmn[2 * i] = min(lmn[2 * i], lo); lmx[2 * i] = max(lmx[2 * i], lo);
      lmn[2 * i + 1] = min(lmn[2 * i + 1], hi); lmx[2 * i + 1] = max(lmx[2 * i + 1], hi);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) { s_mn[slot][vec * 8 + i] = lmn[i]; s_mx[slot][vec * 8 + i] = lmx[i]; }
  __syncthreads();
  const int c = threadIdx.x;
  int a = INT_MAX, b = INT_MIN;
#pragma unroll
  for (int s = 0; s < 8; s++) { a = min(a, s_mn[s][c]); b = max(b, s_mx[s][c]); }
  if (a != INT_MAX) { atomicMin(&mn[c], a); atomicMax(&mx[c], b); }
}

int read_col_ranges(const void *dev_ranges, ColStats *out, hipStream_t stream) {
  int res[384];
  {
    HostRead hr_(stream);
    TM_TRY(hr_.get(res, dev_ranges, sizeof(res)));
    TM_TRY(hr_.wait());
  }
  memcpy(out->mn, res, sizeof(int) * 192);
  memcpy(out->mx, res + 192, sizeof(int) * 192);
  return TM_OK;
}

int col_stats(const void *feat, int64_t n, ColStats *out, DevBuf &scratch, hipStream_t stream) {
  TM_TRY(scratch.alloc(384 * sizeof(int)));
  int init[384];
  for (int i = 0; i < 192; i++) { init[i] = INT_MAX; init[192 + i] = INT_MIN; }
  TM_HIP(hipMemcpyAsync(scratch.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
  if (n > 0) {
    int grid = (int)std::min<int64_t>((n + 7) / 8, 2048);
    hipLaunchKernelGGL(k_col_minmax, dim3(grid), dim3(192), 0, stream, (const int16_t *)feat, n, scratch.as<int>(),
                       scratch.as<int>() + 192);
    TM_HIP(hipGetLastError());
  }
  return read_col_ranges(scratch.p, out, stream);
}

// Per-side digit plan.  For every column pick the centre (midpoint of the query range, of the union or of the database)
// that needs the fewest int8 products, then nest the smaller big-set into the larger one so both are prefixes.
static int make_plan_scaled(const ColStats &ts, const ColStats &qs, KnnPlan *plan, int tscale) {
  bool tb[192], qb[192];
  plan->tscale = tscale;
  for (int c = 0; c < 192; c++) {
    int tlo = ts.mn[c], thi = ts.mx[c], qlo = qs.mn[c], qhi = qs.mx[c];
    if (tlo > thi) { tlo = qlo; thi = qhi; }
    if (qlo > qhi) { qlo = tlo; qhi = thi; }
    if (tlo > thi) { tlo = thi = qlo = qhi = 0; }
    const int ulo = std::min(tlo, qlo), uhi = std::max(thi, qhi);
    // the queries' midpoint first: among centres of equal digit cost it is the one about which the radial box dimension prunes best
    // (measured on the bench clip: 272 instead of 326 tiles read per query group, 1.93 % instead of 2.04 % of the pairs evaluated)
    const int cand[3] = {qlo + (qhi - qlo) / 2, ulo + (uhi - ulo) / 2, tlo + (thi - tlo) / 2};
    int best_cost = 99, best_c = cand[0];
    bool bt = true, bq = true;
    for (int k = 0; k < 3; k++) {
      const int cc = cand[k];
      const bool t2 = (tscale * (thi - cc) > 127) || (tscale * (cc - tlo) > 127), q2 = (qhi - cc > 127) || (cc - qlo > 127);
      const int cost = 1 + (t2 ? 1 : 0) + (q2 ? 1 : 0) + (t2 && q2 ? 1 : 0);
      if (cost < best_cost) { best_cost = cost; best_c = cc; bt = t2; bq = q2; }
    }
    plan->centre[c] = (int16_t)best_c;
    tb[c] = bt;
    qb[c] = bq;
  }
  int nt = 0, nq = 0, nu = 0;
  for (int c = 0; c < 192; c++) { nt += tb[c]; nq += qb[c]; nu += (tb[c] || qb[c]); }
  auto chunks = [](int n) { return (n + 31) / 32; };
  // option A: queries' set inside the database's (database digits widened to the union); option B the other way round
  const int costA = chunks(nu) + 2 * chunks(nq), costB = chunks(nu) + 2 * chunks(nt);
  const bool a = costA <= costB;
  const bool *inner = a ? qb : tb;
  // Inside each class the widest columns come first: a 32-row tile whose values all stay within one digit on a chunk of 32 columns has
  // an all-zero high-digit chunk there, and the scan skips the products with it (k3_chain, tm_knn3_block.h) -- with the wide columns (the DC terms,
  // the lowest frequencies) packed into the first chunks, the later chunks are empty for most tiles.
  int order[192];
  for (int c = 0; c < 192; c++) order[c] = c;
  auto halfrange = [&](int c) {
    const int lo = std::min(ts.mn[c] <= ts.mx[c] ? ts.mn[c] : INT_MAX, qs.mn[c] <= qs.mx[c] ? qs.mn[c] : INT_MAX);
    const int hi = std::max(ts.mn[c] <= ts.mx[c] ? ts.mx[c] : INT_MIN, qs.mn[c] <= qs.mx[c] ? qs.mx[c] : INT_MIN);
    return hi >= lo ? std::max(hi - (int)plan->centre[c], (int)plan->centre[c] - lo) : 0;
  };
  std::stable_sort(order, order + 192, [&](int x, int y) { return halfrange(x) > halfrange(y); });
  int p = 0;
  for (int i = 0; i < 192; i++) { const int c = order[i]; if (inner[c]) plan->perm[p++] = (int16_t)c; }
  for (int i = 0; i < 192; i++) { const int c = order[i]; if (!inner[c] && (tb[c] || qb[c])) plan->perm[p++] = (int16_t)c; }
  for (int i = 0; i < 192; i++) { const int c = order[i]; if (!tb[c] && !qb[c]) plan->perm[p++] = (int16_t)c; }
  plan->ht = a ? chunks(nu) : chunks(nt);
  plan->hq = a ? chunks(nq) : chunks(nu);
  plan->nbig_t = nt;
  plan->nbig_q = nq;
  return TM_OK;
}

// does `plan` represent every value of one side's statistics exactly?  (both signs are checked: queries are negated)
bool plan_covers(const KnnPlan &plan, const ColStats &st, int hch, int scale) {
  for (int p = 0; p < 192; p++) {
    const int c = plan.perm[p];
    if (st.mn[c] > st.mx[c]) continue;
    const int lo = scale * (st.mn[c] - plan.centre[c]), hi = scale * (st.mx[c] - plan.centre[c]);
    if (p >= hch * 32) {
      if (lo < -127 || hi > 127) return false;
    } else {
      if (lo < -32000 || hi > 32000) return false;
    }
  }
  return true;
}

// The database digits doubled whenever the doubled values still fit two digits and cost no more products than the plain plan: the
// scan's block epilogue is 16 vector instructions shorter with them.
int make_plan(const ColStats &ts, const ColStats &qs, KnnPlan *plan) {
  KnnPlan p2, p1;
  make_plan_scaled(ts, qs, &p2, 2);
  make_plan_scaled(ts, qs, &p1, 1);
  auto cost = [](const KnnPlan &p) { return p.ht + p.hq + std::min(p.ht, p.hq); };
  if (plan_covers(p2, ts, p2.ht, 2) && plan_covers(p2, qs, p2.hq) && cost(p2) <= cost(p1)) { *plan = p2; return TM_OK; }
  *plan = p1;
  return TM_OK;
}

int upload_plan(tm_knn_index_impl *ix, hipStream_t stream) {
  TM_TRY(ix->plan_dev.alloc(384 * sizeof(int16_t)));
  int16_t host[384];
  memcpy(host, ix->plan.centre, sizeof(int16_t) * 192);
  memcpy(host + 192, ix->plan.perm, sizeof(int16_t) * 192);
  TM_HIP(hipMemcpyAsync(ix->plan_dev.p, host, sizeof(host), hipMemcpyHostToDevice, stream));
  TM_HIP(hipStreamSynchronize(stream));  // host[] is on the stack
  return TM_OK;
}

}  // namespace tmx
