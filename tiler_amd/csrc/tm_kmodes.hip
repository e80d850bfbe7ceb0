// tm_kmodes.hip -- A17: TKModes.ComputeKModes (kmodes.pas:923-1094) for rows of cKModesFeatureCount = 80 bytes.
//
// Unreachable in the reference snapshot (nothing calls it) but named by the north star, so it is built as an operator of its
// own: tm_stage_kmodes (host pointers, like the Pascal arrays) and tm_stage_kmodes_dev (device pointers).  Everything the clustering
// keeps -- memberships, member counts, the k x 80 x num_modalities histograms of MovePointCat, the modes, the LCG's seed -- lives in HBM:
//   * MatchingDissim (kmodes.pas:248-259) = sum |a - b| + 2048 x #(a != b) over the 80 bytes of a row: twenty v_sad_u8
//     (four bytes each) plus a count of the non-zero bytes of a XOR b, the GPU form of the reference's psadbw / pcmpeqb / popcnt
//     (kmodes.pas:314-450);
//   * GetMinMatchingDissim for a range of points against the k modes (the LAST minimum wins, `dis <= best`);
//   * the farthest-first initialisation's min-distance update and its pick (the LAST largest among unused points wins, 757-762);
//   * KModesIter (851-921) bin by bin, as the reference walks it (a bin of 960 points is scored against the modes as they stand at its
//     start, then its points move one after the other), with Huang's online mode update MovePointCat (774-803) and the empty-cluster
//     repair with RandInt (88-92).
// What bounds it is that bin-serial rule, not bytes.  The host keeps the stopping rule with its three graces (1040-1049) and reads one
// KmScalars per iteration.
//
// The files:
//   tm_kmodes.h         what they share: the constants, MatchingDissim, the owners' key, KmState and its scalars, the owner's LDS layout,
//                       the histogram-row helpers (GetMaxValueIndex), KmBuffers, and what the files below call of each other
//   tm_kmodes_init.hip  before the iterations: the check of the values, k_kmodes_argmin (score), farthest-first, the initial assignment
//   tm_kmodes_iter.hip  KModesIter: k_kmodes_owner + k_kmodes_walker per bin as one graph per iteration, and k_kmodes_fast, the later
//                       iterations' one launch over many bins
//   tm_kmodes.hip       this driver: the starting points, the buffers, the stopping rule, the runs and their best, the C entries
#include <chrono>
#include <cmath>

#include "tm_kmodes.h"

namespace tmx {
namespace {

// 952-964: the starting point itself (num_init <= 0: point -num_init), or a golden-ratio-like spread of num_init of them, Single arithmetic
int kmodes_starts(int64_t n, int num_init, std::vector<int64_t> *out) {
  std::vector<int64_t> &starts = *out;
  starts.assign((size_t)std::max(1, num_init), 0);
  if (num_init <= 0) {
    starts[0] = -(int64_t)num_init;
  } else {
    const float ratio = (float)std::pow((double)n, 1.0 / (double)num_init);
    float acc = 1.0f;
    for (int i = 0; i < num_init; i++) {
      starts[(size_t)i] = (int64_t)std::nearbyint((double)acc) - 1;  // Round: half to even
      if (i > 0 && starts[(size_t)i] <= starts[(size_t)i - 1]) starts[(size_t)i] = std::min(n - 1, starts[(size_t)i - 1] + 1);
      acc = acc * ratio;
    }
  }
  for (int64_t sp : starts) TM_CHECK(sp >= 0 && sp < n, TM_E_INVAL, "kmodes: starting point %lld outside the %lld points", (long long)sp, (long long)n);
  return TM_OK;
}

// The argument checks, stated here alone.  run_kmodes_dev is where they belong; run_kmodes asks first because it sizes allocations by n and k.
int check_arguments(const void *rows, int64_t n, int k, int nmod, const void *labels_out, const void *cent_out) {
  TM_CHECK(rows && labels_out && cent_out, TM_E_INVAL, "kmodes: null argument");
  TM_CHECK(n >= 1 && n < (1ll << 31), TM_E_INVAL, "kmodes: %lld points", (long long)n);  // (the move list's point index is an int)
  TM_CHECK(k >= 1 && k <= KM_MAX_CLUSTERS, TM_E_INVAL, "kmodes: %d clusters outside 1..%d", k, KM_MAX_CLUSTERS);
  TM_CHECK(nmod >= 1 && nmod <= 256, TM_E_INVAL, "kmodes: %d modalities outside 1..256", nmod);
  return TM_OK;
}

int read_scalars(const KmBuffers &b, KmScalars *h) {
  TM_HIP(hipMemcpyAsync(h, b.scal.p, sizeof(KmScalars), hipMemcpyDeviceToHost, b.stream));
  TM_HIP(hipStreamSynchronize(b.stream));
  TM_CHECK(h->bad != 1, TM_E_INVAL, "kmodes: a value is not below the %d modalities", b.nmod);
  TM_CHECK(h->bad == 0, TM_E_INVAL, "kmodes: empty-cluster repair found no donor");
  return TM_OK;
}

// The stopping rule with its three graces (1040-1049): an iteration that does not lower the cost ends the run, unless the cost is the same
// within a thousandth (SameValue(cost, prevcost, prevcost div 1000), 1041) -- that is forgiven twice; no move ends it at once.
struct KmStop {
  uint64_t prevcost = ~0ull;
  int worse = 0;
  bool step(uint64_t cost, int moves) {  // true: converged
    bool converged = cost >= prevcost;
    if (converged) {
      const double a = (double)cost, b = (double)prevcost;
      double eps = (double)(prevcost / 1000);
      if (eps == 0) eps = std::max(std::min(std::fabs(a), std::fabs(b)) * 1e-12, 1e-12);
      const bool same = a > b ? (a - b) <= eps : (b - a) <= eps;
      if (same) { worse++; if (worse < 3) converged = false; }
    }
    prevcost = cost;
    return converged || moves == 0;
  }
};

}  // namespace

int KmBuffers::alloc(const uint8_t *rows_, int64_t n_, int k_, int nmod_, hipStream_t stream_) {
  rows = rows_; n = n_; k = k_; nmod = nmod_; stream = stream_;
  nbins = (n + KM_BIN - 1) / KM_BIN;
  G = std::min(k, KM_MAX_OWNERS);
  ff_blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  ff_partial_host.resize((size_t)ff_blocks);
  which_host.resize((size_t)k);
  TM_TRY(clust.alloc((size_t)n * 4)); TM_TRY(dis.alloc((size_t)n * 4)); TM_TRY(memb.alloc((size_t)n * 4)); TM_TRY(members.alloc((size_t)k * 4));
  TM_TRY(freq.alloc((size_t)k * KM_ATTRS * nmod * 4)); TM_TRY(cent.alloc((size_t)k * KM_ATTRS)); TM_TRY(used.alloc((size_t)n)); TM_TRY(mind.alloc((size_t)n * 4));
  TM_TRY(ff_partial.alloc((size_t)ff_blocks * 8)); TM_TRY(which.alloc((size_t)k * 8)); TM_TRY(scal.alloc(sizeof(KmScalars))); TM_TRY(mlist.alloc((size_t)KM_MLIST_CAP * sizeof(int3)));
  TM_TRY(best_memb.alloc((size_t)n * 4)); TM_TRY(best_cent.alloc((size_t)k * KM_ATTRS));
  TM_TRY(keys.alloc((size_t)KM_BIN * G * 4)); TM_TRY(handover.alloc(sizeof(KmHandover)));
  KmScalars *const s = scal.as<KmScalars>();
  st.memb = memb.as<int32_t>(); st.clust = clust.as<int32_t>(); st.dis = dis.as<unsigned>(); st.members = members.as<int32_t>(); st.freq = freq.as<int32_t>();
  st.cent = cent.as<uint8_t>(); st.mlist = mlist.as<int3>();
  st.seed = &s->seed; st.cost = &s->cost; st.moves = &s->moves; st.nmoves = &s->nmoves; st.bad = &s->bad;
  KmScalars init = {};
  init.seed = 0x42381337u;  // 933
  TM_HIP(hipMemcpyAsync(s, &init, sizeof init, hipMemcpyHostToDevice, stream));
  TM_HIP(hipMemsetAsync(handover.p, 0, sizeof(KmHandover), stream));
  TM_HIP(hipStreamSynchronize(stream));  // init is on the stack
  return TM_OK;
}

// TKModes.ComputeKModes on DEVICE pointers: rows [n][80], labels [n], centroids [k][80]; the host keeps the stopping rule
// and the run bookkeeping, one small read-back per iteration.
int run_kmodes_dev(const uint8_t *rows, int64_t n, int k, int num_init, int nmod, int max_iter, int32_t *labels_out, uint8_t *cent_out, uint64_t *cost_out,
                   int *iters_out, int64_t *point_iters_out, hipStream_t stream) {
  TM_TRY(require_device());
  TM_TRY(check_arguments(rows, n, k, nmod, labels_out, cent_out));
  if (max_iter < 0) max_iter = INT_MAX;
  std::vector<int64_t> starts;
  TM_TRY(kmodes_starts(n, num_init, &starts));
  KmBuffers b;
  TM_TRY(b.alloc(rows, n, k, nmod, stream));
  TM_TRY(validate_values(b));
  IterGraph graph;
  TM_TRY(graph.build(b));
  TM_TRY(score_prepare(k));
  KmScalars h;
  TM_TRY(read_scalars(b, &h));  // nothing below may index a histogram with a value that is not a modality
  const bool fast_ok = !knobs().kmodes_binwise;
  uint64_t all_best = ~0ull;
  int all_iters = 0;
  int64_t point_iters = 0;
  for (size_t run = 0; run < starts.size(); run++) {
    TM_TRY(farthest_first(b, starts[run]));
    TM_TRY(initial_assignment(b));
    int itr = 0, bestitr = 0;
    long long prev_moves = LLONG_MAX;
    bool converged = false;
    uint64_t bestcost = ~0ull;
    KmStop stop;
    while (itr < max_iter && !converged) {
      itr++;
      point_iters += n;
      // ---- KModesIter (851-921): bins of 960 points, each scored against the modes as they stand when its turn comes
      TM_HIP(hipMemsetAsync(&b.scal.as<KmScalars>()->cost, 0, offsetof(KmScalars, nmoves) - offsetof(KmScalars, cost), stream));  // cost, moves
      const auto t_it0 = std::chrono::steady_clock::now();
      int64_t bin = 0;  // where the bin-by-bin launches take over
      // (not where the iteration before moved more than 16 points a bin: with that many movers nearly every bin changes a mode or has more
      // moves than the one workgroup's move-by-move MovePointCat is good for)
      if (fast_ok && itr >= 2 && (prev_moves <= 16 * b.nbins || knobs().kmodes_fast_always)) {
        // the fast leg (k_kmodes_fast): all remaining points scored at once, bins walked by one launch until a mode changes
        int stops = 0;
        while (bin < b.nbins && stops < KM_FAST_STOPS) {
          TM_TRY(score(b, bin * KM_BIN, n));
          TM_TRY(fast_leg(b, bin, &bin));
          if (bin < b.nbins) stops++;
        }
        if (knobs().pp_debug) fprintf(stderr, "[tm_kmodes] iteration %d: the fast leg walked %lld of %lld bins (%d stops)\n", itr, (long long)bin, (long long)b.nbins, stops);
      }
      // the modes keep moving, or the leg was not tried: the (rest of the) iteration bin by bin, by the graph
      if (bin < b.nbins) TM_TRY(graph.launch_from(b, bin));
      TM_TRY(read_scalars(b, &h));
      const uint64_t cost = h.cost;
      const int moves = (int)h.moves;
      if (knobs().pp_debug)
        fprintf(stderr, "[tm_kmodes] run %d iteration %d: cost %llu, %d moves, %.2f ms (mode words changed so far, counted by a diagnostic build: %u)\n", (int)run, itr,
                (unsigned long long)cost, moves, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_it0).count(), h.mode_words_changed);
      converged = stop.step(cost, moves);
      if (cost < bestcost) {
        bestitr = itr; bestcost = cost;
        TM_HIP(hipMemcpyAsync(b.best_memb.p, b.memb.p, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
        TM_HIP(hipMemcpyAsync(b.best_cent.p, b.cent.p, (size_t)k * KM_ATTRS, hipMemcpyDeviceToDevice, stream));
      }
      prev_moves = moves;
    }
    if (bestcost < all_best) {  // 1078-1085: the first run with the strictly smallest cost
      all_best = bestcost;
      all_iters = bestitr;
      TM_HIP(hipMemcpyAsync(labels_out, b.best_memb.p, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
      TM_HIP(hipMemcpyAsync(cent_out, b.best_cent.p, (size_t)k * KM_ATTRS, hipMemcpyDeviceToDevice, stream));
    }
  }
  TM_HIP(hipStreamSynchronize(stream));
  if (cost_out) *cost_out = all_best;
  if (iters_out) *iters_out = all_iters;
  if (point_iters_out) *point_iters_out = point_iters;
  return TM_OK;
}

// the Pascal arrays' form: HOST pointers, an upload and a read-back round the device run
int run_kmodes(const uint8_t *rows, int64_t n, int k, int num_init, int nmod, int max_iter, int32_t *labels_out, uint8_t *cent_out, uint64_t *cost_out,
               int *iters_out, hipStream_t stream) {
  TM_TRY(require_device());
  TM_TRY(check_arguments(rows, n, k, nmod, labels_out, cent_out));
  DevBuf drows, dlab, dcen;
  TM_TRY(drows.alloc((size_t)n * KM_ATTRS)); TM_TRY(dlab.alloc((size_t)n * 4)); TM_TRY(dcen.alloc((size_t)k * KM_ATTRS));
  TM_HIP(hipMemcpyAsync(drows.p, rows, (size_t)n * KM_ATTRS, hipMemcpyHostToDevice, stream));
  TM_TRY(run_kmodes_dev(drows.as<uint8_t>(), n, k, num_init, nmod, max_iter, dlab.as<int32_t>(), dcen.as<uint8_t>(), cost_out, iters_out, nullptr, stream));
  TM_HIP(hipMemcpyAsync(labels_out, dlab.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipMemcpyAsync(cent_out, dcen.p, (size_t)k * KM_ATTRS, hipMemcpyDeviceToHost, stream));
  TM_HIP(hipStreamSynchronize(stream));
  return TM_OK;
}

}  // namespace tmx

extern "C" int tm_stage_kmodes_dev(const uint8_t *dev_rows, int64_t n, int num_clusters, int num_init, int num_modalities, int max_iter, int32_t *dev_labels,
                                   uint8_t *dev_centroids, uint64_t *host_cost, int *host_iters, int64_t *host_point_iters, void *stream) {
  return tmx::run_kmodes_dev(dev_rows, n, num_clusters, num_init, num_modalities, max_iter, dev_labels, dev_centroids, host_cost, host_iters, host_point_iters, (hipStream_t)stream);
}

extern "C" int tm_stage_kmodes(const uint8_t *host_rows, int64_t n, int num_clusters, int num_init, int num_modalities, int max_iter, int32_t *host_labels,
                               uint8_t *host_centroids, uint64_t *host_cost, int *host_iters, void *stream) {
  return tmx::run_kmodes(host_rows, n, num_clusters, num_init, num_modalities, max_iter, host_labels, host_centroids, host_cost, host_iters, (hipStream_t)stream);
}
