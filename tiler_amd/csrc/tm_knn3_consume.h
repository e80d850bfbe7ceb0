// tm_knn3_consume.h -- the third kernel of the third scan shape (tm_knn3.h): persistent workgroups that consume the groups' tile lists.
#pragma once
#include "tm_knn3_block.h"

namespace tmx {

constexpr int K3_XCD_RUN = 32 * K3_WGS;  // groups dealt to one XCD at a time (neighbours on the curve)

// TOPK: collection mode for the k nearest rows (ann_kdtree_short_search_multi, tilingencoder.pas:1563).  Every query comes with a threshold
// (an upper bound of its k-th smallest SSD, a.tau); nothing is seeded, the lists are judged against the thresholds' bounds, and instead of
// keeping a minimum the epilogue appends every row within the threshold to the query's candidate list and walks the threshold down its
// ladder (k3_epilogue_topk).  One sub-tile fewer per group pays for the ladder's counters in LDS.  a.split > 1: the group's list is
// shared by that many workgroups (passes over few queries would otherwise leave most of the chip idle).
template <int HT, int HQ, bool TD, bool TOPK>
__global__ __launch_bounds__(K3_NT) void k_knn_consume(const Knn3Args a) {
  constexpr int KT = 6 + HT, KQ = 6 + HQ;
  constexpr int T_BYTES = knn_pack_bytes(KT, 1), Q_BYTES = knn_pack_bytes(KQ, 0);
  constexpr int NS = TOPK ? k3_ns_topk(KQ) : k3_ns(KQ), NSP = (NS + 1) & ~1, NW = K3_NW, NT = K3_NT, LCAP = K3_LCAP;
  // one LDS object, carved by hand (16-byte aligned pieces)
  // (the collection mode's ladder base stands between the bests and the boxes; the nearest-neighbour scan has nothing there)
  constexpr int OFF_QN = NS * KQ * 1024, OFF_BEST = OFF_QN + NS * 128, OFF_BASE = OFF_BEST + NS * 256, OFF_QBOX = OFF_BASE + (TOPK ? NS * 128 : 0),
                OFF_QNP = OFF_QBOX + NS * 64, OFF_SMAX = OFF_QNP + NS * 128, OFF_QMASK = OFF_SMAX + 64, OFF_CTL = OFF_QMASK + 64, OFF_TROW = OFF_CTL + 64,
                OFF_TIDX = OFF_TROW + NW * 128, OFF_LTILE = OFF_TIDX + NW * 128, OFF_LLB = OFF_LTILE + LCAP * 4,
                OFF_RING = OFF_LLB + LCAP * NSP * 2, OFF_LAD = OFF_RING + K3_RING_BYTES, LDS_TOTAL = OFF_LAD + (TOPK ? NS * 32 * 16 : 0);
  static_assert(OFF_LAD == k3_lds_bytes(NS, KQ) + (TOPK ? NS * 128 : 0) && LDS_TOTAL <= K3_LDS, "LDS carve");
  __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_TOTAL];
  int *const s_qn = reinterpret_cast<int *>(lds + OFF_QN);                                  // [NS][32] 2 * (|q-c|^2 >> 1)
  unsigned long long *const s_best = reinterpret_cast<unsigned long long *>(lds + OFF_BEST);  // [NS][32] (d'' + 1) << 32 | original index
  [[maybe_unused]] unsigned *const s_base = reinterpret_cast<unsigned *>(lds + OFF_BASE);   // TOPK: [NS][32] the ladder's base
  [[maybe_unused]] int *const s_qbox = reinterpret_cast<int *>(lds + OFF_QBOX);             // [NS][16] (kept in the carve: the dense mode's home)
  unsigned *const s_smax = reinterpret_cast<unsigned *>(lds + OFF_SMAX);                    // [16] upper bound of sqrt(largest best + 1)
  unsigned *const s_qmask = reinterpret_cast<unsigned *>(lds + OFF_QMASK);                  // [16] non-zero high-digit chunks of each sub-tile
  int *const s_qnp = reinterpret_cast<int *>(lds + OFF_QNP);                                // [NS][32] |q-c|^2 over the first chunk's columns
  int *const s_ctl = reinterpret_cast<int *>(lds + OFF_CTL);                                // [0] list length, [1] cursor, [3] group, [K3_CTL_HEAD], [K3_CTL_TAIL] the ring's tickets
  unsigned *const s_ltile = reinterpret_cast<unsigned *>(lds + OFF_LTILE);                  // [LCAP]
  uint16_t *const s_llb = reinterpret_cast<uint16_t *>(lds + OFF_LLB);                      // [LCAP][NSP]
  [[maybe_unused]] unsigned *const s_lad = reinterpret_cast<unsigned *>(lds + OFF_LAD);     // TOPK: [NS][32][4] the ladder's 7 x 16-bit counters
  // The survivor queue (k3_ring_push / k3_ring_pop; nearest-neighbour lists with the first-chunk look): a wave either LOOKS -- pops a list
  // entry, loads the tile's chunk 0 and judges every sub-tile that wants the tile on it -- or RUNS CHAINS for a tile some look let through:
  // loads the tile whole and runs the chain of every surviving sub-tile from its start.  A tile none of whose blocks gets past its look is
  // never loaded beyond chunk 0.  Why the results are those of the loop that did both in one go:
  //   * a look against an older bound is only more permissive: bounds and bests only fall;
  //   * the chain task judges each survivor again, by pick's test on the entry's bound read again and the sub-tile's bound as it is now;
  //   * every row that reaches or ties a best still arrives at k3_epilogue's 64-bit atomic minimum, whose result does not depend on the
  //     order of arrival;
  //   * the stop rule of a sorted segment speaks about entries not yet popped and is untouched.
  // Chains run a little later than they did, so the bounds tighten a little later and a few more blocks pass their looks: the counters move,
  // the bests do not.
  [[maybe_unused]] unsigned long long *const s_ring = reinterpret_cast<unsigned long long *>(lds + OFF_RING);  // [K3_RING]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), half = lane >> 5;
  [[maybe_unused]] const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) uint8_t *)lds;  // the carve's own LDS address (0 where it is the kernel's only object)
#if TM_KNN3_STAMPS
  unsigned long long st_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, st_last = __builtin_amdgcn_s_memtime();
  const unsigned long long st_begin = st_last;
#endif
  // Persistent workgroups (one per CU): a workgroup draws query groups until none is left.  Groups are dealt in runs of K3_XCD_RUN
  // consecutive groups per XCD (the id is read from the hardware: placement is a matter of speed only); an XCD whose share is exhausted
  // helps the next one.
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  long long nblocks = 0, nloads = 0, npairs = 0, nlisted = 0, npopped = 0, nmfma = 0, nstopped = 0, nspairs = 0;
  unsigned nnosurv = 0, npushed = 0, nringfull = 0, nwhole = 0;
  const bool dense = a.mode == K3_MODE_DENSE, ordered = a.list_order != 0 && !dense;
  const bool chunk_first = !TOPK && a.first_chunk != 0 && !dense;  // a block is judged on its first chunk before its chain runs (k3_chunk_look)
  uint8_t *const s_trow = lds + OFF_TROW + wave * 128;  // this wave's tile: its 32 row terms over the first chunk's columns
  [[maybe_unused]] const unsigned *const s_tidx = reinterpret_cast<const unsigned *>(lds + OFF_TIDX + wave * 128);  // ... and its 32 original indices
  const int split = TOPK ? max(1, a.split) : 1;
  // the ring starts empty, once: its tickets run on from segment to segment and from group to group (the loop's first barrier orders this)
  if (tid < K3_RING) s_ring[tid] = 0;
  if (tid == 0) s_ctl[K3_CTL_HEAD] = s_ctl[K3_CTL_TAIL] = 0;
  const int64_t n_units = a.n_groups * split;  // what the tickets deal: (group, part of its list)
  for (;;) {
  __syncthreads();  // the previous group's LDS is no longer read
  if (tid == 0) {
    int64_t gsel = -1;
    for (int k = 0; k < 8 && gsel < 0; k++) {
      const unsigned x = (xcc + k) & 7u;
      const unsigned t = atomicAdd(&a.tickets[x], 1u);
      const int64_t gg = ((int64_t)(t / K3_XCD_RUN) * 8 + x) * K3_XCD_RUN + (t % K3_XCD_RUN);
      if (gg < n_units) gsel = gg;
    }
    s_ctl[3] = (int)gsel;
  }
  __syncthreads();
  const int64_t unit = __builtin_amdgcn_readfirstlane(s_ctl[3]);
  if (unit < 0) break;
  const int64_t g = unit / split;
  const int part = (int)(unit - g * split);
  const int64_t st0 = g * NS;
  const int nvalid = (int)min((int64_t)NS, a.n_qtiles - st0);
  const int64_t n_ttiles = a.n_ttiles;

  // ---- prologue: the group's query operands, norms, and what the seeds left
  // (each phase outside the consume loop takes its thread index afresh, through an empty asm the compiler cannot see through: otherwise
  // the addresses it derives from it are computed once, before the persistent loop, and live -- spilled -- across the consume loop)
  int tp = threadIdx.x;
  asm volatile("" : "+v"(tp));
  for (int piece = wave; piece < NS * KQ; piece += NW) {
    const int s = piece / KQ, kc = piece - s * KQ;
    const int64_t st = min(st0 + s, a.n_qtiles - 1);
    const uint8_t *src = a.qpack + st * (int64_t)Q_BYTES + kc * 1024 + lane * 16;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)(lds + piece * 1024), 16, 0, 0);
  }
  for (int i = tp; i < NS * 32; i += NT) {
    const int64_t st = min(st0 + (i >> 5), a.n_qtiles - 1);
    const bool real = (i >> 5) < nvalid && !dense;
    s_qn[i] = reinterpret_cast<const int *>(a.qpack + st * (int64_t)Q_BYTES + knn_pack_row_terms(KQ))[i & 31] & ~1;
    if constexpr (!TOPK) s_qnp[i] = reinterpret_cast<const int *>(a.qpack + st * (int64_t)Q_BYTES + knn_pack_first_terms(KQ, 0))[i & 31];
    if constexpr (TOPK) {  // (tau + 1) << 32 | rung spacing; queries that are padding get tau = -1: nothing is within it
      const bool qreal = real && st0 * 32 + i < a.nq;
      const int tau = qreal ? a.tau[st0 * 32 + i] : -1;
      int stp = tau > 0 ? tau >> 3 : 0;  // (seven rungs fit below the threshold whatever the host asks for)
      if (a.step && qreal && stp > 0) stp = min(stp, max(1, a.step[st0 * 32 + i]));
      s_best[i] = ((unsigned long long)(unsigned)(tau + 1) << 32) | (unsigned)stp;
      s_base[i] = (unsigned)(tau + 1);  // the ladder's base
      for (int w = 0; w < 4; w++) s_lad[i * 4 + w] = 0;
    } else {
      s_best[i] = real ? a.gbest[st0 * 32 + i] : ~0ull;
    }
  }
  if (tp < 16) {
    s_smax[tp] = (tp < nvalid && !dense) ? a.gsmax[st0 + tp] : K3_LB_MAX;
    s_qmask[tp] = tp < nvalid ? (unsigned)a.qmeta[qmeta_at(st0 + tp, QMETA_HMASK)] : 0u;
  }
  const int nseg = dense ? (int)((n_ttiles + LCAP - 1) / LCAP) : a.nsegs[g];
  __syncthreads();  // (waits for the LDS-DMA pieces too)
  // Where this lane's query sits in a sub-tile's operands, bests and norms (LDS byte offsets): a block adds the sub-tile's part, which is
  // wave-uniform, with one instruction each (made from the sub-tile's index per block, the three addresses took six, a multiply among them)
  // (made per group from a thread index taken afresh, like the other phases' addresses: see the prologue)
  unsigned tb = threadIdx.x;
  asm volatile("" : "+v"(tb));
  const unsigned qmask_v = s_qmask[tb & 15u];  // lane s: sub-tile s's mask of non-zero high-digit chunks
  unsigned a_q = (tb & 63u) * 16u, a_best = (unsigned)OFF_BEST + (tb & 31u) * 8u, a_qn = (unsigned)OFF_QN + (tb & 31u) * 4u;
  asm volatile("" : "+v"(a_q), "+v"(a_best), "+v"(a_qn));
  K3_STAMP(0);  // prologue

  for (int seg = 0; seg < nseg; seg++) {
    // ---------------------------------------------------------------- the next segment of the group's tile list, into LDS
    int list_n;
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    if (dense) {  // every tile, every sub-tile
      list_n = (int)min((int64_t)LCAP, n_ttiles - (int64_t)seg * LCAP);
      for (int i = tl; i < list_n; i += NT) {
        s_ltile[i] = k3_entry(seg * LCAP + i, a.thmask);
        for (int p = 0; p < NSP; p++) s_llb[i * NSP + p] = p < nvalid ? 0 : K3_LB_NONE;
      }
    } else {
      const uint2 sg = a.segs[g * a.max_segs + seg];
      list_n = (int)sg.y;
      if (list_n != 0 && ((unsigned long long)sg.x + sg.y > a.arena_cap || list_n > LCAP)) {  // never by construction (a segment that did not fit the arena has 0 entries): a guard against a corrupted segment table
        if (tl == 0) atomicMax(a.stats + K3S_GUARD, 0x100000000ull | sg.y);
        list_n = 0;
      }
      for (int i = tl; i < list_n; i += NT) s_ltile[i] = a.ltile[sg.x + i];
      const unsigned *src = reinterpret_cast<const unsigned *>(a.llb) + (size_t)sg.x * (NSP / 2);
#pragma unroll 1
      for (int i = tl; i < list_n * (NSP / 2); i += NT) reinterpret_cast<unsigned *>(s_llb)[i] = src[i];
    }
    if (tl == 0) s_ctl[1] = 0;
    __syncthreads();
    K3_STAMP(1);  // segment load
    // ---------------------------------------------------------------- consume: every wave on its own
    {
      nlisted += (wave == 0) ? (TOPK ? (list_n - part + split - 1) / split : list_n) : 0;  // (a split list: this part's entries)
      auto next_entry = [&](int &j_o, int &tile_o, unsigned &tm_o, int &lb_o, unsigned &mask_o) -> bool {
        for (;;) {
          int j = 0;
          if (lane == 0) j = atomicAdd(&s_ctl[1], 1);
          j = __builtin_amdgcn_readfirstlane(j);
          if (TOPK) j = j * split + part;  // a split group: this workgroup takes every split-th entry
          if (j >= list_n) return false;
          npopped++;
#if TM_KNN3_REFRESH_EVERY
          if ((j & (TM_KNN3_REFRESH_EVERY - 1)) == TM_KNN3_REFRESH_EVERY - 1)
            for (int s = 0; s < nvalid; s++)  // every so many entries the popping wave makes every sub-tile's bound anew from its bests: what the
                                              // races of the refresh rule left loose ends here (the second shape did this at every list's end)
              K3_REFRESH_BOUND(&s_smax[s], reinterpret_cast<unsigned *>(s_best) + (s * 32 + (lane & 31)) * 2 + 1);
#endif
          const int t = (int)s_ltile[j];
          const int lb = lane < NSP ? (int)s_llb[j * NSP + lane] : (int)K3_LB_NONE;
          const int sm = lane < NS ? (int)k3_peek(&s_smax[lane]) : -1;
          const unsigned m = (unsigned)__builtin_amdgcn_ballot_w64(lb <= sm);
          if (m) { j_o = j; tile_o = __builtin_amdgcn_readfirstlane((int)k3_entry_tile((unsigned)t)); tm_o = k3_entry_mask((unsigned)__builtin_amdgcn_readfirstlane(t)); lb_o = lb; mask_o = m; return true; }
          // Nobody wants the entry.  In a sorted segment (k_knn_lists' flush) its smallest listed bound is the smallest of every entry behind
          // it as well, and a sub-tile's bound only falls: once that key lies above the largest bound of the group, no later entry can be
          // wanted by anyone, now or later -- today's skip rule applied to the segment's tail at once.  The pop counter goes to the end so that
          // the other waves stop too.  (A tile holding a row at some query's current minimum has a bound within its sub-tile's: what raises a tie
          // flag is never behind the stop.  Collection mode: the same rule on thresholds that only fall; a part of a split list sees its own
          // entries in ascending order.)
          if (ordered) {
            const unsigned smx = k3_wave_umax(lane < nvalid ? (unsigned)sm : 0u);
            if (__builtin_amdgcn_ballot_w64(lb <= (int)smx) == 0) {
              if (lane == 0) atomicMax(&s_ctl[1], list_n);
              return false;
            }
          }
        }
      };
      // a list entry outside the database -- never by construction: a guard, the loads must not follow it.  The wave takes no more entries.
      auto tile_in_range = [&](int tile) -> bool {
        if (tile < n_ttiles) return true;
        if (lane == 0) atomicMax(a.stats + K3S_GUARD, 0x200000000ull | (unsigned)tile);
        return false;
      };
      // the next sub-tile of `mask` that still wants the tile (its best may have tightened since the entry was popped; `lbv`: lane s holds the
      // entry's bound for sub-tile s); -1: none left
      auto pick = [&](unsigned &mask, int lbv, unsigned &sm_o) -> int {
        while (mask) {
          const int s = __builtin_ctz(mask);
          mask &= mask - 1;
          const int lbs = __builtin_amdgcn_readlane(lbv, s);
          const unsigned sm_now = (unsigned)__builtin_amdgcn_readfirstlane((int)k3_peek(&s_smax[s]));  // (the bound as it is now, not as the pop saw it)
          if (lbs > (int)sm_now) continue;
          sm_o = sm_now;
          return s;
        }
        return -1;
      };
      // One block from its chain on: sub-tile s0 against the tile in T / cin / pwh.
      // The sub-tile's mask comes out of a register (lane s of qmask_v), the query's best and norm are asked for before the chain: every
      // LDS round trip a block can do without, or start early, is one the wave does not sit out between its matrix instructions
      // (s_setprio 2 around the chain -- a wave inside its chain ahead of the waves between chains -- measured: no change)
      // (measured in round 5 and dropped: every product's operand read one product ahead -- the reads issued whatever the predicates say, with
      // no lane enabled where the product will not run, so that the waits can name the read they need: 13.5 against 11.8 ms; the thirteen
      // reads that read nothing still pass through the CU's one LDS queue)
      auto run_block = [&](const v4i (&T)[KT], const v16i &cin, unsigned pwh, int tile, int vt, unsigned tm, int s0, unsigned sm0) {
        const unsigned qm0 = (unsigned)__builtin_amdgcn_readlane((int)qmask_v, s0);
        unsigned long long *const bp = reinterpret_cast<unsigned long long *>(lds + (a_best + (unsigned)s0 * 256u));  // &s_best[s0 * 32 + (lane & 31)]
        const unsigned cur0 = TOPK ? 0u : k3_peek(reinterpret_cast<unsigned *>(bp) + 1);
        const unsigned qn0 = (unsigned)*reinterpret_cast<const int *>(lds + (a_qn + (unsigned)s0 * 128u));  // s_qn[s0 * 32 + (lane & 31)]
        // (the sub-tile's operands begin at s0 * KQ KB: a product the compiler makes on the vector unit, a 24-bit multiply, unless told otherwise)
        unsigned q_off;
        asm("s_mul_i32 %0, %1, %2" : "=s"(q_off) : "s"(s0), "n"(KQ * 1024));
        const v16i acc = k3_chain<HT, HQ, TD>(T, cin, lds + (a_q + q_off), tm, qm0);
        nmfma += k3_chain_products<HT, HQ>(tm, qm0);
        K3_STAMP(6);  // the chain, up to the issue of its last matrix instruction
        // the block's epilogue and the refresh of its sub-tile's bound
        bool refresh;
        if constexpr (TOPK) {
          const int qi = s0 * 32 + (lane & 31);
          const int64_t q = (st0 + s0) * 32 + (lane & 31);
          // (the last database tile pads with copies of its last row: they are candidates like any row -- the select stage drops them --
          // but must not count towards a rung)
          refresh = k3_epilogue_topk<TD>(acc, pwh, tile, tile != (int)n_ttiles - 1, half, qn0, &s_best[qi], &s_lad[qi * 4], &s_base[qi], q < a.nq, q, a, sm0);
        } else {
          refresh = k3_epilogue<TD, true>(acc, pwh, s_tidx, half, qn0, bp, sm0, cur0);
        }
        if (__builtin_amdgcn_ballot_w64(refresh)) K3_REFRESH_BOUND(&s_smax[s0], reinterpret_cast<unsigned *>(bp) + 1);  // the sub-tile's largest best may have moved
        nblocks++;
        npairs += (long long)vt * (int)min((int64_t)32, a.nq - (st0 + s0) * 32);
        K3_STAMP(7);  // the epilogue (behind the wait for the chain's result)
      };
      if constexpr (TOPK) {
        // ------------------------------------------------ collection mode: every popped tile is loaded whole, every block runs its chain
        int j = 0, tile = 0, lbv = 0;
        unsigned mask = 0, tmw = 0;
        bool have = next_entry(j, tile, tmw, lbv, mask);
        while (have && tile_in_range(tile)) {
          const unsigned tm = tmw;
          v4i T[KT];
          v16i cin;
          unsigned pwh;
          if constexpr (!TOPK)  // (asked for first: whatever later load of the tile the wave waits for, this one is older)
            k3_stage_tile_idx(a.tpack + (int64_t)tile * T_BYTES + knn_pack_indices(KT), (unsigned)(OFF_TIDX + wave * 128) + lds_base, lane);
          k3_load_tile_masked<KT>(a.tpack + (int64_t)tile * T_BYTES, lane, half, tm, T, cin, pwh);
          nloads++;
          // the entry after this one is chosen while the loads fly
          int nj = 0, ntile = 0, nlb = 0;
          unsigned nmask = 0, ntm = 0;
          const bool nhave = next_entry(nj, ntile, ntm, nlb, nmask);
#if TM_KNN3_STAMPS
          K3_STAMP(2);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          K3_STAMP(4);  // waiting for the tile's loads (what is left of their latency behind the choice of the next entry)
#endif
          const int vt = (int)min((int64_t)32, a.nt_rows - (int64_t)tile * 32);
          for (;;) {
            unsigned sm0 = 0;
            const int s0 = pick(mask, lbv, sm0);
            K3_STAMP(5);  // choosing the block's sub-tile (the bound's fresh look)
            if (s0 < 0) break;
            run_block(T, cin, pwh, tile, vt, tm, s0, sm0);
          }
          tile = ntile; tmw = ntm; lbv = nlb; mask = nmask; have = nhave;
        }
      } else {
        // ------------------------------------------------ two tasks: looks, and chains for the tiles a look has let through (the survivor queue)
        // Without the look (dense mode, TM_KNN_FIRST_CHUNK=0) the look task only pops: every sub-tile the pop found wanting is a survivor, and
        // the wave runs the chain task for the entry itself, at once -- every popped tile loaded whole, every block's chain run, through the
        // one chain task the kernel has.
        // a popped entry's chunk 0: all a look reads of the tile (k3_load_tile_chunk0)
        int j = 0, tile = 0, lbv = 0;
        unsigned mask = 0, tmw = 0;
        v4i c0 = {0, 0, 0, 0}, c6 = {0, 0, 0, 0};
        unsigned rowp = 0;
        auto load_chunk0 = [&](int tile_, unsigned tm_, v4i &c0_, v4i &c6_, unsigned &rowp_) {
          v4i T[KT];
          int tk = threadIdx.x;
          asm volatile("" : "+v"(tk));
          k3_load_tile_chunk0<KT>(a.tpack + (int64_t)tile_ * T_BYTES, tk & 63, tm_, T, rowp_);
          c0_ = T[0];
          if constexpr (KT > 6) c6_ = T[6];
        };
        // (what steers the loop is wave-uniform, and passes through readfirstlane so that the compiler knows: taken for lane masks, the flags and
        // every counter behind them went to vector registers, the counters to scratch)
        auto uniform = [](bool b) -> bool { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; };
        bool have = uniform(next_entry(j, tile, tmw, lbv, mask) && tile_in_range(tile));
        if (have && chunk_first) load_chunk0(tile, tmw, c0, c6, rowp);
        unsigned own = 0;       // a survivor entry the ring had no room for: this wave's next task
        bool draining = false;  // behind the segment's first barrier: nobody pushes any more
        for (;;) {
          // a wave prefers the queue: a survivor if one is ready, a list entry otherwise; no wave waits for another (k3_ring_pop)
          unsigned ent = own;
          own = 0;
          if (ent == 0) ent = k3_ring_pop(s_ring, &s_ctl[K3_CTL_HEAD], lane);
          ent = (unsigned)__builtin_amdgcn_readfirstlane((int)ent);
          if (ent == 0) {
            if (draining) break;
            if (!have) {  // the list is at its end and the ring looked empty: what the last lookers pushed is taken behind this barrier
              __syncthreads();
              draining = true;
              continue;
            }
            // -------------------------------------------- look task: chunk 0 of the entry against every sub-tile that still wants the tile
            // (the entry after this one is popped, and its chunk 0 asked for, before the look: a looker holds nine registers of a tile where the
            // whole tile takes 44, so the next tile's latency passes behind this tile's looks)
            int nj = 0, ntile = 0, nlb = 0;
            unsigned nmask = 0, ntm = 0;
            v4i n0 = {0, 0, 0, 0}, n6 = {0, 0, 0, 0};
            unsigned nrowp = 0;
            const bool nhave = uniform(next_entry(nj, ntile, ntm, nlb, nmask) && tile_in_range(ntile));
            if (nhave && chunk_first) load_chunk0(ntile, ntm, n0, n6, nrowp);
            nloads++;
            K3_STAMP(2);
            const int vt = (int)min((int64_t)32, a.nt_rows - (int64_t)tile * 32);
            // (the wave's own 128 bytes: its looks at the tile before read them in program order, its looks at this one read what is written here)
            if (chunk_first) {
              int tw = threadIdx.x;
              asm volatile("" : "+v"(tw));
              if ((tw & 63) < 32) reinterpret_cast<unsigned *>(s_trow)[tw & 63] = rowp;
            }
            K3_STAMP(4);  // waiting for the tile's chunk 0
            v4i T[KT];
            T[0] = c0;
            if constexpr (KT > 6) T[6] = c6;
            unsigned surv = chunk_first ? 0u : mask;
            // a block's operands, norm and best for its look
            auto q_of = [&](int s_) -> const uint8_t * {
              // (the sub-tile's operands begin at s * KQ KB: a product the compiler makes on the vector unit, a 24-bit multiply, unless told otherwise)
              unsigned q_off;
              asm("s_mul_i32 %0, %1, %2" : "=s"(q_off) : "s"(s_), "n"(KQ * 1024));
              return lds + (a_q + q_off);
            };
            auto qnp_of = [&](int s_) { return reinterpret_cast<const int *>(lds + (a_qn + (unsigned)(OFF_QNP - OFF_QN) + (unsigned)s_ * 128u)); };  // &s_qnp[s * 32 + (lane & 31)]
            auto cur_of = [&](int s_) { return k3_peek(reinterpret_cast<unsigned *>(lds + (a_best + (unsigned)s_ * 256u)) + 1); };
            // the verdict of a look: a survivor, or a block that ends here (no query of the sub-tile can gain from the tile, or tie with it)
            auto verdict = [&](int s_, bool in) {
              if (__builtin_amdgcn_ballot_w64(in) != 0) {
                surv |= 1u << s_;
              } else {
                nstopped++;
                nspairs += (long long)vt * (int)min((int64_t)32, a.nq - (st0 + s_) * 32);  // (counted apart: `pairs` are those of the blocks that ran to completion)
              }
            };
            while (chunk_first) {
              // two sub-tiles at a time (k3_chunk_look2), an odd one on its own
              unsigned sm0 = 0;
              const int sa = pick(mask, lbv, sm0);
              if (sa < 0) break;
              const int sb = pick(mask, lbv, sm0);
              if (sb >= 0) {
                bool ina, inb;
                k3_chunk_look2<HT, HQ, TD>(T, s_trow, half, q_of(sa), q_of(sb), qnp_of(sa), qnp_of(sb), cur_of(sa), cur_of(sb), ina, inb);
                nmfma += 2 * k3_chunk_look2_products<HT, HQ>();
                verdict(sa, ina);
                verdict(sb, inb);
              } else {
                const unsigned qm0 = (unsigned)__builtin_amdgcn_readlane((int)qmask_v, sa);
                const bool in = k3_chunk_look<HT, HQ, TD>(T, s_trow, half, q_of(sa), tmw, qm0, qnp_of(sa), cur_of(sa));
                nmfma += k3_chunk_look_products<HT, HQ>(tmw, qm0);
                verdict(sa, in);
              }
            }
            K3_STAMP(5);  // the looks
            surv = (unsigned)__builtin_amdgcn_readfirstlane((int)surv);  // (wave-uniform, and the compiler is to know)
            if (surv == 0) {
              nnosurv++;  // nothing else of the tile is ever loaded
            } else {
              const unsigned e = k3_surv_make(j, surv);
              if (!chunk_first) own = e;  // (not counted: the queue is not in use)
              else if (k3_ring_push(s_ring, &s_ctl[K3_CTL_HEAD], &s_ctl[K3_CTL_TAIL], e, lane)) npushed++;
              else { nringfull++; own = e; }  // a full ring is not waited on
            }
            j = nj; tile = ntile; tmw = ntm; lbv = nlb; mask = nmask; have = nhave;
            c0 = n0; c6 = n6; rowp = nrowp;
            continue;
          }
          // ---------------------------------------------- chain task: the whole tile, and a chain for every survivor that still wants it
          const int ej = (int)k3_surv_entry(ent);
          unsigned surv = k3_surv_mask(ent);
          const unsigned tw = (unsigned)__builtin_amdgcn_readfirstlane((int)s_ltile[ej]);
          const int ctile = (int)k3_entry_tile(tw);
          const unsigned ctm = k3_entry_mask(tw);
          if (!tile_in_range(ctile)) continue;  // (the look's guard has seen the entry: twice never)
          v4i T[KT];
          v16i cin;
          unsigned pwh;
          // (each task takes its thread index afresh, like the phases outside the loop: the addresses of one task's loads are not kept, spilled,
          // across the other)
          int tc = threadIdx.x;
          asm volatile("" : "+v"(tc));
          k3_stage_tile_idx(a.tpack + (int64_t)ctile * T_BYTES + knn_pack_indices(KT), (unsigned)(OFF_TIDX + wave * 128) + lds_base, tc & 63);
          k3_load_tile_masked<KT>(a.tpack + (int64_t)ctile * T_BYTES, tc & 63, (tc >> 5) & 1, ctm, T, cin, pwh);
#if TM_KNN3_STAMPS
          K3_STAMP(2);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          K3_STAMP(4);  // waiting for the whole tile
#endif
          const int cvt = (int)min((int64_t)32, a.nt_rows - (int64_t)ctile * 32);
          nwhole++;
          while (surv) {
            const int s0 = __builtin_ctz(surv);
            surv &= surv - 1;
            // pick's test again, with the entry's bound read again and the sub-tile's bound as it is now
            const int lbs = __builtin_amdgcn_readfirstlane((int)s_llb[ej * NSP + s0]);
            const unsigned sm0 = (unsigned)__builtin_amdgcn_readfirstlane((int)k3_peek(&s_smax[s0]));
            K3_STAMP(5);
            if (lbs > (int)sm0) {  // the bound fell below the tile while the entry waited: the block ends behind its look after all
              if (chunk_first) {
                nstopped++;
                nspairs += (long long)cvt * (int)min((int64_t)32, a.nq - (st0 + s0) * 32);
              }
              continue;
            }
            run_block(T, cin, pwh, ctile, cvt, ctm, s0, sm0);
          }
        }
      }
    }
    K3_STAMP(2);  // consuming
    __syncthreads();  // (the two-task loop: its second barrier -- every survivor's chain has run)
    if (seg + 1 < nseg)
      for (int s = wave; s < nvalid; s += NW)  // every sub-tile's bound made anew from its bests: what the races of the refresh rule left loose ends here
        K3_REFRESH_BOUND(&s_smax[s], reinterpret_cast<unsigned *>(s_best) + (s * 32 + (lane & 31)) * 2 + 1);
    K3_STAMP(3);  // waiting for the other waves at the end of a segment
  }

  // ---- results, in the format k_knn_refine reads
  int tr = threadIdx.x;
  asm volatile("" : "+v"(tr));
  for (int i = tr; i < NS * 32; i += NT) {
    const int64_t st = st0 + (i >> 5);
    if (st >= a.n_qtiles) continue;
    const unsigned long long k = s_best[i];
    const unsigned hi = (unsigned)(k >> 32);
    const int64_t q = st * 32 + (i & 31);
    if constexpr (TOPK) {  // the final threshold: k_topk_select drops the stored candidates above it
      if (q < a.nq && hi > 0) atomicMin(&a.tau[q], (int)(hi - 1u));
    } else {
      a.best_key[q] = (int)(hi - 1u);
      a.best_tile[q] = (int)(unsigned)k;  // the winner's original index
    }
  }
  K3_STAMP(0);  // results (counted with the prologue)
  }  // next query group
#if TM_KNN3_STAMPS
  if (a.stats && lane == 0) {
    for (int i = 0; i < 5; i++) atomicAdd(a.stats + K3S_STAMPS + i, st_acc[i]);
    atomicAdd(a.stats + K3S_STAMPS + 5, __builtin_amdgcn_s_memtime() - st_begin);
    for (int i = 5; i < 8; i++) atomicAdd(a.stats + K3S_STAMPS_IN + (i - 5), st_acc[i]);  // inside "consume"
  }
#endif
  if (a.stats && lane == 0) {
    atomicAdd(a.stats + K3S_BLOCKS, (unsigned long long)nblocks);
    atomicAdd(a.stats + K3S_TILES, (unsigned long long)nloads);
    atomicAdd(a.stats + K3S_PAIRS, (unsigned long long)npairs);
    if (wave == 0) atomicAdd(a.stats + K3S_LISTED, (unsigned long long)nlisted);
    atomicAdd(a.stats + K3S_POPPED, (unsigned long long)npopped);
    atomicAdd(a.stats + K3S_MFMA, (unsigned long long)nmfma);  // matrix instructions issued (a full chain has 6 + HT + HQ + min(HT, HQ)), the first-chunk looks' included
    if (nstopped) { atomicAdd(a.stats + K3S_STOPPED, (unsigned long long)nstopped); atomicAdd(a.stats + K3S_STOPPED_PAIRS, (unsigned long long)nspairs); }
    if (nnosurv) atomicAdd(a.stats + K3S_NOSURV, (unsigned long long)nnosurv);
    if (npushed) atomicAdd(a.stats + K3S_PUSHED, (unsigned long long)npushed);
    if (nringfull) atomicAdd(a.stats + K3S_RINGFULL, (unsigned long long)nringfull);
    if (nwhole) atomicAdd(a.stats + K3S_WHOLE, (unsigned long long)nwhole);
  }
}

}  // namespace tmx
