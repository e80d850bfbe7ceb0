"""The cases of tests/palette_cases.py reach what they claim to reach -- asserted on the oracle's output alone (no GPU, no library): which
blocks and shares of k_pp_pick the seeds fall in, how wide the masses get, which palettes tie, how many distinct colours a palette holds.
The GPU comparisons on the same inputs are in tests/test_gpu_prepare_palettes.py."""
import numpy as np
import pytest

from tests import palette_cases as pc


@pytest.fixture(scope="module")
def size_seeds(oracle):
    """(kind, n) -> the oracle's seeds, for every size case of the seeding"""
    out = {}
    for kind, n in pc.SEED_SIZE_CASES:
        pts, w, k = pc.seed_size_case(kind, n)
        out[kind, n] = oracle.kmeans_pp_seeds(pts, w, k)
    return out


def test_seed_sizes_cover_the_block_and_share_counts():
    assert [pc.pp_blocks(n) for n in pc.SEED_SIZES] == [1, 1, 1, 2, 3, 256, 257, 391, 513]
    assert [pc.pp_per(n) for n in pc.SEED_SIZES] == [1, 1, 1, 1, 1, 1, 2, 2, 3]
    assert all(pc.seed_k(n) == (4 if n > 2000 else 16) for n in pc.SEED_SIZES)
    for kind, n in pc.SEED_SIZE_CASES:
        assert np.abs(pc.seed_size_case(kind, n)[0]).max() <= pc.COORD
    for name in pc.SEED_EDGE_CASES:
        assert np.abs(pc.seed_edge_case(name)[0]).max() <= pc.COORD
    for name, _, _ in pc.PALETTIZE_CASES:
        assert np.abs(pc.palettize_case(name)[0]).max() <= pc.COORD


def test_seeds_fall_where_the_group_claims(size_seeds):
    found = {"last-index": [], "last-partial-block": [], "block-0": [], "not-first-of-share": [], "last-share": [], "every-pick-made": True}
    for (kind, n), seeds in size_seeds.items():
        nb, per = pc.pp_blocks(n), pc.pp_per(n)
        assert len(seeds) == min(pc.seed_k(n), n) and len(set(seeds.tolist())) == len(seeds), (kind, n)
        last_share = (nb - 1) // per  # the last thread of k_pp_pick that owns a block
        for s in seeds.tolist():
            assert 0 <= s < n
            b = s // pc.PP_BLOCK
            if s == n - 1:
                found["last-index"].append((kind, n))
            if b == nb - 1 and n % pc.PP_BLOCK:
                found["last-partial-block"].append((kind, n))
            if b == 0 and nb > 1:
                found["block-0"].append((kind, n))
            if per >= 2 and b % per != 0:
                found["not-first-of-share"].append((kind, n))
            if per >= 2 and b // per == last_share:
                found["last-share"].append((kind, n))
    for what in ("last-index", "last-partial-block", "block-0", "not-first-of-share", "last-share"):
        assert found[what], what
    # each of them at a size with more than one block a thread, and per = 3 reaches the second and the third block of a share
    for what in ("last-index", "last-partial-block", "block-0"):
        assert any(pc.pp_per(n) >= 2 for _, n in found[what]), what
    rests = {(s // pc.PP_BLOCK) % 3 for kind in ("plain", "shaped") for s in size_seeds[kind, 262145].tolist()}
    assert rests == {0, 1, 2}


def test_plain_twins_pick_away_from_the_heavy_points(size_seeds):
    """the plain cases are not the shaped ones again: their picks are decided by sums of many small masses"""
    for n in (131073, 200000, 262145):
        assert set(size_seeds["plain", n].tolist()) != set(size_seeds["shaped", n].tolist())


def test_wide_masses_need_the_high_word(oracle):
    pts, w, k = pc.seed_edge_case("wide-masses")
    assert pts.shape[0] == pc.WIDE_N and int(w.min()) >= 1 << 31
    seeds = oracle.kmeans_pp_seeds(pts, w, k)
    assert len(seeds) == k
    total = sum(pc.pp_masses(pts, w, seeds[:1]))
    assert total > 1 << 64 and total.bit_length() >= 80
    assert sum(pc.pp_masses(pts, w, [])) < 1 << 64  # (the first pick's total is the sum of the weights)


def test_one_wide_mass_is_the_only_high_word(oracle):
    pts, w, k = pc.seed_edge_case("one-wide-mass")
    assert int((w >= 1 << 31).sum()) == 1 and int(w[pc.WIDE_POINT]) >= 1 << 31
    seeds = oracle.kmeans_pp_seeds(pts, w, k)
    assert len(seeds) == k and seeds[0] != pc.WIDE_POINT  # still unpicked at the second pick
    mass = pc.pp_masses(pts, w, seeds[:1])
    assert [i for i, m in enumerate(mass) if m >> 64] == [pc.WIDE_POINT]
    assert sum(mass) > 1 << 64
    lows = sum(m & ((1 << 64) - 1) for m in mass)
    assert lows >> 64  # the low words carry on their own


def test_no_weights_case(oracle):
    pts, w, k = pc.seed_edge_case("no-weights")
    assert w is None and pts.shape[0] == 1025 and len(oracle.kmeans_pp_seeds(pts, w, k)) == k


@pytest.mark.parametrize("name", ["zero-weights-third", "zero-weights-end-blocks"])
def test_zero_weights_are_never_seeds(oracle, name):
    pts, w, k = pc.seed_edge_case(name)
    assert pts.shape[0] == 1500 and int((w == 0).sum()) >= 500
    if name == "zero-weights-end-blocks":
        assert not w[:512].any() and not w[1024:].any() and w[512:1024].all()
    seeds = oracle.kmeans_pp_seeds(pts, w, k)
    assert len(seeds) == k and (w[seeds] > 0).all()


def test_duplicates_end_the_seeding_on_a_zero_total(oracle):
    pts, w, k = pc.seed_edge_case("duplicates")
    assert pts.shape[0] == 1300 and len(np.unique(pts, axis=0)) == 5 and k == 16
    seeds = oracle.kmeans_pp_seeds(pts, w, k)
    assert len(seeds) == 5
    assert sum(pc.pp_masses(pts, w, seeds)) == 0 and sum(pc.pp_masses(pts, w, seeds[:4])) > 0


def test_palettize_cases(oracle):
    names = [c[0] for c in pc.PALETTIZE_CASES]
    assert {"full-%d-%d" % (n, p) for n in (1500, 3000) for p in (1, 2, 16, 40)} <= set(names)
    feat, use = pc.palettize_case("one-iteration")
    assert feat.shape[0] == 140000 and pc.pp_per(feat.shape[0]) == 2 and (feat.shape[0] + 255) // 256 > 512
    # two palettes end with equal tile counts, and they are different palettes: the rank of each is decided by the initial order alone
    feat, use = pc.palettize_case("ranking-tie")
    idx = oracle.palettize(feat, use, 4)
    assert sorted(np.bincount(idx, minlength=4).tolist(), reverse=True) == sorted(pc.TIE_SIZES, reverse=True)
    assert np.bincount(idx, minlength=4)[1] == np.bincount(idx, minlength=4)[2] == 400
    # fewer distinct points than palettes: the palettes beyond the five found own no tile and rank last
    feat, use = pc.palettize_case("duplicates")
    idx = oracle.palettize(feat, use, 16)
    cnt = np.bincount(idx, minlength=16)
    assert (cnt[:5] > 0).all() and not cnt[5:].any()


def test_long_resident_cases_reuse_a_delta_buffer(oracle):
    for name, npal, workgroups in pc.LONG_RESIDENT_CASES:
        feat, use = pc.palettize_case(name)
        assert (feat.shape[0] + 1023) // 1024 == workgroups < 4 and npal == 16
        kk, assign, _, iters = oracle.kmeans_pp(feat, use, npal)
        assert kk == 16 and iters >= 9, (name, iters)
        assert np.bincount(assign, minlength=16)[5:].all()  # the centroids whose sums lie beyond the first 1 024 entries of a buffer own tiles


def test_km3_size_cases_are_distinct_colours():
    assert sorted({n for n, _ in pc.KM3_SIZE_CASES}) == [4095, 4096, 4097, 12289, 40000]
    assert {k for n, k in pc.KM3_SIZE_CASES if n == 12289} == {2, 16, 64}
    for n in sorted({n for n, _ in pc.KM3_SIZE_CASES}):
        pts, w = pc.km3_size_case(n)
        assert pts.shape == (n, 3) and len(np.unique(pts, axis=0)) == n and pts.min() >= 0 and pts.max() <= 255
        assert 4000 < int(w.max()) <= 5000 and int(w.min()) >= 1


def test_km3_edge_cases(oracle):
    for name in pc.KM3_EDGE_CASES:
        pts, w, k = pc.km3_edge_case(name)
        assert pts.shape[0] > 2 * pc.P3_ROWS and k == 16 and pts.min() >= 0 and pts.max() <= 255  # three workgroups
    pts, w, k = pc.km3_edge_case("lattice-ties")
    assert not (pts % 32).any() and len(np.unique(pts, axis=0)) < pts.shape[0] // 10
    pts, w, k = pc.km3_edge_case("one-cluster-far")
    far = (pts > 200).all(1)
    assert int(far.sum()) == 40 and pts[~far].max() <= 40
    # the farthest-first tie: three points at the largest distance from point 0, one per workgroup; the lowest index wins
    pts, w, k = pc.km3_edge_case("pick-tie-across-workgroups")
    d2 = ((pts.astype(np.int64) - pts[0]) ** 2).sum(1)
    assert sorted(np.nonzero(d2 == d2.max())[0].tolist()) == list(pc.TIE_AT) and [i // pc.P3_ROWS for i in pc.TIE_AT] == [0, 1, 2]
    assert np.sqrt(np.delete(d2, pc.TIE_AT).max()) < 200
    kk, _, cent, _ = oracle.kmeans(pts, w, 2, max_iter=0)  # the initial centres themselves
    assert kk == 2 and cent[0].tolist() == [0, 0, 0] and cent[1].tolist() == pts[pc.TIE_AT[0]].tolist() == [0, 0, 255]
    pts, w, k = pc.km3_edge_case("few-distinct")
    assert len(np.unique(pts, axis=0)) == 10 and len(np.unique(pts[:pc.P3_ROWS], axis=0)) == 10
    assert oracle.kmeans(pts, w, k)[0] == 10


@pytest.mark.parametrize("pal_size", [2, 16, 64])
def test_quantize_palette_sizes(pal_size):
    tiles, pal_idx = pc.qp_sizes_case(pal_size)
    got = [len(np.unique(tiles[pal_idx == p] & 0xffffff)) for p in range(pc.QP_NPAL)]
    want = pc.qp_distinct_counts(pal_size)
    assert 12700 <= got[0] <= 12800 and got[0] > 3 * pc.P3_ROWS
    assert got[1:] == want[1:] and got[pc.QP_EMPTY] == 0
    assert (tiles[pal_idx == pc.QP_TOP_BYTE] >> 24).all() and not (tiles[pal_idx != pc.QP_TOP_BYTE] >> 24).any()
    first = np.nonzero(pal_idx == 0)[0]
    assert np.diff(first).max() > 1  # the palettes' tiles are interleaved


def test_quantize_many_palettes():
    tiles, pal_idx, npal = pc.qp_many_palettes_case()
    assert npal == 300 and (np.bincount(pal_idx, minlength=npal) == 2).all() and npal > 256
