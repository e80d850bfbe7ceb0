"""PreparePalettes against the oracle where more than one workgroup takes part: the D^2 seeding of the tile -> palette clustering
(k_pp_mass / k_pp_pick through the seam stages.pp_seeds), palettize end to end, the resident pixel k-means (k_kmeans3_persistent through
stages.kmeans, d = 3) and quantize_palettes with palettes of very different sizes.  All comparisons are exact.  The inputs and what each
of them reaches are in tests/palette_cases.py; tests/test_palette_cases_host.py asserts those claims on the oracle alone."""
import numpy as np
import pytest

from tests import palette_cases as pc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _seeds_match(oracle, pts, w, k):
    from tiler_amd import stages
    want = oracle.kmeans_pp_seeds(pts, w, k)
    kk, got = stages.pp_seeds(_dev(pts), _dev(w), k)
    print("seeds: oracle %s, library %d: %s" % (want.tolist(), kk, got.tolist()))
    assert kk == len(want) and got.shape == (k,)
    assert np.array_equal(got[:kk], want) and (got[kk:] == -1).all()
    return want


# ---- the seeding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", pc.SEED_SIZE_CASES)
def test_pp_seeds_sizes(oracle, kind, n):
    """1, 2, 3, 256, 257, 391 and 513 blocks of 512 points: one block a thread of k_pp_pick exactly, the first size with two (the last share
    holds one block) and three; "shaped" weights put seeds at index n - 1, in a last partial block, in block 0, in the second and third
    block of a share and in the last share, "plain" ones let every pick hang on the sums of many small masses"""
    pts, w, k = pc.seed_size_case(kind, n)
    _seeds_match(oracle, pts, w, k)


@pytest.mark.parametrize("name", pc.SEED_EDGE_CASES)
def test_pp_seeds_edges(oracle, name):
    """masses of up to 2^82 (the high words of the 128-bit sums, in every lane and in one lane only), no weights at all (w == nullptr in both
    kernels), zero weights (a third of the points; the whole first and last block), and fewer distinct points than centres (a zero total
    ends the seeding: kk = 5, the rest -1)"""
    pts, w, k = pc.seed_edge_case(name)
    want = _seeds_match(oracle, pts, w, k)
    if name == "duplicates":
        assert len(want) == 5


# ---- palettize --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,npal,max_iter", pc.PALETTIZE_CASES)
def test_palettize(oracle, name, npal, max_iter):
    """the clustering end to end over several blocks of the seeding (40 palettes: the iterations that are not resident); one iteration
    over 274 blocks (the seeds handed over on the device at more than one block a thread, the tile counts and the rank look-up past one
    grid stride); two palettes with equal tile counts (the initial order holds); fewer distinct points than palettes (the palettes beyond
    the centres found own no tile and rank last)"""
    from tiler_amd import stages
    feat, use = pc.palettize_case(name)
    want = oracle.palettize(feat, use, npal, max_iter)
    got = stages.palettize(_dev(feat), _dev(use), npal, max_iter).cpu().numpy()
    # up to 16 palettes and more than the five plain iterations: k_h_resident, and its barrier did not give up (the launches would give the same result)
    assert stages.kmeans_last_resident() == (npal <= 16 and max_iter > 5)
    print("tiles per palette: oracle %s, library %s" % (np.bincount(want, minlength=npal).tolist(), np.bincount(got.clip(0, npal - 1), minlength=npal).tolist()))
    assert np.array_equal(got, want)


# ---- the pixel k-means ------------------------------------------------------------------------------------------------------------------
def _kmeans3_matches(oracle, pts, w, k):
    from tiler_amd import stages
    kk, assign, cent, iters = oracle.kmeans(pts, w, k)
    g_kk, g_assign, g_cent, g_iters = stages.kmeans(_dev(pts), _dev(w), k)
    assert stages.kmeans_last_resident()  # k_kmeans3_persistent to the end: a barrier that gave up would hand the clustering to the launches
    g_assign = g_assign.cpu().numpy()
    print("kk %d / %d, iterations %d / %d, %d assignments differ" % (kk, g_kk, iters, g_iters, int((g_assign != assign).sum())))
    assert g_kk == kk and g_iters == iters
    assert np.array_equal(g_assign, assign)
    assert np.array_equal(g_cent.cpu().numpy()[:kk].view(np.uint64), cent[:kk].view(np.uint64)), "centroids must match bit for bit"
    return kk


@pytest.mark.parametrize("n,k", pc.KM3_SIZE_CASES)
def test_kmeans3_over_several_workgroups(oracle, n, k):
    """distinct colours with weights up to 5 000 around the 4 096 a workgroup holds (one short of it, exactly, one over) and in 4 and 10
    workgroups: the palette's barrier, the farthest-first pick through atomicMax and the carried sums with more than one participant"""
    pts, w = pc.km3_size_case(n)
    _kmeans3_matches(oracle, pts, w, k)


@pytest.mark.parametrize("name", pc.KM3_EDGE_CASES)
def test_kmeans3_bounds_and_picks_over_three_workgroups(oracle, name):
    """the Hamerly bounds of the d = 3 kernel on data that stresses them (lattice colours with many exactly equal distances, clusters tighter
    than the bounds' margin, one far cluster: large displacements early on); a farthest-first tie between three workgroups (the lowest
    index wins); fewer distinct colours than centres (the "no distinct point left" exit behind a barrier)"""
    pts, w, k = pc.km3_edge_case(name)
    kk = _kmeans3_matches(oracle, pts, w, k)
    if name == "few-distinct":
        assert kk == 10


# ---- quantize_palettes ------------------------------------------------------------------------------------------------------------------
def _quantize_matches(oracle, tiles, pal_idx, npal, pal_size):
    from tiler_amd import stages
    want = np.stack([oracle.quantize_palette(tiles[pal_idx == p].ravel(), pal_size) for p in range(npal)])
    got = stages.quantize_palettes(_dev(tiles), _dev(pal_idx), npal, pal_size).cpu().numpy()
    assert stages.kmeans_last_resident()
    print("palettes that differ: %s" % np.nonzero((got != want).any(1))[0].tolist())
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("pal_size", [2, 16, 64])
def test_quantize_palettes_of_very_different_sizes(oracle, pal_size):
    """one call, seven palettes: about 12 800 colours (four workgroups), exactly 4 096 and 4 097 (one workgroup, two), none at all in the
    middle of the numbering, a single colour, one colour fewer than the palette has slots, and pixels with their top byte set"""
    tiles, pal_idx = pc.qp_sizes_case(pal_size)
    got = _quantize_matches(oracle, tiles, pal_idx, pc.QP_NPAL, pal_size)
    assert (got[pc.QP_EMPTY] == -65281).all()  # cDitheringNullColor


def test_quantize_three_hundred_palettes(oracle):
    """the palette field of the pixel keys takes nine bits: one more pass of the radix sort"""
    tiles, pal_idx, npal = pc.qp_many_palettes_case()
    _quantize_matches(oracle, tiles, pal_idx, npal, 16)


def test_quantize_refuses_a_palette_out_of_range():
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    tiles, pal_idx, npal = pc.qp_many_palettes_case()
    bad = pal_idx[:40].copy()
    bad[:] = np.arange(40) % 5
    bad[17] = 5  # = npal
    with pytest.raises(TileMotionError) as e:
        stages.quantize_palettes(_dev(tiles[:40]), _dev(bad), 5, 16)
    assert e.value.code == -1  # TM_E_INVAL
