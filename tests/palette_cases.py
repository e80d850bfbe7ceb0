"""Inputs of the PreparePalettes comparisons past one workgroup (tests/test_gpu_prepare_palettes.py), each with what it claims to reach.
tests/test_palette_cases_host.py asserts those claims on the oracle's output alone; the GPU tests compare the library with the oracle on the
same inputs.  Everything is a pure function of the case's name: both files see the same arrays.

Sizes are read against the kernels' constants: the seeding sums masses per block of 512 points (PP_BLOCK) and k_pp_pick's 256 threads take
per = ceil(blocks / 256) consecutive blocks each; the pixel k-means keeps 4 096 colours per workgroup (P3_ROWS)."""
import functools

import numpy as np

PP_BLOCK, PP_THREADS, P3_ROWS = 512, 256, 4096
PP_SEED, PP_MUL, PP_INC = 0x42381337, 6364136223846793005, 1442695040888963407
COORD = 40000  # |feature| <= 40 000: the range of test_kmeans_pp_seeding_follows_its_stated_rule


def pp_blocks(n):
    return (n + PP_BLOCK - 1) // PP_BLOCK


def pp_per(n):
    """blocks per thread of k_pp_pick"""
    return (pp_blocks(n) + PP_THREADS - 1) // PP_THREADS


def pp_masses(pts, w, seeds):
    """the exact masses (Python integers) of the pick that follows `seeds`: weight x squared distance to the nearest of them"""
    n = pts.shape[0]
    wi = np.ones(n, np.int64) if w is None else w.astype(np.int64)
    if not len(seeds):
        return [int(v) for v in wi]
    p = pts.astype(np.int64)
    mind = np.min([((p - p[s]) ** 2).sum(1) for s in seeds], axis=0)
    return [int(a) * int(b) for a, b in zip(wi, mind)]


# ---- section 3: the D^2 seeding, d = 192 ----------------------------------------------------------------------------------------------
SEED_SIZES = (1, 511, 512, 513, 1025, 131072, 131073, 200000, 262145)


def seed_k(n):
    return 4 if n > 2000 else 16


@functools.lru_cache(maxsize=2)
def _seed_points(n):
    rng = np.random.default_rng(1000 + n)
    pts = rng.integers(-COORD, COORD + 1, size=(n, 192), dtype=np.int32)
    pts.setflags(write=False)
    return pts


# Points whose weight (2^28 against 1..50) draws the picks to them: index n - 1, a last partial block, block 0, a block that is not the first of
# its thread's share (per >= 2), the last share.  The "plain" twin of every size has the light weights only: there every pick moves when a
# partial sum is off by one point's mass.
_HEAVY = {
    511: (510, 0, 300),
    512: (511, 0),
    513: (512, 5, 511),
    1025: (1024, 3, 600),
    131072: (131071, 17, 512 * 100 + 7, 512 * 255 + 1),
    131073: (131072, 700, 3, 512 * 201 + 9),            # per 2: block 256 is the last share's only block, blocks 1 and 201 are second in theirs
    200000: (199999, 100, 512 * 389 + 5, 512 * 390 + 10),  # per 2: block 390 (320 points) is the last share's only block, 389 is second in its share
    262145: (262144, 40, 512 * 511 + 77, 512 * 5 + 1),    # per 3: the last share is blocks 510..512, block 512 holds one point
}
SEED_SIZE_CASES = [("plain", n) for n in SEED_SIZES] + [("shaped", n) for n in SEED_SIZES if n in _HEAVY]


def seed_size_case(kind, n):
    """-> (pts int32 [n][192], weights uint32 [n], k)"""
    rng = np.random.default_rng(2000 + n)
    w = rng.integers(1, 51, size=n).astype(np.uint32)
    if kind == "shaped":
        w[list(_HEAVY[n])] = 1 << 28
    return _seed_points(n), w, seed_k(n)


SEED_EDGE_CASES = ("wide-masses", "one-wide-mass", "no-weights", "zero-weights-third", "zero-weights-end-blocks", "duplicates")
WIDE_N, WIDE_POINT = 2000, 1400


def seed_edge_case(name):
    """-> (pts, weights or None, k)"""
    rng = np.random.default_rng(3000 + SEED_EDGE_CASES.index(name))
    if name == "wide-masses":  # every weight in [2^31, 2^32): from the second pick on the totals pass 2^64 (about 2^82)
        return _seed_points(WIDE_N), rng.integers(1 << 31, 1 << 32, size=WIDE_N, dtype=np.uint64).astype(np.uint32), 16
    if name == "one-wide-mass":
        # one such weight only, the others below 2^22: at the second pick exactly one point's mass has a high word (the others stay below
        # 2^22 x 2^41 = 2^63), so the high word enters the wave's reduction in one lane while the low words carry in many
        w = rng.integers(1, 1 << 22, size=WIDE_N).astype(np.uint32)
        w[WIDE_POINT] = (1 << 32) - 12345
        return _seed_points(WIDE_N), w, 16
    if name == "no-weights":
        return _seed_points(1025), None, 16
    if name == "zero-weights-third":
        w = rng.integers(1, 51, size=1500).astype(np.uint32)
        w[1::3] = 0
        return _seed_points(1500), w, 16
    if name == "zero-weights-end-blocks":  # blocks 0 and 2 (the last, 476 points) weigh nothing at all
        w = rng.integers(1, 51, size=1500).astype(np.uint32)
        w[:512] = 0
        w[1024:] = 0
        return _seed_points(1500), w, 16
    if name == "duplicates":  # 5 distinct rows: the sixth pick finds a zero total
        rows = rng.integers(-COORD, COORD + 1, size=(5, 192), dtype=np.int32)
        return np.ascontiguousarray(rows[rng.integers(0, 5, size=1300)]), rng.integers(1, 51, size=1300).astype(np.uint32), 16
    raise KeyError(name)


# ---- section 4: palettize end to end ---------------------------------------------------------------------------------------------------
def _clustered(rng, n, ncentres, spread, lo=-3000, hi=3000):
    centres = rng.integers(lo, hi, size=(ncentres, 192))
    return (centres[rng.integers(0, ncentres, size=n)] + rng.integers(-spread, spread, size=(n, 192))).astype(np.int32)


PALETTIZE_CASES = [("full-%d-%d" % (n, npal), npal, 300) for n in (1500, 3000) for npal in (1, 2, 16, 40)] + \
                  [("one-iteration", 16, 1), ("ranking-tie", 4, 300), ("duplicates", 16, 300), ("one-workgroup-long", 16, 300)]
# k_h_resident (at most 16 palettes) runs one workgroup per 1 024 tiles and reuses each of its three delta buffers every third iteration, from
# iteration 8 on; with fewer than four workgroups a workgroup's share of a buffer is longer than the workgroup.  These run that long:
LONG_RESIDENT_CASES = (("full-1500-16", 16, 2), ("full-3000-16", 16, 3), ("one-workgroup-long", 16, 1))  # (name, palettes, workgroups)
TIE_SIZES = (600, 400, 400, 200)


@functools.lru_cache(maxsize=2)
def palettize_case(name):
    """-> (feat int32 [n][192], use uint32 [n])"""
    if name.startswith("full-"):
        n = int(name.split("-")[1])
        rng = np.random.default_rng(4000 + n)
        return _clustered(rng, n, 5, 200), rng.integers(1, 50, size=n).astype(np.uint32)
    if name == "one-iteration":  # 274 blocks (per = 2 in k_pp_pick), 547 workgroups of 256 for the count (its grid stops at 512) and the look-up
        rng = np.random.default_rng(4100)
        return _clustered(rng, 140000, 40, 700, -1500, 1500), rng.integers(1, 9, size=140000).astype(np.uint32)
    if name == "ranking-tie":  # four clusters far apart, two of them with 400 tiles each
        rng = np.random.default_rng(4200)
        centres = rng.integers(-COORD + 500, COORD - 500, size=(4, 192))
        which = rng.permutation(np.repeat(np.arange(4), TIE_SIZES))
        pts = (centres[which] + rng.integers(-200, 200, size=(which.size, 192))).astype(np.int32)
        return pts, rng.integers(1, 50, size=which.size).astype(np.uint32)
    if name == "duplicates":
        pts, w, _ = seed_edge_case("duplicates")
        return pts, w
    if name == "one-workgroup-long":  # spread in three dimensions only: some twenty iterations where clusters in 192 dimensions settle in five
        rng = np.random.default_rng(4300)
        pts = rng.integers(-3000, 3000, size=(1024, 192)).astype(np.int32)
        pts[:, 3:] //= 200
        return pts, rng.integers(1, 50, size=1024).astype(np.uint32)
    raise KeyError(name)


# ---- section 6: the pixel k-means, d = 3 ------------------------------------------------------------------------------------------------
KM3_SIZE_CASES = [(n, 16) for n in (4095, 4096, 4097, 12289, 40000)] + [(12289, 2), (12289, 64)]
KM3_EDGE_CASES = ("lattice-ties", "tight-clusters", "one-cluster-far", "pick-tie-across-workgroups", "few-distinct")
TIE_AT = (100, 5000, 9000)  # one in each of three workgroups


def _distinct_colours(rng, n):
    c = np.unique(rng.integers(0, 1 << 24, size=2 * n + 64))
    c = rng.permutation(c)[:n]
    assert c.size == n
    return np.stack([c & 0xff, (c >> 8) & 0xff, c >> 16], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def km3_size_case(n):
    """-> (pts int32 [n][3], distinct; weights uint32 [n] up to 5 000)"""
    rng = np.random.default_rng(6000 + n)
    return _distinct_colours(rng, n), rng.integers(1, 5001, size=n).astype(np.uint32)


def km3_edge_case(name):
    """-> (pts int32 [n][3], weights uint32 [n], k)"""
    rng = np.random.default_rng(6500 + KM3_EDGE_CASES.index(name))
    n = 9000
    if name == "lattice-ties":  # 512 lattice colours, each many times: equal distances everywhere
        pts = (rng.integers(0, 8, size=(n, 3)) * 32).astype(np.int32)
    elif name == "tight-clusters":  # half-distances between centroids inside one cluster are below the bounds' margin of one unit (1/128 step)
        centres = rng.integers(2, 254, size=(24, 3))
        pts = (centres[rng.integers(0, 24, size=n)] + rng.integers(-1, 2, size=(n, 3))).astype(np.int32)
    elif name == "one-cluster-far":
        pts = rng.integers(0, 41, size=(n, 3)).astype(np.int32)
        far = rng.choice(n, size=40, replace=False)
        pts[far] = 250 + rng.integers(-4, 5, size=(40, 3))
    elif name == "pick-tie-across-workgroups":
        n = 9100
        pts = rng.integers(0, 116, size=(n, 3)).astype(np.int32)  # within 115 sqrt(3) < 200 of point 0
        pts[0] = (0, 0, 0)
        pts[TIE_AT[0]], pts[TIE_AT[1]], pts[TIE_AT[2]] = (0, 0, 255), (255, 0, 0), (0, 255, 0)
    elif name == "few-distinct":
        pts = _distinct_colours(rng, 10)[rng.integers(0, 10, size=n)]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(pts), rng.integers(1, 5001, size=pts.shape[0]).astype(np.uint32), 16


# ---- section 7: quantize_palettes ---------------------------------------------------------------------------------------------------------
QP_NPAL, QP_EMPTY, QP_TOP_BYTE = 7, 3, 6


def _tiles_of(rng, colours, ntiles):
    """ntiles x 64 pixels that show every colour at least once (the rest are repeats)"""
    colours = np.asarray(colours, np.uint32)
    px = np.concatenate([colours, rng.choice(colours, size=ntiles * 64 - colours.size)])
    return rng.permutation(px).reshape(ntiles, 64)


def qp_distinct_counts(pal_size):
    """distinct colours each palette is built to hold (None: about 12 800, the host test gives the range)"""
    return [None, P3_ROWS, P3_ROWS + 1, 0, 1, pal_size - 1, 300]


@functools.lru_cache(maxsize=None)
def qp_sizes_case(pal_size):
    """-> (tiles uint32 [n][64] 0x..BBGGRR, pal_idx int32 [n]): seven palettes of very different sizes, their tiles interleaved"""
    rng = np.random.default_rng(7000 + pal_size)
    pool = rng.permutation(np.unique(rng.integers(0, 1 << 24, size=40000)).astype(np.uint32))
    take = iter(np.split(pool, np.cumsum([P3_ROWS, P3_ROWS + 1, 1, pal_size - 1, 300])))
    groups = {
        0: rng.integers(0, 1 << 24, size=(200, 64)).astype(np.uint32),  # several workgroups
        1: _tiles_of(rng, next(take), 70),
        2: _tiles_of(rng, next(take), 70),
        4: _tiles_of(rng, next(take), 3),
        5: _tiles_of(rng, next(take), 4),
        QP_TOP_BYTE: _tiles_of(rng, next(take), 6) | (rng.integers(1, 256, size=(6, 64)).astype(np.uint32) << 24),
    }
    tiles = np.concatenate([groups[p] for p in sorted(groups)])
    pal_idx = np.concatenate([np.full(groups[p].shape[0], p, np.int32) for p in sorted(groups)])
    order = rng.permutation(tiles.shape[0])
    return np.ascontiguousarray(tiles[order]), np.ascontiguousarray(pal_idx[order])


@functools.lru_cache(maxsize=None)
def qp_many_palettes_case():
    """-> (tiles, pal_idx, npal): 300 palettes of two tiles each -- the palette field of the pixel keys takes nine bits"""
    rng = np.random.default_rng(7300)
    npal = 300
    tiles = rng.integers(0, 1 << 24, size=(2 * npal, 64)).astype(np.uint32)
    tiles[:, 32:] = tiles[:, :32]  # repeats inside a tile: weights above 1
    return tiles, rng.permutation(np.repeat(np.arange(npal, dtype=np.int32), 2)), npal
