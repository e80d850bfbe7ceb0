"""Seeded sets of 8 x 8 RGB tiles of every kind the feature kernels are held to the oracle on.  Test infrastructure only."""
import numpy as np

WHITE = 0xFFFFFF
N_EDGE_TILES = 4 + 4 * 64  # what edges=True plants, see tile_kinds


def tile_kinds(n, seed, edges=False):
    """noise, flat, two-colour, grey ramps, near-black and plain noise again: the kinds test_features_first_look_agrees_with_reference_order builds.
    -> (tiles uint32 [n][64], mirror flags uint8 [n])

    edges=True overwrites the head of the last sixth (plain noise) with the tiles at the ends of the colour range: all 0, all 0xFFFFFF,
    the one-pixel checkerboard of the two and its inverse, and tiles with a single live pixel at each of the 64 positions -- white on
    black, black on white, a random colour on black and a random colour on a random flat ground.  The other tiles and the flags are
    the same with and without it."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 1 << 24, size=(n, 64), dtype=np.uint32)
    k = n // 6
    t[k:2 * k] = t[k:2 * k, :1]
    two = rng.integers(0, 1 << 24, size=(k, 2), dtype=np.uint32)
    t[2 * k:3 * k] = np.take_along_axis(two, rng.integers(0, 2, size=(k, 64)), axis=1)
    v = np.clip((np.arange(64) % 8)[None, :] * rng.integers(0, 32, size=(k, 1)) + rng.integers(0, 32, size=(k, 1)), 0, 255).astype(np.uint32)
    t[3 * k:4 * k] = v | (v << 8) | (v << 16)
    t[4 * k:5 * k] &= 0x070707
    flags = rng.integers(0, 4, size=n).astype(np.uint8)
    if edges:
        assert n - 5 * k >= N_EDGE_TILES, "edges=True needs %d tiles in the last sixth" % N_EDGE_TILES
        e = t[5 * k:5 * k + N_EDGE_TILES]
        y, x = np.divmod(np.arange(64), 8)
        checker = np.where((x + y) & 1, WHITE, 0).astype(np.uint32)
        e[0], e[1], e[2], e[3] = 0, WHITE, checker, WHITE - checker
        eye = np.eye(64, dtype=bool)
        colour = rng.integers(1, 1 << 24, size=(2, 64, 1), dtype=np.uint32)
        ground = rng.integers(0, 1 << 24, size=(64, 1), dtype=np.uint32)
        e[4:68] = np.where(eye, WHITE, 0)
        e[68:132] = np.where(eye, 0, WHITE)
        e[132:196] = np.where(eye, colour[0], 0)
        e[196:260] = np.where(eye, colour[1], ground)
    return t, flags
