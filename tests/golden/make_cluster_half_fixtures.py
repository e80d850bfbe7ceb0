"""Fixture for the in-doubt branch of the clustering features (k_features_cluster_i32, tm_features_cluster.hip) -> tests/golden/cluster_half_tiles.npz.

The kernel takes a separable first look at every coefficient and sums it in the reference's order only where the first look lands within
1e-6 of a half-integer: about two coefficients in a million on random tiles, so a test that draws its tiles never holds that branch to
anything.  This script searches once.  It draws tiles of every kind (tests/tile_kinds.py, edges included) from a fixed seed, evaluates them
with the project's own oracle (Oracle.features_f64 on Lab planes: the doubles the clustering features are rounded from) and keeps, for each
DCT mode (0, 1, 3, 4), the first 32 tiles that have a coefficient f with |f - floor(f) - 0.5| < 1e-6.

The file holds data only:
  modes  int32  [4]          the TPsyVisMode of each row below
  tiles  uint32 [4][32][64]  the tiles, 0x00BBGGRR as the encoder holds them
  coef   int32  [4][32]      the index (in the features' own order, 0..191) of the tile's first coefficient on the edge
tests/test_gpu_dithering_modes.py checks from the oracle alone that every listed coefficient is on the edge before it compares anything.

32 a mode is a condition: if the pool runs out first the script fails, and the pool is to be enlarged.
Run:  python tests/golden/make_cluster_half_fixtures.py        (about a quarter of a minute a mode)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = (0, 1, 3, 4)
PER_MODE = 32
EDGE = 1e-6
BATCH = 6000       # tiles drawn at a time, seeds SEED, SEED + 1, ...
MAX_BATCHES = 100  # the pool: 600 000 tiles a mode (32 are expected within some 85 000)
SEED = 419


def on_edge(f):
    return np.abs(f - np.floor(f) - 0.5) < EDGE


def main():
    from tests.oracle_binding import Oracle
    from tests.tile_kinds import tile_kinds
    oracle = Oracle(os.path.join(ROOT, "oracle", "libtm_oracle.so"))
    tiles = np.zeros((len(MODES), PER_MODE, 64), np.uint32)
    coef = np.zeros((len(MODES), PER_MODE), np.int32)
    for m, mode in enumerate(MODES):
        found = drawn = 0
        for b in range(MAX_BATCHES):
            pool, _ = tile_kinds(BATCH, SEED + b, edges=True)
            for t in pool:
                drawn += 1
                hit = np.flatnonzero(on_edge(oracle.features_f64(t, mode, use_lab=True)))
                if hit.size:
                    tiles[m, found], coef[m, found] = t, hit[0]
                    found += 1
                    if found == PER_MODE:
                        break
            if found == PER_MODE:
                break
        assert found == PER_MODE, "mode %d: %d of %d tiles in a pool of %d -- enlarge MAX_BATCHES" % (mode, found, PER_MODE, drawn)
        print("mode %d: %d tiles with a coefficient on the edge among the first %d drawn" % (mode, found, drawn))
    np.savez(os.path.join(HERE, "cluster_half_tiles.npz"), modes=np.array(MODES, np.int32), tiles=tiles, coef=coef)


if __name__ == "__main__":
    main()
