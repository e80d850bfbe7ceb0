"""k_dither_yliluoma (DitheringUseThomasKnoll = 0) through stages.dither against the oracle's DeviseBestMixingPlanYliluoma: every list
length the doubling of the mixed count can end on, palettes of every width with null slots, luma ties in the lists the lanes sort, and
blocks that take several tiles and so reuse, reload or drop the plan they hold.  Everything is integer: np.array_equal."""
import numpy as np
import pytest

from tests import yliluoma_cases as yc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NULL = yc.NULL


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _gpu(tiles, flags, pal_idx, palettes, mixed):
    from tiler_amd import stages
    return stages.dither(_dev(tiles), _dev(flags), _dev(pal_idx), _dev(palettes), False, mixed).cpu().numpy()


@pytest.mark.parametrize("pal_size", [2, 16, 17, 64])
@pytest.mark.parametrize("mixed", [1, 2, 3, 5, 8, 15, 16])
def test_dither_yliluoma_mixed_counts_and_palette_sizes(oracle, mixed, pal_size):
    """the plan grows 1, 2, 4, 8, ... entries at a time, so the mixed count decides the lengths a list can end on (3: 3..4, 5: 5..8, 15 and
    16: up to 30); the candidate averages go through the reciprocal table 65536 div t, not a division.  Palettes: full, the upper half
    null, and one live colour in the last slot -- which the oracle answers for every pixel.  Half of the tiles are noise, half lie near
    their palette's colours; the top byte of a pixel is not colour."""
    rng = np.random.default_rng(1000 * pal_size + mixed)
    n = 64
    palettes = rng.integers(0, 1 << 24, size=(3, pal_size), dtype=np.int32)
    palettes[1, pal_size // 2:] = NULL
    palettes[2, :pal_size - 1] = NULL
    pal_idx = rng.integers(0, 3, size=n, dtype=np.int32)
    flags = (np.arange(n) % 4).astype(np.uint8)
    tiles = rng.integers(0, 1 << 24, size=(n, 64), dtype=np.int64)
    live = [p[p != NULL] for p in palettes]
    for t in range(n // 2, n):
        near = rng.choice(live[pal_idx[t]], size=64).astype(np.int64)
        ch = np.clip(np.stack([(near >> s) & 255 for s in (0, 8, 16)], -1) + rng.integers(-40, 41, size=(64, 3)), 0, 255)
        tiles[t] = ch[:, 0] | (ch[:, 1] << 8) | (ch[:, 2] << 16)
    tiles = (tiles | (rng.integers(1, 256, size=(n, 64)) << 24)).astype(np.uint32)
    exp = oracle.dither(tiles, flags, pal_idx, palettes, False, mixed)
    assert (exp[pal_idx == 2] == pal_size - 1).all() and (pal_idx == 2).any()
    got = _gpu(tiles, flags, pal_idx, palettes, mixed)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("mixed", yc.TIE_MIXED)
def test_dither_yliluoma_luma_ties(oracle, mixed):
    """lists of 2..30 entries that mix different colours of one luma, and one colour held by two slots: the lane's literal QuickSort must
    leave them where the reference's unstable one does (extern.pas:370-418).  That the inputs tell the sorts apart is measured on the
    oracle alone: a quarter of the pixels or more have a list that a sort by (luma, slot) would order differently."""
    palettes = yc.tie_palettes()
    tiles, flags, pal_idx = yc.tie_tiles(palettes, 64)
    assert set(flags) == {0, 1, 2, 3}
    differ, lengths = yc.tie_discrimination(oracle, palettes, tiles, pal_idx, mixed)
    assert differ * 4 >= tiles.size, (differ, tiles.size)
    assert mixed < 3 or len(lengths) > 1
    assert mixed != 16 or max(lengths) == 30
    exp = oracle.dither(tiles, flags, pal_idx, palettes, False, mixed)
    got = _gpu(tiles, flags, pal_idx, palettes, mixed)
    assert np.array_equal(got, exp)


def test_dither_yliluoma_blocks_that_take_several_tiles(oracle):
    """the grid is min(n, 10240) blocks of one tile each at a time; with n = 2 x 10240 + 300 block b takes tiles b, b + 10240 and, below
    300, b + 20480, and keeps the plan of the palette it prepared last.  By block, pal_idx runs through: the same palette twice and then
    another; a different palette each visit; the all-null palette between two visits of one palette (the oracle gives zeros for it, and
    the plan must be prepared again after it); an index out of range (-1, npal) in the first or the middle visit.  Tiles that name no
    palette are not part of the oracle's call and come back as zeros; every other tile is the oracle's."""
    rng = np.random.default_rng(41)
    grid, n = 10240, 2 * 10240 + 300
    palettes = rng.integers(0, 1 << 24, size=(5, 16), dtype=np.int32)
    palettes[1, 9:] = NULL
    palettes[4, :] = NULL
    npal, null_pal = 5, 4
    b = np.arange(grid)
    p = (b // 7) % 4
    q, r = (p + 1) % 4, (p + 2) % 4
    visits = {0: (p, p, q), 1: (p, q, r), 2: (p, np.full(grid, null_pal), p), 3: (np.full(grid, -1), p, p), 4: (p, np.full(grid, npal), p),
              5: (np.full(grid, npal), p, q), 6: (p, np.full(grid, -1), q)}
    by_visit = np.stack([np.select([b % 7 == k for k in range(7)], [visits[k][v] for k in range(7)]) for v in range(3)])
    pal_idx = by_visit.reshape(-1)[:n].astype(np.int32)
    assert all((b[:300] % 7 == k).any() for k in range(7))  # every pattern among the blocks that make the third visit
    pool = rng.integers(0, 1 << 24, size=48, dtype=np.uint32)
    tiles = pool[rng.integers(0, 48, size=(n, 64))] | (rng.integers(1, 256, size=(n, 1)).astype(np.uint32) << 24)
    flags = rng.integers(0, 4, size=n, dtype=np.uint8)
    good = (pal_idx >= 0) & (pal_idx < npal)
    assert (~good).sum() > 4000 and (pal_idx == null_pal).sum() > 1000
    exp = oracle.dither(tiles[good], flags[good], pal_idx[good], palettes, False, 4)
    assert not exp[pal_idx[good] == null_pal].any()
    got = _gpu(tiles, flags, pal_idx, palettes, 4)
    assert not got[~good].any()
    assert np.array_equal(got[good], exp)


def test_dither_settings_out_of_bounds_are_refused():
    """DitheringYliluoma2MixedColors outside 1..16 (tilingencoder.pas:2922) is refused when the Yliluoma planner would read it and ignored
    under Thomas-Knoll; PaletteSize outside 2..64 (2965) is refused under both"""
    from tiler_amd import stages, TileMotionError
    rng = np.random.default_rng(2)
    tiles = _dev(rng.integers(0, 1 << 24, size=(4, 64), dtype=np.int32))
    flags = _dev(np.zeros(4, np.uint8))
    pal_idx = _dev(np.zeros(4, np.int32))
    pal16 = _dev(rng.integers(0, 1 << 24, size=(1, 16), dtype=np.int32))
    for mixed in (0, 17):
        with pytest.raises(TileMotionError) as ei:
            stages.dither(tiles, flags, pal_idx, pal16, False, mixed)
        assert ei.value.code == -1  # TM_E_INVAL
        assert stages.dither(tiles, flags, pal_idx, pal16, True, mixed).shape == (4, 64)
    for size in (1, 65):
        pal = _dev(rng.integers(0, 1 << 24, size=(1, size), dtype=np.int32))
        for tk in (False, True):
            with pytest.raises(TileMotionError) as ei:
                stages.dither(tiles, flags, pal_idx, pal, tk, 4)
            assert ei.value.code == -1
