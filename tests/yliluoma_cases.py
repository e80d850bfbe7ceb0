"""Inputs for the Yliluoma dither tests whose plans mix palette entries of equal luma, and the oracle-only measure of how many of those
plans an order-preserving sort would get wrong.  Shared by tests/test_gpu_dither_yliluoma.py (GPU) and tests/test_yliluoma_cases_host.py."""
import numpy as np

NULL = -65281  # cDitheringNullColor $FFFF00FF as int32
TIE_MIXED = (2, 3, 4, 8, 16)
TIE_BASES = ((100, 120, 60), (40, 200, 90), (180, 60, 30), (20, 30, 200), (210, 230, 150))  # r + 30 <= 255, g - 18 >= 0, b + 14 <= 255


def _rgb(r, g, b):
    return (b << 16) | (g << 8) | r


def tie_palettes(seed=5):
    """two 16-colour palettes: five triples (r + 15 s, g - 9 s, b + 7 s), s = 0, 1, 2, of different colours with one luma each
    (299 * 15 - 587 * 9 + 114 * 7 = 0), and one colour twice, in shuffled slot order"""
    rng = np.random.default_rng(seed)
    pals = np.empty((2, 16), np.int32)
    for p in range(2):
        cols = [_rgb(r + 15 * s, g - 9 * s, b + 7 * s) for r, g, b in TIE_BASES for s in range(3)]
        cols.append(cols[int(rng.integers(0, 15))])  # the identical pair
        pals[p] = np.array(cols, np.int32)[rng.permutation(16)]
    return pals


def tie_tiles(palettes, n, seed=7):
    """n tiles whose pixels lie within +-12 a channel of a tied colour of their palette (tile t takes palette t % len(palettes)), with a
    non-zero top byte, and mirror flags over all four values.
    Where in that box: the reference's QuickSort swaps a list of two equal-luma entries, so a two-entry plan (mixed = 2) differs from slot
    order only when its first pick -- the colour nearest the pixel -- sits in the lower slot.  Pixels drawn evenly around the tied colours
    mix two of them a third of the time and have the nearer one in the lower slot half of that: a sixth of the lists would tell the sorts
    apart.  So every pixel lies between two neighbours of a triple, on the lower slot's half of the segment (lo + f (hi - lo), f in
    [0, 0.5): at most 7.5 a channel), plus noise of +-4 a channel.  The last eighth of the tiles is drawn evenly over the box instead: plans
    that gather 15 entries before their last step, and so end on 30, come from there."""
    rng = np.random.default_rng(seed)
    pal_idx = (np.arange(n) % palettes.shape[0]).astype(np.int32)
    base = np.array(TIE_BASES)[rng.integers(0, len(TIE_BASES), size=(n, 64))]
    step = np.array([15, -9, 7])
    a = base + step * rng.integers(0, 2, size=(n, 64, 1))
    b = a + step
    pack = lambda c: c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
    first_slot = lambda c: np.argmax(palettes[pal_idx][:, None, :] == pack(c)[..., None], axis=-1)
    a_low = (first_slot(a) < first_slot(b))[..., None]
    lo, hi = np.where(a_low, a, b), np.where(a_low, b, a)
    ch = np.rint(lo + rng.uniform(0, 0.5, size=(n, 64, 1)) * (hi - lo)).astype(np.int64) + rng.integers(-4, 5, size=(n, 64, 3))
    even = np.arange(n) >= n - n // 8  # the last eighth of the tiles: evenly around the tied colours, for the longest lists
    ch[even] = lo[even] + rng.integers(-12, 13, size=(int(even.sum()), 64, 3))
    assert np.abs(ch - lo).max() <= 12
    ch = np.clip(ch, 0, 255)
    tiles = (pack(ch) | (rng.integers(1, 256, size=(n, 64)) << 24)).astype(np.uint32)
    flags = (np.arange(n) // palettes.shape[0] % 4).astype(np.uint8)
    return tiles, flags, pal_idx


def tie_discrimination(oracle, palettes, tiles, pal_idx, mixed):
    """over every pixel: (how many oracle lists differ from the same entries in (luma, slot) order, the set of list lengths).  The
    oracle's list is what the reference's unstable QuickSort (extern.pas:370-418) leaves; (luma, slot) is what a stable sort, or one
    that compares whole entries, would leave."""
    plans = [oracle.prepare_plan(p, mixed) for p in palettes]
    differ, lengths, memo = 0, set(), {}
    for t in range(tiles.shape[0]):
        pi = int(pal_idx[t])
        plan = plans[pi]
        luma, remap = np.array(plan.luma[:]), np.array(plan.remap[:])
        for c in tiles[t]:
            key = (pi, int(c) & 0xFFFFFF)
            if key not in memo:
                lst = oracle.mixing_plan_yliluoma(plan, c)
                slots = remap[lst]
                by_slot = slots[np.lexsort((slots, luma[lst]))]
                memo[key] = (not np.array_equal(slots, by_slot), len(lst))
            d, ln = memo[key]
            differ += d
            lengths.add(ln)
    return differ, lengths
