"""The inputs of the Yliluoma luma-tie test (tests/yliluoma_cases.py) judged on the oracle alone: they must tell the reference's
unstable QuickSort from a sort that keeps or imposes slot order, whatever machine the suite runs on."""
import numpy as np
import pytest

from tests import yliluoma_cases as yc


def test_tie_palettes_hold_equal_lumas_in_different_colours():
    for pal in yc.tie_palettes():
        r, g, b = pal & 255, (pal >> 8) & 255, (pal >> 16) & 255
        luma = r * 299 + g * 587 + b * 114
        vals, counts = np.unique(luma, return_counts=True)
        assert sorted(counts) == [3, 3, 3, 3, 4]  # five triples; the colour held twice makes one of them four
        assert len(np.unique(pal)) == 15


@pytest.mark.parametrize("mixed", yc.TIE_MIXED)
def test_tie_inputs_discriminate(oracle, mixed):
    palettes = yc.tie_palettes()
    tiles, flags, pal_idx = yc.tie_tiles(palettes, 64)
    assert (tiles >> 24).min() > 0
    differ, lengths = yc.tie_discrimination(oracle, palettes, tiles, pal_idx, mixed)
    assert differ * 4 >= tiles.size, (differ, tiles.size)
    assert mixed < 3 or len(lengths) > 1
    assert mixed != 16 or max(lengths) == 30
    assert max(lengths) <= 30  # the room of the kernel's 64-entry list


def test_oracle_plan_binding(oracle):
    """Plan mirrors tmo_plan: live entries in slot order, Remap back to the slots, and a sorted list over them"""
    pal = np.array([0x102030, yc.NULL, 0x0000FF, 0xFFFFFF], np.int32)
    plan = oracle.prepare_plan(pal, 3)
    assert plan.count == 3 and list(plan.remap[:3]) == [0, 2, 3] and plan.y2_mixed_colors == 3
    assert list(plan.y2[1]) == [255, 0, 0, 76] and plan.luma[1] == 255 * 299
    lst = oracle.mixing_plan_yliluoma(plan, 0xFF0000FF)  # the top byte is not colour
    assert 3 <= len(lst) <= 4 and (lst == 1).all()
    out = oracle.dither(np.full((1, 64), 0xFF, np.uint32), None, np.zeros(1, np.int32), pal[None], False, 3)
    assert (out == 2).all()
