"""The cases of tests/load_cases.py reach what they claim to reach -- asserted on the oracle's output alone (no GPU): which chunk, batch,
strip and grid boundaries the sizes cross, that the Pearson inputs tell one order of summation from another, which tiles tie under the mirror
rule, how wide the window features get, where the oracle puts its key frames.  tm_pearson_finish_host (host arithmetic) is held to the oracle
here as well.  The GPU comparisons on the same inputs are in tests/test_gpu_load_front.py."""
import ctypes

import numpy as np
import pytest

from tests import load_cases as lc
from tests import oracle_pipeline


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- Pearson ----------------------------------------------------------------------------------------------------------------------------
def test_pearson_sizes_cover_the_groups_and_the_chunks():
    s = lc.PEARSON_SIZES
    for edge in (lc.PC_GROUP_F64, lc.PC_GROUP_F32, lc.PC):
        assert {edge - 1, edge, edge + 1} <= set(s)
    assert {lc.PC + lc.PC_GROUP_F64, lc.PC + lc.PC_GROUP_F32 - 1, lc.PC + lc.PC_GROUP_F32, 2 * lc.PC, 2 * lc.PC + 1, 3 * lc.PC + 1} <= set(s)
    assert [lc.pearson_chunks(n) for n in s] == [1] * 12 + [2] * 5 + [3, 4, 22]
    assert 43200 % lc.PC == 192 and 192 in s  # Load's size at 720p: 21 chunks and the three groups of 64 that size 192 has alone
    assert 6145 % lc.PC == 1 and 2111 % lc.PC == lc.PC_GROUP_F32 - 1  # chunks that end one by one


def test_pearson_restatement_equals_the_oracle(oracle):
    """the numpy restatement (sequential sums through cumsum) is the oracle's arithmetic: the sums below are the right ones to finish"""
    for kind in lc.PEARSON_KINDS:
        for per in lc.PEARSON_SIZES:
            lab = lc.pearson_case(kind, per, 7)
            for f in range(1, 7):
                got = lc.pearson_finish(lc.pearson_sums(lab[f - 1], lab[f]))
                assert _bits(got) == _bits(oracle.pearson(lab[f - 1], lab[f])), (kind, per, f)


def test_pearson_finish_host_against_the_oracle(oracle):
    """tm_pearson_finish_host on the sequential Single sums of every Pearson case, den == 0 included"""
    from tiler_amd import lib
    zero_den = 0
    for kind in lc.PEARSON_KINDS:
        for per in lc.PEARSON_SIZES:
            for nframes in lc.PEARSON_FRAMES:
                lab = lc.pearson_case(kind, per, nframes)
                sums = np.full((nframes, 3), np.nan, np.float32)  # frame 0's sums are not read
                exp = np.zeros(nframes, np.float32)
                for f in range(1, nframes):
                    sums[f] = lc.pearson_sums(lab[f - 1], lab[f])
                    exp[f] = oracle.pearson(lab[f - 1], lab[f])
                    zero_den += int(sums[f, 1] == 0 or sums[f, 2] == 0)
                got = np.full(nframes, np.nan, np.float32)
                assert lib().tm_pearson_finish_host(sums.ctypes.data_as(ctypes.c_void_p), nframes, got.ctypes.data_as(ctypes.c_void_p)) == 0
                assert np.array_equal(_bits(got), _bits(exp)), (kind, per, nframes, got, exp)
    assert zero_den > 100


def test_pearson_constant_frames_give_exactly_one(oracle):
    for kind in ("const-one", "const-both"):
        for per in lc.PEARSON_SIZES:
            lab = lc.pearson_case(kind, per, 7)
            assert all(oracle.pearson(lab[f - 1], lab[f]) == 1.0 for f in range(1, 7)), (kind, per)
    for per in lc.PEARSON_SIZES:  # (and the other kinds are not degenerate past a handful of values)
        if per >= 31:
            lab = lc.pearson_case("near", per, 2)
            assert 0.9 < oracle.pearson(lab[0], lab[1]) < 1.0
            lab = lc.pearson_case("indep", per, 2)
            assert abs(oracle.pearson(lab[0], lab[1])) < 0.6


def test_pearson_cases_tell_the_order_of_summation(oracle):
    """for every size from 2047 up, a near or indep case changes in bits when the three Single sums are added pairwise instead of in sequence
    (the means in double either way): a kernel that adds in another order past the first groups cannot pass"""
    for per in lc.PEARSON_SIZES:
        if per < 2047:
            continue
        differ = total = 0
        for kind in ("near", "indep"):
            for nframes in (2, 7):
                lab = lc.pearson_case(kind, per, nframes)
                for f in range(1, nframes):
                    other = lc.pearson_finish(lc.pearson_sums(lab[f - 1], lab[f], pairwise=True))
                    differ += int(_bits(other).item() != _bits(oracle.pearson(lab[f - 1], lab[f])).item())
                    total += 1
        assert differ >= 1, per
        print("per %d: %d of %d cases differ" % (per, differ, total))


def test_pearson_tiny_products_are_subnormal():
    tiny = np.finfo(np.float32).tiny
    for per in lc.PEARSON_SIZES:
        lab = lc.pearson_case("tiny", per, 2)
        x, y = lab[0], lab[1]
        dx = x - np.float32(np.cumsum(x.astype(np.float64))[-1] / per)
        dy = y - np.float32(np.cumsum(y.astype(np.float64))[-1] / per)
        p = np.abs(np.concatenate([dx * dy, dx * dx, dy * dy]))
        assert p.max() < 1e-35 and (per < 31 or np.count_nonzero((p > 0) & (p < tiny)) >= per // 16), (per, p.max())
        s = lc.pearson_sums(x, y)
        assert per < 3 or (s[1] > 0 and s[2] > 0), (per, s)  # a device that flushed them all would find den == 0


# ---- Load -------------------------------------------------------------------------------------------------------------------------------
def test_load_shapes_cover_the_batches_and_the_grid():
    per = [s[3] * s[4] for s in lc.LOAD_SHAPES]
    assert per == [1, 1, 104, 91, 9, 100, 30, 8250]
    assert per[2] % lc.LT_BATCH == 0 and per[3] % lc.LT_BATCH != 0 and per[4] % lc.LT_BATCH != 0 and per[4] > lc.LT_BATCH
    big = lc.LOAD_SHAPES[-1]
    assert big[0] * per[-1] == 66000 and lc.load_batches(big) > lc.LOAD_GRID  # a workgroup's second batch
    assert all(lc.load_batches(s) <= lc.LOAD_GRID for s in lc.LOAD_SHAPES[:-1])
    f, h, w, tm_w, tm_h = lc.LOAD_SHAPES[5]
    assert tm_w * 8 > w and tm_h * 8 > h  # tiles beyond the image
    f, h, w, tm_w, tm_h = lc.LOAD_SHAPES[6]
    assert tm_w * 8 < w and tm_h * 8 < h  # an image beyond the tile map


def test_mirror_ties_get_the_flags_they_claim(oracle):
    tiles, flags = lc.mirror_tie_tiles()
    n = tiles.shape[0]
    loaded = oracle.load_from_image(lc.tiles_to_image(tiles, 1, n), n, 1)
    _, got = oracle.canonicalise(loaded)
    assert np.array_equal(got, flags)
    assert np.count_nonzero(flags == 0) >= 24 and all(np.count_nonzero(flags == v) >= 6 for v in (1, 2, 3))
    # the one-unit tiles really are one unit apart: 299 R + 587 G + 114 B over the halves
    luma = 299 * ((tiles >> 16) & 0xFF).astype(np.int64) + 587 * ((tiles >> 8) & 0xFF).astype(np.int64) + 114 * (tiles & 0xFF).astype(np.int64)
    lr = luma[:, :, 4:].sum((1, 2)) - luma[:, :, :4].sum((1, 2))
    tb = luma[:, 4:, :].sum((1, 2)) - luma[:, :4, :].sum((1, 2))
    assert np.all(np.abs(lr[-24:]) == 1) and np.all(np.abs(tb[-24:]) == 1) and np.count_nonzero(lr == 0) >= 18 and np.count_nonzero(tb == 0) >= 18


def test_load_contents_differ_only_as_claimed(oracle):
    shape = lc.LOAD_SHAPES[3]
    for base in ("synth", "noise"):
        a, b = lc.load_case(base, shape), lc.load_case(base + "-alpha", shape)
        assert np.array_equal(a & 0xFFFFFF, b & 0xFFFFFF) and len(np.unique(b >> 24)) > 200
        assert np.array_equal(oracle.load_from_image(a[0], shape[3], shape[4]), oracle.load_from_image(b[0], shape[3], shape[4]))  # alpha is dropped
    ties = lc.load_case("mirror-ties", shape)
    _, fl = oracle.canonicalise(oracle.load_from_image(ties[0], shape[3], shape[4]))
    assert set(fl.tolist()) == {0, 1, 2, 3}


# ---- window features --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_features(oracle):
    return {(c, b): oracle.window_dcts(lc.frame_buffer(c, b)) for c, b in lc.WINDOW_CASES}


def test_window_buffers_cover_the_strips_and_the_grid():
    assert [lc.window_strips(b) for b in lc.WINDOW_BUFFERS] == [1, 1, 1, 1, 1, 4, 4, 2, 3, 32]
    assert [lc.window_strips(b) for b in lc.WINDOW_BUFFERS_LARGE] == [1025, 1032]
    assert all(lc.window_strips(b) > lc.WD_GRID for b in lc.WINDOW_BUFFERS_LARGE)
    assert (72 - 7) * (2759 - 7) == 178880 and (39 - 7, 15 - 7) == (lc.WD_CX, lc.WD_RY)


def test_window_features_ignore_alpha_and_stay_in_the_matrix_range(window_features):
    for b in lc.WINDOW_BUFFERS:
        assert np.array_equal(window_features["noise", b], window_features["noise-alpha", b])
        assert np.any(lc.frame_buffer("noise-alpha", b) >> 24)
    largest = {}
    for (c, b), feat in window_features.items():
        largest[c] = max(largest.get(c, 0), int(np.abs(feat.astype(np.int32)).max()))
    print(largest)
    assert set(largest) == set(lc.WINDOW_CONTENTS) and all(v <= lc.MM_LIMIT6 for v in largest.values()), largest


def test_window_contents_are_what_they_claim(window_features):
    b = (104, 64)
    flat = window_features["flat", b]
    assert np.all(flat == flat[0]) and np.count_nonzero(flat[0]) <= 3  # the same three DC terms in every window
    two = window_features["two-level", b].astype(np.int32)
    ac = np.delete(two, [0, 64, 128], axis=1)
    assert np.count_nonzero(ac == 0) > 0.2 * ac.size and np.count_nonzero(np.abs(ac) == 1) > 0.02 * ac.size  # roundings on either side of +-0.5
    per = window_features["periodic", b].reshape(64 - 7, 104 - 7, 192)
    assert np.array_equal(per[:-8], per[8:]) and np.array_equal(per[:, :-8], per[:, 8:]) and not np.array_equal(per[:-1], per[1:])  # windows recur
    fb = lc.frame_buffer("checker", b)
    assert set(np.unique(fb).tolist()) == {0, 0xFFFFFF}
    assert np.all(fb[5:13, 6:13] != fb[5:13, 5:12]) and np.all(fb[6:13, 5:13] != fb[5:12, 5:13]) and fb[0, 4] == fb[0, 5] and fb[4, 0] == fb[5, 0]  # the phase flips at 5, 13, ...


# ---- motion search from a frame buffer --------------------------------------------------------------------------------------------------
def test_motion_cases_move_tiles_and_settle_ties(oracle):
    grid = (13, 8)
    assert len(lc.MOTION_CASES) == (5 * 4 + 1) * len(lc.WINDOW_CONTENTS)
    for content, moves in (("synth", True), ("flat", False), ("periodic", True)):
        win = oracle.window_dcts(lc.motion_frame_buffer(content, grid))
        cur = oracle.features_rgb(lc.screen_to_tiles(lc.motion_second_frame(content, grid)), None, 1, False)
        err, px, py = oracle.motion_search(cur, grid[0], grid[1], win, 32)
        assert bool(np.any(px != 0) or np.any(py != 0)) == moves, content
        if content == "periodic":  # equal candidates a period apart: the penalty takes the nearest
            assert np.abs(px).max() <= 7 and np.abs(py).max() <= 7
    for g in lc.MOTION_GRIDS:  # both sides of every search stay in the matrix form's range: the default form is the matrix search
        for content in lc.WINDOW_CONTENTS:
            win = oracle.window_dcts(lc.motion_frame_buffer(content, g))
            cur = oracle.features_rgb(lc.screen_to_tiles(lc.motion_second_frame(content, g)), None, 1, False)
            assert max(np.abs(win.astype(np.int32)).max(), np.abs(cur.astype(np.int32)).max()) <= lc.MM_LIMIT6, (content, g)
    second = lc.motion_second_frame("ramps", grid)
    fb = lc.motion_frame_buffer("ramps", grid)
    quiet = np.abs((second[:-2, 3:] & 0xFF).astype(int) - (fb[2:, :-3] & 0xFF).astype(int))
    assert quiet.max() <= 2 and np.count_nonzero(quiet) > 0  # moved by (+3, -2), +-2 of noise


# ---- the Load step -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.STEP_CLIPS))
def test_step_clips_cut_where_they_claim(oracle, name):
    n, w, h, cut, values, keyframes = lc.STEP_CLIPS[name]
    frames = lc.step_clip(name)
    assert frames.shape == (n, h, w) and ((w + 7) // 8) * ((h + 7) // 8) * 3 == values and lc.pearson_chunks(values) >= 2
    short = oracle_pipeline.run(oracle, frames, fps=lc.STEP_FPS, min_s=0.05, stop_after="load")
    assert short["keyframes"].tolist() == keyframes
    plain = oracle_pipeline.run(oracle, frames, fps=lc.STEP_FPS, stop_after="load")
    assert plain["keyframes"].tolist() == [0]
    assert np.array_equal(_bits(plain["correl"]), _bits(short["correl"]))
