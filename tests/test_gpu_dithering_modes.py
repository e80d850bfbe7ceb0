"""DitheringMode (TPsyVisMode) 0, 1, 3 and 4 -- the four DCT modes -- held to the oracle wherever the setting reaches: PreparePalettes'
clustering features (k_features_cluster_i32: another LUT, another cosine table for the first look and, in modes 0 and 3, the unweighted leg
of the in-order sum), the int16 entry points, and Run(esAll).  Mode 2 (pvsWavelets) has its own kernel and its own checker
(tests/test_gpu_wavelet_features.py).  Everything is compared bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.test_gpu_encoder import _assert_run_equals_oracle, _run_encoder
from tests.tile_kinds import N_EDGE_TILES, tile_kinds

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DCT_MODES = (0, 1, 3, 4)
N_CLUSTER = 24000
GRID_CAP = 256 * 8  # grid_for's cap (tm_common.h): k_features_cluster_i32 takes four tiles a workgroup, so 4 x GRID_CAP + 1 tiles send the
#                     first workgroup round a second time (the other LDS buffer) with one live wave
HALF_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_half_tiles.npz")


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _set_form(monkeypatch, form):
    """default: the separable first look, the reference's order only where the rounding is in doubt; plain: TM_FEATURES_PLAIN=1, every
    coefficient in the reference's order"""
    monkeypatch.delenv("TM_FEATURES_PLAIN", raising=False)
    if form == "plain":
        monkeypatch.setenv("TM_FEATURES_PLAIN", "1")


def _assert_features_equal(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d coefficients differ, first at tile %d coefficient %d: %d, the oracle has %d" % (
        what, bad.shape[0], bad[0][0], bad[0][1], got[bad[0][0], bad[0][1]], exp[bad[0][0], bad[0][1]])


def _oracle_cluster(oracle, tiles, mode, threads=8):
    """oracle.features_cluster with the tiles shared out over threads (ctypes drops the GIL)"""
    n = tiles.shape[0]
    parts = [slice(i * n // threads, (i + 1) * n // threads) for i in range(threads)]
    with ThreadPoolExecutor(threads) as ex:
        return np.concatenate(list(ex.map(lambda sl: oracle.features_cluster(tiles[sl], mode), parts)))


# ---- 1. the clustering features of every DCT mode -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster_set(oracle):
    """24 000 tiles of every kind, the edge tiles among them, and the oracle's clustering features of them under each DCT mode (made once)"""
    tiles, _ = tile_kinds(N_CLUSTER, 3133, edges=True)
    exp = {mode: _oracle_cluster(oracle, tiles, mode) for mode in DCT_MODES}
    for a in DCT_MODES:  # the modes are four different answers: a kernel that took one for another cannot pass
        for b in DCT_MODES:
            assert a >= b or (exp[a] != exp[b]).any(axis=1).mean() > 0.5, (a, b)
    k = 5 * (N_CLUSTER // 6)
    for mode in DCT_MODES:  # the edge tiles are where tile_kinds says: black is all zeros, white a DC and (plain cosines) no AC
        black, white = exp[mode][k], exp[mode][k + 1]
        assert not black.any() and white[0] > 0 and (mode in (3, 4) or not white[1:64].any())
    return tiles, exp


@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("mode", DCT_MODES)
def test_features_cluster_every_dct_mode_against_the_oracle(cluster_set, monkeypatch, mode, form):
    """stages.features_cluster(tiles, mode) == oracle.features_cluster(tiles, mode) over the whole set, and over its first n tiles at the
    counts where the kernel's loop changes shape: nothing, one to five tiles (a workgroup's four waves, then a second workgroup with one),
    and 4 x the grid's cap + 1 (a workgroup's second round, in the other LDS buffer, with one live wave)"""
    from tiler_amd import stages
    tiles, exp = cluster_set
    td = _dev(tiles)
    _set_form(monkeypatch, form)
    for n in (N_CLUSTER, 0, 1, 2, 3, 4, 5, 4 * GRID_CAP + 1):
        got = stages.features_cluster(td[:n].contiguous(), mode).cpu().numpy()
        _assert_features_equal(got, exp[mode][:n], "mode %d (%s), the first %d tiles" % (mode, form, n))


# ---- 2. the in-doubt branch at coefficients on a rounding edge ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def half_tiles(oracle):
    """tests/golden/cluster_half_tiles.npz (make_cluster_half_fixtures.py): per DCT mode 32 tiles with a coefficient within 1e-6 of a
    half-integer.  Checked here from the oracle alone, before anything is compared with it."""
    z = np.load(HALF_FIXTURE)
    assert tuple(z["modes"].tolist()) == DCT_MODES and z["tiles"].shape == (4, 32, 64) and z["coef"].shape == (4, 32)
    out = {}
    for m, mode in enumerate(DCT_MODES):
        tiles, coef = np.ascontiguousarray(z["tiles"][m], np.uint32), z["coef"][m]
        assert tiles.shape[0] >= 32 and coef.shape[0] == tiles.shape[0]
        for t, c in zip(tiles, coef):
            f = oracle.features_f64(t, mode, use_lab=True)[c]
            assert abs(f - np.floor(f) - 0.5) < 1e-6, "mode %d coefficient %d = %r is not on a rounding edge" % (mode, c, f)
        out[mode] = tiles
    return out


@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("mode", DCT_MODES)
def test_features_cluster_at_coefficients_on_a_rounding_edge(oracle, half_tiles, monkeypatch, mode, form):
    """the first look cannot settle these coefficients: the wave takes the in-order sum (its weighted leg in modes 1 and 4, the unweighted
    one in modes 0 and 3) and must round what the oracle rounds.  Then the same tiles at each of a workgroup's four positions with random
    tiles at the other three: the ballot that sends a wave down the in-order sum is the wave's own, and its neighbours' results stand."""
    from tiler_amd import stages
    tiles = half_tiles[mode]
    _set_form(monkeypatch, form)
    got = stages.features_cluster(_dev(tiles), mode).cpu().numpy()
    _assert_features_equal(got, oracle.features_cluster(tiles, mode), "mode %d (%s), the edge tiles" % (mode, form))
    rng = np.random.default_rng(50 + mode)
    for pos in range(4):
        mixed = rng.integers(0, 1 << 24, size=(4 * tiles.shape[0], 64), dtype=np.uint32)
        mixed[pos::4] = tiles
        got = stages.features_cluster(_dev(mixed), mode).cpu().numpy()
        _assert_features_equal(got, oracle.features_cluster(mixed, mode), "mode %d (%s), the edge tiles at position %d of four" % (mode, form, pos))


# ---- 3. the int16 entry points --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_set():
    return tile_kinds(6000, 3103, edges=True)


@pytest.mark.parametrize("mirrors", [False, True])
@pytest.mark.parametrize("use_lab", [False, True])
@pytest.mark.parametrize("mode", DCT_MODES)
def test_features_rgb_every_dct_mode_against_the_oracle(oracle, rgb_set, monkeypatch, mode, use_lab, mirrors):
    from tiler_amd import stages
    tiles, flags = rgb_set
    monkeypatch.delenv("TM_FEATURES_PLAIN", raising=False)
    monkeypatch.delenv("TM_FEATURES_BY_TILE", raising=False)
    exp = oracle.features_rgb(tiles, flags if mirrors else None, mode, use_lab)
    got = stages.features_rgb(_dev(tiles), _dev(flags) if mirrors else None, mode, use_lab).cpu().numpy()
    _assert_features_equal(got, exp, "features_rgb mode %d, use_lab %s, mirrors %s" % (mode, use_lab, mirrors))


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_features_pal_every_dct_mode_against_the_oracle(oracle, monkeypatch, mode):
    """palette-indexed tiles over six palettes, among them two extreme colours, near black and three live colours (the palettes of
    test_features_first_look_in_every_source_instantiation)"""
    from tiler_amd import stages
    monkeypatch.delenv("TM_FEATURES_PLAIN", raising=False)
    rng = np.random.default_rng(4570)
    n, npal = 2000, 6
    palettes = rng.integers(0, 1 << 24, size=(npal, 16)).astype(np.int32)
    palettes[0] = [0, 0xFFFFFF] * 8
    palettes[1] = np.arange(16) * 0x010101
    palettes[2, 2:] = palettes[2, 0]
    pal_idx = (np.arange(n) % npal).astype(np.int32)  # every palette is used
    pal_px = rng.integers(0, 16, size=(n, 64)).astype(np.uint8)
    pal_px[: n // 4] &= 1  # two-colour tiles
    exp = oracle.features_pal(pal_px, pal_idx, palettes, mode)
    got = stages.features_pal(_dev(pal_px), _dev(pal_idx), _dev(palettes), mode).cpu().numpy()
    _assert_features_equal(got, exp, "features_pal mode %d" % mode)


# ---- 4. Run(esAll) ----------------------------------------------------------------------------------------------------------------------------
# clips and settings on which the mode changes the oracle's clustering (tiles whose palette differs from mode 4's, of the global tiles:
# 292 / 221 / 377 of 526, 7 / 78 / 6 of 523, 6 / 203 / 6 of 300 for modes 0 / 1 / 3)
RUN_CASES = {"5-palettes": ((7, 52, 100), dict(palette_count=5, motion_radius=0)),
             "motion-epu": ((10, 64, 64), dict(palette_count=4, motion_radius=32, epu=True)),  # the re-rank reads the other clustering's palettes
             "budget-300": ((7, 52, 100), dict(palette_count=3, motion_radius=5, tile_count=300))}
_RUN_EXP = {}


def _run_expected(oracle, case, mode):
    """the oracle pipeline's tables for a case under a mode (made once: both k-means paths are compared with the same ones)"""
    from tiler_amd import synth
    from tests import oracle_pipeline
    if (case, mode) not in _RUN_EXP:
        shape, kw = RUN_CASES[case]
        frames = synth.video(shape[0], shape[2], shape[1], cut=4)
        _RUN_EXP[(case, mode)] = (frames, oracle_pipeline.run(oracle, frames, min_s=0.1, dithering_mode=mode, **kw))
    return _RUN_EXP[(case, mode)]


@pytest.mark.parametrize("km", ["resident", "launches"])
@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("case", list(RUN_CASES))
def test_run_with_a_dct_dithering_mode_matches_pipeline(oracle, monkeypatch, case, mode, km):
    """Run(esAll) with DitheringMode = 0, 1, 3 against the oracle pipeline, the tile k-means resident and with launches per iteration.
    A case in which the mode changed nothing would prove nothing: the oracle's two clusterings must differ before the encoder runs."""
    monkeypatch.delenv("TM_KM_LAUNCHES", raising=False)
    if km == "launches":
        monkeypatch.setenv("TM_KM_LAUNCHES", "1")
    shape, kw = RUN_CASES[case]
    frames, exp = _run_expected(oracle, case, mode)
    _, exp4 = _run_expected(oracle, case, 4)
    assert exp["pal_idx"].shape == exp4["pal_idx"].shape
    assert int((exp["pal_idx"] != exp4["pal_idx"]).sum()) >= 1, "DitheringMode %d clusters the tiles of %s as mode 4 does" % (mode, case)
    settings = dict(PaletteCount=kw["palette_count"], ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=kw["motion_radius"],
                    FrameTilingExtendedPaletteUsage=kw.get("epu", False), DitheringMode=mode)
    if "tile_count" in kw:
        settings["GlobalTilingTileCount"] = kw["tile_count"]
    enc = _run_encoder(frames, **settings)
    assert enc.DitheringMode == mode
    _assert_run_equals_oracle(oracle, enc, exp, shape[0])
    enc.close()


def test_dithering_mode_setter_clamps():
    """SetDitheringMode through the C ABI: 0..4 (the host-side statement of the same, without an encoder: tests/test_abi.py)"""
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    assert enc.DitheringMode == 4  # pvsWeightedSpeDCT
    for v, want in ((-1, 0), (0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 4), (99, 4)):
        enc.DitheringMode = v
        assert enc.DitheringMode == want
    enc.close()
