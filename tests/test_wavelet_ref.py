"""The CPU restatement of the reference's Haar wavelet (tests/wavelet_ref.py) against the reference's own check: its Test
property (tilingencoder.pas:3872-3898) feeds the tile ToRGB(i*8, j*32, i*j) through ComputeTilePsyVisFeatures(pvsWavelets,
YUV) and ComputeInvTilePsyVisFeatures and asserts the same RGB bytes come back ('WL/InvWL mismatch')."""
import ctypes

import numpy as np
import pytest

from tests import wavelet_ref


def _round_trip(oracle, tile, snk):
    cpn = np.zeros(192, np.float32)
    oracle.L.tmo_cpn_from_rgb(tile.ctypes.data_as(ctypes.c_void_p), 0, 0, 0, cpn.ctypes.data_as(ctypes.c_void_p))  # YUV planes
    feat = wavelet_ref.features_f64(cpn, snk)
    planes = wavelet_ref.inv_features_f64(feat, snk)
    f32 = lambda v: float(np.float32(v))  # FromCpn's TFloat (Single) locals
    return np.array([oracle.yuv_to_rgb(f32(planes[p]), f32(planes[64 + p]), f32(planes[128 + p])) for p in range(64)], np.uint32)


def test_factor_is_the_double_step_value():
    assert wavelet_ref.FACTOR == 0.7071067811865475
    assert np.nextafter(wavelet_ref.FACTOR, 1.0) == 0.7071067811865476  # one ulp below the correctly rounded 1/sqrt(2)


def test_reference_test_tile_round_trips(oracle):
    snk = wavelet_ref.snake(oracle)
    assert sorted(snk.tolist()) == list(range(64))
    tile = np.array([(i * 8) | ((j * 32) << 8) | ((i * j) << 16) for i in range(8) for j in range(8)], np.uint32)  # ToRGB(i*8, j*32, i*j)
    assert np.array_equal(_round_trip(oracle, tile, snk), tile)


def test_random_tiles_round_trip(oracle):
    snk = wavelet_ref.snake(oracle)
    rng = np.random.default_rng(2727)
    bad = 0
    for k in range(300):
        if k % 3 == 0:
            tile = rng.integers(0, 1 << 24, 64, dtype=np.uint32)
        else:  # smooth tiles: zero high-pass coefficients take the inverse's interpolating branches
            base = rng.integers(0, 200, 3)
            y, x = np.mgrid[0:8, 0:8]
            ch = [np.clip(base[c] + (x if c != 1 else y) * rng.integers(0, 4) + rng.integers(0, 2, (8, 8)) * (k % 2), 0, 255) for c in range(3)]
            tile = (ch[0] | (ch[1] << 8) | (ch[2] << 16)).astype(np.uint32).ravel()
        bad += int(not np.array_equal(_round_trip(oracle, tile, snk), tile))
    assert bad == 0


def test_wavelet_is_not_the_dct(oracle):
    """the oracle's mode 2 is a plain DCT (it has no wavelet branch): the restatement must not be that"""
    snk = wavelet_ref.snake(oracle)
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 1 << 24, (64, 64), dtype=np.uint32)
    got = wavelet_ref.features_cluster_wavelet(wavelet_ref.lab_planes(oracle, tiles), snk)
    assert not np.array_equal(got, oracle.features_cluster(tiles, 2))


@pytest.mark.parametrize("seed", [0, 1])
def test_vectorised_form_equals_the_line_by_line_one(oracle, seed):
    snk = wavelet_ref.snake(oracle)
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 1 << 24, (40, 64), dtype=np.uint32)
    tiles[:8] = tiles[:8, :1]  # flat tiles
    planes = wavelet_ref.lab_planes(oracle, tiles)
    got = wavelet_ref.features_cluster_wavelet(planes, snk)
    for t in range(tiles.shape[0]):
        cpn = np.zeros(192, np.float32)
        oracle.L.tmo_cpn_from_rgb(tiles[t].ctypes.data_as(ctypes.c_void_p), 1, 0, 0, cpn.ctypes.data_as(ctypes.c_void_p))
        assert np.array_equal(cpn.view(np.uint32), planes[t].reshape(-1).view(np.uint32))  # ConvertToCpnPixels with UseLAB
        want = np.rint(np.array(wavelet_ref.features_f64(cpn, snk))).astype(np.int32)
        assert np.array_equal(got[t], want)
