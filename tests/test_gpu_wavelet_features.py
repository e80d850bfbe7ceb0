"""DitheringMode = pvsWavelets (2): PreparePalettes' clustering features through the Haar branch of ComputeTilePsyVisFeatures
(tilingencoder.pas:3150-3157, WaveletGS 2727-2764), against the CPU restatement in tests/wavelet_ref.py (the oracle has no
wavelet branch: its mode 2 is a plain DCT, so it is never the expected value here)."""
import numpy as np
import pytest

from tests import wavelet_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class WaveletOracle:
    """the oracle, with features_cluster(mode = 2) answered by the restatement (oracle_pipeline calls it for PreparePalettes)"""

    def __init__(self, oracle):
        self._o = oracle
        self._snake = wavelet_ref.snake(oracle)

    def __getattr__(self, name):
        return getattr(self._o, name)

    def features_cluster(self, tiles, mode=4):
        if mode == 2:
            return wavelet_ref.features_cluster_wavelet(wavelet_ref.lab_planes(self._o, tiles), self._snake)
        return self._o.features_cluster(tiles, mode)


def run_encoder(frames, **settings):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in settings.items():
        setattr(enc, k, v)
    nf, h, w = frames.shape
    enc.SetVideo(w, h, 24.0, nf)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    enc.Run()
    return enc


def assert_matches_pipeline(oracle, enc, exp, nf):
    """everything test_gpu_encoder.test_run_all_matches_oracle compares"""
    c = enc.counts()
    assert np.array_equal(enc.FrameCorrelations().view(np.uint32), exp["correl"].view(np.uint32))
    assert np.array_equal(enc.KeyFrames(), exp["keyframes"])
    assert c["tiles"] == exp["final_T"]
    hdr, pal, rgb = enc.Tiles()
    assert np.array_equal(pal, exp["final_pal_px"])
    assert np.array_equal(hdr["UseCount"], exp["final_use"])
    assert np.array_equal(hdr["PalIdx_Initial"], exp["final_pal_idx"])
    assert np.array_equal(rgb, exp["final_rgb"])
    assert np.array_equal(enc.Palettes(), exp["palettes"])
    per = exp["per"]
    for f in range(nf):
        tm = enc.TileMap(f)
        sl = slice(f * per, (f + 1) * per)
        assert np.array_equal(tm["TileIdx"], exp["final_tm_tile"][sl])
        assert np.array_equal(tm["PalIdx"], exp["tm_pal"][sl])
        assert np.array_equal(tm["Flags"] & 3, exp["flags"][sl])
        assert np.array_equal((tm["Flags"] >> 2) & 1, exp["is_predicted"][sl])
        assert np.array_equal(tm["PredictedX"], exp["pred_x"][sl]) and np.array_equal(tm["PredictedY"], exp["pred_y"][sl])
        psnr = np.array([oracle.L.tmo_euclidean_to_psnr(int(e)) for e in exp["tm_err"][sl]], np.float32)
        assert np.allclose(tm["PSNR"], psnr, rtol=1e-6)
    q = enc.PSNR()
    allp = np.array([oracle.L.tmo_euclidean_to_psnr(int(e)) for e in exp["tm_err"]], np.float64)
    kf = list(exp["keyframes"]) + [nf]
    assert np.allclose(q["per_keyframe"], [allp[a * per:b * per].mean() for a, b in zip(kf[:-1], kf[1:])], rtol=1e-6)
    assert np.isclose(q["global"], allp.mean(), rtol=1e-6)


def _tile_set(n_random=60000, seed=3150):
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, 1 << 24, (n_random, 64), dtype=np.uint32)]
    # gradients: each channel a ramp along x, y or the diagonal, random start and slope
    ng = 30000
    y, x = np.mgrid[0:8, 0:8]
    ramps = np.stack([x, y, x + y, 7 - x]).reshape(4, 64)
    ch = []
    for c in range(3):
        r = ramps[rng.integers(0, 4, ng)]
        ch.append(np.clip(rng.integers(0, 256, ng)[:, None] + rng.integers(-18, 19, ng)[:, None] * r, 0, 255).astype(np.uint32))
    parts.append(ch[0] | (ch[1] << 8) | (ch[2] << 16))
    # flat tiles, every grey level and random colours
    flat = np.concatenate([np.arange(256, dtype=np.uint32) * 0x010101, rng.integers(0, 1 << 24, 9744, dtype=np.uint32)])
    parts.append(np.repeat(flat[:, None], 64, 1))
    # saturated colours: every channel 0 or 255
    sat = np.array([0xFF * ((k >> 0) & 1) | (0xFF00 * ((k >> 1) & 1)) | (0xFF0000 * ((k >> 2) & 1)) for k in range(8)], np.uint32)
    parts.append(sat[rng.integers(0, 8, (2000, 64))])
    # the reference's Test tile ToRGB(i*8, j*32, i*j) (tilingencoder.pas:3872-3874)
    parts.append(np.array([[(i * 8) | ((j * 32) << 8) | ((i * j) << 16) for i in range(8) for j in range(8)]], np.uint32))
    return np.ascontiguousarray(np.concatenate(parts)), n_random


def test_features_cluster_wavelets_bit_exact(oracle):
    from tiler_amd import stages
    tiles, n_random = _tile_set()
    assert tiles.shape[0] >= 100_000
    snk = wavelet_ref.snake(oracle)
    want = wavelet_ref.features_cluster_wavelet(wavelet_ref.lab_planes(oracle, tiles), snk)
    td = torch.from_numpy(tiles.view(np.int32)).cuda()
    got = stages.features_cluster(td, 2).cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:1]], want[bad[:1]])
    dct = stages.features_cluster(td[:n_random], 0).cpu().numpy()
    assert (dct != got[:n_random]).any(axis=1).all()  # a different transform on every random tile
    assert np.abs(got).max() <= 8 * 331  # the k-means' distance bound (tm_kmeans.hip): |v| <= 8 x the largest Lab magnitude (330.9)


def test_wavelets_on_int16_vectors_are_refused():
    """ComputeCpnPixelsPsyVisFeatures asserts 'Wavelets on SmallInt vector unimplemented!' (tilingencoder.pas:3111)"""
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    td = torch.zeros((4, 64), dtype=torch.int32, device="cuda")
    with pytest.raises(TileMotionError):
        stages.features_rgb(td, None, 2)
        torch.cuda.synchronize()


@pytest.mark.parametrize("radius,pc", [(0, 1), (0, 3), (32, 1), (32, 3)])
@pytest.mark.parametrize("km", ["resident", "launches"])
def test_run_with_wavelet_dithering_mode_matches_pipeline(oracle, radius, pc, km, monkeypatch):
    from tiler_amd import synth
    from tests import oracle_pipeline
    monkeypatch.delenv("TM_KM_LAUNCHES", raising=False)
    if km == "launches":
        monkeypatch.setenv("TM_KM_LAUNCHES", "1")
    shape = (8, 56, 72)
    frames = synth.video(shape[0], shape[2], shape[1], cut=4)
    exp = oracle_pipeline.run(WaveletOracle(oracle), frames, palette_count=pc, min_s=0.1, motion_radius=radius, dithering_mode=2)
    enc = run_encoder(frames, PaletteCount=pc, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=radius, DitheringMode=2,
                      FrameTilingExtendedPaletteUsage=False)
    assert enc.DitheringMode == 2
    assert_matches_pipeline(oracle, enc, exp, shape[0])
    enc.close()
