"""GlobalTilingUseTargetPSNR: Reduce makes the single STCGREval(GlobalTilingTargetPSNR) probe instead of SolveTileCount's search
(tilingencoder.pas:1916-1919, 4014-4041).  An item stays predicted when its motion PSNR -- divided by 10 on the first frame of a
key frame's group -- exceeds the target; every other item's tile is a global tile, with no tile budget."""
import numpy as np
import pytest

from tests.test_gpu_wavelet_features import assert_matches_pipeline, run_encoder

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class TargetOracle:
    """the oracle, with SolveTileCount replaced by the one probe at the target: oracle_pipeline then marks predicted = eff > x"""

    def __init__(self, oracle, target):
        self._o = oracle
        self._target = target

    def __getattr__(self, name):
        return getattr(self._o, name)

    def solve_tile_count(self, sorted_min_psnr, target):
        return self._target, 1


def _frames():
    from tiler_amd import synth
    return synth.video(10, 64, 64, cut=4)


@pytest.mark.parametrize("target", [20.0, 30.0, 38.0, 45.0, 100.0])
@pytest.mark.parametrize("pc", [1, 3])
def test_target_psnr_with_motion_matches_pipeline(oracle, target, pc):
    """radius 32; 100 dB is clamped to the PSNR ceiling (10 log10(255^2 / 0.5)), above every item's: nothing is predicted"""
    from tests import oracle_pipeline
    frames = _frames()
    enc = run_encoder(frames, PaletteCount=pc, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=32, FrameTilingExtendedPaletteUsage=False,
                      GlobalTilingUseTargetPSNR=True, GlobalTilingTargetPSNR=target, GlobalTilingTileCount=40)
    x = float(enc.GlobalTilingTargetPSNR)
    assert x == min(target, 10 * np.log(255 * 255 / 0.5) / np.log(10.0))
    exp = oracle_pipeline.run(TargetOracle(oracle, x), frames, palette_count=pc, min_s=0.1, motion_radius=32, tile_count=40)
    assert exp["threshold"] == x and exp["probes"] == 1
    if target == 100.0:
        assert not exp["predicted_reduce"].any()
    assert_matches_pipeline(oracle, enc, exp, frames.shape[0])
    enc.close()


@pytest.mark.parametrize("epu", [False, True])
def test_target_psnr_without_motion_keeps_every_distinct_tile(oracle, epu):
    """radius 0: no item has a motion PSNR, STCGREval predicts nothing, so every distinct tile is a global tile whatever
    GlobalTilingTileCount says"""
    from tests import oracle_pipeline
    frames = _frames()
    q = frames.shape[0] * (64 // 8) * (64 // 8)
    enc = run_encoder(frames, PaletteCount=2, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=epu,
                      GlobalTilingUseTargetPSNR=True, GlobalTilingTargetPSNR=30.0, GlobalTilingTileCount=25)
    exp = oracle_pipeline.run(oracle, frames, palette_count=2, min_s=0.1, motion_radius=0, tile_count=q, epu=epu)
    assert exp["T"] > 25
    assert_matches_pipeline(oracle, enc, exp, frames.shape[0])
    enc.close()


def _reduce_only(frames, radius, **settings):
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount = 2
    enc.ShotTransMinSecondsPerKF = 0.1
    enc.MotionPredictRadius = radius
    for k, v in settings.items():
        setattr(enc, k, v)
    nf, h, w = frames.shape
    enc.SetVideo(w, h, 24.0, nf)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    enc.Run(S.esLoad)
    enc.Run(S.esPredictMotion)
    enc.Run(S.esReduce)
    return enc


def _reduce_state(enc, nf):
    hdr, _, rgb = enc.Tiles()
    return rgb, hdr["UseCount"].copy(), [enc.TileMap(f)["TileIdx"].copy() for f in range(nf)], [enc.TileMap(f)["Flags"].copy() for f in range(nf)]


def test_tile_count_does_not_fall_as_the_target_rises():
    from tiler_amd.encoder import TEncoderStep as S
    frames = _frames()
    # (from 10 dB up: a key frame's first frame compares PSNR / 10, at most 5.1, so some items always stay unpredicted)
    enc = _reduce_only(frames, 32, GlobalTilingUseTargetPSNR=True, GlobalTilingTargetPSNR=10.0)
    ts = []
    for x in np.arange(10.0, 52.0, 1.5):
        enc.GlobalTilingTargetPSNR = float(x)
        enc.Run(S.esReduce)
        ts.append(enc.counts()["tiles"])
    assert all(a <= b for a, b in zip(ts, ts[1:])), ts
    assert ts[0] < ts[-1]
    enc.close()


@pytest.mark.parametrize("radius", [0, 32])
def test_tile_count_setting_has_no_effect_under_the_flag(radius):
    frames = _frames()
    nf = frames.shape[0]
    states = []
    for tc in (10, 60, 0):
        enc = _reduce_only(frames, radius, GlobalTilingUseTargetPSNR=True, GlobalTilingTargetPSNR=33.0, **({"GlobalTilingTileCount": tc} if tc else {}))
        states.append(_reduce_state(enc, nf))
        enc.close()
    for s in states[1:]:
        for a, b in zip(states[0], s):
            if isinstance(a, list):
                assert all(np.array_equal(u, v) for u, v in zip(a, b))
            else:
                assert np.array_equal(a, b)
    # and the flag is what makes the difference: the budget search with the smallest of those counts keeps fewer tiles
    enc = _reduce_only(frames, radius, GlobalTilingTileCount=10)
    assert enc.counts()["tiles"] < states[0][0].shape[0]
    enc.close()


def test_gtm_settings_carry_the_flag(oracle, tmp_path):
    from tests import gtm_reader
    frames = _frames()
    path = str(tmp_path / "tp.gtm")
    enc = run_encoder(frames, PaletteCount=2, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=32, FrameTilingExtendedPaletteUsage=False,
                      GlobalTilingUseTargetPSNR=True, GlobalTilingTargetPSNR=36.5, OutputFileName=path)
    enc.close()
    _, pl = gtm_reader.play(oracle, open(path, "rb").read())
    lines = pl.settings.split("\r\n")
    assert "GlobalTilingUseTargetPSNR=1" in lines and "GlobalTilingTargetPSNR=36.5" in lines


def test_gtm_settings_carry_the_dithering_mode(oracle, tmp_path):
    """a stream saved with DitheringMode = 1 says so in its settings text, and LoadSettings of that text brings the 1 back.  ReloadGTM
    itself leaves the setting alone, as the reference does: LoadStream seeks past the settings record (tilingencoder.pas:5057-5060)
    and takes only what the stream's commands carry -- the palettes' size and count."""
    from tests import gtm_reader
    from tiler_amd.encoder import TilingEncoder
    frames = _frames()
    nf, h, w = frames.shape
    path = str(tmp_path / "dm.gtm")
    enc = run_encoder(frames, PaletteCount=2, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False,
                      DitheringMode=1, OutputFileName=path)
    enc.close()
    _, pl = gtm_reader.play(oracle, open(path, "rb").read())
    assert "DitheringMode=1" in pl.settings.split("\r\n")
    ini = tmp_path / "dm.ini"
    ini.write_bytes(pl.settings.encode("latin-1"))
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    assert enc.DitheringMode == 4
    enc.LoadSettings(ini)
    assert enc.DitheringMode == 1 and enc.PaletteCount == 2
    enc.LoadDefaultSettings()
    enc.DitheringMode = 3
    enc.SetVideo(w, h, 24.0, nf)
    enc.ReloadGTM(path)
    assert enc.PaletteCount == 2 and enc.DitheringMode == 3
    enc.close()


def test_target_psnr_at_full_size(oracle):
    """the 720p x 300 clip at radius 32 with a target above the one the default budget lands on: more global tiles than the
    budget (320 705) has ever carried through PreparePalettes, Dither, Reconstruct and Reindex"""
    from tiler_amd import stages
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    from tests.test_gpu_fullsize import SIZES, device_video, exact_nn
    w, h, nf, npal = SIZES["720p300"]
    frames = device_video(w, h, nf)
    tm_w, tm_h = w // 8, h // 8
    per, q = tm_w * tm_h, nf * tm_w * tm_h
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount = npal
    enc.FrameTilingExtendedPaletteUsage = False
    budget = 320705  # the clip's default GlobalTilingTileCount
    enc.SetVideo(w, h, 24.0, nf)
    enc.SetFramesDevice(frames)
    enc.Run(S.esLoad)
    enc.Run(S.esPredictMotion)
    enc.GlobalTilingUseTargetPSNR = True
    T = 0
    for x in np.arange(10.0, 51.5, 1.0):  # the lowest whole-dB target whose probe keeps more than the budget
        enc.GlobalTilingTargetPSNR = float(x)
        enc.Run(S.esReduce)
        T = enc.counts()["tiles"]
        if T > budget:
            break
    assert T > budget, T
    print(f"\ntarget PSNR {float(x)}: T = {T}, Reduce {enc.StageMs()[int(S.esReduce)]:.2f} ms")
    # Reduce: distinct tiles; the unpredicted items are exactly the ones the tile map points at, and the use counts sum to them
    hdr, _, rgb = enc.Tiles()
    use = hdr["UseCount"].astype(np.int64)
    assert use.min() >= 1 and np.all(np.diff(use) <= 0)
    tms = enc.TileMaps()
    ti = tms["TileIdx"].reshape(-1)
    pred = ((tms["Flags"].reshape(-1) >> 2) & 1).astype(bool)
    assert np.array_equal(ti < 0, pred)
    assert use.sum() == (~pred).sum()
    assert np.array_equal(np.bincount(ti[ti >= 0], minlength=T), use)
    del tms, ti, pred
    for st in (S.esPreparePalettes, S.esDither, S.esReconstruct):
        enc.Run(st)
    assert enc.counts()["tiles"] == T
    hdr, pal_px, rgb = enc.Tiles()
    pals = enc.Palettes()
    pal_idx = hdr["PalIdx_Initial"]
    assert pal_idx.min() >= 0 and pal_idx.max() < npal
    # Reconstruct: a 4 096-query sample of three frames against an exact fp64 scan of the whole database
    gen = torch.Generator(device="cuda").manual_seed(7)
    db = stages.features_pal(torch.from_numpy(pal_px).cuda(), torch.from_numpy(pal_idx.astype(np.int32)).cuda(), torch.from_numpy(pals).cuda(), 1)
    for f in torch.randint(0, nf, (3,), generator=gen, device="cuda").tolist():
        ft, _, _ = stages.load(frames[f:f + 1], tm_w, tm_h)
        qf = stages.features_rgb(ft, None, 1, False)
        tmap = enc.TileMap(f)
        got = torch.from_numpy(tmap["TileIdx"].astype(np.int64)).cuda()
        live = torch.nonzero(got >= 0)[:, 0]  # (a perfect motion match leaves no tile)
        pick = live[torch.randperm(live.shape[0], generator=gen, device="cuda")[:4096]]
        idx, _ = exact_nn(qf[pick], db)
        assert torch.equal(got[pick], idx)
    del db
    enc.Run(S.esReindex)
    hdr2, _, _ = enc.Tiles()
    tms = enc.TileMaps()
    ti2 = tms["TileIdx"].reshape(-1)
    assert hdr2["UseCount"].astype(np.int64).sum() == (ti2 >= 0).sum()
    assert ti2.max() < hdr2.shape[0]
    enc.close()
