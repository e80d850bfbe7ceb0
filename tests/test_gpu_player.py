"""The .gtm player on the device (tm_player_*, tiler_amd.player.GtmPlayer, tm_stage_play_frame) and .gtm streams as Load's input: every
frame bit for bit what tm_reload_gtm + tm_render_frames give, in calls of any size, to device and host memory, after any seek."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gtm_reader, player_streams as ps  # noqa: E402
from tests.test_gpu_render import CASES, _chain_depth, _encode, _pan_clip, _swap_rb  # noqa: E402


@pytest.fixture(scope="module")
def L():
    return ps.write_lib()


def _reload_render(path, w, h, fps, nf):
    """what the code before the player gives for a file: a fresh encoder, ReloadGTM, RenderFrames"""
    from tiler_amd.encoder import TilingEncoder
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.SetVideo(w, h, fps, nf)
    fresh.ReloadGTM(str(path))
    out = fresh.RenderFrames(device=False)
    fresh.close()
    return out


def _play(path, step, device):
    """all frames of the file, read `step` at a time (None: in one call)"""
    from tiler_amd.player import GtmPlayer
    parts = []
    with GtmPlayer(path) as p:
        n = p.info()["frames"]
        while p.Tell() < n:
            r = p.Read(step, device=device)
            assert r.shape[0] == min(step or n, n - sum(x.shape[0] for x in parts))
            parts.append(r.cpu().numpy().view(np.uint32) if device else r)
        assert p.Read(2, device=device).shape[0] == 0  # at the end of the stream
    return np.concatenate(parts)


ENCODED = [(c, None) for c in CASES] + [(((40, 48, 64), 8, False), 20)]


@pytest.mark.parametrize("case,min_depth", ENCODED)
def test_encoded_clips_equal_the_render(tmp_path, monkeypatch, case, min_depth):
    """clips the encoder saved (the shapes and settings of test_gpu_render's CASES, several key frames; a 40-frame pan with a prediction
    chain >= 20 deep): the player's frames = RenderFrames of the encoder = RenderFrames after ReloadGTM, read 1, 3 and all at a time, to
    device and to host memory"""
    from tiler_amd import synth
    from tiler_amd.player import GtmPlayer
    (nf, h, w), radius, epu = case
    out = str(tmp_path / "clip.gtm")
    if min_depth is None:
        enc = _encode(synth.video(nf, w, h, cut=3), PaletteCount=3, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=radius,
                      FrameTilingExtendedPaletteUsage=epu, OutputFileName=out)
    else:
        enc = _encode(_pan_clip(nf, w, h, 4), PaletteCount=3, MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=epu,
                      ShotTransMaxSecondsPerKF=1000.0, ShotTransMinSecondsPerKF=1000.0, OutputFileName=out)
        c = enc.counts()
        depth = _chain_depth(enc.TileMaps(), c["tm_w"], c["tm_h"])
        assert depth >= min_depth, depth
        monkeypatch.setenv("TM_PLAYER_CHUNK_FRAMES", "3")  # 40 frames walk the two staging buffers many times
    c = enc.counts()
    want = enc.RenderFrames(device=False)
    kf = enc.KeyFrames()
    if min_depth is None:
        assert len(kf) > 1
    enc.close()
    assert np.array_equal(_reload_render(out, w, h, 24.0, nf), want)
    with GtmPlayer(out) as p:
        i = p.info()
        assert (i["width"], i["height"], i["tm_w"], i["tm_h"], i["frames"], i["keyframes"]) == (c["tm_w"] * 8, c["tm_h"] * 8, c["tm_w"], c["tm_h"], nf, len(kf))
        assert i["fps"] == pytest.approx(24.0, rel=1e-6) and i["pal_size"] == 16 and i["pal_count"] == 3 and i["encoder_version"] == 4
        assert np.array_equal(p.KeyFrames(), kf) and "MotionPredictRadius=%d" % radius in p.SettingsText()
    for step in (1, 3, None):
        for device in (True, False):
            got = _play(out, step, device)
            assert got.shape == want.shape
            for f in range(nf):
                assert np.array_equal(got[f], want[f]), (step, device, f)


@pytest.mark.parametrize("tm_w,tm_h,pal_size,mode", [(33, 17, 2, "inside"), (33, 17, 64, "inside"), (33, 17, 64, "border"), (33, 17, 2, "border"), (5, 3, 64, "border")])
def test_every_command_form_on_the_device(L, oracle, tmp_path, monkeypatch, tm_w, tm_h, pal_size, mode):
    """hand-made streams with all seven item commands (561 and 15 items: the last workgroup is partial).  Offsets that stay inside the picture:
    the frames are the reference player's (tests/gtm_reader.Player; R and B swapped, alpha dropped).  Offsets that leave it at all four
    borders and corners: the JavaScript player does not clamp, so ReloadGTM + RenderFrames is the oracle"""
    path = tmp_path / "made.gtm"
    s = ps.write_stream(L, path, tm_w, tm_h, pal_size, nframes=6, kf=(0, 3), mode=mode)
    monkeypatch.setenv("TM_PLAYER_CHUNK_FRAMES", "2")
    got = _play(path, None, True)
    assert got.shape == (6, tm_h * 8, tm_w * 8)
    if mode == "inside":
        hdr, pl = gtm_reader.play(oracle, s["data"])
        assert {it[0] for fr in pl.items for it in fr} == ps.ITEM_KINDS
        for f in range(6):
            assert np.array_equal(got[f], _swap_rb(np.asarray(pl.frames[f]) & 0xFFFFFF)), f
    else:
        tm = s["tilemaps"]
        pred = (tm["Flags"] & 4) != 0
        per_row = np.arange(tm_w * tm_h) % tm_w
        per_col = np.arange(tm_w * tm_h) // tm_w
        x = per_row[None, :] * 8 + tm["PredictedX"].astype(int)
        y = per_col[None, :] * 8 + tm["PredictedY"].astype(int)
        for leaves in (x < 0, x > tm_w * 8 - 8, y < 0, y > tm_h * 8 - 8, (x < 0) & (y < 0), (x > tm_w * 8 - 8) & (y > tm_h * 8 - 8)):
            assert (pred & leaves).any()
    want = _reload_render(path, tm_w * 8, tm_h * 8, 25.0, 6)
    for f in range(6):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(_play(path, 1, False), want)


def test_seek(L, tmp_path):
    """three key frames: after a seek to any frame, one frame and the rest of the stream are the sequential play's; a seek backwards after
    the end works; a seek out of range is TM_E_INVAL"""
    from tiler_amd._lib import TileMotionError
    from tiler_amd.player import GtmPlayer
    path = tmp_path / "made.gtm"
    ps.write_stream(L, path, 5, 3, 64, nframes=12, kf=(0, 4, 8), mode="border", n_shared=48)
    seq = _play(path, None, True)
    with GtmPlayer(path) as p:
        assert p.info()["keyframes"] == 3
        for f in list(range(12)) + [5, 2, 11, 0]:
            p.Seek(f)
            assert p.Tell() == f
            assert np.array_equal(p.Read(1, device=False), seq[f:f + 1]), f
            p.Seek(f)
            assert np.array_equal(p.Read().cpu().numpy().view(np.uint32), seq[f:]), f
            assert p.Tell() == 12
        p.Seek(12)
        assert p.Read(1).shape[0] == 0
        p.Seek(3)  # backwards after the end
        assert np.array_equal(p.Read(2, device=False), seq[3:5])
        for bad in (-1, 13):
            with pytest.raises(TileMotionError) as ei:
                p.Seek(bad)
            assert ei.value.code == -1
        assert np.array_equal(p.Read(1, device=False), seq[5:6])  # a refused seek moves nothing


def test_damaged_later_key_frame_ends_the_call_before_it(L, tmp_path):
    """the second of three key frames damaged behind an intact index: open succeeds (it reads the first only); a read of everything is
    TM_E_IO, has delivered the first key frame's frames, and stands at the damaged one; a seek past it plays on"""
    from tiler_amd._lib import TileMotionError
    from tiler_amd.player import GtmPlayer
    path = tmp_path / "made.gtm"
    s = ps.write_stream(L, path, 5, 3, 64, nframes=12, kf=(0, 4, 8), mode="border", n_shared=48)
    seq = _play(path, None, True)
    hdr = gtm_reader.read_header(s["data"])
    blob = bytearray(s["data"])
    at = hdr["whole"] + hdr["kf"][0]["comp"]
    for i in range(at + 13, at + hdr["kf"][1]["comp"]):  # the range coder's bytes of key frame 1
        blob[i] ^= 0x5A
    bad = tmp_path / "bad.gtm"
    bad.write_bytes(bytes(blob))
    for worker in ("0", "1"):
        os.environ["TM_PLAYER_NO_WORKER"] = worker
        try:
            with GtmPlayer(bad) as p:
                buf = torch.zeros((12, 24, 40), dtype=torch.int32, device="cuda")
                with pytest.raises(TileMotionError) as ei:
                    p.Read(12, out=buf)
                assert ei.value.code == -5 and "key frame 1" in str(ei.value)
                assert p.Tell() == 4
                assert np.array_equal(buf[:4].cpu().numpy().view(np.uint32), seq[:4]) and not buf[4:].any()
                with pytest.raises(TileMotionError):
                    p.Read(1)
                assert p.Tell() == 4
                p.Seek(9)
                assert np.array_equal(p.Read(device=False), seq[9:])
                p.Seek(2)
                assert np.array_equal(p.Read(2, device=False), seq[2:4])
        finally:
            del os.environ["TM_PLAYER_NO_WORKER"]


def test_callers_buffer_may_be_overwritten_between_calls(L, tmp_path):
    """two calls into the same device buffer with junk written between them: the second call's first frame (predicted items) is right"""
    from tiler_amd.player import GtmPlayer
    path = tmp_path / "made.gtm"
    s = ps.write_stream(L, path, 5, 3, 64, nframes=8, kf=(0,), mode="border", n_shared=48)
    assert (s["tilemaps"]["Flags"][4] & 4).any()
    seq = _play(path, None, True)
    with GtmPlayer(path) as p:
        buf = torch.empty((4, 24, 40), dtype=torch.int32, device="cuda")
        assert np.array_equal(p.Read(4, out=buf).cpu().numpy().view(np.uint32), seq[:4])
        buf.fill_(0x00C0FFEE)
        torch.cuda.synchronize()
        assert np.array_equal(p.Read(4, out=buf).cpu().numpy().view(np.uint32), seq[4:])


def _saved_source(tmp_path):
    """-> path of a saved 8-frame 100 x 52 stream (104 x 56 in tiles), its frames as the player gives them, and a maker of encoders that take it as input"""
    from tiler_amd import synth
    from tiler_amd.encoder import TilingEncoder
    nf, h, w = 8, 52, 100
    src = str(tmp_path / "src.gtm")
    _encode(synth.video(nf, w, h, cut=4), PaletteCount=3, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False,
            OutputFileName=src).close()

    def opened(devices=None, **kw):
        enc = TilingEncoder()
        enc.LoadDefaultSettings()
        enc.PaletteCount = 3
        enc.InputFileName = src
        for k, v in kw.items():
            setattr(enc, k, v)
        if devices:
            enc.SetDevices(devices)
        return enc

    return src, _play(src, None, True), opened


def test_gtm_as_load_input(tmp_path):
    """OpenInput on a saved stream: the video is the stream's; after Run(esLoad) the input render is the player's frames; StartFrame /
    FrameCount select; a whole Run with Save gives a stream that plays; Scaling != 1 is refused before Load"""
    from tiler_amd._lib import TileMotionError
    from tiler_amd.encoder import TEncoderStep
    nf = 8
    src, played, opened = _saved_source(tmp_path)
    enc = opened()
    assert enc.OpenInput() == dict(width=104, height=56, fps=pytest.approx(24.0, rel=1e-6), frames=nf)
    enc.Run(TEncoderStep.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), played)
    enc.close()
    enc = opened(StartFrame=2, FrameCount=5)
    assert enc.OpenInput()["frames"] == 5
    enc.Run(TEncoderStep.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), played[2:7])
    enc.close()
    out = str(tmp_path / "again.gtm")
    enc = opened(OutputFileName=out, ShotTransMinSecondsPerKF=0.1)
    enc.Run()  # Load opens the input by itself
    assert enc.VideoInfo()["frames"] == nf and len(enc.KeyFrames()) >= 1
    want = enc.RenderFrames(device=False)
    enc.close()
    assert np.array_equal(_play(out, 3, False), want)
    enc = opened(Scaling=0.5)
    with pytest.raises(TileMotionError) as ei:
        enc.OpenInput()
    assert ei.value.code == -6 and "Scaling" in str(ei.value)
    enc.close()


def test_gtm_as_load_input_of_two_shards(tmp_path):
    """a device group of two shards loads the same clip as one device: each shard plays what its Load reads"""
    from tiler_amd import lib
    from tiler_amd.encoder import TEncoderStep
    if lib().tm_device_count() < 2:
        pytest.skip("one device visible: the two-shard Load is not run")
    src, played, opened = _saved_source(tmp_path)
    enc = opened(devices=[0, 1])
    enc.OpenInput()
    enc.Run(TEncoderStep.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), played)
    enc.close()


def _frame_by_rule(recs, intra, tiles, palettes, prev, tm_w, tm_h):
    """DESIGN.md section 16 'What is drawn', restated: one frame from records"""
    W, H = tm_w * 8, tm_h * 8
    out = np.zeros((H, W), np.uint32)
    pal_size = palettes.shape[1]
    for i, r in enumerate(recs):
        y0, x0 = (i // tm_w) * 8, (i % tm_w) * 8
        a, pal, fl = int(r["a"]), int(r["pal"]), int(r["flags"])
        if fl & 4:
            ox, oy = (a & 127) - (a & 128), ((a >> 8) & 127) - ((a >> 8) & 128)
            for y in range(8):
                for x in range(8):
                    out[y0 + y, x0 + x] = 0 if prev is None else prev[min(max(y0 + y + oy, 0), H - 1), min(max(x0 + x + ox, 0), W - 1)]
            continue
        src = intra if fl & 8 else tiles
        if a >= src.shape[0] or pal >= palettes.shape[0]:
            continue
        t = src[a].reshape(8, 8)
        t = t[:, ::-1] if fl & 1 else t
        t = t[::-1, :] if fl & 2 else t
        col = np.where(t < pal_size, palettes[pal].astype(np.uint32)[np.minimum(t, pal_size - 1)], 0)
        out[y0:y0 + 8, x0:x0 + 8] = _swap_rb(col)
    return out


def test_stage_seam_single_frames():
    """tm_stage_play_frame on hand-made records: colour indices >= the palette size, tile / palette / intra indices out of range, every mirror
    flag, predicted items with a zeroed and with no previous frame, offsets past every border -- against the rule restated above"""
    from tiler_amd import player
    rng = np.random.default_rng(5)
    tm_w, tm_h, pal_size = 5, 3, 5
    tiles = rng.integers(0, 8, (7, 64), dtype=np.uint8)   # indices 5 .. 7 are beyond the palette size
    intra = rng.integers(0, 8, (3, 64), dtype=np.uint8)
    palettes = rng.integers(1, 1 << 24, (4, pal_size)).astype(np.int32)
    recs = np.zeros(15, ps.RECORD)
    recs[0] = (0, 0, 0, 0)
    recs[1] = (6, 3, 1, 0)
    recs[2] = (3, 2, 2, 0)
    recs[3] = (5, 1, 3, 0)
    recs[4] = (7, 0, 0, 0)            # tile index out of range
    recs[5] = (2, 4, 0, 0)            # palette index out of range
    recs[6] = (0xFFFFFFFF, 0, 0, 0)   # a tile index that is negative as int32
    recs[7] = (2, 1, 8 | 1, 0)        # intra, mirrored
    recs[8] = (3, 1, 8, 0)            # intra index out of range
    recs[9] = (0, 0, 4, 0)            # SkipBlock's item
    recs[10] = ((-100 & 255) | ((-100 & 255) << 8), 0, 4, 0)
    recs[11] = (100 | (100 << 8), 0, 4, 0)
    recs[12] = (5 | ((-3 & 255) << 8), 0, 4, 0)
    recs[13] = ((-128 & 255) | (127 << 8), 0, 4, 0)
    recs[14] = (1, 2, 8 | 2, 0)
    prev = rng.integers(0, 1 << 24, (tm_h * 8, tm_w * 8)).astype(np.uint32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype != np.int32 else a).cuda()  # noqa: E731
    d_recs, d_intra, d_tiles, d_pal = cu(recs), cu(intra), cu(tiles), cu(palettes)
    for pv in (prev, np.zeros_like(prev), None):
        d_prev = None if pv is None else torch.from_numpy(pv.view(np.int32)).cuda()
        got = player.play_frame(d_recs, d_intra, d_tiles, d_pal, d_prev, tm_w, tm_h).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, _frame_by_rule(recs, intra, tiles, palettes, pv, tm_w, tm_h))


def test_memory_does_not_grow_with_the_clip(L, tmp_path):
    """200 frames at 64 x 48 with a key frame every 10 against the same stream cut to 20 frames: the player reports the same host and device
    allocation after playing either to the end"""
    from tiler_amd.player import GtmPlayer
    kf20 = (0, 10)
    tm20 = ps.tilemaps(8, 6, 20, kf20, "border", n_shared=48)
    used = {}
    for name, reps in (("short", 1), ("long", 10)):
        path = tmp_path / (name + ".gtm")
        ps.write_arrays(L, path, 8, 6, 16, np.tile(tm20, (reps, 1)), [f + 20 * r for r in range(reps) for f in kf20], n_shared=48)
        with GtmPlayer(path) as p:
            assert p.info()["frames"] == 20 * reps and p.info()["keyframes"] == 2 * reps
            n = 0
            while True:
                r = p.Read(7, device=(n % 2 == 0))
                if r.shape[0] == 0:
                    break
                n += r.shape[0]
            assert n == 20 * reps
            i = p.info()
            used[name] = (i["host_bytes"] - 24 * i["keyframes"], i["device_bytes"])  # (the index itself is 24 bytes per key frame in memory: KfEntry)
    assert used["long"] == used["short"] and used["short"][0] > 0 and used["short"][1] > 0
