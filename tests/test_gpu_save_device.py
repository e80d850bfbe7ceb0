"""Save with the match lists from the device finder and the key frames coded side by side: the file is the same bytes under every
TM_SAVE_FINDER / TM_HOST_THREADS, and the bytes tm_write_gtm_host makes of the encoder's read-back tables; SaveStats says what ran."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gtm_reader, player_streams as ps  # noqa: E402
from tests.test_gpu_render import CASES as RENDER_CASES  # noqa: E402  (shapes and settings only)


def _encode(frames, **settings):
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


def _save(enc, path, monkeypatch, finder=None, threads=None, window=None):
    for key, v in (("TM_SAVE_FINDER", finder), ("TM_HOST_THREADS", threads), ("TM_LZ_WINDOW", window)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    enc.Save(str(path))
    data = open(path, "rb").read()
    st = enc.SaveStats()
    hdr = gtm_reader.read_header(data)
    assert st["raw_bytes"] == sum(k["raw"] for k in hdr["kf"]) and st["comp_bytes"] == sum(k["comp"] for k in hdr["kf"])
    assert st["key_frames"] == len(hdr["kf"]) and st["ms_wall"] > 0
    if finder:
        assert st["finder"] == finder
    assert (st["ms_finder"] > 0) == (st["finder"] == "device")
    return data, st


def _host_writer(enc, settings, path, fps):
    """tm_write_gtm_host fed with the encoder's read-back tables"""
    L = ps.write_lib()
    c = enc.counts()
    hdr, pal_px, _ = enc.Tiles()
    tm = np.ascontiguousarray(enc.TileMaps())
    assert tm.dtype.itemsize == 18
    kf = np.ascontiguousarray(enc.KeyFrames(), np.int32)
    use = np.ascontiguousarray(hdr["UseCount"], np.uint32)
    pal_px = np.ascontiguousarray(pal_px, np.uint8)
    palettes = np.ascontiguousarray(enc.Palettes(), np.int32)
    rc = L.tm_write_gtm_host(os.fsencode(str(path)), c["tm_w"], c["tm_h"], c["frames"], fps, kf.ctypes.data, kf.size, pal_px.ctypes.data, use.ctypes.data,
                             use.size, palettes.ctypes.data, palettes.shape[0], palettes.shape[1], tm.ctypes.data, settings)
    assert rc == 0, L.tm_last_error()
    return open(path, "rb").read()


def _settings_of(data):
    """the settings text the file embeds: ExtendedCommand 0, a 32-bit length, the bytes (first key frame)"""
    _, raws = ps.raw_keyframes(ps.write_lib(), data)
    n = int.from_bytes(raws[0][2:6], "little")
    return raws[0][6:6 + n]


@pytest.mark.parametrize("shape,radius,epu", RENDER_CASES)
def test_save_is_the_same_file_under_either_finder(monkeypatch, tmp_path, shape, radius, epu):
    """the clips of tests/test_gpu_render.py: motion on and off, a partial last tile row"""
    from tiler_amd import synth
    nf, h, w = shape
    enc = _encode(synth.video(nf, w, h, cut=3), PaletteCount=3, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=epu)
    default, st = _save(enc, tmp_path / "default.gtm", monkeypatch)
    device, st_d = _save(enc, tmp_path / "device.gtm", monkeypatch, finder="device", window=1000)  # (windows end inside matches)
    host, st_h = _save(enc, tmp_path / "host.gtm", monkeypatch, finder="host")
    assert default == host and device == host
    assert st_d["finder"] == "device" and st_h["finder"] == "host" and st_h["ms_finder"] == 0
    assert _host_writer(enc, _settings_of(host), tmp_path / "writer.gtm", 24.0) == host
    enc.close()


@pytest.fixture()
def three_key_frames(tmp_path):
    """the stream tests/test_gpu_player.py seeks in (key frames at 0, 4, 8), reloaded into an encoder"""
    from tiler_amd.encoder import TilingEncoder
    path = tmp_path / "made.gtm"
    made = ps.write_stream(ps.write_lib(), path, 5, 3, 64, nframes=12, kf=(0, 4, 8), mode="border", n_shared=48)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.SetVideo(40, 24, 25.0, 12)
    enc.ReloadGTM(str(path))
    yield enc, made
    enc.close()


def test_save_is_the_same_file_under_every_thread_count(monkeypatch, tmp_path, three_key_frames):
    enc, made = three_key_frames
    want, st = _save(enc, tmp_path / "h1.gtm", monkeypatch, finder="host", threads=1)  # the one-thread writer of before
    assert st["threads"] == 1 and st["finder"] == "host" and st["key_frames"] == 3
    assert _host_writer(enc, _settings_of(want), tmp_path / "writer.gtm", 25.0) == want
    for finder in ("host", "device", None):
        for threads, ran in ((1, 1), (4, 3), (None, None)):  # at most one thread per key frame
            got, st = _save(enc, tmp_path / "x.gtm", monkeypatch, finder=finder, threads=threads, window=300 if finder == "device" else None)
            assert got == want, (finder, threads)
            assert ran is None or st["threads"] == ran, (finder, threads, st)
            assert 1 <= st["threads"] <= 3


def test_a_reloaded_encoder_saves_the_same_bytes_again(monkeypatch, tmp_path, three_key_frames):
    """Save, ReloadGTM of that file into a fresh encoder, Save: the same file, with either finder"""
    from tiler_amd.encoder import TilingEncoder
    enc, _ = three_key_frames
    first, _ = _save(enc, tmp_path / "a.gtm", monkeypatch)
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.SetVideo(40, 24, 25.0, 12)
    fresh.ReloadGTM(str(tmp_path / "a.gtm"))
    second_dev, _ = _save(fresh, tmp_path / "b.gtm", monkeypatch, finder="device")
    second_host, _ = _save(fresh, tmp_path / "c.gtm", monkeypatch, finder="host", threads=1)
    assert second_dev == second_host
    again, _ = _save(fresh, tmp_path / "d.gtm", monkeypatch)
    assert again == second_dev
    fresh.close()


def test_save_stats_before_a_save(tmp_path):
    from tiler_amd import TileMotionError
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    with pytest.raises(TileMotionError) as ei:
        enc.SaveStats()
    assert ei.value.code == -1
    enc.close()
