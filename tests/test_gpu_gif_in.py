"""GIF input on the device (tm_gif_in.hip): k_gif_lzw and k_gif_compose through their stage seams against the host
twins, byte for byte, and Load of a GIF file and of a lent one under TM_GIF_DECODE=device against the host path and against the
restatement's frames lent as RGB.  The files are written by the tests' own writer (tests/gif_ref.py): no imaging library takes part.
A Load on two different devices is not run here (one device is present where these tests run); two shards on one device are, which is the
same code: every shard decodes from image 0 to the last frame it needs."""
import os

import numpy as np
import pytest

from tests import gif_cases as C
from tests import gif_ref as R
from tiler_amd._lib import TileMotionError
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=150)


@pytest.fixture(scope="module")
def stages():
    import torch
    from tiler_amd import stages
    assert torch.cuda.is_available()
    return stages


def test_every_stream_in_one_launch_equals_the_twin(stages):
    """all case streams in one launch, between guard bytes, damaged streams beside good neighbours: the same bytes, guards included, and
    the same statuses as the host twin (which tests/test_gif_in_host.py holds to the restatement)"""
    items = C.streams()
    blob, at = bytearray(b"\x5a" * 5), []
    for _, span, _, _ in items:
        at.append(len(blob))
        blob += span + b"\xee"
    batch = [(a, len(s[1]), s[2], s[3]) for a, s in zip(at, items)]
    want, want_st, _ = stages.gif_lzw_host(bytes(blob), batch, guard=33)  # (an odd guard: destinations at every alignment)
    got, got_st, _ = stages.gif_lzw(bytes(blob), batch, guard=33)
    assert got_st == want_st
    assert {s[0] for s in got_st} == {0, R.TRUNCATED, R.BAD_CODE}
    assert np.array_equal(got.cpu().numpy(), want)


def test_lzw_batch_refusals(stages):
    for bad in ([(10, 7, 4, 4)], [(0, 4, 1, 4)], [(0, 4, 9, 4)]):
        with pytest.raises(TileMotionError) as e:
            stages.gif_lzw(bytes(16), bad)
        assert e.value.code == -1
    assert stages.gif_lzw(b"", [])[1] == []


def _same(stages, file, first=0, count=None, background=None):
    want, want_st = stages.gif_decode_host(file, first, count, background, fill=FILL)
    got, got_st = stages.gif_decode(file, first, count, background, fill=FILL)
    assert got_st == want_st
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    return want, want_st


CLIPS = [(n, f) for n, f, _ in C.clips()] + [(n, f) for n, f, _ in C.statuses()] + [(n, f) for n, f, _ in C.pictures() if "320x240" in n or "min5" in n]


@pytest.mark.parametrize("chunk", [0, 1, 3])
def test_every_clip_equals_the_twin(stages, monkeypatch, chunk):
    """every clip, whole and from a first frame > 0, with the images in one chunk, one by one and three by three: where a chunk ends
    changes no byte; a refused image delivers nothing from there on (the fill stays)"""
    if chunk:
        monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", str(chunk))
    else:
        monkeypatch.delenv("TM_INPUT_CHUNK_FRAMES", raising=False)
    for name, file in CLIPS:
        n = len(R.parse(file)["images"])
        want, st = _same(stages, file)
        if any(st):
            bad = st.index([s for s in st if s][0])
            assert (want[bad:] == FILL).all() and (want[:bad] != FILL).any() == (bad > 0), name
        for first, count in ((n // 2, None), (n - 1, 1), (1, 0)) if n > 1 else ():
            _same(stages, file, first, count)
    file = dict(CLIPS)["disposal_3_on_frame_0_small"]
    _same(stages, file, 1, 2, 0x00C0FFEE)


def test_the_damage_list_equals_the_twin(stages):
    """the seeded cuts and byte changes the walk lets through: the same statuses and the same bytes as the twin, whatever they are"""
    seen = set()
    for name, file in C.damaged():
        try:
            stages.probe_gif(file)
        except TileMotionError:
            continue
        _, st = _same(stages, file)
        seen.update(st)
    assert seen == {0, R.TRUNCATED, R.BAD_CODE}


def test_the_restatement_directly(stages):
    """one clip straight against the restatement, so that this file stands without the host tests"""
    file = dict(CLIPS)["every_disposal_pair"]
    frames = R.decode(file, 4, 9)[0]
    got, st = stages.gif_decode(file, 4, 9)
    assert not any(st) and np.array_equal(got.cpu().numpy().view(np.uint32), np.stack(frames))


def test_decode_refusals(stages):
    file = dict(CLIPS)["delays_equal"]
    for bad in (lambda: stages.gif_decode(file, 2, 5), lambda: stages.gif_decode(file, 0, 1, 1 << 24), lambda: stages.gif_decode(file, 0, 1, None, 10),
                lambda: stages.gif_decode(C.refused()[9][1], 0, 1)):
        with pytest.raises(TileMotionError):
            bad()


# ---- Load
def _encoder(**kw):
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in {**BASE, **kw}.items():
        setattr(enc, k, v)
    return enc


def _clip_file(nf=7, w=64, h=48, bg_index=3):
    """nf frames: a whole first frame, then rectangles with transparency under every disposal, one interlaced, one with a local table"""
    rng = np.random.default_rng(21)
    y, x = np.mgrid[0:h, 0:w]
    blocks = [R.gce_bytes(1, -1, 4), R.image_bytes(((x // 4 + y // 6) % 16).astype(np.uint8), min_code=4)]
    for i in range(1, nf):
        rw, rh = 20 + 3 * i, 12 + 2 * i
        idx = ((x[:rh, :rw] // 3 + y[:rh, :rw] // 2 + i) % 16).astype(np.uint8)
        idx[rng.random((rh, rw)) < 0.2] = 5
        blocks += [R.gce_bytes(i % 4, 5, 4), R.image_bytes(idx, left=(7 * i) % 40, top=(5 * i) % 30, min_code=4, interlace=i == 2,
                                                              table=[c ^ 0x3F3F3F for c in C.PAL16] if i == 3 else None)]
    return R.write_gif(w, h, blocks, table=C.PAL16, bg_index=bg_index, loop=0)


def _rgb(frames):
    f = np.stack(frames)
    return np.stack([(f >> 16) & 255, (f >> 8) & 255, f & 255], -1).astype(np.uint8)


def test_a_file_on_the_device_equals_the_host_path_and_the_restatement(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    file = _clip_file()
    nf, w, h = 7, 64, 48
    open("clip.gif", "wb").write(file)
    frames = R.decode(file)[0]
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "3")  # 7 images in three chunks, the last one short
    got = {}
    for where in ("host", "device", "rgb"):
        monkeypatch.setenv("TM_GIF_DECODE", where if where != "rgb" else "host")
        enc = _encoder(InputFileName="clip.gif", OutputFileName="out.gtm", MotionPredictRadius=0)  # (the stream holds the settings' text: one name)
        if where == "rgb":  # the restatement's frames, lent as RGB
            assert enc.SetFramesRGB(_rgb(frames), "rgb24", fps=25.0) == dict(width=w, height=h, fps=25.0, frames=nf)
        else:
            assert enc.OpenInput() == dict(width=w, height=h, fps=25.0, frames=nf)
        enc.Run(S.esLoad)
        if where != "rgb":
            st = enc.InputStats()
            assert st["where"] == where and st["kind"] == 16 and st["frames"] == nf and st["file_bytes"] == len(file)
        assert np.array_equal(enc.RenderFrames(input=True, device=False)[:, :h, :w], np.stack(frames))
        enc.Run(S.esLoad)  # a second Load reads the clip it has
        enc.Run()
        enc.Save()
        got[where] = open("out.gtm", "rb").read()
        os.remove("out.gtm")
        enc.close()
    assert got["device"] == got["host"] == got["rgb"] and len(got["host"]) > 1000


def _load(enc, h, w):
    enc.Run(S.esLoad)
    return enc.RenderFrames(input=True, device=False)[:, :h, :w]


@pytest.mark.parametrize("where", ["host", "device"])
def test_ranges_background_lent_file_and_kinds(stages, tmp_path, monkeypatch, where):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_GIF_DECODE", where)
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "2")
    file = _clip_file(6, 40, 32, bg_index=200)  # a background index outside the table: black
    open("clip.gif", "wb").write(file)
    small = dict(CLIPS)["disposal_3_on_frame_0_small"]  # a first frame that leaves the background showing
    open("small.gif", "wb").write(small)
    # StartFrame and FrameCount: the frames before are composited, not delivered
    enc = _encoder(InputFileName="clip.gif", StartFrame=2, FrameCount=3, MotionPredictRadius=0)
    assert enc.OpenInput()["frames"] == 3
    assert np.array_equal(_load(enc, 32, 40), np.stack(R.decode(file, 2, 3)[0]))
    assert enc.InputStats()["frames"] == 3 and enc.InputStats()["kind"] == 16
    # the background
    enc.InputFileName, enc.StartFrame, enc.FrameCount = "small.gif", 0, 0
    assert enc.GifBackground() is None
    enc.OpenInput()
    plain = _load(enc, 20, 24)
    assert np.array_equal(plain, np.stack(R.decode(small)[0]))
    enc.SetGifBackground(0x102030)
    assert enc.GifBackground() == 0x102030
    enc.OpenInput()
    tinted = _load(enc, 20, 24)
    assert np.array_equal(tinted, np.stack(R.decode(small, 0, None, 0x102030)[0])) and not np.array_equal(tinted, plain)
    enc.SetGifBackground(None)
    with pytest.raises(TileMotionError):
        enc.SetGifBackground(1 << 24)
    # the lent file against the file
    assert enc.SetFramesGIF(file) == dict(width=40, height=32, fps=25.0, frames=6)
    lent = _load(enc, 32, 40)
    assert np.array_equal(lent, np.stack(R.decode(file)[0]))
    st = enc.InputStats()
    assert st["kind"] == 20 and st["where"] == where and st["frames"] == 6 and st["file_bytes"] == len(file)
    enc.Run(S.esLoad)  # the clip it has
    assert enc.SetFramesGIF(file, fps=12.5)["fps"] == 12.5
    for bad in (b"", b"GIF89a", file[:100], b"x" * 100):
        with pytest.raises(TileMotionError):
            enc.SetFramesGIF(bad)
    enc.close()


def test_scaling_is_refused_with_nothing_loaded(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("clip.gif", "wb").write(_clip_file(3))
    enc = _encoder(InputFileName="clip.gif", Scaling=0.5)
    with pytest.raises(TileMotionError) as e:
        enc.OpenInput()
    assert e.value.code == -6 and "Scaling" in str(e.value)
    assert enc.VideoInfo()["frames"] == 0
    with pytest.raises(TileMotionError):
        enc.InputStats()
    enc.close()


def test_set_gif_decode_and_the_environment(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("TM_GIF_DECODE", raising=False)
    open("clip.gif", "wb").write(_clip_file(3))
    enc = _encoder(InputFileName="clip.gif")
    assert enc.GifDecode() == "auto"
    for setting, env, want in (("device", None, "device"), ("host", None, "host"), ("host", "device", "device"), ("device", "host", "host")):
        enc.SetGifDecode(setting)
        assert enc.GifDecode() == setting
        if env:
            monkeypatch.setenv("TM_GIF_DECODE", env)
        else:
            monkeypatch.delenv("TM_GIF_DECODE", raising=False)
        enc.OpenInput()
        enc.Run(S.esLoad)
        assert enc.InputStats()["where"] == want, (setting, env)
    with pytest.raises(ValueError):
        enc.SetGifDecode("gpu")
    enc.close()


def test_a_damaged_file_fails_the_load_on_both_paths(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("bad.gif", "wb").write(dict(CLIPS)["second_image_truncated"])
    for where in ("host", "device"):
        monkeypatch.setenv("TM_GIF_DECODE", where)
        enc = _encoder(InputFileName="bad.gif")
        assert enc.OpenInput()["frames"] == 3
        with pytest.raises(TileMotionError) as e:
            enc.Run(S.esLoad)
        assert e.value.code == -5 and "image 1" in str(e.value)
        enc.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_two_shards_on_one_device_equal_one_encoder(stages, tmp_path, monkeypatch, where):
    """a device group's shards each decode from image 0 to the last frame they need (no collective is added): two shards on device 0
    against one encoder, down to the saved .gtm.  Two devices are not needed for that; a Load on two different devices is not run."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_GIF_DECODE", where)
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "5")
    open("clip.gif", "wb").write(_clip_file(12))
    got = []
    for devices in (None, [0, 0]):
        enc = TilingEncoder()
        if devices:
            enc.SetDevices(devices)
        enc.LoadDefaultSettings()
        for k, v in {**BASE, "InputFileName": "clip.gif", "OutputFileName": "out.gtm", "MotionPredictRadius": 0}.items():
            setattr(enc, k, v)
        assert enc.OpenInput() == dict(width=64, height=48, fps=25.0, frames=12)
        enc.Run()
        enc.Save()
        got.append(open("out.gtm", "rb").read())
        os.remove("out.gtm")
        enc.close()
    assert got[0] == got[1] and len(got[0]) > 1000
