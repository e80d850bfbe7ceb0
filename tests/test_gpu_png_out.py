"""The PNG writer on the device (tm_png_out.hip) against its host twin byte for byte -- the stage seams on the cases of
tests/png_cases.py -- and through the encoder: GeneratePNGs at level 1 against RenderFrames, the stored files of level 0, the player's
frames, and a device group."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import png_cases  # noqa: E402
from tests.png_cases import CONTENTS, FILTERS, SHAPES, STREAMS  # noqa: E402


@functools.lru_cache(maxsize=None)
def _expected(content, w, h, frames, level, flt):
    """the host twin's files, computed once"""
    return png_cases.encode_host(png_cases.picture(content, w, h, frames), level, flt)


def _on_device(frames, row_pad=0, frame_pad=0):
    nf, h, w = frames.shape
    buf, stride, frame_px = png_cases.strided(frames, row_pad, frame_pad)
    t = torch.from_numpy(buf.view(np.int32)).cuda()
    return torch.as_strided(t, (nf, h, w), (frame_px, stride, 1))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_stage_png_encode_equals_the_host_twin(shape, content):
    """every strategy, one packed frame and three frames with padded rows and a padded frame stride"""
    from tiler_amd import stages
    w, h = shape
    for flt in FILTERS:
        for nf, row_pad, frame_pad in ((1, 0, 0), (3, 5, 11)):
            got = stages.png_encode(_on_device(png_cases.picture(content, w, h, nf), row_pad, frame_pad), 1, flt)
            want = _expected(content, w, h, nf, 1, flt)
            assert [len(g) for g in got] == [len(x) for x in want], (flt, nf)
            assert got == want, (flt, nf)
    assert stages.png_encode(_on_device(png_cases.picture(content, w, h, 3), 5, 11), 0, "none") == _expected(content, w, h, 3, 0, "none")


def test_stage_png_encode_past_one_chunk():
    """40 frames of 8 x 8: more than the 32 frames a chunk holds"""
    from tiler_amd import stages
    frames = png_cases.picture("palettised", 8, 8, 40)
    assert stages.png_encode(_on_device(frames), 1, "smaller") == _expected("palettised", 8, 8, 40, 1, "smaller")
    assert stages.png_encode(_on_device(frames)[:0], 1, "none") == []


@pytest.mark.parametrize("name", list(STREAMS))
def test_stage_zlib_compress_equals_the_host_twin(name):
    from tiler_amd import stages
    assert stages.zlib_compress(STREAMS[name]) == png_cases.zlib_host(STREAMS[name])


def test_refusals():
    from tiler_amd import lib
    from tiler_amd._lib import PngOptions
    L = lib()
    px = torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda")
    out = np.full(4096, 0xAA, np.uint8)
    offs = (ctypes.c_int64 * 3)(-7, -7, -7)
    pp, op = ctypes.c_void_p(px.data_ptr()), out.ctypes.data_as(ctypes.c_void_p)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, level=1, flt=1, cap=4096, o=offs):
        return L.tm_stage_png_encode(frames, stride, frame_px, nf, w, h, ctypes.byref(PngOptions(level, flt)), op, cap, o, None)
    for kw in (dict(frames=None), dict(level=2), dict(level=-1), dict(flt=4), dict(flt=-1), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769), dict(stride=7),
               dict(frame_px=31), dict(nf=-1), dict(o=None), dict(w=32768, h=32768, stride=32768)):
        assert call(**kw) == -1, kw
        assert (out == 0xAA).all() and list(offs) == [-7, -7, -7], kw
    assert L.tm_stage_png_encode(pp, 8, 32, 2, 8, 4, None, op, 4096, offs, None) == -1
    want = png_cases.encode_host(np.zeros((2, 4, 8), np.uint32), 1, "none")
    assert call(cap=100) == -1 and offs[2] == sum(len(p) for p in want) and (out == 0xAA).all()
    assert call() == 0 and png_cases.split(out, list(offs)) == want
    src = torch.zeros(100, dtype=torch.uint8, device="cuda")
    n = ctypes.c_int64(-5)
    sp = ctypes.c_void_p(src.data_ptr())
    out[:] = 0xAA
    assert L.tm_stage_zlib_compress(None, 100, op, 200, ctypes.byref(n), None) == -1 and n.value == -5
    assert L.tm_stage_zlib_compress(sp, 1 << 31, op, 200, ctypes.byref(n), None) == -1 and n.value == -5
    assert L.tm_stage_zlib_compress(sp, 100, op, 200, None, None) == -1
    assert L.tm_stage_zlib_compress(sp, 100, op, 3, ctypes.byref(n), None) == -1 and n.value == len(png_cases.zlib_host(bytes(100)))
    assert (out == 0xAA).all()


# ---- through the encoder
def _scene(nf, w, h):
    """a smooth textured scene that moves one pixel to the left every other frame"""
    y, x = np.mgrid[0:h, 0:w + nf].astype(np.int64)
    r = (128 + 90 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.int64)
    g = (128 + 80 * np.cos(x / 17.0 + y / 11.0)).astype(np.int64)
    b = (x * 2 + y) % 256
    img = (np.clip(r, 0, 255) << 16) | (np.clip(g, 0, 255) << 8) | b
    return np.stack([img[:, f // 2:f // 2 + w] for f in range(nf)]).astype(np.uint32)


def _encoder(nf, w, h, out, devices=None):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    if devices is not None:
        enc.SetDevices(devices)
    enc.LoadDefaultSettings()
    for k, v in dict(PaletteCount=2, GlobalTilingTileCount=60, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False, OutputFileName=out).items():
        setattr(enc, k, v)
    enc.SetVideo(w, h, 24.0, nf)
    frames = _scene(nf, w, h)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    enc.Run()
    return enc


def _files(base, nf):
    names = sorted(glob.glob(base + "_*.png"))
    assert [os.path.basename(n) for n in names] == ["%s_%04d.png" % (os.path.basename(base), f) for f in range(nf)]
    return [open(n, "rb").read() for n in names]


@pytest.fixture(scope="module", params=[(10, 64, 64), (40, 8, 8)], ids=["64x64x10", "8x8x40"])
def clip(request, tmp_path_factory):
    nf, w, h = request.param
    base = str(tmp_path_factory.mktemp("png") / "clip")
    enc = _encoder(nf, w, h, base + ".gtm")
    yield dict(enc=enc, nf=nf, w=w, h=h, base=base)
    enc.close()


@pytest.mark.parametrize("input", [False, True], ids=["output", "input"])
def test_export_at_level_1(clip, input):
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    assert enc.PngOptions() == {"level": 0, "filter": "auto"}
    frames = enc.RenderFrames(input=input, device=False) & 0xFFFFFF
    enc.GeneratePNGs(input)  # before the option is touched
    before = _files(base, nf)
    assert before == [png_cases.stored_png(frames[f]) for f in range(nf)]
    assert enc.ExportStats()["level"] == 0 and enc.ExportStats()["file_bytes"] == sum(len(b) for b in before)
    enc.SetPngOptions(level=1)
    enc.GeneratePNGs(input)
    coded = _files(base, nf)
    for f in range(nf):
        assert np.array_equal(png_cases.pillow_pixels(coded[f]), frames[f]), f
    flt = "adaptive" if input else "none"  # what AUTO means for the page
    assert coded == stages.png_encode(enc.RenderFrames(input=input), 1, flt)
    sizes = [(len(c), len(b)) for c, b in zip(coded, before)]
    print("level 1 / level 0 bytes per frame:", sizes)
    assert all(c < b for c, b in sizes), sizes  # every file, the 200-byte streams of the 8 x 8 frames too
    st = enc.ExportStats()
    assert st["frames"] == nf and st["file_bytes"] == sum(len(c) for c in coded) and st["level"] == 1 and st["filter"] == flt
    assert st["ms_device"] > 0 and st["ms_write"] > 0 and st["ms_device"] + st["ms_write"] <= st["ms_wall"] * 1.001
    enc.SetPngOptions(level=1, filter="smaller")
    enc.GeneratePNGs(input)
    assert all(len(s) <= len(c) for s, c in zip(_files(base, nf), coded))
    for bad in (dict(level=2), dict(level=0, filter=7)):
        with pytest.raises(TileMotionError) as ei:
            enc.SetPngOptions(**bad)
        assert ei.value.code == -1
    assert enc.PngOptions() == {"level": 1, "filter": "smaller"}
    enc.SetPngOptions(level=0)
    enc.GeneratePNGs(input)
    assert _files(base, nf) == before
    assert enc.PngOptions() == {"level": 0, "filter": "auto"}


def test_player_frames_give_the_encoder_files(clip):
    """the frames the player decodes from the saved stream, coded with stages.png_encode, are the files the encoder writes"""
    from tiler_amd import stages
    from tiler_amd.player import GtmPlayer
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetPngOptions(level=1)
    enc.GeneratePNGs(False)
    enc.SetPngOptions(level=0)
    with GtmPlayer(base + ".gtm") as p:
        played = p.Read(device=True)
    assert played.shape[0] == nf
    assert stages.png_encode(played, 1, "none") == _files(base, nf)


def test_group_writes_shard_0s_files(tmp_path):
    from tiler_amd import stages
    base = str(tmp_path / "grp")
    grp = _encoder(10, 64, 64, base + ".gtm", devices=[0, 0])
    grp.SetPngOptions(level=1, filter="none")
    grp.GeneratePNGs(False)
    files = _files(base, 10)
    frames = grp.RenderFrames(device=False) & 0xFFFFFF
    for f in range(10):
        assert np.array_equal(png_cases.pillow_pixels(files[f]), frames[f]), f
    assert files == stages.png_encode(grp.RenderFrames(), 1, "none")
    assert grp.ExportStats()["frames"] == 10
    grp.close()
