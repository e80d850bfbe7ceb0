"""The WebP writer on the device (tm_webp_out.hip) against its host twin byte for byte on the cases of
tests/webp_out_cases.py, which tests/test_webp_out_host.py holds to the restatement and to two readers -- and through the encoder:
GenerateWebP read by Pillow against RenderFrames, at colour counts a GIF keeps exact and at ones it cannot."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import webp_out_cases as C  # noqa: E402

NAMES = [c["name"] for c in C.clips() + C.device_clips()]
KEYS = ("frames", "frames_indexed", "segments", "tokens", "matches", "file_bytes")


def _clip(name):
    return next(c for c in C.clips() + C.device_clips() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """the host twin's file and stats of a clip, computed once"""
    from tiler_amd import stages
    c = _clip(name)
    got = stages.webp_encode_host(c["frames"], c["fps"], full=True, **c["opt"])
    assert got["rc"] == 0
    return got["file"], got["stats"]


def _on_device(frames, row_pad=5, frame_pad=11):
    """the frames as a CUDA tensor [F][H][W] with padded rows and frames"""
    nf, h, w = frames.shape
    stride, frame_px = w + row_pad, (w + row_pad) * h + frame_pad
    store = np.full(nf * frame_px + 1, 0x00C0FFEE, np.uint32)
    for f in range(nf):
        store[f * frame_px:f * frame_px + stride * h].reshape(h, stride)[:, :w] = frames[f]
    t = torch.from_numpy(store.view(np.int32)).cuda()
    return torch.as_strided(t, (nf, h, w), (frame_px, stride, 1))


def _pillow_frames(file):
    from PIL import Image
    im = Image.open(io.BytesIO(file))
    out = []
    for f in range(getattr(im, "n_frames", 1)):
        im.seek(f)
        a = np.asarray(im.convert("RGBA")).astype(np.uint32)
        assert (a[..., 3] == 255).all()
        out.append(a[..., 0] << 16 | a[..., 1] << 8 | a[..., 2])
    return np.stack(out), im.info


@pytest.mark.parametrize("name", NAMES)
def test_stage_webp_encode_equals_the_host_twin(name):
    """padded rows and frames, guard bytes on both sides of the output, at every chunk_frames of the case"""
    from tiler_amd import stages
    c = _clip(name)
    want, host = _expected(name)
    dev = _on_device(c["frames"])
    for chunk in c["chunks"]:
        got = stages.webp_encode(dev, c["fps"], chunk_frames=chunk, guard=64, full=True, **c["opt"])
        assert got["rc"] == 0 and got["bytes"] == len(want), chunk
        assert got["file"] == want, chunk
        assert (got["buffer"][:64] == 0xA5).all() and (got["buffer"][64 + len(want):] == 0xA5).all(), chunk
        assert {k: got["stats"][k] for k in KEYS} == {k: host[k] for k in KEYS}, chunk


def test_a_cap_too_small_and_the_exact_cap():
    from tiler_amd import lib, stages
    c = _clip("clip_diff")
    dev = _on_device(c["frames"], 3, 7)
    want = _expected("clip_diff")[0]
    need = len(want)
    for cap in (0, need - 1):
        got = stages.webp_encode(dev, c["fps"], cap=cap, guard=64, full=True)
        assert got["rc"] == -1 and got["bytes"] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.webp_encode(dev, c["fps"], cap=need, guard=64, full=True)
    assert got["rc"] == 0 and got["file"] == want and (got["buffer"][64 + need:] == 0xA5).all()


def test_refusals_come_before_any_device_call():
    from tiler_amd import lib, stages
    from tiler_amd._lib import WebpOptions
    L = lib()
    px = torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda")
    out = np.full(4096, 0xAA, np.uint8)
    need = ctypes.c_int64(-7)
    pp, op = ctypes.c_void_p(px.data_ptr()), ctypes.c_void_p(out.ctypes.data)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, fps=25.0, opt=(1, 0, 1, 16384, 0, 0), chunk=0, cap=4096, n=ctypes.byref(need)):
        return L.tm_stage_webp_encode(frames, stride, frame_px, nf, w, h, fps, ctypes.byref(WebpOptions(*opt)), chunk, op, cap, n, None, None)
    for kw, code in ((dict(frames=None), -1), (dict(w=0), -1), (dict(h=0), -1), (dict(nf=0), -1), (dict(stride=7), -1), (dict(frame_px=31), -1), (dict(n=None), -1),
                     (dict(cap=-1), -1), (dict(fps=0.0), -1), (dict(fps=0.00001), -1), (dict(opt=(2, 0, 1, 0, 0, 0)), -1), (dict(opt=(1, 2, 1, 0, 0, 0)), -1),
                     (dict(opt=(1, 0, 2, 0, 0, 0)), -1), (dict(opt=(1, 0, 1, -1, 0, 0)), -1), (dict(opt=(1, 0, 1, 0, 65536, 0)), -1), (dict(opt=(1, 0, 1, 0, 0, 1 << 24)), -1),
                     (dict(w=16385, stride=16385, h=1, nf=1), -6), (dict(w=1, stride=1, h=16385, nf=1), -6)):
        assert call(**kw) == code, kw
        assert (out == 0xAA).all() and need.value == -7, kw
    assert L.tm_stage_webp_encode(pp, 8, 32, 2, 8, 4, 25.0, None, 0, op, 4096, ctypes.byref(need), None, None) == -1
    assert call() == 0 and need.value > 0
    for name, frames, fps, opt, code in C.refused():
        got = stages.webp_encode(_on_device(frames), fps, full=True, **opt)
        assert got["rc"] == code and got["file"] is None and (got["buffer"] == 0xA5).all(), name


def test_past_one_chunk():
    """40 frames of 8 x 8: more than the 32 frames a chunk holds"""
    from tiler_amd import stages
    rng = np.random.default_rng(12)
    frames = C.PAL256[rng.integers(0, 9, (40, 8, 8))]
    assert stages.webp_encode(torch.from_numpy(frames.view(np.int32)).cuda(), 24.0) == stages.webp_encode_host(frames, 24.0)
    assert stages.webp_encode(torch.from_numpy(frames.view(np.int32)).cuda(), 24.0, chunk_frames=64) == stages.webp_encode_host(frames, 24.0)


# ---- through the encoder
def _scene(nf, w, h):
    """a smooth textured scene that moves one pixel to the left every other frame"""
    y, x = np.mgrid[0:h, 0:w + nf].astype(np.int64)
    r = (128 + 90 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.int64)
    g = (128 + 80 * np.cos(x / 17.0 + y / 11.0)).astype(np.int64)
    b = (x * 2 + y) % 256
    img = (np.clip(r, 0, 255) << 16) | (np.clip(g, 0, 255) << 8) | b
    return np.stack([img[:, f // 2:f // 2 + w] for f in range(nf)]).astype(np.uint32)


def _encoder(nf, w, h, out, palette_count):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in dict(PaletteCount=palette_count, GlobalTilingTileCount=60, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False, OutputFileName=out).items():
        setattr(enc, k, v)
    enc.SetVideo(w, h, 24.0, nf)
    frames = _scene(nf, w, h)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    enc.Run()
    return enc


@pytest.fixture(scope="module", params=[(10, 64, 64, 2), (40, 8, 8, 2), (4, 64, 64, 24)], ids=["64x64x10", "8x8x40", "64x64x4_24_palettes"])
def clip(request, tmp_path_factory):
    nf, w, h, palettes = request.param
    base = str(tmp_path_factory.mktemp("webp") / "clip")
    enc = _encoder(nf, w, h, base + ".gtm", palettes)
    yield dict(enc=enc, nf=nf, w=w, h=h, base=base, palettes=palettes)
    enc.close()


@pytest.mark.parametrize("diff", [True, False], ids=["diff", "whole"])
def test_generate_webp_reads_back_as_the_rendered_frames(clip, diff):
    """with 2 palettes of 16 a frame holds at most 32 colours; with 24 it passes 256, which a GIF cannot keep exact and this file does"""
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetWebpOptions()
    assert enc.WebpOptions() == dict(diff=True, palette="auto", lz77=True, segment_pixels=4096, loop=0, duration_ms=0)
    frames = enc.RenderFrames(device=False)
    most = max(len(np.unique(f)) for f in frames)
    assert most > 256 if clip["palettes"] == 24 else most <= 256
    enc.SetWebpOptions(diff=diff, segment_pixels=1024)
    enc.GenerateWebP(base + ".webp")
    file = open(base + ".webp", "rb").read()
    assert file == stages.webp_encode_host(frames, 24.0, diff=diff, segment_pixels=1024)
    shown, info = _pillow_frames(file)
    assert np.array_equal(shown, frames & 0xFFFFFF) and info.get("loop", 0) == 0
    st = enc.WebpExportStats()
    assert st["frames"] == nf and st["file_bytes"] == len(file) and st["segments"] >= nf and st["tokens"] >= st["segments"] and 0 <= st["matches"] <= st["tokens"]
    assert (st["frames_indexed"] < nf) if clip["palettes"] == 24 and not diff else (st["frames_indexed"] <= nf)
    assert st["ms_device"] > 0 and st["ms_device"] + st["ms_write"] <= st["ms_wall"] * 1.001
    enc.GenerateWebP(base + "_input.webp", input=True)
    source = enc.RenderFrames(input=True, device=False)
    file = open(base + "_input.webp", "rb").read()
    assert file == stages.webp_encode_host(source, 24.0, diff=diff, segment_pixels=1024)
    assert np.array_equal(_pillow_frames(file)[0], source & 0xFFFFFF)
    for bad in (dict(diff=2), dict(palette=2), dict(lz77=2), dict(segment_pixels=-1), dict(loop=-1), dict(loop=65536), dict(duration_ms=1 << 24)):
        with pytest.raises(TileMotionError) as ei:
            enc.SetWebpOptions(**bad)
        assert ei.value.code == -1
    assert enc.WebpOptions()["segment_pixels"] == 1024
    with pytest.raises(TileMotionError):
        enc.GenerateWebP("")
    enc.SetWebpOptions()


def test_generate_webp_refuses_what_generate_pngs_refuses(tmp_path):
    """an encoder that has reconstructed nothing: the same refusal, and no file"""
    from tiler_amd._lib import TileMotionError
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    try:
        enc.LoadDefaultSettings()
        enc.OutputFileName = str(tmp_path / "none.gtm")
        enc.SetVideo(16, 16, 24.0, 2)
        with pytest.raises(TileMotionError) as png:
            enc.GeneratePNGs(False)
        with pytest.raises(TileMotionError) as webp:
            enc.GenerateWebP(str(tmp_path / "none.webp"))
        assert webp.value.code == png.value.code and not os.path.exists(str(tmp_path / "none.webp"))
        with pytest.raises(TileMotionError):
            enc.WebpExportStats()
    finally:
        enc.close()
