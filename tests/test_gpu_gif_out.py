"""The GIF writer on the device (tm_gif_out.hip) against its host twin byte for byte -- the stage seams on the cases
of tests/gif_out_cases.py, which tests/test_gif_out_host.py holds to the restatement and to three readers -- and through the encoder:
GenerateGIF against RenderFrames, the file read back by Load on the device, and GeneratePNGs / GenerateMJPEG left as they were."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gif_out_cases as C  # noqa: E402

NAMES = [c["name"] for c in C.clips()]


def _clip(name):
    return next(c for c in C.clips() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """the host twin's file of a clip, computed once"""
    from tiler_amd import stages
    c = _clip(name)
    return stages.gif_encode_host(c["frames"], c["fps"], **c["opt"])


def _on_device(frames, row_pad=5, frame_pad=11):
    """the frames as a CUDA tensor [F][H][W] with padded rows and frames"""
    nf, h, w = frames.shape
    stride, frame_px = w + row_pad, (w + row_pad) * h + frame_pad
    store = np.full(nf * frame_px + 1, 0x00C0FFEE, np.uint32)
    for f in range(nf):
        store[f * frame_px:f * frame_px + stride * h].reshape(h, stride)[:, :w] = frames[f]
    t = torch.from_numpy(store.view(np.int32)).cuda()
    return torch.as_strided(t, (nf, h, w), (frame_px, stride, 1))


@pytest.mark.parametrize("name", NAMES)
def test_stage_gif_encode_equals_the_host_twin(name):
    """padded rows and frames, guard bytes on both sides of the output, at every chunk_frames of the case"""
    from tiler_amd import stages
    c = _clip(name)
    want = _expected(name)
    dev = _on_device(c["frames"])
    for chunk in c["chunks"]:
        got = stages.gif_encode(dev, c["fps"], chunk_frames=chunk, guard=64, full=True, **c["opt"])
        assert got["rc"] == 0 and got["bytes"] == len(want), chunk
        assert got["file"] == want, chunk
        assert (got["buffer"][:64] == 0xA5).all() and (got["buffer"][64 + len(want):] == 0xA5).all(), chunk
        host = stages.gif_encode_host(c["frames"], c["fps"], full=True, **c["opt"])["stats"]
        assert {k: got["stats"][k] for k in ("frames", "frames_exact", "frames_quantised", "segments", "file_bytes")} == {
            k: host[k] for k in ("frames", "frames_exact", "frames_quantised", "segments", "file_bytes")}


def test_the_lzw_seam_equals_its_twin():
    from tiler_amd import stages
    for name, idx, mn, seg, _ in C.streams():
        assert stages.gif_lzw_pack(torch.from_numpy(idx).cuda(), mn, seg) == stages.gif_lzw_pack_host(idx, mn, seg), name


def test_the_table_seam_equals_its_twin():
    from tiler_amd import stages
    for c in C.clips():
        opt = {k: v for k, v in c["opt"].items() if k in ("colours", "max_colours")}
        ta, ea, ia = stages.gif_palettise(_on_device(c["frames"])[0], **opt)
        tb, eb, ib = stages.gif_palettise_host(c["frames"][0], **opt)
        assert np.array_equal(ta, tb) and ea == eb and np.array_equal(ia, ib), c["name"]


def test_a_cap_too_small_and_the_exact_cap():
    from tiler_amd import lib, stages
    c = _clip("clip_diff")
    dev = _on_device(c["frames"], 3, 7)
    want = _expected("clip_diff")
    need = len(want)
    for cap in (0, need - 1):
        got = stages.gif_encode(dev, c["fps"], cap=cap, guard=64, full=True)
        assert got["rc"] == -1 and got["bytes"] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.gif_encode(dev, c["fps"], cap=need, guard=64, full=True)
    assert got["rc"] == 0 and got["file"] == want and (got["buffer"][64 + need:] == 0xA5).all()


def test_refusals_come_before_any_device_call():
    from tiler_amd import lib, stages
    from tiler_amd._lib import GifOptions
    L = lib()
    px = torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda")
    out = np.full(4096, 0xAA, np.uint8)
    need = ctypes.c_int64(-7)
    pp, op = ctypes.c_void_p(px.data_ptr()), ctypes.c_void_p(out.ctypes.data)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, fps=25.0, opt=(0, 256, 1, 16384, 0, 0), chunk=0, cap=4096, n=ctypes.byref(need)):
        return L.tm_stage_gif_encode(frames, stride, frame_px, nf, w, h, fps, ctypes.byref(GifOptions(*opt)), chunk, op, cap, n, None, None)
    for kw, code in ((dict(frames=None), -1), (dict(w=0), -1), (dict(h=0), -1), (dict(nf=0), -1), (dict(stride=7), -1), (dict(frame_px=31), -1), (dict(n=None), -1),
                     (dict(cap=-1), -1), (dict(fps=0.0), -1), (dict(fps=0.001), -1), (dict(opt=(3, 256, 1, 0, 0, 0)), -1), (dict(opt=(0, 1, 1, 0, 0, 0)), -1),
                     (dict(opt=(0, 256, 1, 255, 0, 0)), -1), (dict(opt=(0, 256, 1, 0, 65536, 0)), -1), (dict(opt=(0, 256, 1, 0, 0, 1)), -1),
                     (dict(w=65536, stride=65536, h=1, nf=1), -6), (dict(w=1, stride=1, h=65536, nf=1), -6)):
        assert call(**kw) == code, kw
        assert (out == 0xAA).all() and need.value == -7, kw
    assert L.tm_stage_gif_encode(pp, 8, 32, 2, 8, 4, 25.0, None, 0, op, 4096, ctypes.byref(need), None, None) == -1
    assert call() == 0 and need.value > 0
    for name, frames, fps, opt, code in C.refused():
        got = stages.gif_encode(_on_device(frames), fps, full=True, **opt)
        assert got["rc"] == code and got["file"] is None and (got["buffer"] == 0xA5).all(), name
    stages.gif_encode(_on_device(C.distinct(257).reshape(1, 1, 257)), 25.0, full=True, colours="exact")
    assert "frame 0 holds 257 colours" in lib().tm_last_error().decode()


def test_past_one_chunk():
    """40 frames of 8 x 8: more than the 32 frames a chunk of the writer's own holds"""
    from tiler_amd import stages
    rng = np.random.default_rng(12)
    frames = C.PAL256[rng.integers(0, 9, (40, 8, 8))]
    assert stages.gif_encode(torch.from_numpy(frames.view(np.int32)).cuda(), 24.0) == stages.gif_encode_host(frames, 24.0)


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


@pytest.fixture(scope="module", params=[(10, 64, 64), (40, 8, 8)], ids=["64x64x10", "8x8x40"])
def clip(request, tmp_path_factory):
    nf, w, h = request.param
    base = str(tmp_path_factory.mktemp("gif") / "clip")
    enc = _encoder(nf, w, h, base + ".gtm", 2)
    yield dict(enc=enc, nf=nf, w=w, h=h, base=base)
    enc.close()


@pytest.mark.parametrize("diff", [True, False], ids=["diff", "whole"])
def test_generate_gif_decodes_to_the_rendered_frames(clip, diff):
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetGifOptions()
    assert enc.GifOptions() == dict(colours="auto", max_colours=256, diff=True, segment_pixels=4096, loop=0, delay_cs=0)
    frames = enc.RenderFrames(device=False)
    assert max(len(np.unique(f)) for f in frames) <= 256  # PaletteCount x PaletteSize = 32
    enc.SetGifOptions(diff=diff, segment_pixels=1024)
    enc.GenerateGIF(base + ".gif")
    file = open(base + ".gif", "rb").read()
    assert file == stages.gif_encode_host(frames, 24.0, diff=diff, segment_pixels=1024)
    shown, status = stages.gif_decode_host(file)
    assert status == [0] * nf and np.array_equal(shown, frames & 0xFFFFFF)
    st = enc.GifExportStats()
    assert st["frames"] == st["frames_exact"] == nf and st["frames_quantised"] == 0 and st["file_bytes"] == len(file) and st["segments"] >= nf
    assert st["ms_device"] > 0 and st["ms_device"] + st["ms_write"] <= st["ms_wall"] * 1.001
    enc.GenerateGIF(base + "_input.gif", input=True)
    assert open(base + "_input.gif", "rb").read() == stages.gif_encode_host(enc.RenderFrames(input=True, device=False), 24.0, diff=diff, segment_pixels=1024)
    for bad in (dict(colours=3), dict(max_colours=1), dict(segment_pixels=100), dict(loop=-2), dict(delay_cs=1)):
        with pytest.raises(TileMotionError) as ei:
            enc.SetGifOptions(**bad)
        assert ei.value.code == -1
    assert enc.GifOptions()["segment_pixels"] == 1024
    with pytest.raises(TileMotionError):
        enc.GenerateGIF("")
    enc.SetGifOptions()


def test_the_written_file_loads_on_the_device(clip):
    """a fresh encoder's OpenInput of the exported file with SetGifDecode("device"): Load gives the frames that were rendered"""
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    enc, nf, w, h, base = clip["enc"], clip["nf"], clip["w"], clip["h"], clip["base"]
    enc.SetGifOptions()
    enc.GenerateGIF(base + "_load.gif")
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.InputFileName = base + "_load.gif"
    fresh.OutputFileName = base + "_again.gtm"
    fresh.SetGifDecode("device")
    got = fresh.OpenInput()
    assert (got["width"], got["height"], got["frames"]) == (w, h, nf) and got["fps"] == 25.0  # 24 frames a second is a delay of 4
    fresh.Run(S.esLoad)
    assert fresh.InputStats()["where"] == "device"
    loaded = fresh.RenderFrames(input=True, device=False)
    fresh.close()
    assert np.array_equal(loaded & 0xFFFFFF, enc.RenderFrames(device=False) & 0xFFFFFF)


def test_many_palettes_take_the_quantised_path(tmp_path):
    """PaletteCount 24 x PaletteSize 16 passes 256 colours a frame: AUTO quantises, and the file is the twin's"""
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    base = str(tmp_path / "many")
    enc = _encoder(4, 64, 64, base + ".gtm", 24)
    try:
        frames = enc.RenderFrames(device=False)
        assert len(np.unique(frames[0])) > 256
        enc.GenerateGIF(base + ".gif")
        file = open(base + ".gif", "rb").read()
        assert file == stages.gif_encode_host(frames, 24.0)
        st = enc.GifExportStats()
        assert st["frames_quantised"] >= 1 and st["frames_exact"] + st["frames_quantised"] == 4
        enc.SetGifOptions(colours="exact")
        with pytest.raises(TileMotionError) as ei:
            enc.GenerateGIF(base + "_exact.gif")
        assert ei.value.code == -6 and "frame 0 holds" in str(ei.value) and not os.path.exists(base + "_exact.gif")
    finally:
        enc.close()


def _files(base, nf, ext):
    names = sorted(glob.glob(base + "_[0-9][0-9][0-9][0-9]." + ext))
    assert len(names) == nf
    return [open(n, "rb").read() for n in names]


def test_generate_pngs_and_mjpeg_behave_as_before(clip):
    """SetGifOptions and a GIF export leave GeneratePNGs, GenerateMJPEG, their options and their stats alone"""
    from tiler_amd import stages
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetPngOptions(level=1, filter="none")
    enc.GeneratePNGs(False)
    before = _files(base, nf, "png")
    png_stats = enc.ExportStats()
    enc.SetJpegOptions()
    enc.GenerateMJPEG(base + ".mjpeg")
    mjpeg = open(base + ".mjpeg", "rb").read()
    jpeg_stats = enc.JpegExportStats()
    enc.SetGifOptions(colours="quantise", max_colours=16, diff=False, segment_pixels=0, loop=2, delay_cs=9)
    enc.GenerateGIF(base + "_other.gif")
    assert enc.PngOptions() == {"level": 1, "filter": "none"} and enc.ExportStats() == png_stats and enc.JpegExportStats() == jpeg_stats
    enc.GeneratePNGs(False)
    assert _files(base, nf, "png") == before == stages.png_encode(enc.RenderFrames(), 1, "none")
    enc.GenerateMJPEG(base + ".mjpeg")
    assert open(base + ".mjpeg", "rb").read() == mjpeg == b"".join(stages.jpeg_encode(enc.RenderFrames()))
    enc.SetPngOptions(level=0)
    enc.SetGifOptions()
