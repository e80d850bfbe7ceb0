"""The JPEG writer on the device (tm_jpeg_out.hip) against its host twin byte for byte -- the stage seam on the
pictures of tests/jpeg_out_cases.py, which tests/test_jpeg_out_host.py holds to the restatement and to libjpeg -- and through the encoder:
GenerateJPEGs and GenerateMJPEG against RenderFrames, the files read back by Load, and GeneratePNGs left as it was.

The pictures of one size are the frames of one call, so they go through the same launches; their rows and frames are padded."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import jpeg_out_cases as C  # noqa: E402
from tests import yuv_ref  # noqa: E402
from tests.jpeg_cases import unpack  # noqa: E402

SAMPLINGS = ("420", "422", "444", "grey")


@functools.lru_cache(maxsize=None)
def _expected(size, quality, sampling, restart_rows):
    """the host twin's files of the pictures of one size, computed once"""
    from tiler_amd import stages
    return stages.jpeg_encode_host(C.stack32(C.by_size()[size]), quality, sampling, restart_rows)


def _on_device(names, row_pad=0, frame_pad=0):
    """the named pictures as a CUDA tensor [F][H][W] with padded rows and frames"""
    store, stride, frame_px, h, w = C.strided(names, row_pad, frame_pad)
    t = torch.from_numpy(store.view(np.int32).reshape(-1)).cuda()
    return torch.as_strided(t, (len(names), h, w), (frame_px, stride, 1))


@pytest.mark.parametrize("restart_rows", [0, 1])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_stage_jpeg_encode_equals_the_host_twin(sampling, restart_rows):
    """every picture, at the default quality and at 100 (the most bits, the most FF bytes), between guard bytes"""
    from tiler_amd import stages
    for size, names in C.by_size().items():
        frames = _on_device(names, 5, 11)
        for q in (90, 100):
            want = _expected(size, q, sampling, restart_rows)
            got = stages.jpeg_encode(frames, q, sampling, restart_rows, guard=64, full=True)
            assert got["rc"] == 0, (size, q)
            assert [len(g) for g in got["files"]] == [len(x) for x in want], (size, q)
            assert got["files"] == want, (size, q)
            total = sum(len(x) for x in want)
            assert (got["buffer"][:64] == 0xA5).all() and (got["buffer"][64 + total:] == 0xA5).all(), (size, q)


def test_a_cap_too_small_and_the_exact_cap():
    from tiler_amd import lib, stages
    size = (33, 49)
    dev = _on_device(C.by_size()[size], 3, 7)
    want = _expected(size, 100, "420", 1)
    need = sum(len(x) for x in want)
    for cap in (0, need - 1):
        got = stages.jpeg_encode(dev, 100, "420", 1, cap=cap, guard=64, full=True)
        assert got["rc"] == -1 and got["offsets"][len(want)] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.jpeg_encode(dev, 100, "420", 1, cap=need, guard=64, full=True)
    assert got["rc"] == 0 and got["files"] == want and (got["buffer"][64 + need:] == 0xA5).all()
    assert stages.jpeg_encode(dev[:0], 90, "420", 1) == []


def test_refusals_come_before_any_device_call():
    from tiler_amd import lib
    from tiler_amd._lib import JpegOptions
    L = lib()
    px = torch.zeros((2, 4, 8), dtype=torch.int32, device="cuda")
    out = np.full(4096, 0xAA, np.uint8)
    offs = (ctypes.c_int64 * 3)(-7, -7, -7)
    pp, op = ctypes.c_void_p(px.data_ptr()), out.ctypes.data_as(ctypes.c_void_p)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, q=90, s=0, r=1, cap=4096, o=offs):
        return L.tm_stage_jpeg_encode(frames, stride, frame_px, nf, w, h, ctypes.byref(JpegOptions(q, s, r)), op, cap, o, None)
    for kw in (dict(frames=None), dict(q=0), dict(q=101), dict(s=4), dict(s=-1), dict(r=-1), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769), dict(stride=7),
               dict(frame_px=31), dict(nf=-1), dict(o=None), dict(cap=-1), dict(w=32768, stride=32768, nf=0, s=2, r=16)):
        assert call(**kw) == -1, kw
        assert (out == 0xAA).all() and list(offs) == [-7, -7, -7], kw
    assert L.tm_stage_jpeg_encode(pp, 8, 32, 2, 8, 4, None, op, 4096, offs, None) == -1
    assert call() == 0 and offs[0] == 0 and offs[2] > offs[1] > 0


def test_past_one_chunk():
    """40 frames of 8 x 8: more than the 32 frames a chunk holds"""
    from tiler_amd import stages
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 1 << 24, (40, 8, 8)).astype(np.uint32)
    dev = torch.from_numpy(frames.view(np.int32)).cuda()
    assert stages.jpeg_encode(dev, 90, "420", 0) == stages.jpeg_encode_host(frames, 90, "420", 0)


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_round_trip_through_the_device_reader(sampling):
    """the device's files through stages.jpeg_decode give the planes the host reader makes of the twin's files"""
    from tiler_amd import stages
    size = (72, 64)
    files = stages.jpeg_encode(_on_device(C.by_size()[size]), 90, sampling, 1)
    dev, dstatus, dl = stages.jpeg_decode(files)
    host, hstatus, hl = stages.jpeg_decode_host(list(_expected(size, 90, sampling, 1)))
    assert dstatus == hstatus == [0] * len(files) and dl == hl
    ncomp = 1 if sampling == "grey" else 3
    for c in range(ncomp):
        assert np.array_equal(dev[c].cpu().numpy(), host[c]), c


# ---- through the encoder
def _scene(nf, w, h):
    """a smooth textured scene that moves one pixel to the left every other frame"""
    y, x = np.mgrid[0:h, 0:w + nf].astype(np.int64)
    r = (128 + 90 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.int64)
    g = (128 + 80 * np.cos(x / 17.0 + y / 11.0)).astype(np.int64)
    b = (x * 2 + y) % 256
    img = (np.clip(r, 0, 255) << 16) | (np.clip(g, 0, 255) << 8) | b
    return np.stack([img[:, f // 2:f // 2 + w] for f in range(nf)]).astype(np.uint32)


def _encoder(nf, w, h, out):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in dict(PaletteCount=2, GlobalTilingTileCount=60, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False, OutputFileName=out).items():
        setattr(enc, k, v)
    enc.SetVideo(w, h, 24.0, nf)
    frames = _scene(nf, w, h)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    enc.Run()
    return enc


def _files(base, nf, ext):
    names = sorted(glob.glob(base + "_*." + ext))
    assert [os.path.basename(n) for n in names] == ["%s_%04d.%s" % (os.path.basename(base), f, ext) for f in range(nf)]
    return [open(n, "rb").read() for n in names]


@pytest.fixture(scope="module", params=[(10, 64, 64), (40, 8, 8)], ids=["64x64x10", "8x8x40"])
def clip(request, tmp_path_factory):
    nf, w, h = request.param
    base = str(tmp_path_factory.mktemp("jpeg") / "clip")
    enc = _encoder(nf, w, h, base + ".gtm")
    yield dict(enc=enc, nf=nf, w=w, h=h, base=base)
    enc.close()


@pytest.mark.parametrize("input", [False, True], ids=["output", "input"])
def test_generate_jpegs_and_mjpeg(clip, input):
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetJpegOptions()
    assert enc.JpegOptions() == {"quality": 90, "sampling": "420", "restart_rows": 1}
    frames = enc.RenderFrames(input=input, device=False)
    for opts in (dict(), dict(quality=75, sampling="444", restart_rows=0), dict(quality=100, sampling="grey", restart_rows=2)):
        enc.SetJpegOptions(**opts)
        enc.GenerateJPEGs(input)
        files = _files(base, nf, "jpg")
        assert not os.path.exists(base + ".txt")
        want = stages.jpeg_encode_host(frames, **opts)
        assert files == want, opts
        assert files == stages.jpeg_encode(enc.RenderFrames(input=input), **opts)
        st = enc.JpegExportStats()
        held = {**dict(quality=90, sampling="420", restart_rows=1), **opts}
        assert st["frames"] == nf and st["file_bytes"] == sum(os.path.getsize(n) for n in glob.glob(base + "_*.jpg"))
        assert {k: st[k] for k in held} == held
        assert st["ms_device"] > 0 and st["ms_write"] > 0 and st["ms_device"] + st["ms_write"] <= st["ms_wall"] * 1.001
        enc.GenerateMJPEG(base + ".mjpeg", input)
        assert open(base + ".mjpeg", "rb").read() == b"".join(want)
        st = enc.JpegExportStats()
        assert st["frames"] == nf and st["file_bytes"] == os.path.getsize(base + ".mjpeg")
    for bad in (dict(quality=0), dict(quality=101), dict(sampling=7), dict(restart_rows=-1)):
        with pytest.raises(TileMotionError) as ei:
            enc.SetJpegOptions(**bad)
        assert ei.value.code == -1
    assert enc.JpegOptions() == {"quality": 100, "sampling": "grey", "restart_rows": 2}
    with pytest.raises(TileMotionError):
        enc.GenerateMJPEG("", input)
    enc.SetJpegOptions()


def test_the_written_sequence_loads_on_the_device_as_on_the_host(clip, monkeypatch):
    """a fresh encoder's OpenInput of the exported files: TM_JPEG_DECODE=device gives what the host path gives, and that is the files' planes"""
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    enc, nf, w, h, base = clip["enc"], clip["nf"], clip["w"], clip["h"], clip["base"]
    enc.SetJpegOptions(quality=90, sampling="420", restart_rows=1)
    enc.GenerateJPEGs(False)
    got = {}
    for where in ("host", "device"):
        monkeypatch.setenv("TM_JPEG_DECODE", where)
        fresh = TilingEncoder()
        fresh.LoadDefaultSettings()
        fresh.InputFileName = base + "_%.4d.jpg"
        fresh.OutputFileName = base + "_again.gtm"
        assert fresh.OpenInput() == dict(width=w, height=h, fps=24.0, frames=nf)
        fresh.Run(S.esLoad)
        st = fresh.InputStats()
        assert st["where"] == where and st["kind"] == 8 and st["frames"] == nf
        got[where] = fresh.RenderFrames(input=True, device=False)
        fresh.close()
    assert np.array_equal(got["device"], got["host"])
    # and that is the files' planes through the input rule (JFIF: full-range BT.601, 4:2:0 sited as JPEG has it)
    from tiler_amd import stages
    files = _files(base, nf, "jpg")
    planes, status, layout = stages.jpeg_decode_host(files)
    assert status == [0] * nf
    per_file = [unpack(planes, layout, i, [(w, h), (w // 2, h // 2), (w // 2, h // 2)]) for i in range(nf)]
    t = [torch.from_numpy(np.ascontiguousarray(np.stack([p[c] for p in per_file]))).cuda() for c in range(3)]
    want = stages.yuv_to_rgb32(t[0], t[1], t[2], 2, w, h, yuv_ref.BT601_FULL).cpu().numpy().view(np.uint32)
    assert np.array_equal(got["host"], want)


def test_generate_pngs_behaves_as_before(clip):
    """SetJpegOptions and a JPEG export leave GeneratePNGs, its options and ExportStats alone"""
    from tiler_amd import stages
    enc, nf, base = clip["enc"], clip["nf"], clip["base"]
    enc.SetPngOptions(level=1, filter="none")
    enc.GeneratePNGs(False)
    before = _files(base, nf, "png")
    stats = enc.ExportStats()
    enc.SetJpegOptions(quality=40, sampling="422", restart_rows=3)
    enc.GenerateJPEGs(False)
    assert enc.PngOptions() == {"level": 1, "filter": "none"}
    after = enc.ExportStats()
    assert {k: after[k] for k in ("frames", "file_bytes", "level", "filter")} == {k: stats[k] for k in ("frames", "file_bytes", "level", "filter")}
    assert after == stats
    enc.GeneratePNGs(False)
    assert _files(base, nf, "png") == before == stages.png_encode(enc.RenderFrames(), 1, "none")
    assert os.path.exists(base + ".txt")
    assert enc.JpegExportStats()["quality"] == 40
    enc.SetPngOptions(level=0)
    enc.SetJpegOptions()
