"""The two chunk rules of the host code around the codecs, each past its first chunk.  The render's (at most 32 frames or 256 MB a chunk:
GenerateY4M, RenderFramesYUV, the renders at a caller's size) on a 40-frame clip, every frame against the call for that frame alone; Load's
file chunks (TM_INPUT_CHUNK_FRAMES) on five files in three chunks, both staging slots reused and the last chunk short, against the same
files in one chunk."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import jpeg_cases, png_cases  # noqa: E402
from tests import yuv_out_ref as ref  # noqa: E402
from tests.test_gpu_png_out import _encoder as _encode_scene  # noqa: E402
from tiler_amd import synth  # noqa: E402
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S  # noqa: E402

NF, SIZE, FILTERS = 40, (16, 16), ("lanczos", "nearest")


# ---- the render's chunks
@pytest.fixture(scope="module")
def clip40(tmp_path_factory):
    """40 frames of 8 x 8 with 2 palettes, the export tests' small clip: frames 32 .. 39 are the second chunk"""
    enc = _encode_scene(NF, 8, 8, str(tmp_path_factory.mktemp("chunks") / "clip.gtm"))
    yield enc
    enc.close()


def _np(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32) if a.dtype == np.int32 else a


def _singles(call):
    """the 40 single-frame calls, every plane stacked over the frames"""
    per_frame = [call(f) for f in range(NF)]
    if not isinstance(per_frame[0], tuple):
        return np.concatenate([_np(p) for p in per_frame])
    return tuple(None if per_frame[0][i] is None else np.concatenate([_np(p[i]) for p in per_frame]) for i in range(3))


def _same_planes(got, want, what):
    for name, g, w in zip("yuv", got, want):
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            g = _np(g)
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
            bad = sorted(set(np.argwhere(g != w)[:, 0].tolist()))
            assert not bad, (what, name, "frames", bad)


@pytest.mark.parametrize("input", [False, True], ids=["output", "input"])
def test_generate_y4m_past_a_chunk(clip40, tmp_path, input):
    enc = clip40
    path = tmp_path / "clip.y4m"
    enc.GenerateY4M(str(path), input)
    data = path.read_bytes()
    head = data.index(b"\n") + 1
    assert data[:head].startswith(b"YUV4MPEG2 W8 H8 ") and data[:head].endswith(b" C444\n")
    body = np.frombuffer(data[head:], np.uint8).reshape(NF, 7 + 3 * 64)
    assert all(bytes(fr[:7]) == b"FRAME \n" for fr in body)
    planes = body[:, 7:].reshape(NF, 3, 8, 8)
    file_planes = tuple(planes[:, i] for i in range(3))
    alone = _singles(lambda f: enc.RenderFramesYUV(f, 1, input=input, layout="444", yuv="tiler", device=False))
    _same_planes(file_planes, alone, "the file against the frames alone")
    rgb = _singles(lambda f: enc.RenderFrames(f, 1, input=input, device=False))
    _same_planes(file_planes, ref.planes(rgb, "444", ref.TILER), "the file against the restatement")


@pytest.mark.parametrize("input", [False, True], ids=["output", "input"])
def test_render_frames_yuv_past_a_chunk(clip40, input):
    enc = clip40
    alone = _singles(lambda f: enc.RenderFramesYUV(f, 1, input=input, device=False))
    for device in (False, True):
        _same_planes(enc.RenderFramesYUV(input=input, device=device), alone, "device" if device else "host")


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("input", [False, True], ids=["output", "input"])
def test_scaled_renders_past_a_chunk(clip40, input, filter):
    enc = clip40
    alone = _singles(lambda f: enc.RenderFrames(f, 1, input=input, device=False, size=SIZE, filter=filter))
    assert alone.shape == (NF, 16, 16)
    for device in (False, True):
        got = _np(enc.RenderFrames(input=input, device=device, size=SIZE, filter=filter))
        bad = sorted(set(np.argwhere(got != alone)[:, 0].tolist()))
        assert got.shape == alone.shape and not bad, (device, "frames", bad)
    alone = _singles(lambda f: enc.RenderFramesYUV(f, 1, input=input, device=False, size=SIZE, filter=filter))
    for device in (False, True):
        _same_planes(enc.RenderFramesYUV(input=input, device=device, size=SIZE, filter=filter), alone, "device" if device else "host")


# ---- Load's file chunks
def _five_files(kind):
    frames = synth.video(5, 16, 16, cut=2) & 0xffffff
    if kind == "png":
        return frames, png_cases.encode_host(np.ascontiguousarray(frames, np.uint32), 1, "adaptive")
    rgb = np.stack([(frames >> 16) & 255, (frames >> 8) & 255, frames & 255], -1).astype(np.uint8)
    return frames, [jpeg_cases.encode_rgb(fr, "444", ri=1) for fr in rgb]  # four MCUs, a restart segment each: lanes for the device place


@pytest.mark.parametrize("lent", [False, True], ids=["sequence", "lent"])
@pytest.mark.parametrize("kind,where", [("png", "device"), ("jpeg", "device"), ("jpeg", "host")])
def test_file_chunks_give_the_one_chunk_clip(tmp_path, monkeypatch, kind, where, lent):
    monkeypatch.chdir(tmp_path)
    frames, files = _five_files(kind)
    ext = "png" if kind == "png" else "jpg"
    for f, data in enumerate(files):
        with open("seq_%04d.%s" % (f, ext), "wb") as fh:
            fh.write(data)
    monkeypatch.setenv("TM_%s_DECODE" % kind.upper(), where)
    clips = {}
    for chunk in (None, "2"):  # one chunk; three chunks: slot 0, slot 1, slot 0 again with one file
        if chunk:
            monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", chunk)
        else:
            monkeypatch.delenv("TM_INPUT_CHUNK_FRAMES", raising=False)
        enc = TilingEncoder()
        enc.LoadDefaultSettings()
        enc.MotionPredictRadius = 0
        if lent:
            (enc.SetFramesPNG if kind == "png" else enc.SetFramesJPEG)(files, 24.0)
        else:
            enc.InputFileName = "seq_%.4d." + ext
            enc.OpenInput()
        enc.Run(S.esLoad)
        st = enc.InputStats()
        assert st["where"] == where and st["frames"] == 5 and st["file_bytes"] == sum(len(f) for f in files), (chunk, st)
        clips[chunk] = enc.RenderFrames(input=True, device=False)
        enc.close()
    assert clips[None].shape == (5, 16, 16) and len({fr.tobytes() for fr in clips[None]}) == 5  # (a frame in another's place would show)
    assert np.array_equal(clips["2"], clips[None])
    if kind == "png":
        assert np.array_equal(clips[None], frames)
