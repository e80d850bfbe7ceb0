"""Load reads its input (tm_open_input): Y4M files and PNG sequences, converted and scaled on the device.  The stage seam against the numpy
restatements of the resampling and colour rules, bit for bit; a clip read from a file against the same frames pushed; the exports read
back; manual key frames; a device group; refusals."""
import os

import numpy as np
import pytest

from tests import resample_ref, yuv_ref
from tests.resample_ref import CHROMA_ID, chroma_shape
from tiler_amd import synth
from tiler_amd._lib import TileMotionError
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S, TInputYUV

pytestmark = pytest.mark.gpu

E_INVAL, E_IO, E_UNSUPPORTED = -1, -5, -6
LAYOUTS = ["444", "422", "420jpeg", "420mpeg2", "mono"]
MODES = [yuv_ref.AUTO, yuv_ref.BT601_LIMITED, yuv_ref.BT601_FULL, yuv_ref.TILER]
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=150)


def _planes(rng, nf, w, h, layout):
    y = rng.integers(0, 256, (nf, h, w), dtype=np.uint8)
    if layout == "mono":
        return y, None, None
    ch, cw = chroma_shape(layout, w, h)
    return y, rng.integers(0, 256, (nf, ch, cw), dtype=np.uint8), rng.integers(0, 256, (nf, ch, cw), dtype=np.uint8)


def _stage(y, u, v, layout, dw, dh, mode):
    import torch
    from tiler_amd import stages
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (y, u, v)]
    out = stages.yuv_to_rgb32(dev[0], dev[1], dev[2], CHROMA_ID[layout], dw, dh, mode)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _dst(w, h, sc):
    return max(1, int(np.rint(w * sc))), max(1, int(np.rint(h * sc)))


# ---- 6. the stage seam against the numpy rule
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("w,h", [(100, 52), (64, 48), (101, 53)])
def test_stage_matches_the_numpy_rule_bit_for_bit(layout, w, h):
    rng = np.random.default_rng(w * 1000 + h + len(layout))
    y, u, v = _planes(rng, 2, w, h, layout)  # noise: the hard case for the integer rule
    for sc in (1, 0.5, 0.75, 1.5, 1 / 3):
        dw, dh = _dst(w, h, sc)
        Y, U, V = resample_ref.resample_yuv(y, u, v, layout, dw, dh)
        if sc == 1:
            assert np.array_equal(Y, y)  # equal size: the passes return the input bytes
            if layout == "444":
                assert np.array_equal(U, u) and np.array_equal(V, v)
        for mode in MODES:
            got = _stage(y, u, v, layout, dw, dh, mode)
            want = yuv_ref.to_rgb32(Y, U, V, mode)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (layout, sc, mode, len(bad), bad[:3].tolist(), [hex(got[tuple(b)]) for b in bad[:3]], [hex(want[tuple(b)]) for b in bad[:3]])


@pytest.mark.parametrize("sc", [1, 0.5])
def test_stage_720p(sc):
    rng = np.random.default_rng(720)
    y, u, v = _planes(rng, 2, 1280, 720, "420jpeg")
    dw, dh = _dst(1280, 720, sc)
    want = yuv_ref.to_rgb32(*resample_ref.resample_yuv(y, u, v, "420jpeg", dw, dh), yuv_ref.BT601_LIMITED)
    assert np.array_equal(_stage(y, u, v, "420jpeg", dw, dh, yuv_ref.BT601_LIMITED), want)


def test_stage_takes_strided_planes():
    """planes that sit in a larger buffer (rows and frames with padding), as a caller's decoder leaves them"""
    import torch
    from tiler_amd import stages
    rng = np.random.default_rng(3)
    big = [rng.integers(0, 256, (3, 60, 128), dtype=np.uint8) for _ in range(3)]
    y, u, v = big[0][:, :52, :100], big[1][:, :26, :50], big[2][:, :26, :50]
    dev = [torch.from_numpy(b).cuda() for b in big]
    out = stages.yuv_to_rgb32(dev[0][:, :52, :100], dev[1][:, :26, :50], dev[2][:, :26, :50], CHROMA_ID["420jpeg"], 75, 39, yuv_ref.BT601_FULL)
    want = yuv_ref.to_rgb32(*resample_ref.resample_yuv(y, u, v, "420jpeg", 75, 39), yuv_ref.BT601_FULL)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


def test_stage_refusals():
    rng = np.random.default_rng(4)
    y, u, v = _planes(rng, 1, 100, 52, "444")
    with pytest.raises(TileMotionError) as ei:
        _stage(y, u, v, "444", 12, 52, 0)
    assert ei.value.code == E_UNSUPPORTED and "more than 8" in str(ei.value)
    with pytest.raises(TileMotionError) as ei:
        _stage(y, u, v, "444", 100, 52, 7)
    assert ei.value.code == E_INVAL
    assert _stage(y, u, v, "444", 13, 7, 0).shape == (1, 7, 13)  # the largest reduction still goes through


# ---- 7. every (Y, U, V) triple through each colour rule
@pytest.mark.parametrize("mode", [yuv_ref.BT601_LIMITED, yuv_ref.BT601_FULL, yuv_ref.TILER])
def test_every_triple(mode):
    i = np.arange(1 << 24, dtype=np.uint32).reshape(1, 4096, 4096)
    y, u, v = (((i >> s) & 255).astype(np.uint8) for s in (16, 8, 0))
    got = _stage(y, u, v, "444", 4096, 4096, mode)
    want = yuv_ref.to_rgb32(y, u, v, mode)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert len(bad) == 0, (len(bad), [(hex(int(b)), hex(int(got.ravel()[b])), hex(int(want.ravel()[b]))) for b in bad[:4]])


# ---- 8. a clip from a file against the same frames pushed
def write_y4m(path, y, u, v, layout, header_style, fps="25:1", extra_tags=""):
    """header_style "ffmpeg": 'FRAME\\n', C420jpeg-style tags and an aspect; "own": what tm_generate_y4m writes ('FRAME \\n')"""
    nf, h, w = y.shape
    tag = {"444": "C444", "422": "C422", "420jpeg": "C420jpeg", "420mpeg2": "C420mpeg2", "mono": "Cmono"}[layout]
    with open(path, "wb") as f:
        if header_style == "ffmpeg":
            f.write(f"YUV4MPEG2 W{w} H{h} F{fps} Ip A1:1 {tag} XYSCSS={layout.upper()}{extra_tags}\n".encode())
        else:
            f.write(f"YUV4MPEG2 W{w} H{h} F{fps} Ip {tag}{extra_tags}\n".encode())
        for i in range(nf):
            f.write(b"FRAME\n" if header_style == "ffmpeg" else b"FRAME \n")
            f.write(y[i].tobytes())
            if u is not None:
                f.write(u[i].tobytes() + v[i].tobytes())


def _encoder(**kw):
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in {**BASE, **kw}.items():
        setattr(enc, k, v)
    return enc


def _state(enc):
    nf = enc.counts()["frames"]
    hdr, pal, rgb = enc.Tiles()
    return dict(tilemaps=np.stack([enc.TileMap(f) for f in range(nf)]), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(), keyframes=enc.KeyFrames(),
                correl=enc.FrameCorrelations().view(np.uint32))


def _assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _smooth_clip(nf, w, h, layout, seed=1):
    """planes with structure (a moving gradient and some noise), so that the encode behind them has something to find"""
    rng = np.random.default_rng(seed)
    f, yy, xx = np.mgrid[0:nf, 0:h, 0:w]
    y = ((xx * 2 + yy + f * 5) % 256 + rng.integers(-6, 7, (nf, h, w))).clip(0, 255).astype(np.uint8)
    if layout == "mono":
        return y, None, None
    ch, cw = chroma_shape(layout, w, h)
    f, yy, xx = np.mgrid[0:nf, 0:ch, 0:cw]
    u = ((xx * 3 + f * 2) % 200 + 20 + rng.integers(-3, 4, (nf, ch, cw))).clip(0, 255).astype(np.uint8)
    v = ((yy * 4 + f * 3) % 180 + 40 + rng.integers(-3, 4, (nf, ch, cw))).clip(0, 255).astype(np.uint8)
    return y, u, v


def _pushed_from_planes(y, u, v, layout, start, count, scaling, mode):
    h, w = y.shape[1:]
    dw, dh = _dst(w, h, scaling)
    sl = slice(start, start + count)
    Y, U, V = resample_ref.resample_yuv(y[sl], None if u is None else u[sl], None if v is None else v[sl], layout, dw, dh)
    return yuv_ref.to_rgb32(Y, U, V, mode)


@pytest.mark.parametrize("layout,style", [("420jpeg", "ffmpeg"), ("420jpeg", "own"), ("444", "ffmpeg"), ("444", "own")])
def test_file_equals_pushed_frames(tmp_path, monkeypatch, layout, style):
    monkeypatch.chdir(tmp_path)
    y, u, v = _smooth_clip(9, 96, 64, layout)
    write_y4m("clip.y4m", y, u, v, layout, style)
    settings = dict(InputFileName="clip.y4m", StartFrame=2, FrameCount=5, Scaling=0.75)
    enc = _encoder(OutputFileName="file.gtm", **settings)
    info = enc.OpenInput()
    assert info == dict(width=72, height=48, fps=25.0, frames=5)
    enc.Run()
    want_frames = _pushed_from_planes(y, u, v, layout, 2, 5, 0.75, yuv_ref.BT601_LIMITED)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want_frames)
    got = _state(enc)
    enc.Run(S.esLoad)  # a second Load reads the device clip again
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want_frames)
    enc.close()

    ref = _encoder(OutputFileName="file.gtm", **settings)  # (the .gtm embeds the settings: the same on both sides)
    ref.SetVideo(72, 48, 25.0, 5)
    for f in range(5):
        ref.PushFrame(f, want_frames[f])
    os.rename("file.gtm", "from_file.gtm")
    ref.Run()
    _assert_same(got, _state(ref))
    assert open("from_file.gtm", "rb").read() == open("file.gtm", "rb").read()
    ref.close()


def test_run_opens_the_input_by_itself(tmp_path):
    """LoadSettings(ini); Run() as in the reference: no SetVideo, no OpenInput"""
    y, u, v = _smooth_clip(4, 64, 48, "420mpeg2", seed=2)
    write_y4m(tmp_path / "clip.y4m", y, u, v, "420mpeg2", "ffmpeg", fps="30000:1001", extra_tags=" XCOLORRANGE=FULL")
    a = _encoder(InputFileName=str(tmp_path / "clip.y4m"), Scaling=1.5)
    a.SaveSettings(tmp_path / "s.ini")
    a.close()
    enc = TilingEncoder()
    enc.LoadSettings(tmp_path / "s.ini")
    assert enc.VideoInfo()["frames"] == 0
    enc.Run()
    assert enc.VideoInfo() == dict(width=96, height=72, fps=30000 / 1001, frames=4)
    want = _pushed_from_planes(y, u, v, "420mpeg2", 0, 4, 1.5, yuv_ref.BT601_FULL)  # AUTO follows XCOLORRANGE=FULL
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    enc.InputYUV = TInputYUV.yuvBT601Limited
    assert enc.InputYUV == TInputYUV.yuvBT601Limited
    enc.Run(S.esLoad)  # another colour rule: the clip is decoded again
    want = _pushed_from_planes(y, u, v, "420mpeg2", 0, 4, 1.5, yuv_ref.BT601_LIMITED)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    enc.close()


@pytest.mark.parametrize("chunk", ["1", "2", "4"])
def test_file_read_in_many_chunks(tmp_path, monkeypatch, chunk):
    """the read / upload / convert pipeline with its two staging buffers reused several times over (TM_INPUT_CHUNK_FRAMES)"""
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", chunk)
    y, u, v = _smooth_clip(11, 72, 40, "420jpeg", seed=4)
    write_y4m(tmp_path / "c.y4m", y, u, v, "420jpeg", "ffmpeg")
    enc = _encoder(InputFileName=str(tmp_path / "c.y4m"), StartFrame=1, Scaling=1.0)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _pushed_from_planes(y, u, v, "420jpeg", 1, 10, 1.0, yuv_ref.BT601_LIMITED))
    enc.close()


@pytest.mark.parametrize("layout", ["422", "mono"])
def test_other_layouts_from_a_file(tmp_path, layout):
    y, u, v = _smooth_clip(3, 72, 40, layout, seed=3)  # (odd chroma width for 4:2:2 at 0.5: 36 -> 18 is even, the source's 36 is not the point)
    write_y4m(tmp_path / "c.y4m", y, u, v, layout, "own")
    enc = _encoder(InputFileName=str(tmp_path / "c.y4m"), Scaling=1.0)
    enc.OpenInput()
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _pushed_from_planes(y, u, v, layout, 0, 3, 1.0, yuv_ref.BT601_LIMITED))
    enc.close()


# ---- 9. the exports, read back
def test_exports_read_back(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = synth.video(6, 64, 48, cut=3)
    enc = _encoder(OutputFileName="out.gtm")
    enc.SetVideo(64, 48, 24.0, 6)
    for f in range(6):
        enc.PushFrame(f, frames[f])
    enc.Run()
    src = enc.RenderFrames(input=True, device=False)
    assert np.array_equal(src, frames & 0xffffff)
    enc.GeneratePNGs(input=True)
    enc.GenerateY4M("in.y4m", input=True)
    enc.close()

    png = _encoder(InputFileName="out_%.4d.png")
    assert png.OpenInput() == dict(width=64, height=48, fps=24.0, frames=6)  # counted up to the first gap
    png.Run(S.esLoad)
    assert np.array_equal(png.RenderFrames(input=True, device=False), src)  # PNG is lossless
    png.close()

    raw = open("in.y4m", "rb").read()
    head, body = raw.split(b"\n", 1)
    assert head.endswith(b"C444")
    planes = np.frombuffer(body, np.uint8).reshape(6, len(b"FRAME \n") + 3 * 64 * 48)[:, len(b"FRAME \n"):].reshape(6, 3, 48, 64)
    y4m = _encoder(InputFileName="in.y4m")
    y4m.InputYUV = TInputYUV.yuvTiler
    assert y4m.OpenInput() == dict(width=64, height=48, fps=24.0, frames=6)
    y4m.Run(S.esLoad)
    want = yuv_ref.to_rgb32(planes[:, 0], planes[:, 1], planes[:, 2], yuv_ref.TILER)  # the decode of the file's bytes, not the source
    assert np.array_equal(y4m.RenderFrames(input=True, device=False), want)
    y4m.close()


# ---- 10. manual key frames
def test_png_sequence_takes_its_key_frames_from_kf_files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = synth.video(12, 64, 48, cut=6)  # a scene cut at 6, where no .kf file is
    w = _encoder(OutputFileName="seq.gtm", MotionPredictRadius=0)
    w.SetVideo(64, 48, 24.0, 12)
    for f in range(12):
        w.PushFrame(f, frames[f])
    w.Run()
    auto = w.KeyFrames().tolist()
    assert 6 in auto and auto != [0, 4, 9]
    w.GeneratePNGs(input=True)
    w.close()
    for f in (4, 9):
        open("seq_%04d.kf" % f, "wb").close()
    enc = _encoder(InputFileName="seq_%.4d.png", MotionPredictRadius=0)
    enc.Run()
    assert enc.KeyFrames().tolist() == [0, 4, 9]
    correl = enc.FrameCorrelations()
    assert correl[6] < 0.8 and len(correl) == 12  # still computed and reported
    # pushed frames bring the automatic rule back
    enc.SetVideo(64, 48, 24.0, 12)
    for f in range(12):
        enc.PushFrame(f, frames[f])
    enc.Run()
    assert enc.KeyFrames().tolist() == auto
    enc.close()
    # StartFrame shifts the pattern's numbers: frame i is file i + StartFrame
    enc = _encoder(InputFileName="seq_%.4d.png", StartFrame=2, FrameCount=9, MotionPredictRadius=0)
    enc.Run(S.esLoad)
    assert enc.KeyFrames().tolist() == [0, 2, 7]
    assert np.array_equal(enc.RenderFrames(input=True, device=False), frames[2:11] & 0xffffff)
    enc.close()


# ---- 11. a device group
@pytest.mark.parametrize("radius", [0, 8])
def test_device_group_reads_the_file(tmp_path, radius):
    y, u, v = _smooth_clip(9, 96, 64, "420jpeg")
    write_y4m(tmp_path / "clip.y4m", y, u, v, "420jpeg", "ffmpeg")
    settings = dict(InputFileName=str(tmp_path / "clip.y4m"), StartFrame=2, FrameCount=5, Scaling=0.75, MotionPredictRadius=radius)
    one = _encoder(**settings)
    one.Run()
    want = _state(one)
    one.close()
    grp = TilingEncoder()
    grp.SetDevices([0, 0])
    grp.LoadDefaultSettings()
    for k, val in {**BASE, **settings}.items():
        setattr(grp, k, val)
    grp.Run()
    _assert_same(_state(grp), want)
    assert np.array_equal(grp.RenderFrames(input=True, device=False), _pushed_from_planes(y, u, v, "420jpeg", 2, 5, 0.75, yuv_ref.BT601_LIMITED))
    grp.close()


# ---- 12. refusals leave the encoder usable
def test_refusals_leave_the_encoder_usable(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = synth.video(4, 64, 48, cut=2)
    y, u, v = _smooth_clip(2, 64, 48, "420jpeg")
    write_y4m("ok.y4m", y, u, v, "420jpeg", "ffmpeg")
    open("p10.y4m", "wb").write(open("ok.y4m", "rb").read().replace(b"C420jpeg", b"C420p10", 1))
    open("clip.avi", "wb").write(b"RIFF\0\0\0\0AVI LIST" + bytes(200))
    from PIL import Image
    for i in range(4):
        Image.fromarray(np.zeros((48 if i != 2 else 40, 64, 3), np.uint8), "RGB").save("s_%04d.png" % i)  # another size in the middle
    enc = _encoder()

    def pushed_clip_encodes():
        enc.SetVideo(64, 48, 24.0, 4)
        for f in range(4):
            enc.PushFrame(f, frames[f])
        enc.Run()
        assert enc.counts()["tiles"] > 0 and np.array_equal(enc.RenderFrames(input=True, device=False), frames & 0xffffff)

    for name, code, word, at_open in (("p10.y4m", E_UNSUPPORTED, "C420p10", True), ("clip.avi", E_UNSUPPORTED, "yuv4mpegpipe", True),
                                      ("missing_%.4d.png", E_IO, "missing_0000.png", True), ("s_%.4d.png", E_INVAL, "s_0002.png", False)):
        enc.InputFileName = name
        with pytest.raises(TileMotionError) as ei:
            if not at_open:
                enc.OpenInput()
            enc.Run(S.esLoad) if not at_open else enc.OpenInput()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        pushed_clip_encodes()
    enc.InputFileName = "ok.y4m"
    enc.StartFrame = 1
    enc.FrameCount = 5
    with pytest.raises(TileMotionError) as ei:
        enc.OpenInput()
    assert ei.value.code == E_INVAL
    pushed_clip_encodes()
    enc.close()
