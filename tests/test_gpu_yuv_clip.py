"""Load takes YUV clips lent in memory (tm_set_frames_yuv, tm_stage_yuv_to_rgb32_fmt): planar, NV12, P010 / P016 and deep planar samples, and
the BT.709 rules.  Everything is bit for bit: the stage seam against the numpy restatement (tests/yuv_clip_ref.py), the encoder against the
same frames pushed as RGB32 and against the same planes read from a Y4M file."""
import ctypes
import functools

import numpy as np
import pytest

from tests import resample_ref, yuv_ref, yuv_clip_ref as ref
from tests.resample_ref import CHROMA_ID, chroma_shape
from tests.yuv_clip_ref import U8, U16_LOW, U16_HIGH, BT709_LIMITED, BT709_FULL
from tiler_amd import synth
from tiler_amd._lib import TileMotionError, YuvClip, lib
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S, TInputYUV, TSamples

pytestmark = pytest.mark.gpu

E_INVAL = -1
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=40)  # (fewer than the 72 tiles of the half-size clip)


def _dev(a):
    import torch
    if a is None:
        return None
    if a.dtype == np.uint16:
        a = a.view(np.int16)  # (the words' bits; every torch build has int16)
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared clip is read-only)


def _stage(y, u, v, layout, dw, dh, mode, samples=U8, depth=8):
    import torch
    from tiler_amd import stages
    out = stages.yuv_to_rgb32_fmt(_dev(y), _dev(u), _dev(v), CHROMA_ID[layout], dw, dh, mode, samples, depth)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _pairs(u, v):
    return np.stack([u, v], -1).reshape(u.shape[:-1] + (2 * u.shape[-1],))


def _half(w, h):
    return max(1, int(np.rint(w * 0.5))), max(1, int(np.rint(h * 0.5)))


# (name, layout, samples, depth, interleaved)
FORMATS = ([("nv12 jpeg", "420jpeg", U8, 8, True), ("nv12 mpeg2", "420mpeg2", U8, 8, True), ("pairs 422", "422", U8, 8, True), ("pairs 444", "444", U8, 8, True),
            ("p010", "420jpeg", U16_HIGH, 10, True), ("p016", "420jpeg", U16_HIGH, 16, True)]
           + [("planar low %d %s" % (d, lay), lay, U16_LOW, d, False) for d in (10, 12) for lay in ("420jpeg", "422", "444", "mono")])


def _random_clip(rng, nf, w, h, layout, samples, depth, interleaved):
    """full-range noise in the format's own words: the hard case for the integer rules"""
    def plane(rows, cols):
        if samples == U8:
            return rng.integers(0, 256, (nf, rows, cols), dtype=np.uint8)
        p = rng.integers(0, 1 << depth, (nf, rows, cols)).astype(np.uint16)
        return p << (16 - depth) if samples == U16_HIGH else p
    y = plane(h, w)
    if layout == "mono":
        return y, None, None
    ch, cw = chroma_shape(layout, w, h)
    u, v = plane(ch, cw), plane(ch, cw)
    return (y, _pairs(u, v), None) if interleaved else (y, u, v)


# ---- 1. the stage seam against the numpy rule
@pytest.mark.parametrize("w,h", [(100, 52), (64, 48), (101, 53)])
def test_stage_matches_the_numpy_rule_bit_for_bit(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    for name, layout, samples, depth, inter in FORMATS:
        y, u, v = _random_clip(rng, 2, w, h, layout, samples, depth, inter)
        Y, U, V = ref.narrowed_planes(y, u, v, layout, samples, depth)
        for dw, dh in ((w, h), _half(w, h), (150, 78)):
            planes = resample_ref.resample_yuv(Y, U, V, layout, dw, dh)
            for mode in (yuv_ref.BT601_LIMITED, BT709_LIMITED, BT709_FULL):
                got = _stage(y, u, v, layout, dw, dh, mode, samples, depth)
                want = ref.to_rgb32(*planes, mode)
                assert got.shape == want.shape
                bad = np.argwhere(got != want)
                assert len(bad) == 0, (name, (dw, dh), mode, len(bad), bad[:3].tolist(), [hex(got[tuple(b)]) for b in bad[:3]], [hex(want[tuple(b)]) for b in bad[:3]])


# ---- 2. junk around the samples is ignored
def _stage_raw(bufs, strides, nf, w, h, layout, samples, depth, dw, dh, mode):
    import torch
    out = torch.empty((nf, dh, dw), dtype=torch.int32, device="cuda")
    ptr = [ctypes.c_void_p(b.data_ptr()) if b is not None else None for b in bufs]
    rc = lib().tm_stage_yuv_to_rgb32_fmt(ptr[0], ptr[1], ptr[2], (ctypes.c_int64 * 6)(*strides), nf, w, h, CHROMA_ID[layout], samples, depth, dw, dh, mode,
                                         ctypes.c_void_p(out.data_ptr()), None)
    assert rc == 0, lib().tm_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _padded(plane, pad, extra_rows):
    """the plane's bytes inside a buffer of 0xFF with rows `pad` bytes longer and frames `extra_rows` rows longer: buffer, row stride, frame stride"""
    nf, rows, _ = plane.shape
    raw = np.ascontiguousarray(plane).view(np.uint8).reshape(nf, rows, -1)
    buf = np.full((nf, rows + extra_rows, raw.shape[2] + pad), 0xFF, np.uint8)
    buf[:, :rows, :raw.shape[2]] = raw
    return buf, buf.shape[2], buf.shape[1] * buf.shape[2]


@pytest.mark.parametrize("pad", [2, 6])
def test_padding_and_bits_outside_the_depth_are_ignored(pad):
    import torch
    rng = np.random.default_rng(pad)
    w, h, nf = 101, 53, 2
    for name, layout, samples, depth, inter in FORMATS:
        clean = _random_clip(rng, nf, w, h, layout, samples, depth, inter)
        dirty = []
        for p in clean:
            if p is not None and samples != U8 and depth < 16:
                junk = rng.integers(0, 1 << (16 - depth), p.shape).astype(np.uint16)
                p = p | (junk << depth if samples == U16_LOW else junk)  # above the depth for U16_LOW, below it for U16_HIGH
            dirty.append(p)
        for dw, dh in ((w, h), (76, 40)):
            want = _stage(*clean, layout, dw, dh, yuv_ref.BT601_LIMITED, samples, depth)
            bufs, strides = [], []
            for i, p in enumerate(dirty):
                if p is None:
                    bufs.append(None); strides += [0, 0]
                    continue
                buf, row, frame = _padded(p, pad, 1 + i)
                bufs.append(torch.from_numpy(buf).cuda()); strides += [row, frame]
            got = _stage_raw(bufs, strides, nf, w, h, layout, samples, depth, dw, dh, yuv_ref.BT601_LIMITED)
            assert np.array_equal(got, want), (name, dw, dh)


# ---- 3. every (Y, U, V) triple
def _triples():
    i = np.arange(1 << 24, dtype=np.uint32).reshape(1, 4096, 4096)
    return tuple(((i >> s) & 255).astype(np.uint8) for s in (16, 8, 0))


@pytest.mark.parametrize("mode", [BT709_LIMITED, BT709_FULL])
def test_every_triple_through_bt709(mode):
    y, u, v = _triples()
    got = _stage(y, u, v, "444", 4096, 4096, mode)
    want = ref.to_rgb32(y, u, v, mode)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert len(bad) == 0, (len(bad), [(hex(int(b)), hex(int(got.ravel()[b])), hex(int(want.ravel()[b]))) for b in bad[:4]])


def test_every_triple_as_16_bit_words_equals_the_bytes():
    y, u, v = _triples()
    want = _stage(y, u, v, "444", 4096, 4096, yuv_ref.BT601_LIMITED)
    hi = [p.astype(np.uint16) << 8 for p in (y, u, v)]  # each byte in the high half of a 16-bit sample
    got = _stage(*hi, "444", 4096, 4096, yuv_ref.BT601_LIMITED, U16_HIGH, 16)
    assert np.array_equal(got, want)


# ---- 4. bytes in three planes through the new seam are the old seam
@pytest.mark.parametrize("layout", ["444", "422", "420jpeg", "420mpeg2", "mono"])
def test_planar_bytes_equal_the_existing_seam(layout):
    import torch
    from tiler_amd import stages
    rng = np.random.default_rng(len(layout))
    y, u, v = _random_clip(rng, 2, 101, 53, layout, U8, 8, False)
    for dw, dh in ((101, 53), (76, 40), (150, 78)):
        for mode in (yuv_ref.AUTO, yuv_ref.BT601_FULL, yuv_ref.TILER, BT709_LIMITED):
            old = stages.yuv_to_rgb32(_dev(y), _dev(u), _dev(v), CHROMA_ID[layout], dw, dh, mode)
            torch.cuda.synchronize()
            assert np.array_equal(_stage(y, u, v, layout, dw, dh, mode), old.cpu().numpy().view(np.uint32)), (dw, dh, mode)


# ---- 5. .. 9. the encoder
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


W, H, NF, FPS = 64, 48, 6, 25.0


@functools.lru_cache(maxsize=None)
def _clip():
    y, u, v = _smooth_clip(NF, W, H, "420jpeg")
    for a in (y, u, v):
        a.setflags(write=False)
    return y, u, v


def _encoder(devices=None, **kw):
    enc = TilingEncoder()
    if devices is not None:
        enc.SetDevices(devices)
    enc.LoadDefaultSettings()
    for k, v in {**BASE, "MotionPredictRadius": 0, **kw}.items():
        setattr(enc, k, v)
    return enc


def _state(enc):
    nf = enc.counts()["frames"]
    hdr, pal, rgb = enc.Tiles()
    return dict(tilemaps=np.stack([enc.TileMap(f) for f in range(nf)]), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(), keyframes=enc.KeyFrames(),
                correl=enc.FrameCorrelations().view(np.uint32), source=enc.RenderFrames(input=True, device=False))


def _assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _dst(scaling):
    return max(1, int(np.rint(W * scaling))), max(1, int(np.rint(H * scaling)))


def _pushed_state(scaling, mode, radius=0):
    return _pushed_state_once(float(scaling), int(mode), int(radius))


@functools.lru_cache(maxsize=None)
def _pushed_state_once(scaling, mode, radius):
    """the reference, computed once: the same frames pushed as RGB32 made by the numpy rule (AUTO without a range flag is BT.601 limited)"""
    y, u, v = _clip()
    dw, dh = _dst(scaling)
    frames = ref.clip_to_rgb32(y, u, v, "420jpeg", U8, 8, dw, dh, mode)
    enc = _encoder(Scaling=scaling, MotionPredictRadius=radius)
    enc.SetVideo(dw, dh, FPS, NF)
    for f in range(NF):
        enc.PushFrame(f, frames[f])
    enc.Run()
    st = _state(enc)
    assert np.array_equal(st["source"], frames)
    enc.close()
    return st


def _write_y4m(path, y, u, v):
    nf, h, w = y.shape
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (w, h))
        for i in range(nf):
            f.write(b"FRAME\n" + y[i].tobytes() + u[i].tobytes() + v[i].tobytes())


@pytest.mark.parametrize("scaling,mode", [(1.0, TInputYUV.yuvAuto), (0.5, TInputYUV.yuvAuto), (1.0, TInputYUV.yuvBT709Limited)])
def test_nv12_on_the_device_equals_pushed_frames_and_the_file(tmp_path, scaling, mode):
    y, u, v = _clip()
    want = _pushed_state(scaling, int(mode) or yuv_ref.BT601_LIMITED)
    enc = _encoder(Scaling=scaling)
    enc.InputYUV = mode
    info = enc.SetFramesYUV(_dev(y), _dev(_pairs(u, v)), chroma=CHROMA_ID["420jpeg"], fps=FPS)
    dw, dh = _dst(scaling)
    assert info == dict(width=dw, height=dh, fps=FPS, frames=NF)
    enc.Run()
    _assert_same(_state(enc), want)
    enc.close()

    _write_y4m(tmp_path / "clip.y4m", y, u, v)
    fil = _encoder(Scaling=scaling, InputFileName=str(tmp_path / "clip.y4m"))
    fil.InputYUV = mode
    assert fil.OpenInput() == info
    fil.Run()
    got = _state(fil)
    fil.close()
    # (the settings differ by InputFileName only, which no step reads after Load)
    _assert_same(got, want)


@pytest.mark.parametrize("chunk", ["1", "2", "4"])
def test_planar_clip_in_host_memory(monkeypatch, chunk):
    """pageable memory goes through the encoder's page-locked buffers, page-locked memory is uploaded from where it is; many chunks"""
    import torch
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", chunk)
    want = _pushed_state(1.0, yuv_ref.BT601_LIMITED)
    y, u, v = (np.array(a) for a in _clip())
    pinned = [torch.from_numpy(a).pin_memory() for a in (y, u, v)]
    assert all(t.is_pinned() for t in pinned)
    for planes in ((y, u, v), pinned):
        enc = _encoder()
        enc.SetFramesYUV(*planes, chroma=CHROMA_ID["420jpeg"], fps=FPS)
        enc.Run()
        _assert_same(_state(enc), want)
        enc.close()


def test_strided_planes_in_host_memory(monkeypatch):
    """rows and frames with padding, as a decoder's linesize leaves them: the 2-D and the frame-by-frame copies"""
    import torch
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "4")
    want = _pushed_state(1.0, yuv_ref.BT601_LIMITED)
    for extra_rows in (0, 3):  # frames one after the other, and frames with a gap between them
        for pin in (False, True):
            big = []
            for a in _clip():
                nf, rows, cols = a.shape
                b = np.full((nf, rows + extra_rows, cols + 16), 0xFF, np.uint8)
                b[:, :rows, :cols] = a
                big.append(torch.from_numpy(b).pin_memory() if pin else b)
            planes = [b[:, :a.shape[1], :a.shape[2]] for a, b in zip(_clip(), big)]
            enc = _encoder()
            enc.SetFramesYUV(*planes, chroma=CHROMA_ID["420jpeg"], fps=FPS)
            enc.Run(S.esLoad)
            assert np.array_equal(enc.RenderFrames(input=True, device=False), want["source"]), (extra_rows, pin)
            enc.close()


def test_p010_on_the_device_equals_the_narrowed_clip():
    rng = np.random.default_rng(10)
    y8, u8, v8 = (a[:4] for a in _clip())
    # 10-bit samples around the bytes, in the high bits of the word, with junk below them
    deep = [((a.astype(np.uint16) << 2) + rng.integers(0, 4, a.shape).astype(np.uint16)).clip(0, 1023) for a in (y8, u8, v8)]
    words = [(d << 6) | rng.integers(0, 64, d.shape).astype(np.uint16) for d in deep]
    Y, U, V = (ref.narrow(x, U16_HIGH, 10) for x in words)
    states = []
    for planes, samples, depth in (((words[0], _pairs(words[1], words[2])), TSamples.u16High, 10), ((Y, _pairs(U, V)), TSamples.u8, 8)):
        enc = _encoder()
        enc.SetFramesYUV(_dev(planes[0]), _dev(planes[1]), chroma=CHROMA_ID["420jpeg"], fps=FPS, samples=samples, depth=depth)
        enc.Run()
        states.append(_state(enc))
        enc.close()
    _assert_same(states[0], states[1])
    assert np.array_equal(states[0]["source"], ref.clip_to_rgb32(Y, U, V, "420jpeg", U8, 8, W, H, yuv_ref.BT601_LIMITED))


@pytest.mark.parametrize("radius", [0, 8])
def test_device_group_converts_the_lent_clip(radius):
    y, u, v = _clip()
    want = _pushed_state(1.0, yuv_ref.BT601_LIMITED, radius)
    one = _encoder(MotionPredictRadius=radius)
    one.SetFramesYUV(_dev(y), _dev(_pairs(u, v)), chroma=CHROMA_ID["420jpeg"], fps=FPS)
    one.Run()
    _assert_same(_state(one), want)
    one.close()
    for lend in ("device", "host"):
        grp = _encoder(devices=[0, 0], MotionPredictRadius=radius)
        if lend == "device":
            grp.SetFramesYUV(_dev(y), _dev(_pairs(u, v)), chroma=CHROMA_ID["420jpeg"], fps=FPS)
        else:
            grp.SetFramesYUV(np.array(y), np.array(u), np.array(v), chroma=CHROMA_ID["420jpeg"], fps=FPS)
        grp.Run()
        _assert_same(_state(grp), want)
        grp.close()


def test_life_cycle():
    import torch
    y, u, v = _clip()
    want = _pushed_state(1.0, yuv_ref.BT601_LIMITED)["source"]
    dy, duv = _dev(y), _dev(_pairs(u, v))
    enc = _encoder()
    enc.SetFramesYUV(dy, duv, chroma=CHROMA_ID["420jpeg"], fps=FPS)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    keep = dy.clone(), duv.clone()
    dy.fill_(7); duv.fill_(9)  # the planes are the caller's again
    torch.cuda.synchronize()
    enc.Run(S.esLoad)  # a second Load reads the encoder's own clip
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    enc.InputYUV = TInputYUV.yuvBT709Limited  # another rule needs the planes, which are no longer held
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esLoad)
    assert ei.value.code == E_INVAL and "lend the clip again" in str(ei.value)
    dy.copy_(keep[0]); duv.copy_(keep[1])
    enc.SetFramesYUV(dy, duv, chroma=CHROMA_ID["420jpeg"], fps=FPS)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), ref.clip_to_rgb32(y, u, v, "420jpeg", U8, 8, W, H, BT709_LIMITED))
    # tm_set_video switches the source away, and a pushed clip encodes
    frames = synth.video(4, 64, 48, cut=2)
    enc.SetVideo(64, 48, 24.0, 4)
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esLoad)
    assert "no frames" in str(ei.value)
    for f in range(4):
        enc.PushFrame(f, frames[f])
    enc.Run()
    assert enc.counts()["tiles"] > 0 and np.array_equal(enc.RenderFrames(input=True, device=False), frames & 0xffffff)
    enc.close()


def test_a_refused_clip_leaves_the_encoder_as_it_was():
    y, u, v = _clip()
    want = _pushed_state(1.0, yuv_ref.BT601_LIMITED)["source"]
    enc = _encoder()
    dy, duv = _dev(y), _dev(_pairs(u, v))
    info = enc.SetFramesYUV(dy, duv, chroma=CHROMA_ID["420jpeg"], fps=FPS)
    L = lib()

    def clip(**kw):
        c = YuvClip()
        c.y, c.u, c.y_row, c.y_frame, c.u_row, c.u_frame = dy.data_ptr(), duv.data_ptr(), 2 * W, 2 * W * H, 2 * W, W * H  # (a larger clip, were it taken)
        c.width, c.height, c.frames, c.fps, c.chroma, c.samples, c.depth, c.memory = 2 * W, 2 * H, 2, 50.0, 2, 0, 8, 1
        for k, val in kw.items():
            setattr(c, k, val)
        return c
    for bad in (clip(y=None), clip(u=None), clip(width=0), clip(height=65537), clip(frames=0), clip(fps=0.0), clip(chroma=9), clip(samples=3), clip(memory=2),
                clip(depth=10), clip(samples=1, depth=8), clip(y_row=2 * W - 1), clip(u_row=2 * W - 2), clip(samples=2, depth=10, y_row=4 * W + 1, u_row=4 * W),
                clip(y_frame=-1)):
        assert L.tm_set_frames_yuv(ctypes.c_void_p(enc._h), ctypes.byref(bad)) == E_INVAL
        assert enc.VideoInfo() == info
    assert L.tm_set_frames_yuv(ctypes.c_void_p(enc._h), None) == E_INVAL
    enc.Scaling = 0.05  # more than eightfold: refused like a file, and nothing is taken
    assert L.tm_set_frames_yuv(ctypes.c_void_p(enc._h), ctypes.byref(clip())) == -6
    enc.Scaling = 1.0
    assert enc.VideoInfo() == info
    enc.Run(S.esLoad)  # the clip lent first is still the source
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    enc.close()
