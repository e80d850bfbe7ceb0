"""Frames delivered as YUV on the device (tm_stage_rgb32_to_yuv_fmt, tm_player_read_yuv, tm_render_frames_yuv, tools/play_gtm.py --y4m): every
sample bit for bit the numpy restatement's (tests/yuv_out_ref.py), in every layout, at every alignment, with nothing written outside the rows;
the player's and the encoder's YUV reads against their RGB reads pushed through the restatement; and a .gtm played to a Y4M file that Load
reads back."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import player_streams as ps  # noqa: E402
from tests import yuv_out_ref as ref  # noqa: E402
from tests.test_gpu_render import _encode  # noqa: E402
from tests.yuv_out_ref import BT601_LIMITED, BT601_FULL, TILER, BT709_LIMITED, BT709_FULL, INTEGER_MODES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6
STAGE_LAYOUTS = ["444", "422", "420jpeg", "420mpeg2", "mono", "nv12", "p010", "420p10"]
SIZES = [(1, 1), (3, 5), (17, 9), (40, 24), (67, 35), (264, 136)]
GUARD = 64


def _mode_for(layout, i):
    deep = ref.LAYOUTS[layout][1] != ref.U8
    return (BT601_LIMITED, BT709_LIMITED)[i % 2] if deep else INTEGER_MODES[i % 4]


def _random_frames(seed, nf, h, w):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (nf, h, w), dtype=np.uint64).astype(np.uint32)  # (the top byte is noise: it must not matter)


def _stage(rgb, w, layout, mode, pad_row=0, pad_frame=0, shift=0):
    """the stage seam on rgb [F][H][>= w] into pattern-filled buffers with a guard band before and after each plane; rows start `shift` bytes
    past a 256-byte boundary + GUARD.  Returns nothing: the whole of every buffer is compared with what the restatement says it must hold"""
    from tiler_amd import lib
    chroma, samples, depth, pairs = ref.LAYOUTS[layout]
    nf, h = rgb.shape[:2]
    want = ref.planes(rgb[:, :, :w], layout, mode)
    src = torch.from_numpy(rgb.view(np.int32)).cuda()
    bufs, exps, ptrs, strides = [], [], [], []
    for i, plane in enumerate(want):
        if plane is None:
            ptrs.append(None)
            strides += [0, 0]
            continue
        rows, rb = plane.shape[1], plane.shape[2] * plane.itemsize
        rs = rb + pad_row
        fs = rs * rows + pad_frame
        size = GUARD + shift + (nf - 1) * fs + (rows - 1) * rs + rb + GUARD
        pattern = ((np.arange(size, dtype=np.int64) * 7 + 3 + 11 * i) % 251).astype(np.uint8)
        exp = pattern.copy()
        raw = np.ascontiguousarray(plane).view(np.uint8).reshape(nf, rows, rb)
        for f in range(nf):
            for r in range(rows):
                at = GUARD + shift + f * fs + r * rs
                exp[at:at + rb] = raw[f, r]
        buf = torch.from_numpy(pattern).cuda()
        assert buf.data_ptr() % 256 == 0
        bufs.append(buf)
        exps.append(exp)
        ptrs.append(buf.data_ptr() + GUARD + shift)
        strides += [rs, fs]
    L = lib()
    rc = L.tm_stage_rgb32_to_yuv_fmt(ctypes.c_void_p(src.data_ptr()), rgb.shape[2], nf, w, h, *(ctypes.c_void_p(p) for p in ptrs), (ctypes.c_int64 * 6)(*strides), chroma,
                                     samples, depth, mode, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tm_last_error()
    torch.cuda.synchronize()
    for i, (buf, exp) in enumerate(zip(bufs, exps)):
        got = buf.cpu().numpy()
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (layout, mode, "plane %d" % i, len(bad), [(int(b), int(got[b]), int(exp[b])) for b in bad[:6]])


# ---- 1. the stage seam
@pytest.mark.parametrize("layout", STAGE_LAYOUTS)
def test_stage_is_the_restatement_bit_for_bit(layout):
    """a single sample, odd edges in both axes, a partial last vector and workgroup, more than one workgroup per row; the sizes below the
    largest meet every colour rule the layout takes"""
    deep = ref.LAYOUTS[layout][1] != ref.U8
    for i, (w, h) in enumerate(SIZES):
        rgb = _random_frames(100 + i, 3, h, w)
        modes = [_mode_for(layout, i)] if (w, h) == SIZES[-1] else ([BT601_LIMITED, BT709_LIMITED] if deep else list(INTEGER_MODES))
        for mode in modes:
            _stage(rgb, w, layout, mode)


@pytest.mark.parametrize("layout", STAGE_LAYOUTS)
def test_stage_strides_and_alignment(layout):
    """padded row and frame strides; planes that start at an odd byte address (U8) and 2, 4, 8 bytes past a 16-byte boundary; a source
    stride_px larger than the width.  Padding, gaps and guard bands come back unchanged (_stage compares whole buffers)"""
    words = ref.LAYOUTS[layout][1] != ref.U8
    for i, (w, h) in enumerate([(67, 35), (264, 136)]):
        rgb = _random_frames(200 + i, 3, h, w + 3)
        mode = _mode_for(layout, i + 1)
        _stage(rgb[:, :, :w].copy(), w, layout, mode, pad_row=6 if words else 5, pad_frame=10)
        _stage(rgb[:, :, :w].copy(), w, layout, mode, pad_row=8, pad_frame=16, shift=2 if words else 1)
        for shift in (2, 4, 8) if words else (3, 4, 8):
            _stage(rgb[:, :, :w].copy(), w, layout, mode, shift=shift)
        _stage(rgb, w, layout, mode)


@pytest.fixture(scope="module")
def colours():
    a = ref.all_colours().reshape(1, 4096, 4096)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("mode", list(INTEGER_MODES) + [TILER])
def test_stage_every_colour(colours, mode):
    from tiler_amd import stages
    y, u, v = stages.rgb32_to_yuv(torch.from_numpy(colours.view(np.int32).copy()).cuda(), layout="444", yuv=mode)
    torch.cuda.synchronize()
    ey, eu, ev = ref.pixels(colours, mode)
    for name, got, exp in (("y", y, ey), ("u", u, eu), ("v", v, ev)):
        bad = np.flatnonzero(got.cpu().numpy().ravel() != exp.ravel())
        assert len(bad) == 0, (name, len(bad), [hex(int(b)) for b in bad[:6]])


def test_flat_colours_give_the_444_samples_in_every_layout():
    from tiler_amd import stages
    rng = np.random.default_rng(5)
    cols = rng.integers(0, 1 << 24, 64, dtype=np.int64).astype(np.int32)
    rgb = torch.from_numpy(np.broadcast_to(cols[:, None, None], (64, 16, 24)).copy()).cuda()
    for mode in (BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL):
        y8, u8, v8 = (a[:, 0, 0].cpu().numpy() for a in stages.rgb32_to_yuv(rgb, layout="444", yuv=mode))
        for layout in ("422", "420", "420mpeg2", "nv12"):
            y, u, v = stages.rgb32_to_yuv(rgb, layout=layout, yuv=mode)
            y, u = y.cpu().numpy(), u.cpu().numpy()
            assert np.all(y == y8[:, None, None]), (mode, layout)
            if v is None:
                assert np.all(u[:, :, 0::2] == u8[:, None, None]) and np.all(u[:, :, 1::2] == v8[:, None, None]), (mode, layout)
            else:
                assert np.all(u == u8[:, None, None]) and np.all(v.cpu().numpy() == v8[:, None, None]), (mode, layout)
    for mode in (BT601_LIMITED, BT709_LIMITED):  # deep samples: 4:4:4 at 10 bits in the low bits is the reference
        y10, u10, v10 = (a[:, 0, 0].cpu().numpy().view(np.uint16) for a in stages.rgb32_to_yuv(rgb, layout=(ref.C444, ref.U16_LOW, 10, False), yuv=mode))
        y, u, v = (a.cpu().numpy().view(np.uint16) for a in stages.rgb32_to_yuv(rgb, layout=(ref.C420JPEG, ref.U16_LOW, 10, False), yuv=mode))
        assert np.all(y == y10[:, None, None]) and np.all(u == u10[:, None, None]) and np.all(v == v10[:, None, None])
        y, uv, _ = stages.rgb32_to_yuv(rgb, layout="p010", yuv=mode)
        y, uv = y.cpu().numpy().view(np.uint16), uv.cpu().numpy().view(np.uint16)
        assert np.all(y == (y10 << 6)[:, None, None]) and np.all(uv[:, :, 0::2] == (u10 << 6)[:, None, None]) and np.all(uv[:, :, 1::2] == (v10 << 6)[:, None, None])


def test_stage_refusals_write_nothing():
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    rgb = torch.zeros((1, 8, 16), dtype=torch.int32, device="cuda")
    out = tuple(torch.full(s, 77, dtype=torch.uint8, device="cuda") for s in ((1, 8, 16), (1, 4, 8), (1, 4, 8)))
    for kw, code in ((dict(layout="420", yuv=TILER), E_INVAL), (dict(layout="420", yuv=6), E_INVAL), (dict(layout="420", yuv=-1), E_INVAL)):
        with pytest.raises(TileMotionError) as ei:
            stages.rgb32_to_yuv(rgb, out=out, **kw)
        assert ei.value.code == code
    with pytest.raises(ValueError):  # 4:2:2 planes are 8 rows: these are too short, which only the binding can see
        stages.rgb32_to_yuv(rgb, layout="422", out=out)
    words = tuple(torch.full(s, 77, dtype=torch.int16, device="cuda") for s in ((1, 8, 16), (1, 4, 16)))
    with pytest.raises(TileMotionError) as ei:
        stages.rgb32_to_yuv(rgb, layout="p010", yuv="bt709-full", out=words)
    assert ei.value.code == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((a == 77).all()) for a in out + words)


# ---- 2. the player
def _want_planes(rgb, layout, mode):
    return ref.planes(rgb, layout, mode)


def _np(a):
    if a is None:
        return None
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _same(got, want, what):
    for name, g, w in zip("yuv", got, want):
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            g = _np(g)
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
            assert np.array_equal(g, w), (what, name)


def _read_all_yuv(path, step, layout, mode, kind):
    """all frames of the file through ReadYUV, `step` at a time: kind "device", "pageable", "pinned" (torch CPU tensors, page-locked) or
    "padded" (pageable numpy planes with padded rows and gaps between the frames: the copies are 2-D)"""
    from tiler_amd import yuv_out
    from tiler_amd.player import GtmPlayer
    with GtmPlayer(path) as p:
        i = p.info()
        n, h, w = i["frames"], i["tm_h"] * 8, i["tm_w"] * 8
        cap = n  # (a last call may ask for more frames than are left: the room is measured against what it delivers)
        if kind == "device":
            full = yuv_out.alloc(layout, cap, h, w, "cuda")
        elif kind == "pageable":
            full = yuv_out.alloc(layout, cap, h, w)
        elif kind == "pinned":
            full = tuple(None if s is None else torch.zeros(s, dtype=torch.uint8, pin_memory=True) for s in yuv_out.plane_shapes(layout, cap, h, w))
        else:
            full = tuple(None if s is None else np.full((s[0], s[1] + 1, s[2] + 5), 99, np.uint8)[:, :s[1], :s[2]] for s in yuv_out.plane_shapes(layout, cap, h, w))
        while p.Tell() < n:
            at = p.Tell()
            got = p.ReadYUV(step, layout=layout, yuv=mode, device=kind == "device", out=tuple(None if a is None else a[at:] for a in full))
            assert got[0].shape[0] == min(step or n, n - at) and p.Tell() == at + got[0].shape[0]
        assert p.ReadYUV(2, layout=layout, yuv=mode, device=kind == "device")[0].shape[0] == 0  # at the end of the stream
        if kind == "padded":
            assert all(a is None or bool((a.base[:, a.shape[1]:, :] == 99).all() and (a.base[:, :, a.shape[2]:] == 99).all() and (a[n:] == 99).all()) for a in full)
    return tuple(None if a is None else a[:n] for a in full)


def _play_rgb(path):
    from tiler_amd.player import GtmPlayer
    with GtmPlayer(path) as p:
        return p.Read(device=False), p.info()


@pytest.fixture(scope="module")
def encoded(tmp_path_factory):
    """the small motion-predicted clip of tests/test_gpu_player.py (7 frames of 100 x 52, radius 8), saved; the encoder stays open for the render tests"""
    from tiler_amd import synth
    out = str(tmp_path_factory.mktemp("yuv_out") / "clip.gtm")
    enc = _encode(synth.video(7, 100, 52, cut=3), PaletteCount=3, ShotTransMinSecondsPerKF=0.1, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False,
                  OutputFileName=out)
    assert ((enc.TileMaps()["Flags"] >> 2) & 1).any()
    yield enc, out
    enc.close()


def _stream_path(which, tmp_path, encoded):
    if which == "encoded":
        return encoded[1]
    L = ps.write_lib()
    path = tmp_path / "made.gtm"
    if which == "5x3":
        ps.write_stream(L, path, 5, 3, 64, nframes=12, kf=(0, 4, 8), mode="border", n_shared=48)
    else:
        ps.write_stream(L, path, 33, 17, 64, nframes=6, kf=(0, 3), mode="border")
    return str(path)


@pytest.mark.parametrize("which", ["5x3", "33x17", "encoded"])
def test_player_read_yuv_equals_read_through_the_restatement(which, tmp_path, monkeypatch, encoded):
    monkeypatch.setenv("TM_PLAYER_CHUNK_FRAMES", "2")  # the two rings are reused several times over
    path = _stream_path(which, tmp_path, encoded)
    rgb, _ = _play_rgb(path)
    for layout, mode in (("nv12", BT601_LIMITED), ("420", BT709_FULL)):
        want = _want_planes(rgb, "420jpeg" if layout == "420" else layout, mode)
        for step in (1, 3, None):
            for kind in ("device", "pageable", "pinned"):
                _same(_read_all_yuv(path, step, layout, mode, kind), want, (which, layout, step, kind))
        _same(_read_all_yuv(path, 3, layout, mode, "padded"), want, (which, layout, "padded"))
    _same(_read_all_yuv(path, None, "p010", BT709_LIMITED, "device"), _want_planes(rgb, "p010", BT709_LIMITED), (which, "p010"))
    _same(_read_all_yuv(path, 3, "444", "tiler", "pageable"), _want_planes(rgb, "444", TILER), (which, "tiler"))


def test_player_read_yuv_interleaves_with_read_and_seek(tmp_path, encoded):
    from tiler_amd._lib import TileMotionError
    from tiler_amd.player import GtmPlayer
    from tiler_amd import yuv_out
    path = _stream_path("5x3", tmp_path, encoded)
    rgb, info = _play_rgb(path)
    n, h, w = info["frames"], info["tm_h"] * 8, info["tm_w"] * 8
    want = _want_planes(rgb, "nv12", BT601_LIMITED)
    cut = lambda a, b: tuple(None if x is None else x[a:b] for x in want)  # noqa: E731
    with GtmPlayer(path) as p:
        _same(p.ReadYUV(2), cut(0, 2), "first two")
        assert p.Tell() == 2
        assert np.array_equal(p.Read(1, device=False), rgb[2:3]) and p.Tell() == 3
        _same(p.ReadYUV(3, device=False), cut(3, 6), "across a key frame")
        p.Seek(1)
        _same(p.ReadYUV(3), cut(1, 4), "after a seek backwards")
        assert p.Tell() == 4
        p.Seek(9)
        _same(p.ReadYUV(5, device=False), cut(9, n), "to the end: got < count")
        assert p.Tell() == n and p.ReadYUV(1)[0].shape[0] == 0
        assert p.ReadYUV(0)[0].shape[0] == 0
        # refused descriptors leave position and destination untouched
        p.Seek(5)
        for device in (True, False):
            planes = tuple(torch.full(s, 55, dtype=torch.uint8, device="cuda") if device else np.full(s, 55, np.uint8) for s in yuv_out.plane_shapes("nv12", 2, h, w)[:2])
            bad_size = tuple(torch.full(s, 55, dtype=torch.uint8, device="cuda") if device else np.full(s, 55, np.uint8) for s in yuv_out.plane_shapes("nv12", 2, h + 2, w)[:2])
            for args, kw, code in (((2,), dict(out=bad_size), E_INVAL),                        # a size that differs from the frames'
                                   ((3,), dict(out=planes), E_INVAL),                          # more frames than the destination holds
                                   ((2,), dict(out=planes, yuv=7), E_INVAL),
                                   ((2,), dict(out=planes, yuv="tiler"), E_INVAL),             # TILER is 4:4:4 / mono only
                                   ((2,), dict(out=(planes[0], None, None)), E_INVAL)):        # chroma pointers missing
                with pytest.raises(TileMotionError) as ei:
                    p.ReadYUV(*args, device=device, **kw)
                assert ei.value.code == code and p.Tell() == 5
            words = tuple(torch.full(s, 55, dtype=torch.int16, device="cuda") if device else np.full(s, 55, np.uint16) for s in yuv_out.plane_shapes("p010", 2, h, w)[:2])
            with pytest.raises(TileMotionError) as ei:
                p.ReadYUV(2, layout="p010", yuv="bt601-full", device=device, out=words)
            assert ei.value.code == E_UNSUPPORTED and p.Tell() == 5
            if device:
                torch.cuda.synchronize()
            assert all(bool((a == 55).all()) for a in planes + bad_size + words)
        with pytest.raises(TileMotionError) as ei:  # host planes named as device memory
            host = yuv_out.alloc("nv12", 2, h, w)
            d = yuv_out.descriptor(host, "nv12")
            d.memory = 1
            got = ctypes.c_int()
            from tiler_amd._lib import check
            check(p._L.tm_player_read_yuv(ctypes.c_void_p(p._h), 2, ctypes.byref(d), 0, ctypes.byref(got)))
        assert ei.value.code == E_INVAL and p.Tell() == 5 and not host[0].any()
        _same(p.ReadYUV(2), cut(5, 7), "after the refusals")


# ---- 3. the encoder's render
def test_render_frames_yuv_equals_render_frames_through_the_restatement(encoded, tmp_path):
    from tiler_amd._lib import TileMotionError
    from tiler_amd.encoder import TilingEncoder
    from tiler_amd import yuv_out
    enc, path = encoded
    c = enc.counts()
    nf, h, w = c["frames"], c["tm_h"] * 8, c["tm_w"] * 8
    for input in (False, True):
        rgb = enc.RenderFrames(input=input, device=False)
        for layout, mode in (("nv12", BT601_LIMITED), ("420mpeg2", BT601_FULL), ("p010", BT709_LIMITED), ("444", TILER)):
            want = _want_planes(rgb, layout, mode)
            for device in (True, False):
                _same(enc.RenderFramesYUV(input=input, layout=layout, yuv=mode, device=device), want, (input, layout, device))
        want = _want_planes(rgb[2:5], "nv12", BT709_LIMITED)
        _same(enc.RenderFramesYUV(2, 3, input=input, yuv="bt709-limited"), want, (input, "a range"))
        padded = tuple(np.full((3, s[1] + 2, s[2] + 3), 9, np.uint8)[:, :s[1], :s[2]] for s in yuv_out.plane_shapes("nv12", 3, h, w)[:2])
        _same(enc.RenderFramesYUV(2, 3, input=input, yuv="bt709-limited", device=False, out=padded), want, (input, "padded host planes"))
        assert all(bool((a.base[:, a.shape[1]:, :] == 9).all() and (a.base[:, :, a.shape[2]:] == 9).all()) for a in padded)
    # refusals as tm_render_frames, and the descriptor's
    for bad in ((-1, 1), (0, nf + 1), (nf, 1)):
        with pytest.raises(TileMotionError) as ei:
            enc.RenderFramesYUV(*bad)
        assert ei.value.code == E_INVAL
    small = tuple(np.full(s, 9, np.uint8) for s in yuv_out.plane_shapes("nv12", 2, h, w)[:2])
    for args, kw, code in (((0, 3), dict(out=small), E_INVAL), ((0, 2), dict(out=small, yuv=9), E_INVAL), ((0, 2), dict(out=small, yuv="tiler"), E_INVAL)):
        with pytest.raises(TileMotionError) as ei:
            enc.RenderFramesYUV(*args, device=False, **kw)
        assert ei.value.code == code
    assert all(bool((a == 9).all()) for a in small)
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.SetVideo(w, h, 24.0, nf)
    with pytest.raises(TileMotionError) as ei:  # nothing reconstructed or reloaded yet
        fresh.RenderFramesYUV()
    assert ei.value.code == E_INVAL
    fresh.ReloadGTM(path)
    _same(fresh.RenderFramesYUV(device=False), _want_planes(enc.RenderFrames(device=False), "nv12", BT601_LIMITED), "after ReloadGTM")
    with pytest.raises(TileMotionError) as ei:  # the source frames are not in memory
        fresh.RenderFramesYUV(input=True)
    assert ei.value.code == E_INVAL
    fresh.close()


# ---- 4. closure: a .gtm played to a Y4M file that Load reads
def test_play_gtm_y4m_is_read_back_by_load(encoded, tmp_path):
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    _, path = encoded
    rgb, info = _play_rgb(path)
    out = str(tmp_path / "played.y4m")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "play_gtm.py"), path, "--y4m", out, "--chroma", "444", "--yuv", "bt601-full"])
    head = open(out, "rb").readline()
    nf, h, w = rgb.shape
    assert head == b"YUV4MPEG2 W%d H%d F%d:1000000 Ip C444 XCOLORRANGE=FULL\n" % (w, h, round(info["fps"] * 1000000))
    assert os.path.getsize(out) == len(head) + nf * (len(b"FRAME\n") + 3 * w * h)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.InputFileName = out
    enc.Scaling = 1.0
    got = enc.OpenInput()
    assert (got["width"], got["height"], got["frames"]) == (w, h, nf) and got["fps"] == pytest.approx(info["fps"], abs=1e-6)
    enc.Run(S.esLoad)
    back = enc.RenderFrames(input=True, device=False)
    enc.close()
    worst = max(int(np.abs(((back >> s) & 255).astype(np.int64) - ((rgb >> s) & 255).astype(np.int64)).max()) for s in (16, 8, 0))
    print("worst channel error after .gtm -> y4m (bt601-full, 444) -> Load: %d" % worst)
    assert worst <= 1
