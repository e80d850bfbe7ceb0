"""Decoded frames at a caller's size: tm_stage_scale_rgb32 bit for bit the numpy restatement's (tests/scale_ref.py) and
the host twin's on every shape, stride and alignment, with nothing written outside the rows; the player's and the encoder's scaled reads
against their native reads pushed through the restatement; and a .gtm played to a scaled Y4M file that Load reads back."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import player_streams as ps  # noqa: E402
from tests import scale_ref as ref  # noqa: E402
from tests import yuv_out_ref  # noqa: E402
from tests.test_gpu_render import _encode, _pan_clip  # noqa: E402
from tests.test_gpu_yuv_out import _same  # noqa: E402
from tests.test_scale_host import _host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6
GUARD = 64  # pixels
PATTERN = 0x5A17C3E9

_cases = {}


def _case(src, dst, filter):
    """two frames of the shape (noise in all four bytes; hard 0 / 255 edges) and what the restatement makes of them; made once, read-only"""
    key = (src, dst, filter)
    if key not in _cases:
        (sw, sh), (dw, dh) = src, dst
        frames = np.concatenate([ref.random_frames(sw * 1000 + dw, 1, sh, sw), ref.edge_frames(2, sh, sw)[1:]])
        want = ref.scale(frames, dw, dh, filter)
        frames.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (frames, want)
    return _cases[key]


def _pattern(n, k):
    return ((np.arange(n, dtype=np.int64) * 2654435761 + k) & 0xFFFFFFFF).astype(np.uint32)


def _stage(frames, want, filter, src_pad=(0, 0), dst_pad=(0, 0), dst_shift=0):
    """the stage seam from and into pattern-filled buffers with a guard band of GUARD pixels before and after; *_pad: (pixels added to the row
    stride, pixels added to the frame stride); the destination starts dst_shift pixels past a 256-byte boundary + GUARD pixels.  The whole of
    both buffers is compared with what they must hold"""
    from tiler_amd import lib
    nf, sh, sw = frames.shape
    _, dh, dw = want.shape

    def lay(data, pad, shift, k):
        n, h, w = data.shape
        rs, fs = w + pad[0], (w + pad[0]) * h + pad[1]
        size = GUARD + shift + (n - 1) * fs + (h - 1) * rs + w + GUARD
        buf = _pattern(size, k)
        exp = buf.copy()
        for f in range(n):
            for r in range(h):
                at = GUARD + shift + f * fs + r * rs
                exp[at:at + w] = data[f, r]
        return buf, exp, rs, fs

    _, sexp, srs, sfs = lay(frames, src_pad, 0, 1)
    dbuf, dexp, drs, dfs = lay(want, dst_pad, dst_shift, 2)
    s = torch.from_numpy(sexp.view(np.int32)).cuda()
    d = torch.from_numpy(dbuf.view(np.int32)).cuda()
    assert s.data_ptr() % 256 == 0 and d.data_ptr() % 256 == 0
    L = lib()
    rc = L.tm_stage_scale_rgb32(ctypes.c_void_p(s.data_ptr() + 4 * GUARD), srs, sfs, nf, sw, sh, ctypes.c_void_p(d.data_ptr() + 4 * (GUARD + dst_shift)), drs, dfs, dw, dh,
                                ref.FILTERS[filter], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.tm_last_error()
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != dexp)
    assert len(bad) == 0, (filter, frames.shape, want.shape, src_pad, dst_pad, dst_shift, len(bad), [(int(b), hex(int(got[b])), hex(int(dexp[b]))) for b in bad[:6]])
    assert np.array_equal(s.cpu().numpy().view(np.uint32), sexp)


# ---- 1. the stage seam
@pytest.mark.parametrize("filter", ["lanczos", "nearest"])
@pytest.mark.parametrize("src,dst", ref.SHAPES)
def test_stage_is_the_restatement_and_the_host_twin_bit_for_bit(src, dst, filter):
    """a partial last tile in x (131, 199, 396), several tile heights (the 8 x shrink forces a short tile, the 2 x shrink the tallest), more
    than one tile row, a destination narrower than one tile (33, 5); dense buffers: 16-byte stores where the width is a multiple of 4"""
    frames, want = _case(src, dst, filter)
    for f in range(frames.shape[0]):
        assert np.array_equal(_host(frames[f], dst[0], dst[1], filter), want[f]), ("the host twin", f)
    _stage(frames, want, filter)


@pytest.mark.parametrize("filter", ["lanczos", "nearest"])
@pytest.mark.parametrize("src,dst", ref.SHAPES)
def test_stage_strides_and_alignment(src, dst, filter):
    """padded row strides and padded frame strides on both sides (multiples of 4 pixels: still 16-byte stores; odd ones: 4-byte stores), and a
    destination 4 bytes past a 16-byte boundary (the 4-byte store path with every stride a multiple of 4)"""
    frames, want = _case(src, dst, filter)
    _stage(frames, want, filter, src_pad=(3, 7), dst_pad=(4, 8))
    _stage(frames, want, filter, src_pad=(4, 0), dst_pad=(5, 3))
    _stage(frames, want, filter, dst_shift=1)
    _stage(frames, want, filter, src_pad=(1, 2), dst_pad=(4, 4), dst_shift=1)


def test_stage_python_wrapper_and_tile_heights():
    """stages.scale_rgb32 on tensors, with `out` and without; the tile heights the shapes take are 16, 8 and 4 (the tables' choice, restated:
    the largest th of 16, 8, 4, 2, 1 whose tiles reach at most 80 source rows)"""
    from tiler_amd import stages
    from tests import resample_ref

    def tile_height(n, m):
        t = resample_ref.taps(n, m, n, 1, 0.0)
        win = []
        for k0, c in t:
            nz = [i for i, v in enumerate(c) if v != 0]
            win.append((k0 + nz[0], k0 + nz[-1] + 1))
        for th in (16, 8, 4, 2, 1):
            if all(max(b for _, b in win[y:y + th]) - min(a for a, _ in win[y:y + th]) <= 80 for y in range(0, m, th)):
                return th
        return 0
    assert [tile_height(136, m) for m in (272, 68, 67, 17)] == [16, 16, 16, 4] and tile_height(24, 3) == 16 and tile_height(1088, 272) == 8
    frames, want = _case((264, 136), (131, 67), "lanczos")
    src = torch.from_numpy(frames.view(np.int32).copy()).cuda()
    assert np.array_equal(stages.scale_rgb32(src, (131, 67)).cpu().numpy().view(np.uint32), want)
    out = torch.full((2, 67 + 1, 131 + 2), 7, dtype=torch.int32, device="cuda")
    stages.scale_rgb32(src, (131, 67), out=out[:, :67, :131])
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :67, :131].view(np.uint32), want) and (o[:, 67:, :] == 7).all() and (o[:, :, 131:] == 7).all()
    big = torch.from_numpy(ref.random_frames(3, 1, 1088, 64).view(np.int32)).cuda()  # th = 8: a 4 x shrink in y
    assert np.array_equal(stages.scale_rgb32(big, (64, 272)).cpu().numpy().view(np.uint32), ref.scale(big.cpu().numpy().view(np.uint32), 64, 272))
    nearest = stages.scale_rgb32(src, (32, 16), filter="nearest")  # beyond 8: the gather has no limit
    assert np.array_equal(nearest.cpu().numpy().view(np.uint32), ref.scale(frames, 32, 16, "nearest"))


def test_stage_refusals_leave_the_destination_alone():
    from tiler_amd import lib
    L = lib()
    src = torch.zeros((2, 24, 40), dtype=torch.int32, device="cuda")
    dst = torch.full((2 * 60 * 100 + 64,), 0x1234567, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp, dp = src.data_ptr(), dst.data_ptr()

    def call(s=sp, srs=40, sfs=960, nf=2, sw=40, sh=24, d=dp, drs=100, dfs=6000, dw=100, dh=60, flt=ref.LANCZOS3):
        return L.tm_stage_scale_rgb32(ctypes.c_void_p(s), srs, sfs, nf, sw, sh, ctypes.c_void_p(d), drs, dfs, dw, dh, flt, stream)
    assert call(dw=0) == E_INVAL and call(sh=0) == E_INVAL and call(dh=-3) == E_INVAL
    assert call(flt=2) == E_INVAL
    assert call(s=0) == E_INVAL and call(d=0) == E_INVAL
    assert call(srs=39) == E_INVAL and call(drs=99) == E_INVAL
    assert call(dfs=5999) == E_INVAL and call(sfs=900) == E_INVAL
    assert call(s=dp, srs=100, sfs=6000, sw=100, sh=30, d=dp + 4 * 100 * 29, dw=100, dh=30, nf=1) == E_INVAL and b"overlap" in L.tm_last_error()
    assert call(dw=4, drs=4) == E_UNSUPPORTED and call(dh=2) == E_UNSUPPORTED
    assert call(dw=32769, drs=32769, flt=ref.NEAREST) == E_UNSUPPORTED
    assert call(dw=4, drs=4, dh=2, dfs=8, flt=ref.NEAREST) == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[16:] == 0x1234567).all() and (got[:16] == 0).all()  # the accepted nearest call wrote its 2 x 2 x 4 pixels, the refused ones nothing


# ---- 2. the player
PLAYER_SIZES = {"33x17": [(528, 272, "nearest"), (396, 204, "lanczos"), (132, 68, "lanczos"), (33, 17, "lanczos")],
                "5x3": [(80, 48, "nearest"), (60, 36, "lanczos"), (20, 12, "lanczos"), (5, 3, "lanczos")]}


def _made(which, tmp_path):
    L = ps.write_lib()
    path = tmp_path / "made.gtm"
    if which == "5x3":
        ps.write_stream(L, path, 5, 3, 64, nframes=12, kf=(0, 4, 8), mode="border", n_shared=48)
    else:
        ps.write_stream(L, path, 33, 17, 64, nframes=6, kf=(0, 3), mode="border")
    return str(path)


def _read_all(p, step, device, shape):
    """all frames from the start, `step` at a time (None: in one call); device reads go into ONE buffer of the caller's that is overwritten
    between the calls"""
    p.Seek(0)
    n = p.info()["frames"]
    parts = []
    buf = torch.empty((step or n,) + shape, dtype=torch.int32, device="cuda") if device else None
    while p.Tell() < n:
        at = p.Tell()
        if device:
            got = p.Read(step, out=buf).cpu().numpy().view(np.uint32).copy()
            buf.fill_(0x00C0FFEE)
            torch.cuda.synchronize()
        else:
            got = p.Read(step, device=False)
        assert got.shape == (min(step or n, n - at),) + shape and p.Tell() == at + got.shape[0]
        parts.append(got)
    assert p.Read(2, device=device).shape == (0,) + shape
    return np.concatenate(parts)


@pytest.mark.parametrize("which", ["5x3", "33x17"])
def test_player_scaled_read_equals_the_native_read_scaled(which, tmp_path, monkeypatch):
    from tiler_amd.player import GtmPlayer
    monkeypatch.setenv("TM_PLAYER_CHUNK_FRAMES", "2")  # the rings are reused several times over
    path = _made(which, tmp_path)
    with GtmPlayer(path) as p:
        i = p.info()
        native = p.Read(device=False)
        nshape = (i["tm_h"] * 8, i["tm_w"] * 8)
        assert p.Output() == (0, 0, "lanczos")
        for w, h, flt in PLAYER_SIZES[which]:
            want = ref.scale(native, w, h, flt)
            p.SetOutput(w, h, flt)
            assert p.Output() == (w, h, flt)
            assert (p.info()["width"], p.info()["height"]) == (i["width"], i["height"])  # the stream's size, as before
            for step in (1, 3, None):
                for device in (True, False):
                    assert np.array_equal(_read_all(p, step, device, (h, w)), want), (which, w, h, flt, step, device)
        p.SetOutput(0, 0)
        assert p.Output() == (0, 0, "lanczos")
        assert np.array_equal(_read_all(p, 3, True, nshape), native) and np.array_equal(_read_all(p, None, False, nshape), native)


def test_player_scaled_seek_yuv_and_refusals(tmp_path, monkeypatch):
    from tiler_amd._lib import TileMotionError
    from tiler_amd.player import GtmPlayer
    from tiler_amd import yuv_out
    monkeypatch.setenv("TM_PLAYER_CHUNK_FRAMES", "2")
    path = _made("5x3", tmp_path)
    with GtmPlayer(path) as p:
        native = p.Read(device=False)
        n = native.shape[0]
        p.SetOutput(60, 36)
        want = ref.scale(native, 60, 36)
        # a seek into the middle of a key frame's group (key frames at 0, 4, 8): the catching up is native, the read scaled
        for device in (True, False):
            p.Seek(6)
            got = p.Read(4, device=device)
            got = got.cpu().numpy().view(np.uint32) if device else got
            assert np.array_equal(got, want[6:10]) and p.Tell() == 10
        # YUV at the output size: the scaled frames through the YUV restatement
        for layout, mode, deep in (("nv12", yuv_out_ref.BT601_LIMITED, False), ("420jpeg", yuv_out_ref.BT709_FULL, False), ("p010", yuv_out_ref.BT709_LIMITED, True)):
            planes = yuv_out_ref.planes(want, layout, mode)
            for device in (True, False):
                for step in (3, None):
                    p.Seek(0)
                    parts = []
                    while p.Tell() < n:
                        parts.append(tuple(None if a is None else (a.cpu().numpy() if device else a.copy()) for a in p.ReadYUV(step, layout=layout, yuv=mode, device=device)))
                    got = tuple(None if parts[0][k] is None else np.concatenate([q[k] for q in parts]) for k in range(3))
                    _same(got, planes, (layout, device, step))
        # a destination of the native size while an output size is set: refused, position and destination untouched
        p.Seek(5)
        for device in (True, False):
            small = tuple(torch.full(s, 55, dtype=torch.uint8, device="cuda") if device else np.full(s, 55, np.uint8) for s in yuv_out.plane_shapes("nv12", 2, 24, 40)[:2])
            with pytest.raises(TileMotionError) as ei:
                p.ReadYUV(2, device=device, out=small)
            assert ei.value.code == E_INVAL and p.Tell() == 5
            if device:
                torch.cuda.synchronize()
            assert all(bool((a == 55).all()) for a in small)
        # a refused SetOutput leaves the previous setting
        for args, code in (((4, 36), E_UNSUPPORTED), ((60, 2), E_UNSUPPORTED), ((0, 36), E_INVAL), ((60, -1), E_INVAL), ((60, 36, 5), E_INVAL), ((40000, 36, "nearest"), E_UNSUPPORTED)):
            with pytest.raises(TileMotionError) as ei:
                p.SetOutput(*args)
            assert ei.value.code == code and p.Output() == (60, 36, "lanczos") and p.Tell() == 5
        assert np.array_equal(p.Read(2, device=False), want[5:7])
        p.SetOutput(4, 2, "nearest")  # beyond 8 with the gather
        p.Seek(0)
        assert np.array_equal(p.Read(device=False), ref.scale(native, 4, 2, "nearest"))


def test_player_scaled_memory_does_not_grow_with_the_clip(tmp_path):
    """200 frames at 64 x 48 against the same stream cut to 20, read at 96 x 72 to device, host and YUV: the same allocation"""
    from tiler_amd.player import GtmPlayer
    L = ps.write_lib()
    kf20 = (0, 10)
    tm20 = ps.tilemaps(8, 6, 20, kf20, "border", n_shared=48)
    used = {}
    for name, reps in (("short", 1), ("long", 10)):
        path = tmp_path / (name + ".gtm")
        ps.write_arrays(L, path, 8, 6, 16, np.tile(tm20, (reps, 1)), [f + 20 * r for r in range(reps) for f in kf20], n_shared=48)
        with GtmPlayer(path) as p:
            before = p.info()["device_bytes"]
            p.SetOutput(96, 72)
            n = k = 0
            while True:
                r = p.Read(7, device=(k % 3 == 0)) if k % 3 < 2 else p.ReadYUV(7)[0]
                k += 1
                if r.shape[0] == 0:
                    break
                assert tuple(r.shape[1:]) == (72, 96)
                n += r.shape[0]
            assert n == 20 * reps
            used[name] = p.info()["device_bytes"]
            assert used[name] > before  # the tables and the rings are counted
    assert used["long"] == used["short"]


# ---- 3. the encoder's render
@pytest.fixture(scope="module")
def pan():
    """the 40-frame pan of tests/test_gpu_render.py (64 x 48, one key frame, long prediction chains): 40 frames cross the 32-frame chunk"""
    enc = _encode(_pan_clip(40, 64, 48, 4), PaletteCount=3, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False, ShotTransMaxSecondsPerKF=1000.0,
                  ShotTransMinSecondsPerKF=1000.0)
    yield enc
    enc.close()


def test_render_frames_scaled_equals_the_render_scaled(pan):
    from tiler_amd._lib import TileMotionError
    enc = pan
    nf = enc.counts()["frames"]
    assert nf == 40 and ((enc.TileMaps()["Flags"] >> 2) & 1)[17:22].any()
    for input in (False, True):
        native = enc.RenderFrames(input=input, device=False)
        for (w, h), flt in (((96, 72), "lanczos"), ((31, 23), "lanczos"), ((128, 96), "nearest")):
            want = ref.scale(native, w, h, flt)
            got = enc.RenderFrames(input=input, size=(w, h), filter=flt)  # the whole 40 frames
            assert got.shape == (nf, h, w) and np.array_equal(got.cpu().numpy().view(np.uint32), want), (input, w, h, flt)
            assert np.array_equal(enc.RenderFrames(input=input, size=(w, h), filter=flt, device=False), want)
            part = enc.RenderFrames(17, 5, input=input, size=(w, h), filter=flt, device=False)  # starts inside the key frame's group
            assert np.array_equal(part, want[17:22])
        assert enc.RenderFrames(3, 0, input=input, size=(96, 72)).shape == (0, 72, 96)
    # YUV of the scaled frames
    native = enc.RenderFrames(device=False)
    want = yuv_out_ref.planes(ref.scale(native, 96, 72), "nv12", yuv_out_ref.BT601_LIMITED)
    for device in (True, False):
        _same(enc.RenderFramesYUV(layout="nv12", size=(96, 72), device=device), want, ("nv12", device))
    _same(enc.RenderFramesYUV(17, 5, layout="nv12", size=(96, 72)), tuple(None if a is None else a[17:22] for a in want), "a range")
    # refusals: the range, the size pair, the filter -- nothing is written
    out = np.full((2, 72, 96), 9, np.uint32)
    from tiler_amd._lib import check, c_void_p

    def raw(first, count, w, h, flt):
        check(enc._L.tm_render_frames_scaled(c_void_p(enc._h), first, count, 0, w, h, flt, out.ctypes.data_as(c_void_p), 0))
    for args, code in (((-1, 1, 96, 72, 0), E_INVAL), ((39, 2, 96, 72, 0), E_INVAL), ((0, 2, 7, 72, 0), E_UNSUPPORTED), ((0, 2, 96, 5, 0), E_UNSUPPORTED),
                       ((0, 2, 0, 72, 0), E_INVAL), ((0, 2, 96, 72, 3), E_INVAL), ((0, 2, 96, 40000, 1), E_UNSUPPORTED)):
        with pytest.raises(TileMotionError) as ei:
            raw(*args)
        assert ei.value.code == code, args
    assert (out == 9).all()
    for kw, code in ((dict(first=40, count=1, size=(96, 72)), E_INVAL), (dict(size=(7, 72)), E_UNSUPPORTED), (dict(size=(96, 72), filter=4), E_INVAL)):
        with pytest.raises(TileMotionError) as ei:
            enc.RenderFramesYUV(**kw)
        assert ei.value.code == code, kw


# ---- 4. the tool: a .gtm played to a scaled Y4M file that Load reads
def test_play_gtm_scaled_y4m_is_read_back_by_load(tmp_path):
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    from tiler_amd.player import GtmPlayer
    path = _made("33x17", tmp_path)
    with GtmPlayer(path) as p:
        native, info = p.Read(device=False), p.info()
    out = str(tmp_path / "played.y4m")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "play_gtm.py"), path, "--y4m", out, "--size", "132x68", "--chroma", "444", "--yuv", "bt601-full"])
    head = open(out, "rb").readline()
    nf, w, h = native.shape[0], 132, 68
    assert head == b"YUV4MPEG2 W%d H%d F%d:1000000 Ip C444 XCOLORRANGE=FULL\n" % (w, h, round(info["fps"] * 1000000))
    assert os.path.getsize(out) == len(head) + nf * (len(b"FRAME\n") + 3 * w * h)
    # the file's planes are the scaled frames' (444: one sample per pixel)
    want = yuv_out_ref.planes(ref.scale(native, w, h), "444", yuv_out_ref.BT601_FULL)
    data = np.frombuffer(open(out, "rb").read()[len(head):], np.uint8).reshape(nf, 6 + 3 * w * h)[:, 6:].reshape(nf, 3, h, w)
    assert all(np.array_equal(data[:, k], want[k]) for k in range(3))
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.InputFileName = out
    enc.Scaling = 1.0
    got = enc.OpenInput()
    assert (got["width"], got["height"], got["frames"]) == (w, h, nf)
    enc.Run(S.esLoad)
    back = enc.RenderFrames(input=True, device=False)
    enc.close()
    scaled = ref.scale(native, w, h)
    back = back[:, :h, :w]  # (Load fills up to whole tiles: 136 x 72)
    worst = max(int(np.abs(((back >> s) & 255).astype(np.int64) - ((scaled >> s) & 255).astype(np.int64)).max()) for s in (16, 8, 0))
    print("worst channel error after .gtm -> scaled y4m (bt601-full, 444) -> Load: %d" % worst)
    assert worst <= 1  # the YUV round trip's bound, as tests/test_gpu_yuv_out.py has it for the unscaled file
