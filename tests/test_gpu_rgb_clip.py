"""Load takes RGB clips lent in memory (tm_set_frames_rgb, tm_stage_rgb_to_rgb32): packed, planar and 16-bit layouts, host or device,
Scaling honoured.  Everything is bit for bit: the stage seam against the numpy restatement (tests/rgb_clip_ref.py) and the host twin, the
encoder against the same frames lent as RGB32 with SetFramesDevice."""
import ctypes
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import rgb_clip_ref as ref, scale_ref
from tests.rgb_clip_ref import U8, U16_LOW
from tests.test_rgb_clip_host import FORMATS, IDS, host
from tests.test_gpu_yuv_clip import BASE
from tiler_amd import rgb_in, synth
from tiler_amd._lib import TileMotionError, lib
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S, TInputYUV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6
PATTERN = 0x5A5AA5A5


# ---- 1. the stage seam
def _stage(view, layout, samples, depth, dw, dh, flat=None, guard=4, tweak=None):
    """tm_stage_rgb_to_rgb32 of the numpy view's clip, moved to the device with everything around it, into a pattern-filled destination with
    guard bands, compared whole.  flat: the uint8 buffer the view lies in (default: the view's own bytes); the device tensor is exactly as
    long, so a clip that ends with its buffer ends with its allocation.  guard: int32 elements in front of the frames (4: the frames start
    on a 16-byte boundary, 5: 4 bytes past one, where the scalar stores run)"""
    import torch
    if flat is None:
        view = np.ascontiguousarray(view)
        flat = view.view(np.uint8).reshape(-1)
    clip = rgb_in.describe(view, layout, depth, samples)
    if tweak:
        tweak(clip)  # (a descriptor no layout name makes)
    dev = torch.from_numpy(np.array(flat)).cuda()
    delta = dev.data_ptr() - flat.ctypes.data
    clip.r, clip.g, clip.b, clip.memory = clip.r + delta, clip.g + delta, clip.b + delta, 1
    n = clip.frames
    buf = torch.full((guard + n * dh * dw + 4,), PATTERN, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[guard:guard + n * dh * dw]
    rc = lib().tm_stage_rgb_to_rgb32(ctypes.byref(clip), dw, dh, ctypes.c_void_p(out.data_ptr()), None)
    assert rc == 0, lib().tm_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:guard] == PATTERN).all() and (got[-4:] == PATTERN).all(), "a store outside the frames"
    return got[guard:-4].reshape(n, dh, dw)


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:3].tolist(), [hex(got[tuple(b)]) for b in bad[:3]], [hex(want[tuple(b)]) for b in bad[:3]])


def _half(w, h):
    return max(1, int(np.rint(w * 0.5))), max(1, int(np.rint(h * 0.5)))


@pytest.mark.parametrize("w,h", [(101, 53), (64, 48)])
def test_stage_matches_the_numpy_rule_and_the_host_twin(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    for (layout, samples, depth), name in zip(FORMATS, IDS):
        buf = ref.random_clip(rng, layout, 2, h, w, samples, depth)
        for i, (dw, dh) in enumerate(((w, h), _half(w, h), (150, 78))):
            want = ref.to_rgb32(buf, layout, samples, depth, dw, dh)
            _same(host(buf, layout, samples, depth, dw, dh), want, ("host", name, dw, dh))
            _same(_stage(buf, layout, samples, depth, dw, dh, guard=4 + (i + len(name)) % 2), want, (name, dw, dh))


@pytest.mark.parametrize("src,dst", [((264, 136), (33, 17)), ((264, 136), (528, 272)), ((40, 24), (5, 3))])
def test_stage_tile_heights_and_a_destination_narrower_than_a_tile(src, dst):
    """exactly 8 x (48 taps, 4 rows to a tile), 2 x (16 rows to a tile), and 5 x 3 pixels"""
    rng = np.random.default_rng(src[0] + dst[0])
    (w, h), (dw, dh) = src, dst
    for (layout, samples, depth), name in zip(FORMATS, IDS):
        buf = ref.random_clip(rng, layout, 2, h, w, samples, depth)
        _same(_stage(buf, layout, samples, depth, dw, dh), ref.to_rgb32(buf, layout, samples, depth, dw, dh), (name, src, dst))


def test_stage_scalar_store_path_and_hard_edges():
    """a destination 4 bytes past a 16-byte boundary at widths that are multiples of 4, and frames where the clamp bites"""
    w, h = 64, 48
    frames = scale_ref.edge_frames(2, h, w)
    for layout, samples, depth in (("rgb24", U8, 8), ("rgb48", U16_LOW, 16), ("gbrp", U16_LOW, 10)):
        buf = ref.pack(frames, layout, samples, depth)
        for dw, dh in ((64, 48), (32, 24), (96, 72)):
            want = frames & 0xffffff if (dw, dh) == (w, h) else scale_ref.scale(frames, dw, dh, "lanczos")
            for guard in (4, 5):
                _same(_stage(buf, layout, samples, depth, dw, dh, guard=guard), want, (layout, dw, dh, guard))


@pytest.mark.parametrize("pad", [2, 6])
def test_stage_padding_and_bits_outside_the_depth_are_ignored(pad):
    rng = np.random.default_rng(pad)
    w, h = 101, 53
    for (layout, samples, depth), name in zip(FORMATS, IDS):
        clean = ref.random_clip(rng, layout, 2, h, w, samples, depth)
        view, flat = ref.padded(ref.dirty(rng, clean, samples, depth), layout, pad, 3)
        for dw, dh in ((w, h), (76, 40)):
            _same(_stage(view, layout, samples, depth, dw, dh, flat=flat), ref.to_rgb32(clean, layout, samples, depth, dw, dh), (name, dw, dh))


def test_stage_odd_address_skipped_columns_and_equal_pointers():
    rng = np.random.default_rng(21)
    for layout in ("rgb24", "abgr", "gbrp", "gray"):
        clean = ref.random_clip(rng, layout, 2, 53, 101)
        view, flat = ref.padded(clean, layout, 0, 0, lead=1)
        for dw, dh in ((101, 53), (76, 40)):
            _same(_stage(view, layout, U8, 8, dw, dh, flat=flat), ref.to_rgb32(clean, layout, U8, 8, dw, dh), (layout, dw, dh))
    wide = ref.random_clip(rng, "rgb24", 2, 53, 202)
    for dw, dh in ((101, 53), (76, 40)):
        _same(_stage(wide[:, :, ::2], "rgb24", U8, 8, dw, dh, flat=wide.reshape(-1)), ref.to_rgb32(np.ascontiguousarray(wide[:, :, ::2]), "rgb24", U8, 8, dw, dh), (dw, dh))


def test_stage_interleaved_pixels_wider_than_two_granules():
    """24-byte pixels with R, G, B at bytes 0, 10 and 20 (and 5-word pixels with R, G, B at words 0, 2, 4): within one step of each other,
    but more than the pixel fetch spans -- every sample is loaded on its own"""
    rng = np.random.default_rng(24)
    w, h = 101, 53
    for dtype, nch, at, samples, depth in ((np.uint8, 24, (0, 10, 20), U8, 8), (np.uint16, 5, (0, 2, 4), U16_LOW, 12)):
        buf = rng.integers(0, 1 << depth, (2, h, w, nch)).astype(dtype)
        want_src = np.ascontiguousarray(buf[..., list(at)])

        def spread(clip):
            clip.g, clip.b = clip.r + at[1] * buf.itemsize, clip.r + at[2] * buf.itemsize
        for dw, dh in ((w, h), (76, 40)):
            got = _stage(buf[..., :3], "rgb24" if dtype == np.uint8 else "rgb48", samples, depth, dw, dh, flat=buf.view(np.uint8).reshape(-1), tweak=spread)
            _same(got, ref.to_rgb32(want_src, "rgb24" if dtype == np.uint8 else "rgb48", samples, depth, dw, dh), (nch, dw, dh))


def test_stage_a_clip_that_ends_with_its_allocation():
    """rgb24 at 101 x 53: the last described byte is the last byte of the tensor (the result must be right; that no load reaches past the
    samples' own granules is a property of fetch_rgb, checked by reading it)"""
    rng = np.random.default_rng(22)
    buf = ref.random_clip(rng, "rgb24", 2, 53, 101)
    assert buf.nbytes == 2 * 53 * 101 * 3 and buf.nbytes % 4 != 0
    for dw, dh in ((101, 53), (50, 26), (150, 78)):
        _same(_stage(buf, "rgb24", U8, 8, dw, dh), ref.to_rgb32(buf, "rgb24", U8, 8, dw, dh), (dw, dh))


def test_stage_refusals():
    import torch
    t = torch.zeros((2, 24, 40, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 24, 40), dtype=torch.int32, device="cuda")
    clip = rgb_in.describe(t, "rgb24")
    L = lib()
    assert L.tm_stage_rgb_to_rgb32(ctypes.byref(clip), 40, 24, None, None) == E_INVAL
    assert L.tm_stage_rgb_to_rgb32(ctypes.byref(clip), 4, 24, ctypes.c_void_p(out.data_ptr()), None) == E_UNSUPPORTED  # tenfold
    clip.memory = 0
    assert L.tm_stage_rgb_to_rgb32(ctypes.byref(clip), 40, 24, ctypes.c_void_p(out.data_ptr()), None) == E_INVAL
    clip.memory, clip.step = 1, 0
    assert L.tm_stage_rgb_to_rgb32(ctypes.byref(clip), 40, 24, ctypes.c_void_p(out.data_ptr()), None) == E_INVAL


def test_python_stage_wrapper():
    import torch
    from tiler_amd import stages
    rng = np.random.default_rng(23)
    buf = ref.random_clip(rng, "gbrp", 2, 24, 40, U16_LOW, 10)
    t = torch.from_numpy(buf.view(np.int16)).cuda()
    got = stages.rgb_to_rgb32(t, "gbrp", depth=10)
    _same(got.cpu().numpy().view(np.uint32), ref.unpack(buf, "gbrp", U16_LOW, 10), "unscaled")
    got = stages.rgb_to_rgb32(t, "gbrp", size=(60, 36), depth=10)
    _same(got.cpu().numpy().view(np.uint32), ref.to_rgb32(buf, "gbrp", U16_LOW, 10, 60, 36), "scaled")


# ---- 2. the encoder
W, H, NF, FPS = 96, 64, 5, 25.0
# (layout, samples, depth) of the encoder's cases: every one packs the same pixels, so one reference serves them all
LENT = [("rgb24", U8, 8), ("bgra", U8, 8), ("rgbp", U8, 8), ("gbrp", U16_LOW, 10), ("rgb48", U16_LOW, 16)]


@functools.lru_cache(maxsize=None)
def _frames():
    f = synth.video(NF, W, H, cut=3) & np.uint32(0xffffff)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _packed(layout, samples, depth):
    a = ref.pack(_frames(), layout, samples, depth, np.random.default_rng(depth))
    assert np.array_equal(ref.unpack(a, layout, samples, depth), _frames())
    a.setflags(write=False)
    return a


def _dst(scaling):
    return max(1, int(np.rint(W * scaling))), max(1, int(np.rint(H * scaling)))


@functools.lru_cache(maxsize=None)
def _want_frames(scaling):
    dw, dh = _dst(scaling)
    f = _frames() if (dw, dh) == (W, H) else scale_ref.scale(_frames(), dw, dh, "lanczos")
    f.setflags(write=False)
    return f


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
                source=enc.RenderFrames(input=True, device=False))


def _assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def _cropped(frames):
    h, w = frames.shape[-2:]
    return frames[:, :h // 8 * 8, :w // 8 * 8]


@functools.lru_cache(maxsize=None)
def _want_state(scaling, radius=0):
    """the reference, computed once per Scaling: the numpy rule's frames lent as RGB32 through SetFramesDevice"""
    import torch
    frames = _want_frames(scaling)
    dw, dh = _dst(scaling)
    enc = _encoder(MotionPredictRadius=radius)
    enc.SetVideo(dw, dh, FPS, NF)
    enc.SetFramesDevice(torch.from_numpy(np.array(frames).view(np.int32)).cuda())
    enc.Run()
    st = _state(enc)
    assert np.array_equal(st["source"], _cropped(frames))
    enc.close()
    return st


def _source(a, where):
    """the packed array as SetFramesRGB takes it: on the device, in pageable memory, in page-locked memory"""
    import torch
    if where == "pageable":
        return np.array(a)
    t = torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a))
    if where == "pinned":
        t = t.pin_memory()
        assert t.is_pinned()
        return t
    return t.cuda()


@pytest.mark.parametrize("scaling", [1.0, 0.5, 1.5])
@pytest.mark.parametrize("where", ["device", "pageable", "pinned"])
def test_lent_clip_encodes_as_the_reference_frames_do(monkeypatch, where, scaling):
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "2")  # 5 frames: three chunks, both ring slots, a short last chunk
    want = _want_state(scaling)
    dw, dh = _dst(scaling)
    for layout, samples, depth in LENT:
        enc = _encoder(Scaling=scaling)
        info = enc.SetFramesRGB(_source(_packed(layout, samples, depth), where), layout, fps=FPS, depth=depth, samples=samples)
        assert info == dict(width=dw, height=dh, fps=FPS, frames=NF)
        if where == "device" or layout == "rgb24":
            enc.Run()
            _assert_same(_state(enc), want)
        else:  # (the frames are the reference's: the steps behind Load have nothing else to read)
            enc.Run(S.esLoad)
            assert np.array_equal(enc.RenderFrames(input=True, device=False), want["source"]), (layout, where)
        enc.close()


def test_padded_views_in_host_memory(monkeypatch):
    """rows and frames with padding: the 2-D and the frame-by-frame copies of the staging; a view of every second column"""
    import torch
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "2")
    want = _want_state(1.0)["source"]
    # (rows 6 bytes longer keep their stride in the staging buffers, rows 40 bytes longer -- more than 1/16 -- are packed)
    for layout, samples, depth, pad in (("rgb24", U8, 8, 6), ("rgb24", U8, 8, 40), ("gbrp", U16_LOW, 10, 6), ("gbrp", U16_LOW, 10, 40)):
        for extra_rows in (0, 3):
            for pin in (False, True):
                view, flat = ref.padded(_packed(layout, samples, depth), layout, pad, extra_rows)
                if pin:
                    t = torch.from_numpy(flat).pin_memory()
                    flat2 = t.numpy()
                    view = np.ndarray(view.shape, view.dtype, buffer=flat2, strides=view.strides)
                enc = _encoder()
                enc.SetFramesRGB(view, layout, fps=FPS, depth=depth, samples=samples)
                enc.Run(S.esLoad)
                assert np.array_equal(enc.RenderFrames(input=True, device=False), want), (layout, extra_rows, pin)
                enc.close()
    wide = np.zeros((NF, H, 2 * W, 3), np.uint8)
    wide[:, :, ::2] = _packed("rgb24", U8, 8)
    wide[:, :, 1::2] = 0xEE
    enc = _encoder()
    enc.SetFramesRGB(wide[:, :, ::2], "rgb24", fps=FPS)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
    enc.close()


def test_life_cycle():
    import torch
    src = _source(_packed("bgra", U8, 8), "device")
    enc = _encoder()
    enc.SetFramesRGB(src, "bgra", fps=FPS)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _want_frames(1.0))
    keep = src.clone()
    src.fill_(7)  # the clip is the caller's again
    torch.cuda.synchronize()
    enc.Run(S.esLoad)  # a second Load reads the encoder's own clip
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _want_frames(1.0))
    enc.InputYUV = TInputYUV.yuvBT709Limited  # plays no part: nothing is refused
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _want_frames(1.0))
    src.copy_(keep)
    enc.Scaling = 0.5  # lent again at another Scaling
    assert enc.SetFramesRGB(src, "bgra", fps=FPS) == dict(width=48, height=32, fps=FPS, frames=NF)
    enc.Run()
    _assert_same(_state(enc), _want_state(0.5))
    # SetFramesDevice switches the source away: Scaling is ignored again, and the clip is read as RGB32
    other = torch.from_numpy(np.array(_want_frames(0.5)[::-1]).view(np.int32)).cuda()
    enc.SetFramesDevice(other)
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _want_frames(0.5)[::-1])
    enc.close()


def test_a_refused_clip_leaves_the_encoder_as_it_was():
    src = _source(_packed("rgb24", U8, 8), "device")
    enc = _encoder()
    info = enc.SetFramesRGB(src, "rgb24", fps=FPS)
    L = lib()

    def clip(**kw):
        c = rgb_in.describe(src[:2, :32, :48], "rgb24", fps=50.0)  # (another clip, were it taken)
        for k, val in kw.items():
            setattr(c, k, val)
        return c
    for bad in (clip(r=None), clip(b=None), clip(width=0), clip(height=65537), clip(frames=0), clip(fps=0.0), clip(samples=3), clip(memory=2), clip(depth=10),
                clip(samples=1, depth=8), clip(step=0), clip(row=47 * 3), clip(frame=-1), clip(samples=1, depth=10, step=7)):
        assert L.tm_set_frames_rgb(ctypes.c_void_p(enc._h), ctypes.byref(bad)) == E_INVAL
        assert enc.VideoInfo() == info
    assert L.tm_set_frames_rgb(ctypes.c_void_p(enc._h), None) == E_INVAL
    enc.Scaling = 0.05  # more than eightfold: refused like a file, and nothing is taken
    assert L.tm_set_frames_rgb(ctypes.c_void_p(enc._h), ctypes.byref(clip())) == E_UNSUPPORTED
    enc.Scaling = 1.0
    assert enc.VideoInfo() == info
    enc.Run(S.esLoad)  # the clip lent first is still the source
    assert np.array_equal(enc.RenderFrames(input=True, device=False), _want_frames(1.0))
    # host pointers called device memory are found out at Load
    host_clip = np.array(_packed("rgb24", U8, 8))
    c = rgb_in.describe(host_clip, "rgb24", fps=FPS)
    c.memory = 1
    assert L.tm_set_frames_rgb(ctypes.c_void_p(enc._h), ctypes.byref(c)) == 0
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esLoad)
    assert ei.value.code == E_INVAL and "not device memory" in str(ei.value)
    enc.close()


def test_with_motion_prediction():
    want = _want_state(1.0, 4)
    enc = _encoder(MotionPredictRadius=4)
    enc.SetFramesRGB(_source(_packed("rgb24", U8, 8), "device"), "rgb24", fps=FPS)
    enc.Run()
    _assert_same(_state(enc), want)
    enc.close()


# ---- 3. sharding
@pytest.mark.parametrize("where,scaling", [("device", 1.0), ("pageable", 0.5)])
def test_two_ranks_merge_to_the_single_run(monkeypatch, where, scaling):
    """two ranks (threads, one GPU, collectives through the callback) each convert the share of the clip their Load reads"""
    import torch
    from tests.test_gpu_encoder import _FakeDist
    from tiler_amd import distributed
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "2")
    want = _want_state(scaling)
    world = 2
    fake = _FakeDist(world)
    monkeypatch.setattr(distributed, "dist", fake)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            fake.local.rank = r
            torch.cuda.set_device(0)
            enc = _encoder(Scaling=scaling)
            enc.SetFramesRGB(_source(_packed("gbrp", U16_LOW, 10), where), "gbrp", fps=FPS, depth=10)
            distributed.run_all(enc, NF, r, world)
            hdr, pal, rgb = enc.Tiles()
            out[r] = dict(tilemaps=np.stack([enc.TileMap(f) for f in range(NF)]), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(), keyframes=enc.KeyFrames())
            enc.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            fake.bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    for r in range(world):
        for k in out[r]:
            assert np.array_equal(out[r][k], want[k]), (r, k)


@pytest.mark.parametrize("where", ["device", "pageable"])
def test_device_group_converts_the_lent_clip(monkeypatch, where):
    """two shards of one device: every shard's Load converts what it reads (the one whose device holds the clip in place, through group_each)"""
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "2")
    want = _want_state(0.5)
    grp = _encoder(devices=[0, 0], Scaling=0.5)
    grp.SetFramesRGB(_source(_packed("bgra", U8, 8), where), "bgra", fps=FPS)
    grp.Run()
    _assert_same(_state(grp), want)
    grp.close()


def test_two_devices_convert_the_lent_clip():
    """the clip lies on device 0: the shard on device 1 stages it across"""
    if lib().tm_device_count() < 2:
        pytest.skip("one device visible")
    want = _want_state(1.0)
    grp = TilingEncoder()
    grp.SetDeviceMask(0b11)
    grp.LoadDefaultSettings()
    for k, v in {**BASE, "MotionPredictRadius": 0}.items():
        setattr(grp, k, v)
    grp.SetFramesRGB(_source(_packed("rgb24", U8, 8), "device"), "rgb24", fps=FPS)
    grp.Run()
    _assert_same(_state(grp), want)
    grp.close()


# ---- 4. the tool
def test_encode_file_raw_rgb(tmp_path):
    from tiler_amd.player import GtmPlayer
    raw = tmp_path / "clip.rgb"
    raw.write_bytes(_packed("rgb24", U8, 8).tobytes() + b"\x00" * 100)  # (and the start of a frame cut short)
    out = tmp_path / "clip.gtm"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "encode_file.py"), str(raw), str(out), "--raw-rgb", "rgb24", "--size", "%dx%d" % (W, H),
                           "--fps", "25", "--start", "1", "--frames", "3"], stdout=subprocess.DEVNULL)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.SetFramesRGB(np.array(_packed("rgb24", U8, 8)[1:4]), "rgb24", fps=25.0)
    enc.Run()
    want = enc.RenderFrames(device=False)
    enc.close()
    with GtmPlayer(str(out)) as p:
        got = p.Read(device=False)
    assert got.shape == want.shape == (3, H, W) and np.array_equal(got, want)
