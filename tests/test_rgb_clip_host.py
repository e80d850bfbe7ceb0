"""An RGB clip lent in memory, the host side (no GPU): the host twin tm_rgb_to_rgb32_host against the numpy restatement
(tests/rgb_clip_ref.py: the unpack, then scale_ref's Lanczos rule), bit for bit, over every layout; junk around the samples; strides; and
the checks of tm_set_frames_rgb through their host-only seam tm_probe_rgb_clip_host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import rgb_clip_ref as ref, scale_ref
from tests.rgb_clip_ref import U8, U16_LOW, U16_HIGH
from tiler_amd import rgb_in
from tiler_amd._lib import lib, RgbClip, YuvClip, TileMotionError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6
HOST, DEVICE = 0, 1

# (layout, samples, depth): each of the 10 packed layouts; rgbp and gbrp at 8, 10 (LOW), 12 (LOW) and 16 (HIGH) bits; gray at 8 and 16
FORMATS = ([(l, U8, 8) for l in ref.PACKED8] + [(l, U16_LOW, 16) for l in ref.PACKED16]
           + [(l, s, d) for l in ("rgbp", "gbrp") for s, d in ((U8, 8), (U16_LOW, 10), (U16_LOW, 12), (U16_HIGH, 16))] + [("gray", U8, 8), ("gray", U16_HIGH, 16)])
IDS = ["%s-%d%s" % (l, d, {U8: "", U16_LOW: "low", U16_HIGH: "high"}[s]) for l, s, d in FORMATS]
# source (w, h) -> destination (w, h): itself, shrunk, enlarged; exactly 8 x (48 taps); narrower than a tile
SIZES = [((101, 53), (101, 53)), ((101, 53), (76, 40)), ((101, 53), (150, 78)), ((264, 136), (33, 17)), ((40, 24), (5, 3))]


def host(buf, layout, samples, depth, dw, dh, first=0, count=None, clip=None):
    """tm_rgb_to_rgb32_host of the array as rgb_in.describe sees it (or of `clip`, a descriptor made by hand)"""
    clip = clip or rgb_in.describe(buf, layout, depth, samples)
    count = clip.frames - first if count is None else count
    out = np.full((count, dh, dw), 0xDEADBEEF, np.uint32)
    rc = lib().tm_rgb_to_rgb32_host(ctypes.byref(clip), first, count, dw, dh, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, lib().tm_last_error()
    return out


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:3].tolist(), [hex(got[tuple(b)]) for b in bad[:3]], [hex(want[tuple(b)]) for b in bad[:3]])


# ---- 1. the host twin against the reference
@pytest.mark.parametrize("layout,samples,depth", FORMATS, ids=IDS)
def test_host_twin_matches_the_numpy_rule_bit_for_bit(layout, samples, depth):
    rng = np.random.default_rng(len(layout) * 100 + depth)
    for (w, h), (dw, dh) in SIZES:
        buf = ref.random_clip(rng, layout, 2, h, w, samples, depth)
        _same(host(buf, layout, samples, depth, dw, dh), ref.to_rgb32(buf, layout, samples, depth, dw, dh), (layout, (w, h), (dw, dh)))


@pytest.mark.parametrize("layout,samples,depth", [("rgb24", U8, 8), ("rgb48", U16_LOW, 16)])
def test_hard_edges_where_the_clamp_bites(layout, samples, depth):
    w, h = 101, 53
    frames = scale_ref.edge_frames(2, h, w)
    buf = ref.pack(frames, layout, samples, depth)
    assert np.array_equal(ref.unpack(buf, layout, samples, depth), frames & 0xffffff)
    for dw, dh in ((76, 40), (150, 78)):
        want = scale_ref.scale(frames, dw, dh, "lanczos")
        assert (want & 0xff).min() == 0 and (want & 0xff).max() == 255
        _same(host(buf, layout, samples, depth, dw, dh), want, (layout, dw, dh))


def test_a_range_of_frames():
    rng = np.random.default_rng(3)
    buf = ref.random_clip(rng, "bgra", 5, 9, 7)
    want = ref.unpack(buf, "bgra")
    _same(host(buf, "bgra", U8, 8, 7, 9, first=1, count=3), want[1:4], "frames 1..3")
    assert host(buf, "bgra", U8, 8, 7, 9, first=5, count=0).shape == (0, 9, 7)
    clip = rgb_in.describe(buf, "bgra")
    out = np.zeros((2, 9, 7), np.uint32)
    assert lib().tm_rgb_to_rgb32_host(ctypes.byref(clip), 4, 2, 7, 9, out.ctypes.data_as(ctypes.c_void_p)) == E_INVAL


# ---- 2. junk around the samples is ignored
@pytest.mark.parametrize("pad", [2, 6])
def test_padding_and_bits_outside_the_depth_are_ignored(pad):
    rng = np.random.default_rng(pad)
    w, h = 101, 53
    for layout, samples, depth in FORMATS:
        clean = ref.random_clip(rng, layout, 2, h, w, samples, depth)
        view, _ = ref.padded(ref.dirty(rng, clean, samples, depth), layout, pad, 3)
        assert view.strides != clean.strides
        for dw, dh in ((w, h), (76, 40)):
            _same(host(view, layout, samples, depth, dw, dh), ref.to_rgb32(clean, layout, samples, depth, dw, dh), (layout, depth, dw, dh))


@pytest.mark.parametrize("layout", ["rgb24", "abgr", "gbrp", "gray"])
def test_a_clip_at_an_odd_address(layout):
    rng = np.random.default_rng(11)
    clean = ref.random_clip(rng, layout, 2, 53, 101)
    view, _ = ref.padded(clean, layout, 0, 0, lead=1)
    assert view.ctypes.data % 2 == 1
    for dw, dh in ((101, 53), (76, 40)):
        _same(host(view, layout, U8, 8, dw, dh), ref.to_rgb32(clean, layout, U8, 8, dw, dh), (layout, dw, dh))


# ---- 3. strides
def test_every_second_column_of_an_rgb24_clip():
    rng = np.random.default_rng(5)
    buf = ref.random_clip(rng, "rgb24", 2, 53, 202)
    view = buf[:, :, ::2]
    clip = rgb_in.describe(view, "rgb24")
    assert (clip.step, clip.row, clip.width) == (6, 606, 101)
    for dw, dh in ((101, 53), (76, 40)):
        _same(host(view, "rgb24", U8, 8, dw, dh), ref.to_rgb32(np.ascontiguousarray(view), "rgb24", U8, 8, dw, dh), (dw, dh))


def test_a_bottom_up_view_is_refused_by_the_python_side():
    buf = ref.random_clip(np.random.default_rng(6), "rgb24", 2, 8, 8)
    for view in (buf[:, ::-1], buf[::-1], buf[:, :, ::-1], buf[..., ::-1]):
        with pytest.raises(TileMotionError) as ei:
            rgb_in.describe(view, "rgb24")
        assert ei.value.code == E_INVAL and "negative stride" in str(ei.value)


def test_three_equal_pointers_are_grey():
    rng = np.random.default_rng(7)
    buf = ref.random_clip(rng, "rgb24", 2, 53, 101)
    clip = rgb_in.describe(buf, "rgb24")
    clip.g = clip.b = clip.r
    for dw, dh in ((101, 53), (150, 78)):
        _same(host(None, None, None, None, dw, dh, clip=clip), ref.to_rgb32(np.ascontiguousarray(buf[..., 0]), "gray", U8, 8, dw, dh), (dw, dh))


def test_layouts_of_the_python_side_follow_the_reference():
    assert set(rgb_in.LAYOUTS) == set(ref.PACKED) | set(ref.PLANAR) | {"gray"}
    rng = np.random.default_rng(8)
    for layout in rgb_in.LAYOUTS:
        item = 2 if layout in ref.PACKED16 else 1
        buf = ref.random_clip(rng, layout, 1, 3, 5, U8 if item == 1 else U16_LOW, 8 * item)
        clip = rgb_in.describe(buf, layout)
        got = [int(np.frombuffer(ctypes.string_at(p, item), buf.dtype)[0]) for p in (clip.r, clip.g, clip.b)]
        assert got == [int(c[0, 0, 0]) for c in ref.channels(buf, layout)], layout
    with pytest.raises(ValueError):
        rgb_in.describe(np.zeros((1, 3, 5, 3), np.uint16), "rgb24")
    with pytest.raises(ValueError):
        rgb_in.describe(np.zeros((1, 3, 5), np.uint8), "rgb24")
    with pytest.raises(ValueError):
        rgb_in.describe(np.zeros((1, 3, 5, 3), np.uint8), "yuv")


# ---- 4. the struct
def test_struct_layout_is_the_documented_one(tmp_path):
    want = dict(r=0, g=8, b=16, step=24, row=32, frame=40, width=48, height=52, frames=56, fps=64, samples=72, depth=76, memory=80)
    assert ctypes.sizeof(RgbClip) == 88
    assert {n: getattr(RgbClip, n).offset for n, _ in RgbClip._fields_} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tilemotion.h"\nint main(void) {\n  printf("%zu", sizeof(tm_rgb_clip));\n'
                   + "".join('  printf(" %%zu", offsetof(tm_rgb_clip, %s));\n' % n for n in want) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(t) for t in subprocess.check_output([str(exe)], text=True).split()] == [88] + list(want.values())


# ---- 5. the probe: every refusal, with no device
BUF = (ctypes.c_uint8 * 64)()  # somewhere for the pointers to point: nothing is read through them
ADDR = ctypes.addressof(BUF)


def good(samples=U8, depth=8, w=100, h=52, memory=HOST):
    B = 1 if samples == U8 else 2
    c = RgbClip()
    c.r, c.g, c.b = ADDR, ADDR + B, ADDR + 2 * B
    c.step, c.row, c.frame = 3 * B, 3 * B * w, 3 * B * w * h
    c.width, c.height, c.frames, c.fps = w, h, 3, 25.0
    c.samples, c.depth, c.memory = samples, depth, memory
    return c


def probe(c, scaling=1.0):
    w, h = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib().tm_probe_rgb_clip_host(ctypes.byref(c) if c is not None else None, scaling, ctypes.byref(w), ctypes.byref(h))
    return rc, w.value, h.value, lib().tm_last_error().decode()


def _set(c, **kw):
    for k, v in kw.items():
        setattr(c, k, v)
    return c


REFUSED = [
    ("null struct", lambda: None, "null descriptor"),
    ("null r", lambda: _set(good(), r=None), "null r channel"),
    ("null g", lambda: _set(good(), g=None), "null g channel"),
    ("null b", lambda: _set(good(), b=None), "null b channel"),
    ("width 0", lambda: _set(good(), width=0), "size"),
    ("width 65537", lambda: _set(good(), width=65537, row=3 * 65537), "size"),
    ("height 0", lambda: _set(good(), height=0), "size"),
    ("height 65537", lambda: _set(good(), height=65537), "size"),
    ("frames 0", lambda: _set(good(), frames=0), "frames"),
    ("fps 0", lambda: _set(good(), fps=0.0), "frame rate"),
    ("fps nan", lambda: _set(good(), fps=float("nan")), "frame rate"),
    ("samples 3", lambda: _set(good(), samples=3), "sample format 3"),
    ("samples -1", lambda: _set(good(), samples=-1), "sample format -1"),
    ("memory 2", lambda: _set(good(), memory=2), "memory kind 2"),
    ("depth 10 with bytes", lambda: _set(good(), depth=10), "depth 10"),
    ("depth 8 with words", lambda: good(samples=U16_LOW, depth=8), "depth 8"),
    ("depth 17 with words", lambda: good(samples=U16_HIGH, depth=17), "depth 17"),
    ("step 0", lambda: _set(good(), step=0), "step 0"),
    ("step 1 with words", lambda: _set(good(samples=U16_LOW, depth=10), step=1), "step 1"),
    ("negative step", lambda: _set(good(), step=-3), "step -3"),
    ("row one short", lambda: _set(good(), row=99 * 3), "row stride 297"),
    ("row one short, words", lambda: _set(good(samples=U16_LOW, depth=10), row=99 * 6 + 1), "row stride 595"),
    ("negative row", lambda: _set(good(), row=-300), "row stride -300"),
    ("negative frame", lambda: _set(good(), frame=-1), "negative frame stride"),
    ("odd r pointer, words", lambda: _set(good(samples=U16_LOW, depth=10), r=ADDR + 1), "odd pointer"),
    ("odd b pointer, words", lambda: _set(good(samples=U16_HIGH, depth=12), b=ADDR + 5), "odd pointer"),
    ("odd step, words", lambda: _set(good(samples=U16_LOW, depth=10), step=7, row=7 * 100), "odd pointer, step"),
    ("odd row, words", lambda: _set(good(samples=U16_LOW, depth=10), row=601), "odd pointer, step or stride"),
    ("odd frame, words", lambda: _set(good(samples=U16_LOW, depth=10), frame=600 * 52 + 1), "odd pointer, step or stride"),
]


@pytest.mark.parametrize("name,make,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_bad_clips_are_refused_with_no_device(name, make, word):
    rc, w, h, msg = probe(make())
    assert rc == E_INVAL and word in msg, (name, rc, msg)
    assert (w, h) == (-1, -1)
    L = lib()
    L.tm_set_frames_rgb.restype, L.tm_set_frames_rgb.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RgbClip)]
    c = make()
    assert L.tm_set_frames_rgb(None, ctypes.byref(c) if c is not None else None) == E_INVAL  # (no encoder without a device: TM_E_INVAL too)


def _yuv444(w, h):
    c = YuvClip()
    c.y, c.u, c.v = ADDR, ADDR + 16, ADDR + 32
    c.y_row = c.u_row = c.v_row = w
    c.y_frame = c.u_frame = c.v_frame = w * h
    c.width, c.height, c.frames, c.fps, c.chroma, c.samples, c.depth = w, h, 3, 25.0, 0, 0, 8
    return c


def test_good_clips_get_the_size_a_yuv_clip_would():
    for samples, depth in ((U8, 8), (U16_LOW, 9), (U16_LOW, 10), (U16_HIGH, 16)):
        for memory in (HOST, DEVICE):
            assert probe(good(samples, depth, memory=memory))[:3] == (0, 100, 52)
    for w, h in ((100, 52), (101, 53), (5, 3), (65536, 1)):
        for scaling in (1.0, 0.5, 1.5, 0.124):
            yw, yh = ctypes.c_int(-1), ctypes.c_int(-1)
            yrc = lib().tm_probe_yuv_clip_host(ctypes.byref(_yuv444(w, h)), scaling, ctypes.byref(yw), ctypes.byref(yh))
            rc, dw, dh, msg = probe(good(w=w, h=h), scaling)
            assert (rc, dw, dh) == (yrc, yw.value, yh.value), (w, h, scaling)
            if scaling == 0.124 and (w, h) == (100, 52):  # 12 x 6: 8.33-fold and 8.67-fold
                assert rc == E_UNSUPPORTED and "more than 8" in msg
    assert probe(good(w=101, h=53), 0.5)[:3] == (0, 50, 26)  # Round: half to even
    c = good()
    c.frame = 0                                              # frames may overlap (a still)
    c.row += 5; c.step = 3
    assert probe(c)[0] == 0
    assert probe(_set(good(w=1, h=1), row=1, step=1 << 40))[0] == 0   # one pixel: the step reaches nothing
    assert probe(_set(good(), step=1 << 61, row=(1 << 62)))[0] == E_INVAL  # (width - 1) x step is never multiplied out
