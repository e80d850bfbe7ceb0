"""A YUV clip lent in memory, the host side (no GPU): the depth rule and the BT.709 rules of the numpy restatement against their
description, and the checks of tm_set_frames_yuv through its host-only seam tm_probe_yuv_clip_host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import yuv_clip_ref as ref
from tests.yuv_clip_ref import U8, U16_LOW, U16_HIGH, BT709_LIMITED, BT709_FULL
from tiler_amd._lib import lib, YuvClip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6
C444, C422, C420JPEG, C420MPEG2, MONO = range(5)
HOST, DEVICE = 0, 1


# ---- 1. the depth rule
@pytest.mark.parametrize("depth", [9, 10, 12, 14, 16])
@pytest.mark.parametrize("samples", [U16_LOW, U16_HIGH])
def test_narrowing_over_every_value(samples, depth):
    vals = np.arange(1 << depth, dtype=np.int64)
    words = vals if samples == U16_LOW else vals << (16 - depth)
    got = ref.narrow(words.astype(np.uint16), samples, depth).astype(np.int64)
    assert got[0] == 0 and got[-1] == 255
    assert np.all(np.diff(got) >= 0)
    assert np.array_equal(got, np.minimum(255, (vals + (1 << (depth - 9))) >> (depth - 8)))  # the rule as written, on the sample itself
    if depth == 10:
        assert got[64] == 16 and got[940] == 235
    # the bits outside the depth have no effect: every pattern of them (a sample of the patterns for the shallow depths)
    spare = 16 - depth
    if spare:
        rng = np.random.default_rng(depth)
        for junk in {0, (1 << spare) - 1, *rng.integers(0, 1 << spare, 6).tolist()}:
            dirty = words | (junk << depth) if samples == U16_LOW else words | junk
            assert np.array_equal(ref.narrow(dirty.astype(np.uint16), samples, depth), got)
    assert np.array_equal(ref.narrow(words.astype(np.uint16).view(np.int16), samples, depth), got)  # the carrier's signedness plays no part


def test_bytes_pass_through_and_pairs_split():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.narrow(b, U8, 8), b)
    uv = np.arange(2 * 3 * 8, dtype=np.uint8).reshape(2, 3, 8)
    u, v = ref.split_pairs(uv)
    assert u.shape == v.shape == (2, 3, 4) and np.array_equal(u[0, 0], [0, 2, 4, 6]) and np.array_equal(v[0, 0], [1, 3, 5, 7])


# ---- 2. BT.709
@pytest.mark.parametrize("mode", [BT709_LIMITED, BT709_FULL])
def test_bt709_integers_are_the_rounded_matrix(mode):
    bits, y0, ints = ref.BT709_INT[mode]
    m = ref.bt709_matrix(mode == BT709_LIMITED)
    assert np.array_equal(np.rint(m * (1 << bits)).astype(np.int64), np.array(ints))
    assert y0 == (16 if mode == BT709_LIMITED else 0)
    # the matrix is the inverse of Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr))
    full = ref.bt709_matrix(False)
    kg = 1 - ref.KR - ref.KB
    fwd = np.array([[ref.KR, kg, ref.KB],
                    [-ref.KR / (2 * (1 - ref.KB)), -kg / (2 * (1 - ref.KB)), 0.5],
                    [0.5, -kg / (2 * (1 - ref.KR)), -ref.KB / (2 * (1 - ref.KR))]])
    assert np.allclose(full @ fwd, np.eye(3), atol=1e-12)


@pytest.mark.parametrize("mode", [BT709_LIMITED, BT709_FULL])
def test_bt709_is_within_one_of_the_float_matrix_on_every_triple(mode):
    m = ref.bt709_matrix(mode == BT709_LIMITED)
    y0 = 16 if mode == BT709_LIMITED else 0
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    D, E = (U - 128).astype(np.float64), (V - 128).astype(np.float64)
    worst = 0.0
    for y in range(256):
        got = ref.rgb_channels(np.full_like(U, y), U, V, mode)
        for ch in range(3):
            want = np.clip(m[ch, 0] * (y - y0) + m[ch, 1] * D + m[ch, 2] * E, 0.0, 255.0)
            worst = max(worst, float(np.abs(got[ch] - want).max()))
    print("mode", mode, "largest distance from the float matrix", worst)
    assert worst <= 1.0
    assert ref.to_rgb32(y0, 128, 128, mode) == 0 and ref.to_rgb32(235 if y0 else 255, 128, 128, mode) == 0xffffff


# ---- 3. the struct
def test_struct_layout_is_the_documented_one(tmp_path):
    want = dict(y=0, u=8, v=16, y_row=24, y_frame=32, u_row=40, u_frame=48, v_row=56, v_frame=64, width=72, height=76, frames=80, fps=88, chroma=96,
                samples=100, depth=104, full_range=108, memory=112)
    assert ctypes.sizeof(YuvClip) == 120
    assert {n: getattr(YuvClip, n).offset for n, _ in YuvClip._fields_} == want
    # and the C compiler's view of include/tilemotion.h
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tilemotion.h"\nint main(void) {\n  printf("%zu", sizeof(tm_yuv_clip));\n'
                   + "".join('  printf(" %%zu", offsetof(tm_yuv_clip, %s));\n' % n for n in want) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(t) for t in subprocess.check_output([str(exe)], text=True).split()] == [120] + list(want.values())
    hdr = open(os.path.join(ROOT, "include", "tilemotion.h")).read()
    for text in ("TM_SAMPLES_U8 = 0, TM_SAMPLES_U16_LOW = 1, TM_SAMPLES_U16_HIGH = 2", "TM_MEM_HOST = 0, TM_MEM_DEVICE = 1", "TM_YUV_BT709_LIMITED = 4, TM_YUV_BT709_FULL = 5"):
        assert text in hdr


# ---- 4. the checks, with no device
BUF = (ctypes.c_uint8 * 64)()  # somewhere for the pointers to point: nothing is read through them
ADDR = ctypes.addressof(BUF)


def good(chroma=C420JPEG, samples=U8, depth=8, pairs=False, w=100, h=52, memory=HOST):
    B = 1 if samples == U8 else 2
    cw = w if chroma == C444 else (w + 1) // 2
    ch = (h + 1) // 2 if chroma in (C420JPEG, C420MPEG2) else h
    c = YuvClip()
    c.y, c.y_row, c.y_frame = ADDR, w * B, w * B * h
    if chroma != MONO:
        c.u, c.u_row, c.u_frame = ADDR + 16, cw * B * (2 if pairs else 1), cw * B * (2 if pairs else 1) * ch
        if not pairs:
            c.v, c.v_row, c.v_frame = ADDR + 32, cw * B, cw * B * ch
    c.width, c.height, c.frames, c.fps = w, h, 3, 25.0
    c.chroma, c.samples, c.depth, c.full_range, c.memory = chroma, samples, depth, 0, memory
    return c


def probe(c, scaling=1.0):
    w, h = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib().tm_probe_yuv_clip_host(ctypes.byref(c) if c is not None else None, scaling, ctypes.byref(w), ctypes.byref(h))
    return rc, w.value, h.value, lib().tm_last_error().decode()


def test_good_clips_are_described_as_a_file_would_be():
    for chroma in range(5):
        for samples, depth in ((U8, 8), (U16_LOW, 9), (U16_LOW, 10), (U16_HIGH, 10), (U16_HIGH, 16)):
            for pairs in (False, True):
                for memory in (HOST, DEVICE):
                    assert probe(good(chroma, samples, depth, pairs, memory=memory))[:3] == (0, 100, 52), (chroma, samples, depth, pairs)
    assert probe(good(w=5, h=3), 0.5)[:3] == (0, 2, 2)     # Round: half to even
    assert probe(good(w=5, h=3), 1.5)[:3] == (0, 8, 4)
    assert probe(good(w=5, h=3), 0.3)[:3] == (0, 2, 1)     # at least 1
    assert probe(good(w=101, h=53), 0.75)[:3] == (0, 76, 40)
    assert probe(good(w=65536, h=1))[:3] == (0, 65536, 1)
    rc, _, _, msg = probe(good(w=100, h=4), 0.125)         # 12.5 -> 12: 8.33-fold
    assert rc == E_UNSUPPORTED and "more than 8" in msg
    assert probe(good(w=100, h=4), 0.13)[:3] == (0, 13, 1)
    c = good(chroma=MONO)
    c.u_row = c.v_row = -5                                  # MONO: u and v are not looked at
    assert probe(c)[0] == 0
    c = good()
    c.y_row += 7; c.u_row += 1; c.y_frame = 0               # bytes may have any stride; frames may overlap (a still)
    assert probe(c)[0] == 0


def _set(c, **kw):
    for k, v in kw.items():
        setattr(c, k, v)
    return c


REFUSED = [
    ("null struct", lambda: None, "null"),
    ("null y", lambda: _set(good(), y=None), "y plane"),
    ("no chroma for 4:2:0", lambda: _set(good(), u=None, v=None), "u is null"),
    ("no chroma for pairs", lambda: _set(good(pairs=True), u=None), "u is null"),
    ("v without u", lambda: _set(good(), u=None), "without a u"),
    ("v without u, mono", lambda: _set(good(chroma=MONO), v=ADDR), "without a u"),
    ("width 0", lambda: _set(good(), width=0), "size"),
    ("width 65537", lambda: _set(good(), width=65537, y_row=65537), "size"),
    ("height 0", lambda: _set(good(), height=0), "size"),
    ("height 65537", lambda: _set(good(), height=65537), "size"),
    ("height -1", lambda: _set(good(), height=-1), "size"),
    ("frames 0", lambda: _set(good(), frames=0), "frames"),
    ("frames -3", lambda: _set(good(), frames=-3), "frames"),
    ("fps 0", lambda: _set(good(), fps=0.0), "frame rate"),
    ("fps -1", lambda: _set(good(), fps=-1.0), "frame rate"),
    ("fps nan", lambda: _set(good(), fps=float("nan")), "frame rate"),
    ("chroma 5", lambda: _set(good(), chroma=5), "chroma layout 5"),
    ("chroma -1", lambda: _set(good(), chroma=-1), "chroma layout -1"),
    ("samples 3", lambda: _set(good(), samples=3), "sample format 3"),
    ("samples -1", lambda: _set(good(), samples=-1), "sample format -1"),
    ("memory 2", lambda: _set(good(), memory=2), "memory kind 2"),
    ("memory -1", lambda: _set(good(), memory=-1), "memory kind -1"),
    ("depth 10 with bytes", lambda: _set(good(), depth=10), "depth 10"),
    ("depth 7 with bytes", lambda: _set(good(), depth=7), "depth 7"),
    ("depth 8 with words", lambda: good(samples=U16_LOW, depth=8), "depth 8"),
    ("depth 17 with words", lambda: good(samples=U16_HIGH, depth=17), "depth 17"),
    ("short y rows", lambda: _set(good(), y_row=99), "y row stride"),
    ("short y rows, words", lambda: _set(good(samples=U16_LOW, depth=10), y_row=198), "y row stride"),
    ("short u rows", lambda: _set(good(), u_row=49), "u row stride"),
    ("short v rows", lambda: _set(good(), v_row=49), "v row stride"),
    ("pair rows as long as plane rows", lambda: _set(good(pairs=True), u_row=50), "u row stride"),
    ("pair rows one short", lambda: _set(good(pairs=True, samples=U16_HIGH, depth=10), u_row=198), "u row stride"),
    ("odd width chroma", lambda: _set(good(w=101, h=53), u_row=50), "u row stride"),
    ("negative row stride", lambda: _set(good(), y_row=-100), "y row stride"),
    ("odd y pointer, words", lambda: _set(good(samples=U16_LOW, depth=10), y=ADDR + 1), "odd y"),
    ("odd u pointer, words", lambda: _set(good(samples=U16_LOW, depth=10), u=ADDR + 3), "odd u"),
    ("odd v pointer, words", lambda: _set(good(samples=U16_HIGH, depth=10), v=ADDR + 5), "odd v"),
    ("odd y row stride, words", lambda: _set(good(samples=U16_LOW, depth=10), y_row=201), "odd y"),
    ("odd u row stride, pairs of words", lambda: _set(good(samples=U16_HIGH, depth=10, pairs=True), u_row=201), "odd u"),
    ("odd y frame stride, words", lambda: _set(good(samples=U16_LOW, depth=12), y_frame=100 * 2 * 52 + 1), "odd y"),
    ("odd v frame stride, words", lambda: _set(good(samples=U16_LOW, depth=12), v_frame=50 * 2 * 26 + 1), "odd v"),
    ("negative y frame stride", lambda: _set(good(), y_frame=-5200), "negative y frame stride"),
    ("negative u frame stride", lambda: _set(good(), u_frame=-2), "negative u frame stride"),
    ("negative v frame stride", lambda: _set(good(), v_frame=-1), "negative v frame stride"),
]


@pytest.mark.parametrize("name,make,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_bad_clips_are_refused_with_no_device(name, make, word):
    rc, w, h, msg = probe(make())
    assert rc == E_INVAL and word in msg, (name, rc, msg)
    assert (w, h) == (-1, -1)
    # tm_set_frames_yuv itself: without a device there is no encoder to refuse on behalf of, and that is TM_E_INVAL too
    L = lib()
    L.tm_set_frames_yuv.restype, L.tm_set_frames_yuv.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(YuvClip)]
    c = make()
    assert L.tm_set_frames_yuv(None, ctypes.byref(c) if c is not None else None) == E_INVAL


def test_python_enums_follow_the_header():
    from tiler_amd.encoder import TInputYUV, TSamples, TChroma
    assert (TInputYUV.yuvBT709Limited, TInputYUV.yuvBT709Full) == (4, 5)
    assert [int(v) for v in TInputYUV][:4] == [0, 1, 2, 3]
    assert [int(v) for v in TSamples] == [U8, U16_LOW, U16_HIGH] and [int(v) for v in TChroma] == [0, 1, 2, 3, 4]
