"""The WebP writer's host twin (tm_webp_encode_host) against the plain-Python restatement (tests/webp_out_ref.py)
byte for byte on the cases of tests/webp_out_cases.py, and its files through two readers: Pillow and the restatement's own.  No device."""
import ctypes
import io

import numpy as np
import pytest

from tests import webp_out_cases as C
from tests import webp_out_ref as R

NAMES = [c["name"] for c in C.clips() + C.device_clips()]


def _clip(name):
    return next(c for c in C.clips() + C.device_clips() if c["name"] == name)


def test_the_cases_reach_what_they_claim():
    C.check_claims()


@pytest.mark.parametrize("name", NAMES)
def test_the_twin_equals_the_restatement(name):
    from tiler_amd import stages
    c = _clip(name)
    want, canvas, info = C.expected(name)
    got = stages.webp_encode_host(c["frames"], c["fps"], full=True, guard=64, **c["opt"])
    assert got["rc"] == 0 and got["bytes"] == len(want)
    assert got["file"] == want
    assert (got["buffer"][:64] == 0xA5).all() and (got["buffer"][64 + len(want):] == 0xA5).all()
    st = got["stats"]
    assert st["frames"] == len(info) and st["frames_indexed"] == sum(f["colours"] > 0 for f in info) and st["file_bytes"] == len(want)
    assert [st[k] for k in ("segments", "tokens", "matches")] == [sum(f[k] for f in info) for k in ("segments", "tokens", "matches")]
    _, shown = stages.webp_encode_host(c["frames"], c["fps"], canvas=True, **c["opt"])
    assert np.array_equal(shown, canvas)
    # padded rows and frames change nothing
    nf, h, w = c["frames"].shape
    store = np.full((nf, h + 2, w + 3), 0x00FEDCBA, np.uint32)
    store[:, :h, :w] = c["frames"]
    assert stages.webp_encode_host(store[:, :h, :w], c["fps"], **c["opt"]) == want


@pytest.mark.parametrize("name", NAMES)
def test_two_readers_show_the_source(name):
    from PIL import Image, features
    assert features.check("webp")
    c = _clip(name)
    file, canvas, info = C.expected(name)
    source = c["frames"] & 0xFFFFFF
    assert np.array_equal(canvas, source)
    frames, parsed = R.decode(file)
    assert len(frames) == len(source) and all(np.array_equal(a, b) for a, b in zip(frames, source))
    nf, h, w = source.shape
    assert (parsed["width"], parsed["height"], parsed["loop"]) == (w, h, c["opt"].get("loop", 0))
    duration = c["opt"].get("duration_ms", 0) or max(1, int(np.floor(1000.0 / c["fps"] + 0.5)))
    for f, fr in zip(info, parsed["frames"]):
        assert (fr["x"], fr["y"], fr["w"], fr["h"]) == f["rect"] and fr["duration"] == duration and fr["flags"] == 2
    im = Image.open(io.BytesIO(file))
    assert im.format == "WEBP" and getattr(im, "n_frames", 1) == nf
    for f in range(nf):
        im.seek(f)
        a = np.asarray(im.convert("RGBA")).astype(np.uint32)
        assert (a[..., 3] == 255).all()
        assert np.array_equal(a[..., 0] << 16 | a[..., 1] << 8 | a[..., 2], source[f]), f
        assert im.info.get("duration", duration) == duration
    assert im.info.get("loop", 0) == c["opt"].get("loop", 0)


def test_refusals_and_their_codes():
    from tiler_amd import lib, stages
    from tiler_amd._lib import WebpOptions
    for name, frames, fps, opt, code in C.refused():
        got = stages.webp_encode_host(frames, fps, full=True, **opt)
        assert got["rc"] == code and got["file"] is None and (got["buffer"] == 0xA5).all(), name
    L = lib()
    px = np.zeros((2, 4, 8), np.uint32)
    out = np.full(4096, 0xAA, np.uint8)
    need = ctypes.c_int64(-7)
    pp, op = ctypes.c_void_p(px.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, fps=25.0, opt=(1, 0, 1, 16384, 0, 0), cap=4096, n=ctypes.byref(need)):
        return L.tm_webp_encode_host(frames, stride, frame_px, nf, w, h, fps, ctypes.byref(WebpOptions(*opt)), op, cap, n, None, None)
    for kw, code in ((dict(frames=None), -1), (dict(w=0), -1), (dict(h=0), -1), (dict(nf=0), -1), (dict(stride=7), -1), (dict(frame_px=31), -1), (dict(n=None), -1),
                     (dict(cap=-1), -1), (dict(opt=(1, 2, 1, 0, 0, 0)), -1), (dict(opt=(1, -1, 1, 0, 0, 0)), -1), (dict(opt=(-1, 0, 1, 0, 0, 0)), -1),
                     (dict(w=16385, stride=16385, h=1, nf=1), -6), (dict(w=1, stride=1, h=16385, nf=1), -6)):
        assert call(**kw) == code, kw
        assert (out == 0xAA).all() and need.value == -7, kw
    assert L.tm_webp_encode_host(pp, 8, 32, 2, 8, 4, 25.0, None, op, 4096, ctypes.byref(need), None, None) == -1
    assert call() == 0 and need.value > 0
    bound = ctypes.c_int64(-7)
    assert L.tm_webp_bound_host(8, 4, 2, ctypes.byref(WebpOptions(1, 0, 1, 0, 0, 0)), None) == -1
    assert L.tm_webp_bound_host(8, 4, 2, None, ctypes.byref(bound)) == -1 and L.tm_webp_bound_host(16385, 4, 2, ctypes.byref(WebpOptions(1, 0, 1, 0, 0, 0)), ctypes.byref(bound)) == -6
    assert bound.value == -7


def test_the_bound_and_the_caps():
    from tiler_amd import lib, stages
    for c in C.clips() + C.device_clips():
        nf, h, w = c["frames"].shape
        assert len(C.expected(c["name"])[0]) <= stages.webp_bound(w, h, nf, **c["opt"]), c["name"]
    # the costliest pixels there are: every colour another, nothing to match, every code as long as it gets
    worst = np.random.default_rng(5).integers(0, 1 << 24, (1, 40, 40)).astype(np.uint32)
    assert len(stages.webp_encode_host(worst, 25.0, lz77=False)) <= stages.webp_bound(40, 40, 1)
    c = _clip("clip_diff")
    want = C.expected("clip_diff")[0]
    need = len(want)
    for cap in (0, 1, need - 1):
        got = stages.webp_encode_host(c["frames"], c["fps"], cap=cap, guard=64, full=True)
        assert got["rc"] == -1 and got["bytes"] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.webp_encode_host(c["frames"], c["fps"], cap=need, guard=64, full=True)
    assert got["rc"] == 0 and got["file"] == want and (got["buffer"][64 + need:] == 0xA5).all()


@pytest.mark.parametrize("fps", [0.5, 1.0, 9.0, 10.0, 15.0, 24.0, 25.0, 29.97, 30.0, 50.0, 60.0, 100.0, 1000.0, 5000.0])
def test_the_duration_follows_the_rate(fps):
    from tiler_amd import stages
    want = max(1, int(np.floor(1000.0 / fps + 0.5)))
    _, parsed = R.decode(stages.webp_encode_host(np.zeros((3, 2, 2), np.uint32), fps))
    assert [f["duration"] for f in parsed["frames"]] == [want] * 3
