"""The GIF writer's host twin (tm_gif_encode_host and the seams' twins) against the plain-Python restatement
(tests/gif_out_ref.py) byte for byte on the cases of tests/gif_out_cases.py, and its files through three readers: Pillow, the restatement
of the reader (tests/gif_ref.py) and the project's own (tm_gif_decode_host).  No device."""
import ctypes
import io

import numpy as np
import pytest

from tests import gif_out_cases as C
from tests import gif_out_ref as R
from tests import gif_ref

NAMES = [c["name"] for c in C.clips()]


def _clip(name):
    return next(c for c in C.clips() if c["name"] == name)


def test_the_cases_reach_what_they_claim():
    C.check_claims()


def test_pack_is_gif_ref_pack_codes():
    for name, idx, mn, seg, _ in C.streams():
        if len(idx) > 3000:
            continue
        codes = [c for s in R.segment_codes(idx, mn, seg) for c in s]
        assert R.pack(codes, mn)[0] == gif_ref.pack_codes(codes, mn), name


@pytest.mark.parametrize("name", NAMES)
def test_the_twin_equals_the_restatement(name):
    from tiler_amd import stages
    c = _clip(name)
    want, canvas, info = C.expected(name)
    got = stages.gif_encode_host(c["frames"], c["fps"], full=True, guard=64, **c["opt"])
    assert got["rc"] == 0 and got["bytes"] == len(want)
    assert got["file"] == want
    assert (got["buffer"][:64] == 0xA5).all() and (got["buffer"][64 + len(want):] == 0xA5).all()
    st = got["stats"]
    assert st["frames"] == len(info) and st["frames_exact"] == sum(f["exact"] for f in info) and st["frames_quantised"] == sum(not f["exact"] for f in info)
    assert st["segments"] == sum(f["segments"] for f in info) and st["file_bytes"] == len(want)
    _, shown = stages.gif_encode_host(c["frames"], c["fps"], canvas=True, **c["opt"])
    assert np.array_equal(shown, canvas)
    # padded rows and frames change nothing
    nf, h, w = c["frames"].shape
    store = np.full((nf, h + 2, w + 3), 0x00FEDCBA, np.uint32)
    store[:, :h, :w] = c["frames"]
    assert stages.gif_encode_host(store[:, :h, :w], c["fps"], **c["opt"]) == want


@pytest.mark.parametrize("name", NAMES)
def test_three_readers_show_the_canvas(name):
    from PIL import Image
    from tiler_amd import stages
    c = _clip(name)
    file, canvas, info = C.expected(name)
    frames, status, parsed = gif_ref.decode(file)
    assert status == [0] * len(canvas) and all(np.array_equal(a, b) for a, b in zip(frames, canvas))
    ours, status = stages.gif_decode_host(file)
    assert status == [0] * len(canvas) and np.array_equal(ours, canvas)
    im = Image.open(io.BytesIO(file))
    assert im.n_frames == len(canvas)
    for f in range(len(canvas)):
        im.seek(f)
        a = np.asarray(im.convert("RGB")).astype(np.uint32)
        assert np.array_equal(a[..., 0] << 16 | a[..., 1] << 8 | a[..., 2], canvas[f]), f
    if all(f["exact"] for f in info):
        assert np.array_equal(canvas, c["frames"] & 0xFFFFFF)
    assert parsed["loop"] == c["opt"].get("loop", 0)
    for f, im in zip(info, parsed["images"]):
        assert im["disposal"] == 1 and im["transparent"] == -1 and im["interlaced"] == 0 and im["local_table"] == 1
        assert len(im["table"]) == max(2, 1 << (f["table"] - 1).bit_length()) and im["table"][f["table"]:] == [0] * (len(im["table"]) - f["table"])


def test_refusals_and_their_codes():
    from tiler_amd import lib, stages
    from tiler_amd._lib import GifOptions
    for name, frames, fps, opt, code in C.refused():
        got = stages.gif_encode_host(frames, fps, full=True, **opt)
        assert got["rc"] == code and got["file"] is None and (got["buffer"] == 0xA5).all(), name
    stages.gif_encode_host(C.distinct(257).reshape(1, 1, 257), 25.0, full=True, colours="exact")
    assert "frame 0 holds 257 colours" in lib().tm_last_error().decode()
    two = np.concatenate([np.zeros((1, 1, 300), np.uint32), C.distinct(300).reshape(1, 1, 300)])
    assert stages.gif_encode_host(two, 25.0, full=True, colours="exact", max_colours=100)["rc"] == -6
    assert "frame 1 holds 300 colours" in lib().tm_last_error().decode()
    L = lib()
    px = np.zeros((2, 4, 8), np.uint32)
    out = np.full(4096, 0xAA, np.uint8)
    need = ctypes.c_int64(-7)
    pp, op = ctypes.c_void_p(px.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, fps=25.0, opt=(0, 256, 1, 16384, 0, 0), cap=4096, n=ctypes.byref(need)):
        return L.tm_gif_encode_host(frames, stride, frame_px, nf, w, h, fps, ctypes.byref(GifOptions(*opt)), op, cap, n, None, None)
    for kw, code in ((dict(frames=None), -1), (dict(w=0), -1), (dict(h=0), -1), (dict(nf=0), -1), (dict(stride=7), -1), (dict(frame_px=31), -1), (dict(n=None), -1),
                     (dict(cap=-1), -1), (dict(opt=(3, 256, 1, 0, 0, 0)), -1), (dict(opt=(0, 256, 2, 0, 0, 0)), -1), (dict(w=65536, stride=65536, h=1, nf=1), -6),
                     (dict(w=1, stride=1, h=65536, nf=1), -6)):
        assert call(**kw) == code, kw
        assert (out == 0xAA).all() and need.value == -7, kw
    assert L.tm_gif_encode_host(pp, 8, 32, 2, 8, 4, 25.0, None, op, 4096, ctypes.byref(need), None, None) == -1
    assert call() == 0 and need.value > 0


def test_the_bound_and_the_caps():
    from tiler_amd import lib, stages
    for c in C.clips():
        nf, h, w = c["frames"].shape
        want = C.expected(c["name"])[0]
        opt = {k: v for k, v in c["opt"].items()}
        assert len(want) <= stages.gif_bound(w, h, nf, **opt), c["name"]
    c = _clip("clip_diff")
    want = C.expected("clip_diff")[0]
    need = len(want)
    for cap in (0, 1, need - 1):
        got = stages.gif_encode_host(c["frames"], c["fps"], cap=cap, guard=64, full=True)
        assert got["rc"] == -1 and got["bytes"] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.gif_encode_host(c["frames"], c["fps"], cap=need, guard=64, full=True)
    assert got["rc"] == 0 and got["file"] == want and (got["buffer"][64 + need:] == 0xA5).all()


@pytest.mark.parametrize("fps", [0.5, 1.0, 9.0, 10.0, 15.0, 24.0, 25.0, 29.97, 30.0, 40.0, 50.0, 60.0, 100.0, 1000.0])
def test_the_delay_reads_back_as_the_rate_of_section_42(fps):
    from tiler_amd import stages
    delay = max(2, int(np.floor(100.0 / fps + 0.5)))
    file = stages.gif_encode_host(np.zeros((3, 2, 2), np.uint32), fps)
    info = stages.probe_gif(file)
    assert info["frames"] == 3 and info["uniform_delay"] == 1 and info["loop_count"] == 0
    assert info["fps"] == 100.0 * 3 / (3 * delay)
    assert [f["delay"] for f in stages.gif_frames(file)] == [delay] * 3
    assert stages.probe_gif(stages.gif_encode_host(np.zeros((1, 2, 2), np.uint32), fps, delay_cs=7, loop=-1))["loop_count"] == -1


def test_the_lzw_seam_equals_the_restatement():
    from tiler_amd import stages
    for name, idx, mn, seg, _ in C.streams():
        assert stages.gif_lzw_pack_host(idx, mn, seg) == R.payload(idx, mn, seg)[0], name


def test_the_table_seam_equals_the_restatement():
    from tiler_amd import stages
    for c in C.clips():
        opt = {k: v for k, v in c["opt"].items() if k in ("colours", "max_colours")}
        table, exact, idx = stages.gif_palettise_host(c["frames"][0], **opt)
        rt, re, ri, _ = R.palettise(c["frames"][0], opt.get("colours", "auto"), opt.get("max_colours", 256))
        assert list(table) == rt and exact == re and np.array_equal(idx, ri), c["name"]


def _psnr(a, b):
    ch = lambda v: np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.float64)  # noqa: E731
    return 10 * np.log10(255.0 ** 2 / np.mean((ch(a) - ch(b)) ** 2))


@pytest.mark.parametrize("which", ["all_distinct_192x192", "synth_128x128"])
def test_the_cut_is_as_good_as_pillows(which):
    """Both are median cuts to 256 colours without dithering; Pillow cuts at full precision, this one over 15-bit cells with its own split
    and tie rules.  Measured: all-distinct 25.96 dB here against Pillow's 21.26, the synthetic photograph 33.57
    against 34.54.  The margin is 1.5 dB: a cell is 8 levels wide, so a box border lies up to a uniform error of variance (64 - 1) / 12 =
    5.25 a channel from where a full-precision cut would put it, 0.9 dB at Pillow's 34.5 dB, and the rest is for the different split rule."""
    from PIL import Image
    from tiler_amd import stages, synth
    fr = C.distinct(192 * 192).reshape(192, 192) if which == "all_distinct_192x192" else synth.video(1, 128, 128)[0] & 0xFFFFFF
    rgb = np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8)
    q = np.asarray(Image.fromarray(rgb, "RGB").quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")).astype(np.uint32)
    pillow = _psnr(q[..., 0] << 16 | q[..., 1] << 8 | q[..., 2], fr)
    _, canvas = stages.gif_encode_host(fr[None], 25.0, canvas=True)
    ours = _psnr(canvas[0], fr)
    print("%s: twin %.3f dB, Pillow %.3f dB" % (which, ours, pillow))
    assert ours >= pillow - 1.5
