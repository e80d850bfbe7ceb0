"""The GIF reader's host twin (tm_probe_gif_host, tm_gif_frames_host, tm_gif_lzw_streams_host, tm_gif_decode_host)
against the plain-Python restatement (tests/gif_ref.py) on every case of tests/gif_cases.py, both against Pillow, the damage list, every
refusal with its code and message, and tm_probe_input_host's kind 16.  No GPU."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests import gif_cases as C
from tests import gif_ref as R
from tiler_amd import stages, TileMotionError, lib


def twin(file, first=0, count=None, background=None):
    """the host twin's (frames or None from the first refused image on, statuses), as gif_ref.decode gives them"""
    out, st = stages.gif_decode_host(file, first, count, background, fill=0x5A5A5A5A)
    bad = next((i for i, s in enumerate(st) if s), len(st))
    frames = []
    for i in range(out.shape[0]):
        if first + i < bad:
            frames.append(out[i])
        else:
            assert (out[i] == 0x5A5A5A5A).all()  # nothing is delivered
            frames.append(None)
    return frames, st


def same_frames(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


def pillow_frames(file):
    from PIL import Image
    im = Image.open(io.BytesIO(file))
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        rgb = np.asarray(im.convert("RGB")).astype(np.uint32)
        out.append(rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2])
    return out


def test_the_cases_reach_what_they_claim():
    found = C.check_claims()
    assert all(found.values())


@pytest.mark.parametrize("name,file", [(n, f) for n, f, _ in C.pictures()] + [(n, f) for n, f, _ in C.clips()], ids=lambda v: v if isinstance(v, str) else "")
def test_twin_equals_the_restatement(name, file):
    frames, st, info = R.decode(file)
    got, got_st = twin(file)
    assert got_st == st and not any(st)
    assert same_frames(got, frames)
    p = stages.probe_gif(file)
    assert (p["width"], p["height"], p["frames"], p["version"], p["loop_count"]) == (info["width"], info["height"], len(info["images"]), info["version"], info["loop"])
    assert p["fps"] == info["fps"] and p["uniform_delay"] == info["uniform_delay"]
    assert (p["global_table_size"], p["background_index"], p["background"]) == (len(info["global_table"]), info["bg_index"], info["bg"])
    fr = stages.gif_frames(file)
    assert len(fr) == len(info["images"])
    for a, b in zip(fr, info["images"]):
        for k in ("left", "top", "width", "height", "delay", "disposal", "transparent", "interlaced", "local_table", "min_code_size", "data_off", "data_bytes"):
            assert a[k] == b[k], k
        assert a["table_size"] == len(b["table"])


def test_rate():
    by = {n: f for n, f, _ in C.clips()}
    assert stages.probe_gif(by["delays_0_1"])["fps"] == 10.0 and stages.probe_gif(by["delays_0_1"])["uniform_delay"] == 1  # 0 and 1 count as 10
    assert stages.probe_gif(by["delays_equal"])["fps"] == 25.0 and stages.probe_gif(by["delays_equal"])["uniform_delay"] == 1
    p = stages.probe_gif(by["delays_unequal"])
    assert p["fps"] == 100.0 * 4 / (3 + 20 + 7 + 10) and p["uniform_delay"] == 0
    assert stages.probe_gif(by["extensions_between_frames"])["loop_count"] == 3 and stages.probe_gif(by["no_trailer"])["loop_count"] == -1


def test_lzw_streams_equal_the_restatement():
    """all case streams in one batch, between guard bytes, damaged streams beside good neighbours"""
    items = C.streams()
    blob, at = bytearray(b"\x5a" * 3), []
    for _, span, _, _ in items:
        at.append(len(blob))
        blob += span + b"\xee"
    dst, st, offs = stages.gif_lzw_host(bytes(blob), [(a, len(s[1]), s[2], s[3]) for a, s in zip(at, items)], guard=32)
    seen = set()
    keep = np.ones(dst.size, bool)
    for (name, span, mn, npix), got, off in zip(items, st, offs):
        idx, want, _ = R.lzw_decode(span, mn, npix)
        assert got == want, (name, got, want)
        assert bytes(dst[off:off + want[2]]) == idx, name
        keep[off:off + want[2]] = False
        seen.add(want[0])
    assert (dst[keep] == 0xA5).all()  # nothing outside what a stream says it wrote
    assert seen == {0, R.TRUNCATED, R.BAD_CODE}


def test_lzw_batch_refusals():
    from tiler_amd._lib import GifStreamDesc, GifStatusDesc
    blob = bytes(16)
    dst = np.zeros(16, np.uint8)
    st = (GifStatusDesc * 1)()
    for desc, what in ((GifStreamDesc(10, 0, 7, 4, 4, 0), "outside the blob"), (GifStreamDesc(0, 10, 4, 7, 4, 0), "destination lies outside"),
                       (GifStreamDesc(0, 0, 4, 4, 1, 0), "minimum code size of 1"), (GifStreamDesc(0, 0, 4, 4, 9, 0), "minimum code size of 9")):
        arr = (GifStreamDesc * 1)(desc)
        assert lib().tm_gif_lzw_streams_host(blob, 16, arr, 1, dst.ctypes.data, 16, st) == -1
        assert what in lib().tm_last_error().decode()


@pytest.mark.parametrize("name,file", [(n, f) for n, f, p in C.clips() if p] + [(n, f) for n, f, _ in C.pictures()], ids=lambda v: v if isinstance(v, str) else "")
def test_against_pillow(name, file):
    """Pillow on the subset where frame 0 is opaque and covers the screen and the disposals are 0 and 1, and on every single picture.
    Disposal 3 is not in the subset: Pillow 12.2 does not agree there (test_pillow_and_disposal_3 pins what it does).  Outside the subset
    Pillow fills a first frame's uncovered screen and a disposal-2 rectangle by rules of its own (transparency, not the background
    colour), which is why the other clips are not compared."""
    want = pillow_frames(file)
    frames, st, _ = R.decode(file)
    got, _ = twin(file)
    assert same_frames(frames, want) and same_frames(got, want)


def test_pillow_and_disposal_3():
    """What was found for disposal 3 (clip disposal_0_1_3: disposals 1, 3, 0, 3, 3, 1, 0): Pillow equals the restatement up to frame 2;
    from frame 3 on, the first frame with disposal 3 behind a frame that was kept (disposal 0), Pillow shows frame 0's pixels at places
    where that kept frame had drawn, seeking frame by frame or straight to the frame.  The specification keeps a frame of disposal 0, and
    so do the restatement and the twin; disposal 3 therefore stays outside the subset Pillow is compared on."""
    file = dict((n, f) for n, f, _ in C.clips())["disposal_0_1_3"]
    want, ours = pillow_frames(file), R.decode(file)[0]
    assert same_frames(ours[:3], want[:3])
    if not same_frames(ours, want):  # (a Pillow that agrees is welcome)
        y, x = np.nonzero(ours[3] != want[3])
        assert (want[3][y, x] == ours[0][y, x]).all() and (ours[3][y, x] == ours[2][y, x]).all()


def _pillow_gif(frames, **kw):
    from PIL import Image
    ims = [Image.fromarray(f, "RGB") for f in frames]
    buf = io.BytesIO()
    ims[0].save(buf, "GIF", save_all=len(ims) > 1, append_images=ims[1:], **kw)
    return buf.getvalue()


def test_pillow_written_files():
    """Pillow's own files through the twin: an animation (save_all: sub-rectangles, its choice of disposal), an optimised one, and its
    interlaced single pictures"""
    rng = np.random.default_rng(3)
    base = (rng.integers(0, 4, (40, 56, 3)) * 80).astype(np.uint8)
    frames = []
    for i in range(6):
        f = base.copy()
        f[5 + 3 * i:15 + 3 * i, 4 + 6 * i:20 + 6 * i] = (rng.integers(0, 3, (10, 16, 3)) * 100).astype(np.uint8)
        frames.append(f)
    flat = np.zeros((192, 192, 3), np.uint8)
    flat[:] = (10, 200, 30)
    stripes = np.zeros((70, 70, 3), np.uint8)
    stripes[:, ::2] = 255
    files = [_pillow_gif(frames, duration=[40, 40, 80, 40, 20, 40], loop=0), _pillow_gif(frames, duration=50, optimize=True, disposal=2), _pillow_gif(frames[:1]),
             _pillow_gif(frames[:1], interlace=True), _pillow_gif([flat]), _pillow_gif([stripes]), _pillow_gif([(rng.integers(0, 256, (96, 96, 3)) & 0xE0).astype(np.uint8)])]
    interlaced = 0
    for k, file in enumerate(files):
        want = pillow_frames(file)
        got, st = twin(file)
        assert not any(st)
        interlaced += sum(f["interlaced"] for f in stages.gif_frames(file))
        if k == 1:  # disposal 2 on every frame: outside the subset (see test_against_pillow); the restatement is the reference there
            want = R.decode(file)[0]
        assert same_frames(got, want), k
    assert interlaced >= 1
    assert stages.probe_gif(files[0])["uniform_delay"] == 0 and stages.probe_gif(files[0])["loop_count"] == 0


def test_pillow_reads_a_minimum_code_size_of_1_with_two_symbols():
    """why a minimum code size of 1 is refused and not read as 2: Pillow reads such a file with clear = 2 (a two-symbol alphabet at two
    bits), so data written for 2 comes out differently there; the walk refuses rather than pick a reading"""
    from PIL import Image
    idx = np.array([[0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 1]], np.uint8)
    as2 = R.write_gif(4, 4, [R.image_bytes(idx, min_code=2, min_code_byte=1)], table=C.PAL16[:2])
    with pytest.raises(TileMotionError) as e:
        stages.probe_gif(as2)
    assert e.value.code == C.IO and "minimum code size of 1" in str(e.value)
    try:
        px = np.asarray(Image.open(io.BytesIO(as2)).convert("RGB"))[..., 0] // 255
        same = np.array_equal(px, idx)
    except Exception:
        same = False
    assert not same  # Pillow does not read it as 2


def test_damage_same_verdict_same_bytes():
    for name, file in C.damaged():
        v = C.verdict(file)
        if v[0] == "refused":
            with pytest.raises(TileMotionError) as e:
                stages.probe_gif(file)
            assert e.value.code == v[1], name
            continue
        got, st = twin(file)
        assert st == v[1], name
        assert same_frames(got, v[2]), name


@pytest.mark.parametrize("name,file,code,kind,message", C.refused(), ids=lambda v: v if isinstance(v, str) and " " not in v else "")
def test_refusals(name, file, code, kind, message):
    for call in (lambda: stages.probe_gif(file), lambda: stages.gif_frames(file), lambda: stages.gif_decode_host(file, 0, 1)):
        with pytest.raises(TileMotionError) as e:
            call()
        assert e.value.code == code and message in str(e.value), str(e.value)


@pytest.mark.parametrize("name,file,status", C.statuses())
def test_statuses(name, file, status):
    frames, st, _ = R.decode(file)
    got, got_st = twin(file)
    assert got_st == st and [s for s in st if s][0] == status
    assert same_frames(got, frames)


def test_first_count_and_background():
    file = dict((n, f) for n, f, _ in C.clips())["every_disposal_pair"]
    frames, st, _ = R.decode(file)
    for first, count in ((3, 5), (16, 1), (0, 0), (17, 0)):
        got, got_st = twin(file, first, count)
        assert got_st == st[:first + count] and same_frames(got, frames[first:first + count])
    file = dict((n, f) for n, f, _ in C.clips())["disposal_3_on_frame_0_small"]
    for bg in (0x123456, 0):
        assert same_frames(twin(file, 0, None, bg)[0], R.decode(file, 0, None, bg)[0])
    assert not same_frames(twin(file, 0, None, 0x123456)[0], twin(file)[0])
    for bad in (lambda: stages.gif_decode_host(file, 2, 5), lambda: stages.gif_decode_host(file, 0, 1, 1 << 24), lambda: stages.gif_decode_host(file, 0, 1, None, 10)):
        with pytest.raises(TileMotionError) as e:
            bad()
        assert e.value.code == -1


def _probe_input(name, start=0, count=0, scaling=1.0):
    v = [ctypes.c_int() for _ in range(7)]
    fps = ctypes.c_double()
    rc = lib().tm_probe_input_host(os.fsencode(str(name)), start, count, scaling, *[ctypes.byref(x) for x in v[:5]], ctypes.byref(fps), ctypes.byref(v[5]), ctypes.byref(v[6]))
    return rc, [x.value for x in v], fps.value


def test_probe_input_kind_16(tmp_path):
    file = dict((n, f) for n, f, _ in C.clips())["delays_unequal"]
    path = tmp_path / "clip.gif"
    path.write_bytes(file)
    rc, v, fps = _probe_input(path)
    assert rc == 0 and v[0] == 16 and v[1:5] == [24, 20, 24, 20] and v[5] == 4 and fps == 10.0
    assert _probe_input(path, 1, 0)[1][5] == 3 and _probe_input(path, 1, 2)[1][5] == 2 and _probe_input(path, 3, 1)[1][5] == 1
    for start, count in ((4, 0), (2, 3), (0, 5)):
        assert _probe_input(path, start, count)[0] == -1
    assert _probe_input(path, 0, 0, 0.5)[0] == C.UNSUPPORTED and "Scaling" in lib().tm_last_error().decode()
    bad = tmp_path / "bad.gif"
    bad.write_bytes(C.refused()[9][1])
    assert _probe_input(bad)[0] == C.IO and "introducer" in lib().tm_last_error().decode()


def test_probe_gif_clip():
    file = dict((n, f) for n, f, _ in C.clips())["delays_equal"]
    w, h, n, fps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    assert lib().tm_probe_gif_clip_host(file, len(file), 0.0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(n), ctypes.byref(fps)) == 0
    assert (w.value, h.value, n.value, fps.value) == (24, 20, 3, 25.0)
    assert lib().tm_probe_gif_clip_host(file, len(file), 12.5, None, None, None, ctypes.byref(fps)) == 0 and fps.value == 12.5
    assert lib().tm_probe_gif_clip_host(b"GIF89a", 6, 0.0, None, None, None, None) == C.IO
    assert lib().tm_probe_gif_clip_host(None, 0, 0.0, None, None, None, None) == -1
