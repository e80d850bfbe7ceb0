"""The PNG writer's rule on the host (tm_deflate.h, tm_deflate.hip): the length-limited code lengths, the stream
coder (tm_zlib_compress_host) against zlib and the library's own inflate, and the files (tm_png_encode_host) against Pillow, the library's
PNG reader and Python restatements of the stored writer and of the adaptive filter choice.  No GPU."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import png_cases
from tests.png_cases import CONTENTS, FILTERS, SHAPES, STREAMS


def _code_lengths(freq, max_bits):
    from tiler_amd import lib
    freq = np.asarray(freq, np.uint32)
    lens = np.full(freq.size, 0xff, np.uint8)
    assert lib().tm_deflate_code_lengths_host(freq.ctypes.data_as(ctypes.c_void_p), freq.size, max_bits, lens.ctypes.data_as(ctypes.c_void_p)) == 0
    return lens


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


_ONE = [0] * 30
_ONE[7] = 5
_ZERO_ONLY = [9] + [0] * 29
_TWO = [0] * 30
_TWO[3], _TWO[29] = 1, 1000
CODE_CASES = {
    "fibonacci_40": (_fib(40), 15),  # an unlimited Huffman code would reach 39 bits
    "equal_286": ([1] * 286, 15),
    "cl_19_limit_7": (_fib(19), 7),
    "sparse_286": ([(i % 7 == 0) * (1 + i * i) for i in range(286)], 15),
    "none_used": ([0] * 30, 15),
    "one_used": (_ONE, 15),
    "symbol_0_only": (_ZERO_ONLY, 15),
    "two_used": (_TWO, 15),
}


@pytest.mark.parametrize("name", list(CODE_CASES))
def test_code_lengths(name):
    freq, limit = CODE_CASES[name]
    lens = _code_lengths(freq, limit)
    used = [s for s, f in enumerate(freq) if f]
    assert lens.max() <= limit
    coded = [s for s in range(len(freq)) if lens[s]]
    if len(used) >= 2:
        assert coded == used  # a zero frequency gives a zero length and nothing else does
        assert sum(2 ** (limit - int(l)) for l in lens if l) == 2 ** limit  # Kraft: exactly 1
        by_freq = sorted(used, key=lambda s: freq[s])
        assert all(lens[a] >= lens[b] for a, b in zip(by_freq, by_freq[1:]))  # rarer symbols never get shorter codes
    else:  # padded to two symbols of one bit
        assert len(coded) == 2 and set(used) <= set(coded) and all(lens[s] == 1 for s in coded)
    assert np.array_equal(lens, _code_lengths(freq, limit))


def test_code_lengths_refusals():
    from tiler_amd import lib
    f = np.ones(40, np.uint32)
    l = np.zeros(40, np.uint8)
    fp, lp = f.ctypes.data_as(ctypes.c_void_p), l.ctypes.data_as(ctypes.c_void_p)
    assert lib().tm_deflate_code_lengths_host(None, 40, 15, lp) == -1
    assert lib().tm_deflate_code_lengths_host(fp, 40, 5, lp) == -1  # 40 symbols do not fit in 5 bits
    assert lib().tm_deflate_code_lengths_host(fp, 1, 15, lp) == -1 and lib().tm_deflate_code_lengths_host(fp, 40, 16, lp) == -1


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_coder(name):
    data = STREAMS[name]
    z = png_cases.zlib_host(data)
    assert zlib.decompress(z) == data
    assert png_cases.inflate_host(z, len(data)) == data
    assert png_cases.zlib_host(data) == z
    segments = max(1, -(-len(data) // 32768))
    assert len(z) <= len(data) + 10 * segments + 6  # every segment stored, the empty block behind it, header and Adler-32: the worst case
    if name == "period_32768":
        assert len(z) < 0.4 * len(data)  # the second and third period are matches at distance 32768
    if name == "zeros_3_segments":
        assert len(z) < 300


def test_stream_coder_refusals():
    from tiler_amd import lib
    src = np.zeros(100, np.uint8)
    out = np.full(200, 0xAA, np.uint8)
    n = ctypes.c_int64(-5)
    sp, op = src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert lib().tm_zlib_compress_host(None, 100, op, 200, ctypes.byref(n)) == -1 and n.value == -5
    assert lib().tm_zlib_compress_host(sp, 1 << 31, op, 200, ctypes.byref(n)) == -1 and n.value == -5
    assert lib().tm_zlib_compress_host(sp, 100, op, 3, ctypes.byref(n)) == -1 and n.value == len(png_cases.zlib_host(bytes(100)))
    assert (out == 0xAA).all()


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_png_files(tmp_path, shape, content):
    w, h = shape
    frame = png_cases.picture(content, w, h)[0]
    sizes = {}
    for flt in FILTERS:
        png = png_cases.encode_host(frame[None], 1, flt, row_pad=3 if flt == "adaptive" else 0)[0]
        sizes[flt] = len(png)
        assert np.array_equal(png_cases.pillow_pixels(png), frame), flt
        path = tmp_path / ("%s.png" % flt)
        path.write_bytes(png)
        assert np.array_equal(png_cases.read_png_host(path, w, h), frame), flt
        stream = zlib.decompress(png_cases.idat(png))
        types = np.frombuffer(stream, np.uint8).reshape(h, 1 + 3 * w)[:, 0]
        if flt == "none":
            assert not types.any() and stream == png_cases.filter_rows_host(frame, "none")
        if flt == "adaptive":
            assert np.array_equal(types, png_cases.adaptive_types(frame)) and stream == png_cases.filter_rows_host(frame, "adaptive")
        bound = ctypes.c_int64()
        from tiler_amd import lib
        assert lib().tm_png_bound_host(w, h, ctypes.byref(bound)) == 0 and len(png) <= bound.value
    assert sizes["smaller"] == min(sizes["none"], sizes["adaptive"])
    stored = png_cases.encode_host(frame[None], 0, "adaptive")[0]  # (level 0 ignores the filter)
    assert stored == png_cases.stored_png(frame)
    assert len(stored) <= bound.value
    if content == "constant" and shape == (264, 136):
        assert sizes["none"] < 0.02 * len(stored)  # 418 maximal runs


def test_several_frames_and_strides():
    """frames laid out with padded rows and a padded frame stride give the files of the packed frames, in order"""
    frames = png_cases.picture("palettised", 40, 24, frames=3)
    want = [png_cases.encode_host(frames[f:f + 1], 1, "smaller")[0] for f in range(3)]
    assert png_cases.encode_host(frames, 1, "smaller", row_pad=5, frame_pad=11) == want
    assert len(set(want)) == 3


def test_png_refusals():
    from tiler_amd import lib
    from tiler_amd._lib import PngOptions
    L = lib()
    px = np.zeros((2, 4, 8), np.uint32)
    out = np.full(4096, 0xAA, np.uint8)
    offs = (ctypes.c_int64 * 3)(-7, -7, -7)
    pp, op = px.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

    def call(frames=pp, stride=8, frame_px=32, nf=2, w=8, h=4, level=1, flt=1, cap=4096, o=offs):
        return L.tm_png_encode_host(frames, stride, frame_px, nf, w, h, ctypes.byref(PngOptions(level, flt)), op, cap, o)
    for kw in (dict(frames=None), dict(level=2), dict(level=-1), dict(flt=4), dict(flt=-1), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769), dict(stride=7),
               dict(frame_px=31), dict(nf=-1), dict(o=None), dict(w=32768, h=32768, stride=32768)):
        assert call(**kw) == -1, kw
        assert (out == 0xAA).all() and list(offs) == [-7, -7, -7], kw
    assert L.tm_png_encode_host(pp, 8, 32, 2, 8, 4, None, op, 4096, offs) == -1
    assert call(h=1, stride=0, frame_px=8) == 0  # one row: its stride is not read
    offs[0] = offs[1] = offs[2] = -7
    out[:] = 0xAA
    assert call(cap=100) == -1 and offs[2] == sum(len(p) for p in png_cases.encode_host(px, 1, "none")) and (out == 0xAA).all()
    b = ctypes.c_int64(-3)
    assert L.tm_png_bound_host(0, 4, ctypes.byref(b)) == -1 and L.tm_png_bound_host(32768, 32768, ctypes.byref(b)) == -1 and b.value == -3
    assert L.tm_png_bound_host(8, 4, None) == -1


# The ratio.  Palettised pictures, filter NONE: the IDAT payload against zlib.compress(stream, 1) of the same filtered stream plus 5 %
# (level 1 walks 4 candidates and parses greedily; the 5 % covers the per-segment tables and the empty blocks between segments).
# Measured with the host twin (kDepth 32, greedy, matches of 3 dropped beyond 4096), zlib 1.2.11 beside it:
#     264 x 136:   ours  13 742   zlib level 1  17 895   level 6  13 159   bar  18 789
#   1280 x 720:    ours 240 165   zlib level 1 413 176   level 6 217 000   bar 433 834
@pytest.mark.parametrize("shape", [(264, 136), (1280, 720)], ids=lambda s: "%dx%d" % s)
def test_ratio_against_zlib_level_1(shape):
    w, h = shape
    frame = png_cases.picture("palettised", w, h)[0]
    stream = png_cases.filter_rows_host(frame, "none")
    payload = png_cases.idat(png_cases.encode_host(frame[None], 1, "none")[0])
    assert zlib.decompress(payload) == stream
    level1, level6 = len(zlib.compress(stream, 1)), len(zlib.compress(stream, 6))
    print("ratio %dx%d: ours %d, zlib level 1 %d, level 6 %d" % (w, h, len(payload), level1, level6))
    assert len(payload) <= 1.05 * level1
