"""Seeded inputs of the PNG writer's tests (tests/test_png_out_host.py, tests/test_gpu_png_out.py) and thin wrappers of its host seams:
pictures of four kinds at the smallest shapes at which the writer can go wrong, byte streams for the stream coder alone, and Python
restatements of the parts of the rule that fit in a few lines (the stored writer, the adaptive filter choice)."""
import ctypes
import functools
import struct
import zlib

import numpy as np

# (width, height): the smallest picture; a 48-byte stream (stored wins); one segment; odd row bytes; 107 848 bytes = 3.3 segments; one row
# of 32 770 bytes across a segment edge
SHAPES = [(1, 1), (5, 3), (40, 24), (131, 67), (264, 136), (10923, 1)]
CONTENTS = ["constant", "gradient", "noise", "palettised"]
FILTERS = {"none": 1, "adaptive": 2, "smaller": 3}  # TM_PNG_FILTER_*

_BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38], [60, 28, 52, 20, 62, 30, 54, 22],
                    [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25], [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.float64)


@functools.lru_cache(maxsize=None)
def picture(content, w, h, frames=1, seed=0):
    """uint32 [frames][h][w], 0x00RRGGBB (read-only: shared between tests)"""
    rng = np.random.default_rng([seed, w, h, frames, CONTENTS.index(content)])
    f, y, x = np.meshgrid(np.arange(frames), np.arange(h), np.arange(w), indexing="ij")
    if content == "constant":
        out = np.full((frames, h, w), 0x336699, np.uint32) + f.astype(np.uint32)
    elif content == "gradient":
        r, g, b = (x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y + 9 * f) // 2) % 256
        out = (r.astype(np.uint32) << 16) | (g.astype(np.uint32) << 8) | b.astype(np.uint32)
    elif content == "noise":
        out = rng.integers(0, 1 << 24, size=(frames, h, w), dtype=np.uint32)
    else:  # 16 palettes of 16 colours, one per 8 x 8 tile; a ramp ordered-dithered to the palette's 16 entries
        pals = rng.integers(0, 1 << 24, size=(16, 16), dtype=np.uint32)
        tile_pal = rng.integers(0, 16, size=(frames, (h + 7) // 8, (w + 7) // 8))
        level = (x + 2 * y + 3 * f) * 15.0 / (w + 2 * h + 3 * frames) + (_BAYER8[y % 8, x % 8] + 0.5) / 64.0
        out = pals[tile_pal[f, y // 8, x // 8], np.clip(level.astype(np.int64), 0, 15)]
    out = np.ascontiguousarray(out, np.uint32)
    out.setflags(write=False)
    return out


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


_TEXT = ("The export side gets a PNG writer that runs on the device: filter, match, parse, code and pack. "
         "Only finished file bytes cross the link; the rule is stated once and shared by a host twin. ").encode() * 40
STREAMS = {
    "empty": b"",
    "one": b"\x07",
    "two_equal": b"\x07" * 2,
    "three_equal": b"\x07" * 3,
    "run_259": b"\x07" * 259,
    "zeros_3_segments": bytes(98304),             # runs across segments
    "period_32768": _rand(1, 32768) * 3,          # a distance exactly at the limit
    "period_32769": _rand(2, 32769) * 3,          # one past the limit
    "noise_100000": _rand(3, 100000),
    "text": _TEXT,
}


def _lib():
    from tiler_amd import lib
    return lib()


def _options(level, filter):
    from tiler_amd._lib import png_options
    return png_options(level, filter)


def strided(frames, row_pad=0, frame_pad=0):
    """the frames inside a larger buffer: rows row_pad pixels longer, frames frame_pad pixels further apart; the padding holds 0xFFFFFFFF"""
    nf, h, w = frames.shape
    stride = w + row_pad
    frame_px = h * stride + frame_pad
    buf = np.full(nf * frame_px, 0xFFFFFFFF, np.uint32)
    view = np.lib.stride_tricks.as_strided(buf, (nf, h, w), (frame_px * 4, stride * 4, 4))
    view[...] = frames
    return buf, stride, frame_px


def split(buf, offsets):
    return [bytes(buf[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]


def encode_host(frames, level=1, filter="none", row_pad=0, frame_pad=0):
    """tm_png_encode_host -> list of bytes"""
    nf, h, w = frames.shape
    buf, stride, frame_px = strided(frames, row_pad, frame_pad)
    bound = ctypes.c_int64()
    assert _lib().tm_png_bound_host(w, h, ctypes.byref(bound)) == 0
    out = np.empty(bound.value * max(nf, 1), np.uint8)
    offs = (ctypes.c_int64 * (nf + 1))()
    rc = _lib().tm_png_encode_host(buf.ctypes.data_as(ctypes.c_void_p), stride, frame_px, nf, w, h, ctypes.byref(_options(level, filter)),
                                   out.ctypes.data_as(ctypes.c_void_p), out.size, offs)
    assert rc == 0, _lib().tm_last_error()
    return split(out, list(offs))


def filter_rows_host(frame, filter):
    h, w = frame.shape
    frame = np.ascontiguousarray(frame, np.uint32)
    out = np.empty(h * (1 + 3 * w), np.uint8)
    assert _lib().tm_png_filter_rows_host(frame.ctypes.data_as(ctypes.c_void_p), w, w, h, FILTERS[filter], out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out.tobytes()


def zlib_host(data):
    src = np.frombuffer(data, np.uint8)
    cap = len(data) + 10 * (len(data) // 32768 + 1) + 6
    out = np.empty(cap, np.uint8)
    n = ctypes.c_int64()
    rc = _lib().tm_zlib_compress_host(src.ctypes.data_as(ctypes.c_void_p) if src.size else None, src.size, out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n))
    assert rc == 0, _lib().tm_last_error()
    return out[:n.value].tobytes()


def inflate_host(z, n):
    src = np.frombuffer(z, np.uint8)
    dst = np.empty(max(n, 1), np.uint8)
    got = ctypes.c_size_t()
    assert _lib().tm_inflate_host(src.ctypes.data_as(ctypes.c_void_p), src.size, dst.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(got)) == 0, _lib().tm_last_error()
    return dst[:got.value].tobytes()


def read_png_host(path, w, h):
    out = np.empty((h, w), np.uint32)
    gw, gh = ctypes.c_int(), ctypes.c_int()
    assert _lib().tm_read_png_host(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), w * h, ctypes.byref(gw), ctypes.byref(gh)) == 0, _lib().tm_last_error()
    assert (gw.value, gh.value) == (w, h)
    return out


def pillow_pixels(png):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB"
    a = np.asarray(im).astype(np.uint32)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def chunks(png):
    """[(type, payload)] of a PNG, CRCs checked"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        kind, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data)
        out.append((kind, data))
        at += 12 + n
    return out


def idat(png):
    c = chunks(png)
    assert [k for k, _ in c] == [b"IHDR", b"IDAT", b"IEND"]
    return c[1][1]


def raw_rows(frame):
    """uint8 [h][3 w]: R, G, B of every pixel"""
    return np.stack([(frame >> 16) & 0xff, (frame >> 8) & 0xff, frame & 0xff], axis=-1).astype(np.uint8).reshape(frame.shape[0], -1)


def stored_png(frame):
    """the level-0 writer restated: filter 0 rows in stored blocks of 65535 bytes, zlib header 78 01"""
    h, w = frame.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), raw_rows(frame)], axis=1).tobytes()
    z = b"\x78\x01"
    for off in range(0, max(len(raw), 1), 65535):
        part = raw[off:off + 65535]
        z += struct.pack("<BHH", off + 65535 >= len(raw), len(part), len(part) ^ 0xffff) + part
    z += struct.pack(">I", zlib.adler32(raw))
    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def adaptive_types(frame):
    """the ADAPTIVE rule restated: per row the type 0..4 with the least sum of |(int8) byte|, bpp 3, zeros above row 0, ties to the lowest"""
    x = raw_rows(frame).astype(np.int32)
    a = np.concatenate([np.zeros((x.shape[0], 3), np.int32), x[:, :-3]], axis=1)
    b = np.concatenate([np.zeros((1, x.shape[1]), np.int32), x[:-1]], axis=0)
    c = np.concatenate([np.zeros((x.shape[0], 3), np.int32), b[:, :-3]], axis=1)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    costs = []
    for pred in (0, a, b, (a + b) // 2, paeth):
        v = (x - pred) & 0xff
        costs.append(np.where(v < 128, v, 256 - v).sum(axis=1))
    return np.argmin(np.stack(costs, axis=1), axis=1).astype(np.uint8)
