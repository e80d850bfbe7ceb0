"""Seeded inputs of the PNG reader's tests (tests/test_png_in_host.py, tests/test_gpu_png_in.py) and of the stand-alone sanitizer program
(tests/c/png_inflate.c reads what `python tests/png_in_cases.py FILE` writes), with what each one reaches.

Streams come from Python's zlib -- the reference -- wherever zlib can be made to write the case; what it never writes (a distance of
exactly 32768, a block without a distance code, a single distance code, every damaged header) is written by the small bit writer below.
Pictures are written by the PNG writer below (forced filter types, any IDAT layout), by Pillow, and by this library's level-1 export."""
import functools
import struct
import sys
import zlib

import numpy as np

# ---- a deflate writer of the test's own ------------------------------------------------------------------------------------------------


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):  # lowest bit first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):  # a Huffman code: highest bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """{symbol: (code, length)} of a set of code lengths (RFC 1951, 3.2.2); an over-subscribed set still gets numbers"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def put_tokens(b, tokens, lit_lens, dist_lens):
    """tokens: ints 0..255 (literals), ("m", length, distance), ("lit", symbol) / ("dist", symbol, extra) for raw symbols, "end" """
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if t == "end":
            b.code(*lit[256])
        elif isinstance(t, int):
            b.code(*lit[t])
        elif t[0] == "lit":
            b.code(*lit[t[1]])
        elif t[0] == "dist":
            b.code(*dist[t[1]])
            b.put(t[2], _DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        else:
            _, length, distance = t
            ls = 28 if length == 258 else max(i for i in range(28) if _LEN_BASE[i] <= length)
            b.code(*lit[257 + ls])
            b.put(length - _LEN_BASE[ls], _LEN_EXTRA[ls])
            ds = max(i for i in range(30) if _DIST_BASE[i] <= distance)
            b.code(*dist[ds])
            b.put(distance - _DIST_BASE[ds], _DIST_EXTRA[ds])


def fixed_block(b, tokens, final=True):
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LIT, FIXED_DIST)


def dynamic_block(b, tokens, lit_lens, dist_lens, final=True, cl_lens=None, cl_symbols=None):
    """a dynamic block whose code lengths are sent one by one (no repeats) with a complete code-length code: 0..15 at 4 bits each.
    cl_lens / cl_symbols override the code-length code and the symbols sent with it (damaged headers)."""
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257, 5)
    b.put(len(dist_lens) - 1, 5)
    cl = cl_lens if cl_lens is not None else [4] * 16 + [0, 0, 0]
    b.put(19 - 4, 4)
    for s in _CL_ORDER:
        b.put(cl[s], 3)
    codes = canonical(cl)
    for item in (cl_symbols if cl_symbols is not None else list(lit_lens) + list(dist_lens)):
        sym, extra, ebits = item if isinstance(item, tuple) else (item, 0, 0)
        b.code(*codes[sym])
        b.put(extra, ebits)
    if tokens is not None:
        put_tokens(b, tokens, lit_lens, dist_lens)


def stored_block(b, data, final=True, nlen=None):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.out += struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen) + data


def wrap(body, data, header=b"\x78\x9c"):
    return header + body + struct.pack(">I", zlib.adler32(data))


def first_dynamic_lengths(z):
    """the test's own parser: (literal/length code lengths, distance code lengths) of a zlib stream's first block, which must be dynamic"""
    bits = int.from_bytes(z[2:], "little")
    pos = 0

    def take(n):
        nonlocal pos
        v = (bits >> pos) & ((1 << n) - 1)
        pos += n
        return v
    take(1)
    assert take(2) == 2, "the first block is not dynamic"
    nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(ncode):
        cl[_CL_ORDER[i]] = take(3)
    by_code = {v: s for s, v in canonical(cl).items()}
    lens = []
    while len(lens) < nlen + ndist:
        code, l = 0, 0
        while True:
            code, l = (code << 1) | take(1), l + 1
            if (code, l) in by_code:
                break
            assert l < 8
        s = by_code[(code, l)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    return lens[:nlen], lens[nlen:nlen + ndist]


# ---- streams ---------------------------------------------------------------------------------------------------------------------------

def _rand(seed, n, hi=256):
    return np.random.default_rng(seed).integers(0, hi, size=n, dtype=np.uint8).tobytes()


def _mixed(seed, n):
    """text-like runs, noise and repeats: every kind of block and match at once"""
    rng = np.random.default_rng(seed)
    words = [b"tile", b"palette", b"frame ", b"motion", b" the ", b"\n", b"0123456789", bytes(40), _rand(seed + 1, 64)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))]
        if rng.integers(0, 50) == 0:
            out += _rand(int(rng.integers(0, 1 << 30)), int(rng.integers(1, 400)))
    return bytes(out[:n])


def _deflate(data, level=6, wbits=15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return co.compress(data) + co.flush()


def fibonacci_data():
    """a skewed alphabet, Fibonacci-like: byte i occurs round(1.8^i) times, shuffled -- 27 322 symbols, one block at memLevel 9, a chain of a
    code that the 15-bit limit has to flatten.  (Fibonacci's own numbers leave zlib's tree builder ties, which it settles towards a
    flat tree of at most 12 bits: the steeper ratio leaves none.)"""
    freq = [int(round(1.8 ** i)) for i in range(17)]
    data = np.concatenate([np.full(f, i, np.uint8) for i, f in enumerate(freq)])
    np.random.default_rng(21).shuffle(data)
    return data.tobytes()


def _zlib_host(data):
    import ctypes
    from tiler_amd import lib
    src = np.frombuffer(data, np.uint8)
    cap = len(data) + 10 * (len(data) // 32768 + 1) + 6
    out = np.empty(cap, np.uint8)
    n = ctypes.c_int64()
    assert lib().tm_zlib_compress_host(src.ctypes.data_as(ctypes.c_void_p), src.size, out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)) == 0
    return out[:n.value].tobytes()


@functools.lru_cache(maxsize=None)
def streams():
    """[(name, spans, data, zlib_reads_it)]: spans is the list of byte strings whose concatenation is the zlib stream"""
    out = []

    def add(name, z, data, zlib_ok=True, spans=None):
        out.append((name, tuple(spans) if spans else (z,), data, zlib_ok))
    for n in (0, 1, 2, 100, 32767, 32768, 32769, 65537, 1 << 20):
        add("mixed_%d_l6" % n, _deflate(_mixed(n, n)), _mixed(n, n))
    for n in (0, 100, 32769, 65537):
        for level in (0, 1, 9):
            add("mixed_%d_l%d" % (n, level), _deflate(_mixed(n, n), level), _mixed(n, n))
    d = _mixed(7, 65537)
    add("fixed", _deflate(d, strategy=zlib.Z_FIXED), d)
    add("huffman_only", _deflate(d, strategy=zlib.Z_HUFFMAN_ONLY), d)
    add("rle", _deflate(d, strategy=zlib.Z_RLE), d)
    add("wbits9", _deflate(d, wbits=9), d)
    add("noise", _deflate(_rand(5, 40000)), _rand(5, 40000))
    add("run_of_one_byte", _deflate(b"\x07" * 70000), b"\x07" * 70000)            # distance 1, chains of length 258
    add("period_3", _deflate(b"abc" * 9000), b"abc" * 9000)                          # d < len, d does not divide 64
    add("period_7", _deflate(b"tilemap"[:7] * 5000), b"tilemap"[:7] * 5000)
    fib = fibonacci_data()
    add("fibonacci", _deflate(fib, 6, 15, 9, zlib.Z_HUFFMAN_ONLY), fib)               # 15-bit codes
    # a match at distance exactly 32768 (zlib stops 262 short of it): 32768 stored bytes, then the same bytes as matches
    far = _rand(6, 32768)
    b = Bits()
    stored_block(b, far, final=False)
    fixed_block(b, [("m", 258, 32768)] * 126 + [("m", 3, 32768), "end"])
    add("distance_32768", wrap(b.bytes(), far + far[:258 * 126 + 3]), far + far[:258 * 126 + 3])
    # only literals: one distance code of zero bits
    lit = [0] * 257
    for s in (65, 66, 67, 256):
        lit[s] = 2
    b = Bits()
    dynamic_block(b, [65, 66, 67, 67, 65, "end"], lit, [0])
    add("no_distance_code", wrap(b.bytes(), b"ABCCA"), b"ABCCA")
    # a single distance code: one bit, the other pattern unassigned
    lit = [0] * 258
    for s in (65, 66, 256, 257):
        lit[s] = 2
    b = Bits()
    dynamic_block(b, [65, 66, ("m", 3, 1), ("m", 3, 1), "end"], lit, [1])
    add("single_distance_code", wrap(b.bytes(), b"AB" + b"B" * 6), b"AB" + b"B" * 6)
    # an incomplete literal/length code whose unassigned patterns are never met: this reader's rule, not zlib's
    lit = [0] * 257
    for s in (65, 66, 256):
        lit[s] = 2
    b = Bits()
    dynamic_block(b, [65, 66, 66, "end"], lit, [0])
    add("incomplete_code_unmet", wrap(b.bytes(), b"ABB"), b"ABB", zlib_ok=False)
    # an empty stored block in the middle (a sync flush), and an empty final one
    co = zlib.compressobj(6)
    d1, d2 = _mixed(8, 5000), _mixed(9, 7000)
    add("empty_stored_inside", co.compress(d1) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(d2) + co.flush(), d1 + d2)
    b = Bits()
    fixed_block(b, [104, 105, "end"], final=False)
    stored_block(b, b"")
    add("empty_stored_last", wrap(b.bytes(), b"hi"), b"hi")
    own = _mixed(10, 100000)
    add("own_level1", _zlib_host(own), own)                                           # segments behind empty stored blocks
    # span layouts: 1-byte spans, an empty span inside, a split inside a Huffman code (any odd split of a dynamic block is)
    z, d = _deflate(_mixed(11, 3000)), _mixed(11, 3000)
    add("spans_of_1", z, d, spans=[z[i:i + 1] for i in range(len(z))])
    add("span_empty_inside", z, d, spans=[z[:700], b"", z[700:701], b"", b"", z[701:]])
    add("spans_split_header", z, d, spans=[z[:1], z[1:3], z[3:len(z) - 2], z[len(z) - 2:]])
    return out


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """[(name, stream bytes, cap)]: every one is refused"""
    out = []
    rng = np.random.default_rng(12)
    data = bytes(rng.integers(0, 64, 20000, dtype=np.uint8))
    for level in (0, 6):
        z = zlib.compress(data, level)
        out.append(("short_destination_l%d" % level, z, len(data) - 1))
        for cut in (0, 1, 2, 5, len(z) // 2, len(z) - 5, len(z) - 1):
            out.append(("cut_%d_l%d" % (cut, level), z[:cut], len(data)))
        bad = bytearray(z); bad[-1] ^= 1
        out.append(("adler_l%d" % level, bytes(bad), len(data)))
        bad = bytearray(z); bad[0] = 0x79
        out.append(("header_l%d" % level, bytes(bad), len(data)))
    z = zlib.compress(b"preset dictionary", 6)
    flg = next(f for f in range(0x20, 0x40) if (0x7800 | f) % 31 == 0)
    out.append(("fdict", bytes([0x78, flg]) + z[2:], 100))
    out.append(("window_too_large", bytes([0x88, next(f for f in range(32) if (0x8800 | f) % 31 == 0)]) + z[2:], 100))

    def hand(name, build, data=b"", cap=4096):
        b = Bits()
        build(b)
        out.append((name, wrap(b.bytes(), data), cap))
    hand("distance_past_start", lambda b: fixed_block(b, [97, ("m", 3, 2), "end"]))
    hand("length_symbol_286", lambda b: fixed_block(b, [97, ("lit", 286), ("dist", 0, 0), "end"]))
    hand("distance_symbol_30", lambda b: fixed_block(b, [97, ("lit", 257), ("dist", 30, 0), "end"]))
    hand("block_type_3", lambda b: (b.put(1, 1), b.put(3, 2), b.put(0, 13)))
    hand("stored_nlen", lambda b: stored_block(b, b"abc", nlen=0x1234))
    hand("stored_cut", lambda b: (b.put(1, 1), b.put(0, 2), b.align(), b.out.extend(struct.pack("<HH", 500, 500 ^ 0xffff) + b"abc")))
    over = [0] * 257
    for s in (65, 66, 256):
        over[s] = 1
    hand("over_subscribed", lambda b: dynamic_block(b, None, over, [0]))
    no_eob = [0] * 257
    no_eob[65] = no_eob[66] = 1
    hand("no_end_of_block", lambda b: dynamic_block(b, None, no_eob, [0]))
    hand("over_subscribed_cl", lambda b: dynamic_block(b, None, [0] * 257, [0], cl_lens=[1, 1, 1] + [0] * 16, cl_symbols=[]))
    hand("repeat_first", lambda b: dynamic_block(b, None, [0] * 257, [0], cl_lens=[2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0], cl_symbols=[(16, 0, 2)]))
    hand("lengths_overrun", lambda b: dynamic_block(b, None, [0] * 257, [0], cl_lens=[2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2],
                                                    cl_symbols=[1] + [(18, 127, 7)] * 2))
    lit = [0] * 257
    for s in (65, 66, 256):
        lit[s] = 2
    hand("unassigned_code_met", lambda b: (dynamic_block(b, [65, 66], lit, [0]), b.put(3, 2)))   # the pattern 11 is no code
    hand("match_without_distance_code", lambda b: (dynamic_block(b, [65, ("lit", 257)], [2 if s in (65, 256, 257) else 0 for s in range(258)], [0]), b.put(0, 8)))
    hand("input_ends_in_match", lambda b: (fixed_block(b, [97, ("lit", 285)]), None))
    hand("hlit_287", lambda b: (b.put(1, 1), b.put(2, 2), b.put(30, 5), b.put(0, 5), b.put(0, 4), b.put(0, 64)))
    hand("destination_one_short", lambda b: fixed_block(b, [97, ("m", 258, 1), "end"]), b"a" * 259, cap=258)
    return out


# ---- pictures --------------------------------------------------------------------------------------------------------------------------
# (width, height): 64 x 65 and 3 x 130 cross the 64-row pass with a width below the lanes' skew; 131 x 67 and 264 x 136 have odd row
# bytes and several passes; 10923 x 1 is one row of 32 770 bytes (more than the window)
SHAPES = [(1, 1), (5, 3), (37, 21), (64, 65), (3, 130), (131, 67), (264, 136), (10923, 1)]
COLOUR_TYPES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}  # colour type -> bytes per pixel
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def filter_rows(rows, bpp, types):
    """rows: uint8 [h][w bpp]; types: a filter type per row -> the stream of filtered rows (types above 4 are written as type 0's bytes)"""
    raw = bytearray()
    prev = np.zeros(rows.shape[1], np.int64)
    for y in range(rows.shape[0]):
        cur = rows[y].astype(np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]])
        ft = int(types[y])
        if ft == 1: pred = a
        elif ft == 2: pred = prev
        elif ft == 3: pred = (a + prev) >> 1
        elif ft == 4:
            p = a + prev - c
            pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        else: pred = 0
        raw += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(raw)


def make_png(rows, w, h, ctype, types, palette=None, level=6, layout="one", raw=None):
    """layout: "one" IDAT; "bytes": 1-byte IDATs; "empty_between": an empty IDAT between two; "in_code": a split 3 bytes into the stream,
    inside the dynamic header or the first codes"""
    z = zlib.compress(filter_rows(rows, COLOUR_TYPES[ctype], types) if raw is None else raw, level)
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", palette.astype(np.uint8).tobytes())
    if layout == "one": parts = [z]
    elif layout == "bytes": parts = [z[i:i + 1] for i in range(len(z))]
    elif layout == "empty_between": parts = [z[:len(z) // 2], b"", z[len(z) // 2:]]
    else: parts = [z[:3], z[3:]]
    if layout != "one":
        out += chunk(b"tEXt", b"Comment\0several IDAT chunks follow")
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def _content(w, h, ctype, seed):
    """(rows uint8 [h][w bpp], palette or None): smooth in parts (so that every filter predicts something) and noisy in others"""
    rng = np.random.default_rng([seed, w, h, ctype])
    bpp = COLOUR_TYPES[ctype]
    yy, xx = np.mgrid[0:h, 0:w]
    if ctype == 3:
        pal = rng.integers(0, 256, (200, 3)).astype(np.uint8)
        return rng.integers(0, 200, (h, w)).astype(np.uint8), pal
    ch = [((xx * 7 + yy * 3) & 255), ((yy * 11 + xx) & 255), rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))]
    px = np.stack([ch[k % 4] for k in range(bpp)], 2).astype(np.uint8)
    return px.reshape(h, w * bpp), None


@functools.lru_cache(maxsize=None)
def pictures():
    """[(name, w, h, file bytes)] -- every one decodes"""
    out = []
    for w, h in SHAPES:
        for ctype in COLOUR_TYPES:
            rows, pal = _content(w, h, ctype, 13)
            for ft in range(5):
                out.append(("%dx%d_c%d_f%d" % (w, h, ctype, ft), w, h, make_png(rows, w, h, ctype, [ft] * h, pal)))
            mixed = np.random.default_rng([w, h, ctype]).integers(0, 5, h)
            out.append(("%dx%d_c%d_mixed" % (w, h, ctype), w, h, make_png(rows, w, h, ctype, mixed, pal, level=1)))
    rows, _ = _content(5, 3, 2, 14)
    for layout in ("bytes", "empty_between", "in_code"):
        out.append(("5x3_idat_" + layout, 5, 3, make_png(rows, 5, 3, 2, [4, 3, 1], layout=layout)))
    rows, _ = _content(131, 67, 6, 14)
    for layout in ("empty_between", "in_code"):
        out.append(("131x67_idat_" + layout, 131, 67, make_png(rows, 131, 67, 6, [4] * 67, layout=layout)))
    import io
    from PIL import Image
    for (w, h) in ((37, 21), (264, 136)):
        for mode, ctype in (("L", 0), ("LA", 4), ("RGB", 2), ("RGBA", 6), ("P", 3)):
            rows, pal = _content(w, h, ctype, 15)
            im = Image.fromarray(rows.reshape(h, w, -1).squeeze(), mode)
            if pal is not None:
                im.putpalette(pal.tobytes())
            for level in (0, 1, 9):
                buf = io.BytesIO()
                im.save(buf, "PNG", compress_level=level)
                out.append(("pillow_%dx%d_%s_l%d" % (w, h, mode, level), w, h, buf.getvalue()))
    from tests import png_cases
    for (w, h) in ((37, 21), (264, 136)):
        for content in ("gradient", "palettised"):
            for filt in ("none", "adaptive"):
                f = png_cases.encode_host(png_cases.picture(content, w, h), 1, filt)[0]
                out.append(("own_%dx%d_%s_%s" % (w, h, content, filt), w, h, f))
    return out


@functools.lru_cache(maxsize=None)
def damaged_pictures():
    """[(name, w, h, file bytes)]: the container is sound, decoding refuses each (filter type 5; an index equal to the palette's size;
    a row too few; a byte too many; a damaged stream)"""
    w, h = 37, 70
    rows, _ = _content(w, h, 2, 16)
    types = [4] * h
    types[66] = 5
    out = [("filter_type_5", w, h, make_png(rows, w, h, 2, types))]
    idx, pal = _content(w, h, 3, 16)
    idx = idx.copy()
    idx[65, 20] = 200  # npal = 200
    out.append(("palette_index_npal", w, h, make_png(idx, w, h, 3, [1] * h, pal)))
    raw = filter_rows(rows, 3, [2] * h)
    out.append(("row_missing", w, h, make_png(rows, w, h, 2, None, raw=raw[:-(1 + 3 * w)])))
    out.append(("byte_too_many", w, h, make_png(rows, w, h, 2, None, raw=raw + b"\0")))
    good = make_png(rows, w, h, 2, [2] * h)
    at = good.index(b"IDAT") + 4
    n, = struct.unpack(">I", good[at - 8:at - 4])
    z = bytearray(good[at:at + n])
    z[-1] ^= 1  # the Adler-32
    out.append(("adler", w, h, good[:at - 8] + chunk(b"IDAT", bytes(z)) + good[at + n + 4:]))
    return out


# ---- for tests/c/png_inflate.c ---------------------------------------------------------------------------------------------------------

def dump(path):
    """every case as records: u32 kind (0 a stream that decodes, 1 a damaged stream, 2 a picture that decodes, 3 a damaged picture), then
    kind 0 / 1: u32 cap, u32 nspans, per span u32 length + bytes, u32 data length + bytes (kind 1: 0);  kind 2 / 3: u32 w, u32 h, u32 length + bytes"""
    with open(path, "wb") as f:
        for name, spans, data, _ in streams():
            if len(data) > 200000:
                continue  # (the program's fuzz damages every stream it is given many times over)
            f.write(struct.pack("<III", 0, len(data), len(spans)))
            for s in spans:
                f.write(struct.pack("<I", len(s)) + s)
            f.write(struct.pack("<I", len(data)) + data)
        for name, z, cap in damaged_streams():
            f.write(struct.pack("<IIII", 1, cap, 1, len(z)) + z + struct.pack("<I", 0))
        for kind, cases in ((2, pictures()), (3, damaged_pictures())):
            for name, w, h, png in cases:
                f.write(struct.pack("<IIII", kind, w, h, len(png)) + png)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump(sys.argv[1])
