"""Load's input path, the host side (no GPU): resampling tables, the colour rules, inflate, the PNG reader and the probe of
InputFileName (tm_resample_taps_host, tm_inflate_host, tm_read_png_host, tm_probe_input_host) against numpy restatements, zlib and Pillow."""
import ctypes
import math
import os
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import resample_ref, yuv_ref
from tiler_amd._lib import lib, TileMotionError, check

E_INVAL, E_IO, E_UNSUPPORTED = -1, -5, -6
Y4M, PNGS = 1, 2


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib_taps(n, m, n_plane, s, o_halves):
    first, count = np.zeros(m, np.int32), np.zeros(m, np.int32)
    coef = np.full((m, 64), 12345, np.int32)
    check(lib().tm_resample_taps_host(n, m, n_plane, s, o_halves, _vp(first), _vp(count), _vp(coef)))
    return first, count, coef


def assert_same_taps(n, m, n_plane, s, o):
    first, count, coef = lib_taps(n, m, n_plane, s, int(o * 2))
    ref = resample_ref.taps(n, m, n_plane, s, o)
    assert len(ref) == m
    for j, (k0, c) in enumerate(ref):
        assert (first[j], count[j]) == (k0, len(c)), (n, m, s, o, j)
        assert coef[j, :len(c)].tolist() == c and not coef[j, len(c):].any(), (n, m, s, o, j)
        assert sum(c) == 16384


# ---- 1. the tables
@pytest.mark.parametrize("n", [100, 52, 64, 101, 53, 720])
def test_tap_tables_match_the_numpy_rule(n):
    sizes = sorted({max(1, math.ceil(n / 8)), n // 3, n // 2, round(n * 0.75), n - 1, n, n + 1, round(n * 1.5), n * 2} | set(range(max(1, math.ceil(n / 8)), n * 2, 37)))
    for m in sizes:
        assert_same_taps(n, m, n, 1, 0.0)                  # luma, 4:4:4 chroma
        assert_same_taps(n, m, (n + 1) // 2, 2, 0.0)       # co-sited chroma (4:2:2, 4:2:0 mpeg2 horizontally)
        assert_same_taps(n, m, (n + 1) // 2, 2, 0.5)       # centred chroma (4:2:0 jpeg; mpeg2 vertically)


def test_equal_size_tables_are_the_identity():
    for n in (1, 2, 7, 64, 101):
        first, count, coef = lib_taps(n, n, n, 1, 0)
        for j in range(n):  # (the neighbours at whole distances are in the window with weight sin(k pi) ~ 1e-17: coefficient 0)
            c = coef[j, :count[j]]
            assert np.count_nonzero(c) == 1 and c[j - first[j]] == 16384 and not coef[j, count[j]:].any()
    # the co-sited samples of 4:2:2 / 4:2:0 mpeg2: even luma columns take their chroma sample as it is
    first, count, coef = lib_taps(100, 100, 50, 2, 0)
    for j in range(0, 100, 2):
        c = coef[j, :count[j]]
        assert c.max() == 16384 and np.count_nonzero(c) == 1 and first[j] + int(c.argmax()) == j // 2


def test_tables_refuse_more_than_eightfold_shrinking():
    first, count, coef = np.zeros(12, np.int32), np.zeros(12, np.int32), np.zeros((12, 64), np.int32)
    L = lib()
    assert L.tm_resample_taps_host(100, 12, 100, 1, 0, _vp(first), _vp(count), _vp(coef)) == E_UNSUPPORTED
    assert b"more than 8" in L.tm_last_error()
    assert L.tm_resample_taps_host(100, 12, 50, 2, 0, _vp(first), _vp(count), _vp(coef)) == 0  # the chroma plane shrinks by 4.17 only
    assert L.tm_resample_taps_host(100, 6, 50, 2, 1, _vp(first), _vp(count), _vp(coef)) == E_UNSUPPORTED
    assert L.tm_resample_taps_host(0, 6, 50, 1, 0, _vp(first), _vp(count), _vp(coef)) == E_INVAL
    assert L.tm_resample_taps_host(10, 6, 10, 3, 0, _vp(first), _vp(count), _vp(coef)) == E_INVAL
    with pytest.raises(ValueError):
        resample_ref.taps(100, 12, 100, 1, 0.0)


def test_vertical_sums_fit_32_bits_over_the_supported_range():
    """the bound behind the second refusal, (255 A_h / 128 + 1) A_v < 2^31 with A the largest sum |c| of an axis: over the supported
    ratios the coefficients stay far below it, so that check never fires in range"""
    worst, most = 0, 0
    for n in (100, 101, 720):
        for m in range(math.ceil(n / 8), 2 * n + 1, 7):
            for n_plane, s, oh in ((n, 1, 0), ((n + 1) // 2, 2, 0), ((n + 1) // 2, 2, 1)):
                _, count, coef = lib_taps(n, m, n_plane, s, oh)
                worst, most = max(worst, int(np.abs(coef).sum(1).max())), max(most, int(count.max()))
    assert most <= 64
    assert (255 * worst // 128 + 1) * worst < 2 ** 31, worst


# ---- 2. the rule against Pillow, smooth pictures only
def _smooth(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("w,h", [(100, 52), (64, 48), (1280, 720)])
def test_rule_is_within_one_of_pillow_lanczos_on_a_smooth_picture(w, h):
    img = _smooth(w, h)
    for sc in (0.3, 0.5, 0.75, 1.5):
        dw, dh = int(np.rint(w * sc)), int(np.rint(h * sc))
        got = resample_ref.resample(img, w, h, dw, dh)
        ref = np.asarray(Image.fromarray(img).resize((dw, dh), Image.LANCZOS))
        d = int(np.abs(got.astype(int) - ref.astype(int)).max())
        print(w, h, sc, "max difference", d)
        assert d <= 1


@pytest.mark.parametrize("w,h", [(100, 52), (64, 48)])
def test_centred_half_size_plane_is_within_one_of_pillow(w, h):
    """a half-size plane with s = 2, o = 0.5 (4:2:0 jpeg chroma): scaling it to the luma size times 0.5 .. 1.5 is Pillow's resize of the
    plane by twice that, whose sample centres are the same"""
    plane = _smooth(w // 2, h // 2)
    for sc in (0.5, 0.75, 1.0, 1.5):
        dw, dh = int(np.rint(w * sc)), int(np.rint(h * sc))
        got = resample_ref.resample(plane, w, h, dw, dh, 2, 2, 0.5, 0.5)
        ref = np.asarray(Image.fromarray(plane).resize((dw, dh), Image.LANCZOS))
        d = int(np.abs(got.astype(int) - ref.astype(int)).max())
        print(w, h, sc, "max difference", d)
        assert d <= 1


# ---- 3. colour
def test_tiler_rule_matches_the_oracle(oracle):
    rng = np.random.default_rng(5)
    yuv = np.concatenate([rng.integers(0, 256, (1 << 16, 3)), np.array([[a, b, c] for a in (0, 255) for b in (0, 255) for c in (0, 255)])])
    got = yuv_ref.to_rgb32(yuv[:, 0], yuv[:, 1], yuv[:, 2], yuv_ref.TILER)
    for i, (y, u, v) in enumerate(yuv.tolist()):
        o = oracle.L.tmo_yuv_to_rgb(float(y), float(u - 128), float(v - 128)) & 0xFFFFFFFF  # 0x00BBGGRR
        exp = (o & 0xff) << 16 | (o & 0xff00) | (o >> 16) & 0xff
        assert int(got[i]) == exp, (y, u, v)


def test_bt601_full_is_within_one_of_pillow_on_every_triple():
    Y, U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    R, G, B = yuv_ref.rgb_channels(Y.ravel(), U.ravel(), V.ravel(), yuv_ref.BT601_FULL)
    ycc = np.stack([Y.ravel(), U.ravel(), V.ravel()], 1).reshape(4096, 4096, 3)
    pil = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB")).reshape(-1, 3).astype(np.int64)
    d = int(np.abs(np.stack([R, G, B], 1) - pil).max())
    print("BT601_FULL against Pillow, max difference", d)
    assert d <= 1


def test_bt601_limited_end_points():
    assert yuv_ref.to_rgb32(16, 128, 128, yuv_ref.BT601_LIMITED) == 0 and yuv_ref.to_rgb32(235, 128, 128, yuv_ref.BT601_LIMITED) == 0xffffff
    assert yuv_ref.to_rgb32(0, 128, 128, yuv_ref.AUTO) == 0 and yuv_ref.to_rgb32(255, 128, 128, yuv_ref.BT601_FULL) == 0xffffff


# ---- 4. inflate and the PNG reader
def inflate(data, cap):
    src = np.frombuffer(bytes(data), np.uint8).copy()  # (an exact-size copy: a read past the end is a read past the allocation)
    dst = np.zeros(max(cap, 1), np.uint8)
    n = ctypes.c_size_t(0)
    rc = lib().tm_inflate_host(_vp(src) if len(src) else None, len(src), _vp(dst), cap, ctypes.byref(n))
    return rc, dst[:n.value].tobytes()


def _buffers():
    rng = np.random.default_rng(11)
    words = [b"tile", b"palette", b"frame ", b"motion", b" the ", b"\n", b"0123456789"]
    for n in (0, 1, 2, 100, 4095, 65535, 65536, 70001, 1 << 20):
        yield "random", rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        yield "constant", b"\x5a" * n
        yield "text", b"".join(words[i] for i in rng.integers(0, len(words), n // 5 + 1))[:n]


def test_inflate_matches_zlib():
    for kind, data in _buffers():
        for level in (0, 1, 6, 9):
            rc, out = inflate(zlib.compress(data, level), len(data))
            assert rc == 0 and out == data, (kind, len(data), level)
    # fixed Huffman blocks (what zlib picks for short inputs) and a raw strategy that forces them
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    data = b"abracadabra " * 400
    rc, out = inflate(co.compress(data) + co.flush(), len(data))
    assert rc == 0 and out == data


def test_inflate_refuses_damaged_streams():
    rng = np.random.default_rng(12)
    data = bytes(rng.integers(0, 64, 20000, dtype=np.uint8))
    for level in (0, 6):
        z = zlib.compress(data, level)
        assert inflate(z, len(data) - 1)[0] == E_INVAL               # does not fit
        for cut in (0, 1, 2, 5, len(z) // 2, len(z) - 5, len(z) - 1):  # cut short (the last: inside the Adler-32)
            assert inflate(z[:cut], len(data))[0] == E_INVAL, (level, cut)
        bad = bytearray(z); bad[-1] ^= 1
        assert inflate(bad, len(data))[0] == E_INVAL                  # checksum
        bad = bytearray(z); bad[0] = 0x79
        assert inflate(bad, len(data))[0] == E_INVAL                  # header
        for _ in range(300):                                          # any damage is either refused or decodes to something: never a crash
            bad = bytearray(z)
            for _ in range(int(rng.integers(1, 4))):
                bad[int(rng.integers(2, len(z)))] = int(rng.integers(0, 256))
            rc, out = inflate(bad, len(data) + 100)
            assert rc in (0, E_INVAL) and (rc != 0 or out == data or len(out) <= len(data) + 100)
    for _ in range(300):  # noise behind a valid header
        junk = b"\x78\x9c" + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))
        assert inflate(junk, 4096)[0] in (0, E_INVAL)


def read_png(path, cap=None):
    w, h = ctypes.c_int(), ctypes.c_int()
    check(lib().tm_read_png_host(os.fsencode(str(path)), None, 0, ctypes.byref(w), ctypes.byref(h)))
    out = np.zeros((h.value, w.value), np.uint32)
    rc = lib().tm_read_png_host(os.fsencode(str(path)), _vp(out), out.size if cap is None else cap, ctypes.byref(w), ctypes.byref(h))
    if rc:
        raise TileMotionError(rc, lib().tm_last_error().decode())
    return out


def _filtered_png(rows, w, h, colour_type, bpp, ft, palette=None):
    """a PNG with filter type ft forced on every row (Pillow picks its own filters: this writer is the test's)"""
    import struct
    raw = bytearray()
    prev = np.zeros(w * bpp, np.int64)
    for y in range(h):
        cur = rows[y].astype(np.int64).ravel()
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]])
        if ft == 0: pred = 0
        elif ft == 1: pred = a
        elif ft == 2: pred = prev
        elif ft == 3: pred = (a + prev) >> 1
        else:
            p = a + prev - c
            pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        raw += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    z = zlib.compress(bytes(raw), 6)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", palette.astype(np.uint8).tobytes())
    out += chunk(b"tEXt", b"Comment\0two IDAT chunks follow")
    return out + chunk(b"IDAT", z[:len(z) // 2]) + chunk(b"IDAT", z[len(z) // 2:]) + chunk(b"IEND", b"")


def _pictures():
    rng = np.random.default_rng(13)
    w, h = 37, 21
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(xx * 7 + yy) & 255, (yy * 11) & 255, rng.integers(0, 256, (h, w))], 2).astype(np.uint8)
    alpha = rng.integers(0, 256, (h, w, 1)).astype(np.uint8)
    pal = rng.integers(0, 256, (200, 3)).astype(np.uint8)
    idx = rng.integers(0, 200, (h, w)).astype(np.uint8)
    grey = rgb[:, :, 0]
    as32 = lambda a: (a[..., 0].astype(np.uint32) << 16) | (a[..., 1].astype(np.uint32) << 8) | a[..., 2]
    g32 = grey.astype(np.uint32) * 0x010101
    return [("L", 0, 1, grey, g32, None), ("LA", 4, 2, np.concatenate([grey[..., None], alpha], 2), g32, None), ("RGB", 2, 3, rgb, as32(rgb), None),
            ("RGBA", 6, 4, np.concatenate([rgb, alpha], 2), as32(rgb), None), ("P", 3, 1, idx, as32(pal[idx]), pal)]


def test_png_reader_reads_pillow_files(tmp_path):
    for mode, _, _, data, exp, pal in _pictures():
        im = Image.fromarray(data, mode)
        if pal is not None:
            im.putpalette(pal.tobytes())
        for level in (0, 1, 9):
            p = tmp_path / f"{mode}_{level}.png"
            im.save(p, compress_level=level)
            assert np.array_equal(read_png(p), exp), (mode, level)


def test_png_reader_undoes_every_filter(tmp_path):
    for mode, ctype, bpp, data, exp, pal in _pictures():
        h, w = data.shape[:2]
        for ft in range(5):
            p = tmp_path / f"{mode}_f{ft}.png"
            p.write_bytes(_filtered_png(data.reshape(h, -1), w, h, ctype, bpp, ft, pal))
            assert np.array_equal(np.asarray(Image.open(p).convert("RGB")).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32), exp)  # the writer is right
            assert np.array_equal(read_png(p), exp), (mode, ft)


def test_png_reader_refusals(tmp_path):
    L = lib()
    mode, ctype, bpp, data, exp, _ = _pictures()[2]
    h, w = data.shape[:2]
    good = _filtered_png(data.reshape(h, -1), w, h, ctype, bpp, 4)
    p = tmp_path / "x.png"

    def rc_of(blob, cap=1 << 20):
        p.write_bytes(blob)
        out = np.zeros(1 << 12, np.uint32)
        ww, hh = ctypes.c_int(), ctypes.c_int()
        return L.tm_read_png_host(os.fsencode(str(p)), _vp(out), min(cap, out.size), ctypes.byref(ww), ctypes.byref(hh))
    assert rc_of(good) == 0
    assert rc_of(good, cap=w * h - 1) == E_INVAL
    assert rc_of(b"not a png at all, but long enough to hold a header of one") == E_UNSUPPORTED
    for cut in (20, 40, len(good) // 2, len(good) - 12, len(good) - 1):
        assert rc_of(good[:cut]) in (E_INVAL, E_UNSUPPORTED), cut
    bad = bytearray(good); bad[len(good) // 2] ^= 0x10
    assert rc_of(bytes(bad)) == E_INVAL and b"CRC" in L.tm_last_error()
    im16 = Image.fromarray((np.arange(w * h).reshape(h, w) * 50).astype(np.uint16))
    im16.save(p)
    assert rc_of(p.read_bytes()) == E_UNSUPPORTED and b"bits per sample" in L.tm_last_error()
    import struct
    inter = bytearray(good)
    inter[8 + 8 + 12] = 1  # IHDR's interlace byte; the CRC is mended
    inter[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(inter[12:29])))
    assert rc_of(bytes(inter)) == E_UNSUPPORTED and b"Adam7" in L.tm_last_error()
    assert L.tm_read_png_host(os.fsencode(str(tmp_path / "missing.png")), None, 0, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == E_IO


# ---- 5. the probe
def probe(name, start=0, count=0, scaling=1.0):
    v = [ctypes.c_int() for _ in range(7)]
    fps = ctypes.c_double()
    rc = lib().tm_probe_input_host(os.fsencode(str(name)), start, count, scaling, *[ctypes.byref(x) for x in v[:5]], ctypes.byref(fps), ctypes.byref(v[5]), ctypes.byref(v[6]))
    if rc:
        raise TileMotionError(rc, lib().tm_last_error().decode())
    return dict(kind=v[0].value, w=v[1].value, h=v[2].value, dst_w=v[3].value, dst_h=v[4].value, fps=fps.value, frames=v[5].value, chroma=v[6].value)


def frame_bytes(w, h, layout):
    if layout == "mono":
        return w * h
    ch, cw = resample_ref.chroma_shape(layout, w, h)
    return w * h + 2 * ch * cw


def write_y4m(path, w, h, nframes, tags="F25:1 Ip C420jpeg", layout="420jpeg", frame_header=b"FRAME\n", extra=b""):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d %s\n" % (w, h, tags.encode()))
        for i in range(nframes):
            f.write(frame_header if not callable(frame_header) else frame_header(i))
            f.write(bytes([i & 255]) * frame_bytes(w, h, layout))
        f.write(extra)


def refused(code, word, *a, **k):
    with pytest.raises(TileMotionError) as ei:
        probe(*a, **k)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_probe_reads_both_header_styles(tmp_path):
    p = tmp_path / "a.y4m"
    write_y4m(p, 100, 52, 7, "F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED")  # as FFmpeg writes it
    assert probe(p) == dict(kind=Y4M, w=100, h=52, dst_w=100, dst_h=52, fps=30000 / 1001, frames=7, chroma=2)
    write_y4m(p, 64, 48, 3, "F24000000:1000000 Ip C444", "444", b"FRAME \n")  # as tm_generate_y4m writes it
    assert probe(p) == dict(kind=Y4M, w=64, h=48, dst_w=64, dst_h=48, fps=24.0, frames=3, chroma=0)
    write_y4m(p, 101, 53, 4, "F25:1", "420jpeg", lambda i: b"FRAME Xabc=%d Ip\n" % (10 ** i))  # no I, no C; parameters of changing length on the frames
    assert probe(p) == dict(kind=Y4M, w=101, h=53, dst_w=101, dst_h=53, fps=25.0, frames=4, chroma=2)


def test_probe_accepts_and_refuses_by_tag(tmp_path):
    p = tmp_path / "a.y4m"
    for tag, layout, cid in (("C444", "444", 0), ("C422", "422", 1), ("C420jpeg", "420jpeg", 2), ("C420mpeg2", "420mpeg2", 3), ("Cmono", "mono", 4)):
        for itag in ("Ip", "I?", ""):
            write_y4m(p, 33, 17, 2, f"F25:1 {itag} {tag}", layout)
            r = probe(p)
            assert (r["chroma"], r["frames"]) == (cid, 2), (tag, itag)
    for tag in ("C420paldv", "C420p10", "C422p10", "C444p12", "C444p16", "C444alpha", "Cmono16", "C411", "C420"):
        write_y4m(p, 32, 16, 1, f"F25:1 Ip {tag}")
        refused(E_UNSUPPORTED, tag, p)
    for tag in ("It", "Ib", "Im"):
        write_y4m(p, 32, 16, 1, f"F25:1 {tag} C420jpeg")
        refused(E_UNSUPPORTED, tag, p)
    write_y4m(p, 32, 16, 1, "F25:0 Ip")
    refused(E_INVAL, "25:0", p)
    write_y4m(p, 32, 16, 1, "Ip C444", "444")
    refused(E_INVAL, "frame rate", p)
    p.write_bytes(b"RIFF....AVI LIST and so on, some container that is not ours" * 4)
    refused(E_UNSUPPORTED, "yuv4mpegpipe", p)


def test_probe_rounds_half_to_even_and_keeps_one_pixel(tmp_path):
    p = tmp_path / "a.y4m"
    write_y4m(p, 5, 3, 1, "F25:1 C444", "444")
    r = probe(p, scaling=0.5)        # 2.5 -> 2, 1.5 -> 2
    assert (r["dst_w"], r["dst_h"]) == (2, 2)
    r = probe(p, scaling=1.5)        # 7.5 -> 8, 4.5 -> 4
    assert (r["dst_w"], r["dst_h"]) == (8, 4)
    r = probe(p, scaling=0.3)        # 1.5 -> 2, 0.9 -> 1
    assert (r["dst_w"], r["dst_h"]) == (2, 1)
    write_y4m(p, 100, 4, 1, "F25:1 C444", "444")
    refused(E_UNSUPPORTED, "more than 8", p, scaling=0.125)  # 12.5 -> 12: 8.33-fold
    refused(E_UNSUPPORTED, "more than 8", p, scaling=0.12)
    assert (probe(p, scaling=0.13)["dst_w"], probe(p, scaling=0.13)["dst_h"]) == (13, 1)


def test_probe_frame_range(tmp_path):
    p = tmp_path / "a.y4m"
    write_y4m(p, 16, 8, 10)
    assert probe(p)["frames"] == 10
    assert probe(p, start=3)["frames"] == 7
    assert probe(p, start=3, count=5)["frames"] == 5
    assert probe(p, start=9, count=1)["frames"] == 1
    refused(E_INVAL, "10 whole frames", p, start=3, count=8)
    refused(E_INVAL, "10 whole frames", p, start=10)
    refused(E_INVAL, "StartFrame", p, start=-1)
    # a last frame that is cut short does not count
    write_y4m(p, 16, 8, 4, extra=b"FRAME\n" + b"\0" * (frame_bytes(16, 8, "420jpeg") - 1))
    assert probe(p)["frames"] == 4
    refused(E_INVAL, "4 whole frames", p, count=5)
    write_y4m(p, 16, 8, 2, extra=b"FRAM")
    assert probe(p)["frames"] == 2
    write_y4m(p, 16, 8, 2, extra=b"GARBAGE\n" + b"\0" * 400)
    refused(E_INVAL, "no FRAME header", p)


def test_probe_png_patterns(tmp_path):
    im = Image.fromarray(np.zeros((24, 40, 3), np.uint8), "RGB")
    for i in range(3, 9):
        im.save(tmp_path / f"a_{i:04d}.png")
        im.save(tmp_path / f"b{i}.png")
        im.save(tmp_path / f"100%_{i:02d}.png")
    im.save(tmp_path / "a_0010.png")  # behind a gap
    exp = dict(kind=PNGS, w=40, h=24, dst_w=40, dst_h=24, fps=24.0, chroma=0)
    assert probe(tmp_path / "a_%.4d.png", start=3) == dict(exp, frames=6)
    assert probe(tmp_path / "a_%.4d.png", start=5, scaling=0.5) == dict(exp, frames=4)  # Scaling plays no part
    assert probe(tmp_path / "a_%.4d.png", start=5, count=2) == dict(exp, frames=2)
    assert probe(tmp_path / "b%d.png", start=3) == dict(exp, frames=6)
    assert probe(tmp_path / "100%%_%.2d.png", start=4) == dict(exp, frames=5)
    refused(E_IO, "a_0000.png", tmp_path / "a_%.4d.png")
    refused(E_INVAL, "pattern", tmp_path / "a_0003.pgn")
    refused(E_INVAL, "pattern", tmp_path / "a_%d_%d.png")
    refused(E_INVAL, "%d", tmp_path / "a_%s.png")
    refused(E_INVAL, "empty", "")
