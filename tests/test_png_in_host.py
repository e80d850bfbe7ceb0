"""The PNG reader's rule on the host (tm_inflate.h through tm_inflate_streams_host and tm_png_decode_host; no GPU): held to Python's zlib,
to Pillow, and to the reader it mirrors (tm_inflate_host, tm_read_png_host), which shares no code with it."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import png_in_cases as C
from tiler_amd import lib
from tiler_amd._lib import InflateStatus, file_list, inflate_batch

E_INVAL, E_UNSUPPORTED = -1, -6


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def old_inflate(z, cap):
    """tm_inflate_host: (rc, bytes)"""
    src = np.frombuffer(bytes(z), np.uint8).copy()
    dst = np.zeros(max(cap, 1), np.uint8)
    n = ctypes.c_size_t(0)
    rc = lib().tm_inflate_host(_vp(src) if len(src) else None, len(src), _vp(dst), cap, ctypes.byref(n))
    return rc, dst[:n.value].tobytes()


def new_inflate(streams, caps):
    """tm_inflate_streams_host on a batch: [(code, in_pos, bytes)]; the bytes between and behind the destinations must stay 0xA5"""
    blob, spans, descs, dst_bytes, nspans = inflate_batch(streams, caps)
    dst = np.full(dst_bytes + 64, 0xA5, np.uint8)
    status = (InflateStatus * max(len(streams), 1))()
    rc = lib().tm_inflate_streams_host(_vp(blob), blob.size if nspans else 0, spans, nspans, descs, len(streams), _vp(dst), dst_bytes, status)
    assert rc == 0, lib().tm_last_error()
    out, used = [], np.zeros(dst.size, bool)
    for i in range(len(streams)):
        d, s = descs[i], status[i]
        assert s.out_n <= d.dst_cap
        out.append((s.code, s.in_pos, dst[d.dst_off:d.dst_off + s.out_n].tobytes()))
        used[d.dst_off:d.dst_off + d.dst_cap] = True
    assert np.all(dst[~used] == 0xA5), "a byte outside every destination was written"
    return out


def test_streams_match_zlib_and_the_old_reader():
    cases = C.streams()
    got = new_inflate([list(spans) for _, spans, _, _ in cases], [len(d) for _, _, d, _ in cases])
    for (name, spans, data, zlib_ok), (code, in_pos, out) in zip(cases, got):
        z = b"".join(spans)
        if zlib_ok:
            assert zlib.decompress(z) == data, name
        assert old_inflate(z, len(data)) == (0, data), name
        assert code == 0 and out == data and in_pos == len(z), (name, code, in_pos, len(z))


def test_cases_reach_what_they_name():
    by_name = {name: b"".join(spans) for name, spans, _, _ in C.streams()}
    lit, dist = C.first_dynamic_lengths(by_name["fibonacci"])
    assert max(lit) == 15                                                # 15-bit codes occur
    lit, dist = C.first_dynamic_lengths(by_name["no_distance_code"])
    assert dist == [0]
    lit, dist = C.first_dynamic_lengths(by_name["single_distance_code"])
    assert dist == [1]
    lit, dist = C.first_dynamic_lengths(by_name["incomplete_code_unmet"])
    assert sum(2.0 ** -l for l in lit if l) < 1                          # an under-subscribed code
    assert by_name["empty_stored_inside"].count(b"\x00\x00\xff\xff") >= 1 and by_name["own_level1"].count(b"\x00\x00\xff\xff") >= 3
    # the 1 MiB stream has several dynamic blocks: a symbol takes 48 bits at the most (15 + 5 + 15 + 13) and zlib closes a block after
    # 16 383 symbols, so a body of more than 2 x 16 383 x 48 bits lies in three blocks or more
    big = by_name["mixed_1048576_l6"]
    assert big[2] & 6 == 4 and len(big) * 8 > 2 * 16383 * 48
    names = [n for n, _, _, _ in C.streams()]
    for want in ("run_of_one_byte", "distance_32768", "period_3", "period_7", "spans_of_1", "span_empty_inside", "wbits9", "fixed", "huffman_only", "rle"):
        assert want in names


def test_damaged_streams_are_refused_like_the_old_reader():
    cases = C.damaged_streams()
    assert len(cases) >= 35
    got = new_inflate([z for _, z, _ in cases], [cap for _, _, cap in cases])
    for (name, z, cap), (code, in_pos, out) in zip(cases, got):
        assert old_inflate(z, cap)[0] == E_INVAL, name
        assert code != 0 and out == b"" and in_pos <= len(z), (name, code)
    codes = {name: code for (name, _, _), (code, _, _) in zip(cases, got)}
    print(codes)
    assert codes["fdict"] == 3 and codes["adler_l6"] == 17 and codes["header_l0"] == 2 and codes["over_subscribed"] == 11 and codes["distance_past_start"] == 14
    assert codes["short_destination_l6"] == 15 and codes["destination_one_short"] == 15 and codes["block_type_3"] == 5 and codes["stored_nlen"] == 6
    # (the fixed distance code has 30 symbols: the patterns of 30 and 31 are no codes)
    assert codes["length_symbol_286"] == 13 and codes["distance_symbol_30"] == 12 and codes["no_end_of_block"] == 10 and codes["over_subscribed_cl"] == 8
    assert codes["repeat_first"] == 9 and codes["lengths_overrun"] == 9 and codes["unassigned_code_met"] == 12 and codes["hlit_287"] == 7 and codes["cut_0_l0"] == 1


def test_random_damage_same_verdict_same_bytes():
    """20 000 seeded damages of three streams: 1-3 bytes overwritten, truncations, noise behind a valid header"""
    rng = np.random.default_rng(2024)
    base = [(zlib.compress(C._mixed(31, 3000), 6), 3000), (zlib.compress(C._mixed(32, 2000), 1), 2000), (C._deflate(C._mixed(33, 1500), strategy=zlib.Z_FIXED), 1500)]
    streams, caps = [], []
    for k in range(20000):
        z, n = base[k % 3]
        kind = (k // 3) % 4
        if kind < 2:
            bad = bytearray(z)
            for _ in range(int(rng.integers(1, 4))):
                bad[int(rng.integers(0, len(z)))] = int(rng.integers(0, 256))
        elif kind == 2:
            bad = z[:int(rng.integers(0, len(z)))]
        else:
            bad = z[:2] + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8))
        streams.append(bytes(bad))
        caps.append(n + int(rng.integers(0, 3)) * 50)
    got = new_inflate(streams, caps)
    accepted = 0
    for z, cap, (code, in_pos, out) in zip(streams, caps, got):
        rc, want = old_inflate(z, cap)
        assert (rc == 0) == (code == 0), (z.hex(), cap, rc, code)
        if rc == 0:
            assert out == want
            accepted += 1
    print("accepted", accepted, "of", len(streams))
    assert 0 < accepted < len(streams)


def decode_host(files, w, h, frame_px=None):
    frame_px = w * h if frame_px is None else frame_px
    ptrs, sizes, keep = file_list(files)
    out = np.full((len(files), frame_px), 0xFFFFFFFF, np.uint32)
    status = (ctypes.c_int32 * max(len(files), 1))()
    rc = lib().tm_png_decode_host(ptrs, sizes, len(files), w, h, _vp(out), frame_px, status)
    return rc, out, list(status[:len(files)])


def read_png_old(png, w, h, tmp_path):
    p = tmp_path / "one.png"
    p.write_bytes(png)
    out = np.zeros((h, w), np.uint32)
    gw, gh = ctypes.c_int(), ctypes.c_int()
    rc = lib().tm_read_png_host(str(p).encode(), _vp(out), w * h, ctypes.byref(gw), ctypes.byref(gh))
    return rc, out


def test_pictures_match_the_old_reader_and_pillow(tmp_path):
    import io
    from PIL import Image
    cases = C.pictures()
    assert len(cases) >= 8 * 5 * 6
    for name, w, h, png in cases:
        rc, out, status = decode_host([png], w, h, w * h + 5)
        assert rc == 0 and status == [0], (name, rc, status, lib().tm_last_error())
        got = out[0, :w * h].reshape(h, w)
        assert np.all(out[0, w * h:] == 0xFFFFFFFF)
        rc, want = read_png_old(png, w, h, tmp_path)
        assert rc == 0 and np.array_equal(got, want), name
        pil = np.asarray(Image.open(io.BytesIO(png)).convert("RGB")).astype(np.uint32)
        assert np.array_equal(got, (pil[..., 0] << 16) | (pil[..., 1] << 8) | pil[..., 2]), name


def test_damaged_pictures_have_their_status(tmp_path):
    want = {"filter_type_5": 33, "palette_index_npal": 34, "row_missing": 32, "byte_too_many": 15, "adler": 17}
    for name, w, h, png in C.damaged_pictures():
        assert read_png_old(png, w, h, tmp_path)[0] == E_INVAL, name
        rc, out, status = decode_host([png], w, h)
        assert rc == 0 and status == [want[name]], (name, rc, status)


def test_container_refusals_and_the_probe():
    L = lib()
    name, w, h, good = C.pictures()[12]
    assert decode_host([good], w, h)[0] == 0
    assert decode_host([good], w + 1, h)[0] == E_INVAL and b"file 0" in L.tm_last_error()            # another size
    assert decode_host([b"not a png at all, but long enough to hold a header of one"], w, h)[0] == E_UNSUPPORTED
    bad = bytearray(good); bad[len(good) // 2] ^= 0x10
    assert decode_host([good, bytes(bad)], w, h)[0] == E_INVAL and b"CRC" in L.tm_last_error() and b"file 1" in L.tm_last_error()
    for cut in (20, 40, len(good) - 12, len(good) - 1):
        assert decode_host([good[:cut]], w, h)[0] in (E_INVAL, E_UNSUPPORTED)
    import struct
    inter = bytearray(good)
    inter[8 + 8 + 12] = 1
    inter[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(inter[12:29])))
    assert decode_host([bytes(inter)], w, h)[0] == E_UNSUPPORTED and b"Adam7" in L.tm_last_error()
    deep = bytearray(good)
    deep[8 + 8 + 8] = 16
    deep[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(deep[12:29])))
    assert decode_host([bytes(deep)], w, h)[0] == E_UNSUPPORTED and b"bits per sample" in L.tm_last_error()

    def probe(files, fps=25.0):
        ptrs, sizes, keep = file_list(files)
        gw, gh = ctypes.c_int(), ctypes.c_int()
        return L.tm_probe_png_clip_host(ptrs, sizes, len(files), fps, ctypes.byref(gw), ctypes.byref(gh)), gw.value, gh.value
    assert probe([good, good]) == (0, w, h)
    assert probe([good], fps=0.0)[0] == E_INVAL
    assert probe([good, b""])[0] == E_INVAL
    assert probe([bytes(bad)])[0] == E_INVAL
    assert probe([bytes(inter)])[0] == E_UNSUPPORTED
    assert L.tm_probe_png_clip_host(None, None, 1, 25.0, None, None) == E_INVAL
    ptrs, sizes, keep = file_list([good])
    assert L.tm_probe_png_clip_host(ptrs, sizes, 0, 25.0, None, None) == E_INVAL


def test_batch_refusals():
    L = lib()
    z = zlib.compress(b"abc")
    blob, spans, descs, dst_bytes, nspans = inflate_batch([z], [3])
    dst = np.zeros(16, np.uint8)
    st = (InflateStatus * 1)()
    assert L.tm_inflate_streams_host(_vp(blob), blob.size, spans, 1, descs, 1, _vp(dst), 3, st) == 0 and st[0].code == 0 and bytes(dst[:3]) == b"abc"
    assert L.tm_inflate_streams_host(_vp(blob), blob.size - 1, spans, 1, descs, 1, _vp(dst), 3, st) == E_INVAL      # a span outside the blob
    assert L.tm_inflate_streams_host(_vp(blob), blob.size, spans, 1, descs, 1, _vp(dst), 2, st) == E_INVAL          # a destination outside dst
    assert L.tm_inflate_streams_host(_vp(blob), blob.size, spans, 0, descs, 1, _vp(dst), 3, st) == E_INVAL          # spans outside the list
    assert L.tm_inflate_streams_host(None, blob.size, spans, 1, descs, 1, _vp(dst), 3, st) == E_INVAL
