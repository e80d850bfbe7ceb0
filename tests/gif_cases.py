"""The cases of the GIF reader's tests, with what each one reaches; the claims are asserted on the restatement
(tests/gif_ref.py) alone, by check_claims().  `python tests/gif_cases.py FILE` writes them for tests/c/gif_decode.c (tools/asan_gif_in.sh).

  pictures()  [(name, file, claim)]: single pictures that decode; claim(met) says what the LZW data reaches (gif_ref.lzw_decode's `met`)
  clips()     [(name, file, pillow)]: animations that decode; pillow: inside the subset Pillow is compared on
  refused()   [(name, file, code, kind, fragment of the message)]: what the container walk refuses (TM_E_IO -5, TM_E_UNSUPPORTED -6)
  statuses()  [(name, file, status of the first refused image)]: what only decoding finds
  damaged(n)  n seeded cuts and byte changes of the small files
  TM_GIF_BAD_DESC is the kernel's refusal of a descriptor no entry point makes: no file reaches it."""
import functools
import itertools
import struct
import sys

import numpy as np

try:
    from tests import gif_ref as R
except ImportError:  # run as a script
    import gif_ref as R

IO, UNSUPPORTED = R.IO, R.UNSUPPORTED
PAL16 = [0x000000, 0xFFFFFF, 0xFF0000, 0x00FF00, 0x0000FF, 0xFFFF00, 0x00FFFF, 0xFF00FF, 0x808080, 0x804000, 0x408000, 0x004080, 0xC0C0C0, 0x102030, 0x302010, 0xA0B0C0]
PAL256 = [(i * 0x010203 + 0x050000) & 0xFFFFFF for i in range(256)]


def _one(w, h, indices, table=PAL256, **kw):
    return R.write_gif(w, h, [R.image_bytes(np.asarray(indices, np.uint8).reshape(h, w), **kw)], table=table)


@functools.lru_cache(maxsize=None)
def pictures():
    rng = np.random.default_rng(42)
    out = []
    for (w, h), mn in itertools.product([(1, 1), (1, 9), (9, 1), (17, 33)], range(2, 9)):
        out.append(("two_colour_%dx%d_min%d" % (w, h, mn), _one(w, h, rng.integers(0, 2, w * h), min_code=mn), lambda m: True))
    for p in (1, 2, 3):  # 70 x 70 stripes: the string that is its own prefix, at period p; strings longer than a wave at periods 1 and 2 (57 at 3)
        x = np.arange(70 * 70)
        idx = np.ones(70 * 70, np.uint8) if p == 1 else (x % p == 0).astype(np.uint8)
        out.append(("stripes_70x70_period%d" % p, _one(70, 70, idx, table=PAL16, min_code=2), lambda m, p=p: p in m["kwkwk_periods"] and m["longest"] > (64 if p < 3 else 48)))
    out.append(("flat_192x192", _one(192, 192, np.full(192 * 192, 5), min_code=8), lambda m: m["longest"] > 256 and m["farthest"] > 32768))
    noise = rng.integers(0, 256, 96 * 96)
    out.append(("noise_96x96_clear_at_full", _one(96, 96, noise, min_code=8, clear="full"), lambda m: m["clears"] >= 2))
    out.append(("noise_96x96_deferred_clear", _one(96, 96, noise, min_code=8, clear="never"), lambda m: m["full"] and m["clears"] == 1))
    y, x = np.mgrid[0:240, 0:320]
    busy = ((x // 8 + y // 8) % 7 + (rng.random((240, 320)) < 0.02) * 3).astype(np.uint8)
    out.append(("no_clear_320x240", _one(320, 240, busy, table=PAL16, min_code=4, clear="never", initial_clear=False),
                lambda m: m["clears"] == 0 and m["full"] and m["farthest"] > 65536))
    small = rng.integers(0, 16, 17 * 33)
    out.append(("one_byte_sub_blocks", _one(17, 33, small, table=PAL16, min_code=4, sub=1), lambda m: True))
    for sub in (7, 254):
        out.append(("sub_blocks_of_%d" % sub, _one(17, 33, small, table=PAL16, min_code=4, sub=sub), lambda m: True))
    out.append(("no_eoi_no_initial_clear", _one(17, 33, small, table=PAL16, min_code=4, eoi=False, initial_clear=False), lambda m: m["clears"] == 0))
    more = R.lzw_codes(rng.integers(0, 16, 20 * 20), 4)
    out.append(("data_beyond_the_picture", _one(20, 15, np.zeros(300), table=PAL16, min_code=4, codes=more, after=b"\xff" * 9), lambda m: True))
    out.append(("two_clears_in_a_row", _one(17, 33, small, table=PAL16, min_code=4, codes=[16] + R.lzw_codes(small, 4)), lambda m: m["clears"] == 2))
    out.append(("clear_every_5_codes", _one(17, 33, small, table=PAL16, min_code=4, clear=5), lambda m: m["clears"] > 20))
    return out


def _rect(rng, w, h, colours):
    return rng.integers(0, colours, (h, w)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def clips():
    rng = np.random.default_rng(7)
    W, H = 24, 20
    out = []
    full = lambda: R.image_bytes(_rect(rng, W, H, 16), min_code=4)  # noqa: E731
    # Pillow's subset: frame 0 opaque and covering the screen, disposals 0 and 1 (not 3: tests/test_gif_in_host.py says what was found)
    for name, ds in (("disposal_0_1", (0, 1, 1, 0, 0, 1)), ("disposal_0_1_3", (1, 3, 0, 3, 3, 1, 0))):
        blocks = [R.gce_bytes(ds[0], -1, 5), full()]
        for i, d in enumerate(ds[1:]):
            blocks += [R.gce_bytes(d, 3, 5), R.image_bytes(_rect(rng, 7 + i, 5 + i, 16), left=1 + 2 * i, top=3 + i, min_code=4)]
        out.append((name, R.write_gif(W, H, blocks, table=PAL16, loop=0), 3 not in ds))
    # every ordered pair of disposals, 3 after 3 among them
    ds = (0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 0, 3, 1, 3, 2, 1, 0)
    assert {(a, b) for a, b in zip(ds, ds[1:])} == set(itertools.product(range(4), repeat=2))
    blocks = []
    for i, d in enumerate(ds):
        blocks += [R.gce_bytes(d, 2 if i else -1, 4), full() if i == 0 else R.image_bytes(_rect(rng, 5 + i % 7, 4 + i % 5, 16), left=(3 * i) % 17, top=(5 * i) % 13, min_code=4)]
    out.append(("every_disposal_pair", R.write_gif(W, H, blocks, table=PAL16, bg_index=9), False))
    # disposal 3 on frame 0, which does not cover the screen; then 2 on a frame that does not either
    blocks = [R.gce_bytes(3, -1, 3), R.image_bytes(_rect(rng, 10, 8, 16), left=5, top=6, min_code=4), R.gce_bytes(2, 1, 3),
              R.image_bytes(_rect(rng, 12, 9, 16), left=2, top=2, min_code=4), R.gce_bytes(0, 1, 3), R.image_bytes(_rect(rng, 6, 6, 16), left=15, top=10, min_code=4)]
    out.append(("disposal_3_on_frame_0_small", R.write_gif(W, H, blocks, table=PAL16, bg_index=4), False))
    # no global table: local tables with transparency; a background index that no table holds
    blocks = []
    for i in range(4):
        local = [(c * (i + 3)) & 0xFFFFFF for c in PAL16[:8]]
        blocks += [R.gce_bytes(i % 3, 5 if i else -1, 7), R.image_bytes(_rect(rng, W - 3 * i, H - 2 * i, 8), left=i, top=2 * i, table=local, min_code=3)]
    out.append(("local_tables_only", R.write_gif(W, H, blocks, table=None, bg_index=200), False))
    out.append(("background_index_outside", R.write_gif(W, H, [R.gce_bytes(2, -1, 2), R.image_bytes(_rect(rng, 9, 9, 4), left=3, top=3, min_code=2), R.gce_bytes(0, 0, 2),
                                                            R.image_bytes(_rect(rng, 5, 5, 4), left=10, top=10, min_code=2)], table=PAL16[:4], bg_index=77), False))
    # an index past its (local) table reads black
    out.append(("index_past_the_table", R.write_gif(W, H, [R.image_bytes(_rect(rng, W, H, 16), table=PAL16[1:5], min_code=4)], table=PAL16), False))
    # rectangles at odd offsets, partly and wholly off the screen
    blocks = [full()]
    for i, (l, t, w, h) in enumerate([(17, 13, 11, 11), (23, 19, 5, 5), (1, 15, 30, 3), (24, 0, 4, 4), (3, 20, 4, 4), (0, 0, 40, 40)]):
        blocks += [R.gce_bytes(1 + i % 3, 0, 6), R.image_bytes(_rect(rng, w, h, 16), left=l, top=t, min_code=4)]
    out.append(("off_screen_rectangles", R.write_gif(W, H, blocks, table=PAL16), False))
    # interlaced rectangles of 1 .. 9 rows, and a whole interlaced frame
    blocks = [R.image_bytes(_rect(rng, W, H, 16), min_code=4, interlace=True)]
    for h in range(1, 10):
        blocks += [R.gce_bytes(1, 7, 5), R.image_bytes(_rect(rng, 13, h, 16), left=h, top=h, min_code=4, interlace=True)]
    out.append(("interlaced_heights", R.write_gif(W, H, blocks, table=PAL16), True))
    # delays: 0 and 1 count as 10; equal; unequal
    for name, delays in (("delays_0_1", (0, 1, 10)), ("delays_equal", (4, 4, 4)), ("delays_unequal", (3, 20, 7, 1))):
        blocks = []
        for d in delays:
            blocks += [R.gce_bytes(1, -1, d), full()]
        out.append((name, R.write_gif(W, H, blocks, table=PAL16), True))
    # other extensions between frames, an image without graphic control, no trailer, a GIF87a header, bytes behind the trailer
    blocks = [R.comment(), R.gce_bytes(1, -1, 9), full(), R.plain_text(), R.comment(b"x" * 300), R.image_bytes(_rect(rng, 8, 8, 16), left=4, top=4, min_code=4),
              b"\x21\xff\x0bXMP DataXMP" + R.sub_blocks(b"not a loop count", 255)]
    out.append(("extensions_between_frames", R.write_gif(W, H, blocks, table=PAL16, loop=3), True))
    out.append(("no_trailer", R.write_gif(W, H, [full(), R.gce_bytes(1, -1, 5), full()], table=PAL16, trailer=False), True))
    out.append(("gif87a_bytes_behind_the_trailer", R.write_gif(W, H, [full()], table=PAL16, version=b"87a", after=b"\x2c junk \x21"), True))
    return out


def _good_small():
    return R.write_gif(12, 10, [R.gce_bytes(1, -1, 5), R.image_bytes(np.arange(120).reshape(10, 12) % 16, min_code=4),
                                R.gce_bytes(0, 2, 5), R.image_bytes((np.arange(30).reshape(5, 6) * 7) % 16, left=3, top=2, min_code=4)], table=PAL16)


@functools.lru_cache(maxsize=None)
def refused():
    g = _good_small()
    img = R.image_bytes(np.zeros((4, 4)), min_code=2)
    hdr = lambda w=4, h=4: b"GIF89a" + struct.pack("<HHBBB", w, h, 0x80, 0, 0) + R.table_bytes(PAL16[:2])[0]  # noqa: E731
    cut_at = g.index(b"\x2c") + 10 + 1 + 3  # inside the first image's data
    return [
        ("not_a_gif", b"GIF88a" + g[6:], UNSUPPORTED, "signature", "is not a GIF file"),
        ("too_short_for_a_signature", b"GIF8", UNSUPPORTED, "signature", "is not a GIF file"),
        ("a_png", b"\x89PNG\r\n\x1a\n" + bytes(40), UNSUPPORTED, "signature", "is not a GIF file"),
        ("cut_in_the_screen_descriptor", g[:10], IO, "past the end", "past the end"),
        ("cut_in_the_global_table", g[:20], IO, "past the end", "past the end"),
        ("cut_in_the_image_data", g[:cut_at], IO, "past the end", "past the end"),
        ("cut_in_an_extension", g[:13 + 48 + 3], IO, "past the end", "past the end"),
        ("cut_in_an_image_descriptor", hdr() + img[:6], IO, "past the end", "past the end"),
        ("no_terminator", hdr() + img[:-1], IO, "past the end", "past the end"),
        ("unknown_introducer", hdr() + b"\x2d" + img, IO, "introducer", "unknown block introducer 0x2d"),
        ("no_image_before_the_trailer", hdr() + R.comment() + b"\x3b", IO, "no image", "no image"),
        ("ends_before_an_image", hdr() + R.comment(), IO, "no image", "before its first image"),
        ("screen_width_0", hdr(0, 4) + img + b"\x3b", IO, "empty screen", "a screen of 0x4"),
        ("screen_height_0", hdr(4, 0) + img + b"\x3b", IO, "empty screen", "a screen of 4x0"),
        ("rectangle_width_0", hdr() + b"\x2c" + struct.pack("<HHHHB", 0, 0, 0, 4, 0) + img[10:] + b"\x3b", IO, "empty rectangle", "is 0x4"),
        ("min_code_size_1", hdr() + R.image_bytes(np.zeros((4, 4)), min_code=2, min_code_byte=1) + b"\x3b", IO, "code size", "minimum code size of 1"),
        ("min_code_size_9", hdr() + R.image_bytes(np.zeros((4, 4)), min_code=2, min_code_byte=9) + b"\x3b", IO, "code size", "minimum code size of 9"),
        ("min_code_size_0", hdr() + R.image_bytes(np.zeros((4, 4)), min_code=2, min_code_byte=0) + b"\x3b", IO, "code size", "minimum code size of 0"),
        ("no_colour_table", b"GIF89a" + struct.pack("<HHBBB", 4, 4, 0, 0, 0) + img + b"\x3b", IO, "no table", "no colour table"),
    ]


@functools.lru_cache(maxsize=None)
def statuses():
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 16, (9, 11)).astype(np.uint8)
    codes = R.lzw_codes(idx.reshape(-1), 4)
    one = lambda c, **kw: R.write_gif(11, 9, [R.image_bytes(idx, min_code=4, codes=c, **kw)], table=PAL16)  # noqa: E731
    good = R.image_bytes(idx, min_code=4)
    return [
        ("eoi_too_early", one(codes[:20] + [17]), R.TRUNCATED),
        ("data_ends_early", one(codes[:30]), R.TRUNCATED),
        ("no_data_at_all", one([]), R.TRUNCATED),
        ("only_a_clear", one([16]), R.TRUNCATED),
        ("code_above_the_next_free_entry", one(codes[:10] + [31] + codes[10:]), R.BAD_CODE),
        ("code_one_above_the_next_free_entry", one([16, 1, 2, 20]), R.BAD_CODE),
        ("non_literal_behind_a_clear", one(codes[:12] + [16, 18]), R.BAD_CODE),
        ("non_literal_first", one([19, 1, 2]), R.BAD_CODE),
        ("second_image_truncated", R.write_gif(11, 9, [good, R.image_bytes(idx, min_code=4, codes=codes[:25]), good], table=PAL16), R.TRUNCATED),
        ("first_of_three_bad", R.write_gif(11, 9, [R.image_bytes(idx, min_code=4, codes=[16, 1, 30]), good, good], table=PAL16), R.BAD_CODE),
    ]


def small_files():
    return [f for _, f, _ in pictures() if len(f) < 1500] + [f for _, f, _ in clips()] + [f for _, f, _ in statuses()] + [_good_small()]


@functools.lru_cache(maxsize=None)
def damaged(n=600, seed=5):
    rng = np.random.default_rng(seed)
    files = small_files()
    out = []
    for k in range(n):
        f = bytearray(files[int(rng.integers(len(files)))])
        how = int(rng.integers(4))
        if how == 0:
            f = f[:int(rng.integers(len(f)))]
        else:
            for _ in range(how):
                f[int(rng.integers(len(f)))] = int(rng.integers(256))
        out.append(("damage_%d" % k, bytes(f)))
    return out


def verdict(file):
    """what the restatement makes of a file: ("refused", code, kind) | ("decoded", statuses, frames)"""
    try:
        frames, st, info = R.decode(file)
    except R.Refused as e:
        return ("refused", e.code, e.kind)
    return ("decoded", st, frames)


def streams():
    """[(name, span, min_code_size, npix)]: the LZW data of every picture and of every image of the status cases, and cut and changed
    copies of them: spans that end inside a sub-block, at a length byte, and with a byte changed"""
    out = []
    for name, f, _ in pictures():
        im = R.parse(f)["images"][0]
        out.append((name, f[im["data_off"]:im["data_off"] + im["data_bytes"]], im["min_code_size"], im["width"] * im["height"]))
    for name, f, _ in statuses():
        for i, im in enumerate(R.parse(f)["images"]):
            out.append(("%s_%d" % (name, i), f[im["data_off"]:im["data_off"] + im["data_bytes"]], im["min_code_size"], im["width"] * im["height"]))
    rng = np.random.default_rng(3)
    base = [s for s in out if len(s[1]) < 1200]
    for k in range(40):
        name, span, mn, npix = base[int(rng.integers(len(base)))]
        span = bytearray(span)
        if k % 2:
            span = span[:int(rng.integers(len(span)))]
        else:
            span[int(rng.integers(len(span)))] = int(rng.integers(256))
        out.append(("%s_damage_%d" % (name, k), bytes(span), mn, npix))
    out.append(("empty_span", b"", 4, 10))
    out.append(("no_pixels", out[0][1], out[0][2], 0))
    return out


def check_claims():
    """every claim of this file, on the restatement alone"""
    for name, f, claim in pictures():
        info = R.parse(f)
        im = info["images"][0]
        idx, st, met = R.lzw_decode(f[im["data_off"]:im["data_off"] + im["data_bytes"]], im["min_code_size"], im["width"] * im["height"])
        assert st[0] == 0 and st[2] == im["width"] * im["height"], (name, st)
        assert claim(met), (name, met)
    for name, f, _ in clips():
        v = verdict(f)
        assert v[0] == "decoded" and not any(v[1]), (name, v[:2])
    kinds = set()
    for name, f, code, kind, _ in refused():
        v = verdict(f)
        assert v[0] == "refused" and v[1] == code and v[2].startswith(kind), (name, v)
        kinds.add(kind)
    assert kinds == {"signature", "past the end", "introducer", "no image", "empty screen", "empty rectangle", "code size", "no table"}
    seen = set()
    for name, f, status in statuses():
        v = verdict(f)
        assert v[0] == "decoded" and [s for s in v[1] if s][0] == status, (name, v[:2])
        seen.add(status)
    assert seen == {R.TRUNCATED, R.BAD_CODE}
    found = {"refused": 0, "status": 0, "decoded": 0}
    for name, f in damaged():
        v = verdict(f)
        found["refused" if v[0] == "refused" else "status" if any(v[1]) else "decoded"] += 1
    assert all(found.values()), found
    return found


def dump(path):
    """count, then per case: kind (0 decodes, 1 refused by the walk, 2 a status, 3 damage: any verdict), code, length, bytes"""
    cases = [(0, 0, f) for _, f, _ in pictures()] + [(0, 0, f) for _, f, _ in clips()] + [(1, c, f) for _, f, c, _, _ in refused()]
    cases += [(2, s, f) for _, f, s in statuses()] + [(3, 0, f) for _, f in damaged()]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for kind, code, f in cases:
            fh.write(struct.pack("<IiI", kind, code, len(f)) + f)


if __name__ == "__main__":
    print(check_claims())
    dump(sys.argv[1])
