"""The cases of the GIF writer's tests, with what each one reaches; the claims are asserted on the restatement
(tests/gif_out_ref.py) alone, by check_claims().  `python tests/gif_out_cases.py FILE` writes them, with the restatement's files, for
tests/c/gif_encode.c (tools/asan_gif_out.sh).

  clips()   [dict(name, frames uint32 [F][h][w], fps, opt, claim(info), chunks)]: what is written whole; info: gif_out_ref.encode's, a
            dict per frame; chunks: the chunk_frames the device form is run at (every byte stays equal)
  streams() [(name, indices, min_code, segment_pixels, claim(met))]: the LZW seam; met: gif_out_ref.payload's
  refused() [(name, frames, fps, opt, code)]
The seeds and the segment sizes of the searched cases were found with the restatement; the claims hold them to what they were found for."""
import functools
import struct
import sys

import numpy as np

try:
    from tests import gif_out_ref as R
except ImportError:  # run as a script
    sys.path.insert(0, __file__.rsplit("/", 2)[0])
    from tests import gif_out_ref as R

PAL256 = np.array(sorted((i * 0x9E3779 + 0x050000) & 0xFFFFFF for i in range(256)), np.uint32)
FPS = 25.0


def noise(seed, n, colours):
    return np.random.default_rng(seed).integers(0, colours, n).astype(np.uint8)


def _all_used(seed, w, h, colours):
    """a frame of w x h in which each of the first `colours` entries of PAL256 occurs"""
    idx = np.random.default_rng(seed).integers(0, colours, w * h)
    idx[:colours] = np.arange(colours)
    return PAL256[idx].reshape(1, h, w)


def _row(seed, n):
    return PAL256[np.random.default_rng(seed).integers(0, 256, n)].reshape(1, 1, n)


def distinct(n):
    return ((np.arange(n, dtype=np.uint64) * 0x9E3779 + 12345) & 0xFFFFFF).astype(np.uint32)


# payload bytes -> (pixels of a one-row frame, seed): the sub-block chain's edges
PAYLOADS = {254: (223, 0), 255: (224, 0), 256: (225, 0), 510: (431, 6)}
FILLS_ON_LAST = 3935   # segment_pixels at which noise(5, ., 256) fills the table on segment 0's last index
WIDENS_ON_LAST = 310   # segment_pixels at which noise(6, 2000, 16) ends a segment on the code that widens the width


def _case(name, frames, claim=lambda info: True, chunks=(0,), fps=FPS, **opt):
    return dict(name=name, frames=np.ascontiguousarray(frames, np.uint32), fps=fps, opt=opt, claim=claim, chunks=chunks)


def diff_clip():
    rng = np.random.default_rng(3)
    f0 = PAL256[rng.integers(0, 6, (10, 12))]
    fr = [f0, f0.copy()]
    for y, x in ((0, 0), (0, 11), (9, 0), (9, 11)):
        g = fr[-1].copy()
        g[y, x] ^= 0x010101
        fr.append(g)
    fr.append(fr[-1] ^ 0x020408)
    g = fr[-1].copy()
    g[1:5, 3:8] ^= 0x0F0F0F
    fr.append(g)
    return np.stack(fr)


DIFF_RECTS = [(0, 0, 12, 10), (0, 0, 1, 1), (0, 0, 1, 1), (11, 0, 1, 1), (0, 9, 1, 1), (11, 9, 1, 1), (0, 0, 12, 10), (3, 1, 5, 4)]


@functools.lru_cache(maxsize=None)
def clips():
    out = []
    for w, h, colours in ((1, 1, 1), (2, 1, 2), (3, 5, 3), (17, 33, 5)):
        out.append(_case("size_%dx%d" % (w, h), _all_used(1, w, h, colours), lambda i, c=colours: i[0]["exact"] and i[0]["table"] == c))
    for colours, mn in ((1, 2), (2, 2), (3, 2), (4, 2), (5, 3), (16, 4), (17, 5), (255, 8), (256, 8)):
        out.append(_case("table_of_%d" % colours, _all_used(2, 17, 33, colours), lambda i, c=colours, mn=mn: i[0]["exact"] and i[0]["table"] == c and i[0]["min_code"] == mn))
    many = distinct(257).reshape(1, 1, 257)
    out.append(_case("257_colours_auto", many, lambda i: not i[0]["exact"] and i[0]["colours"] == 257 and i[0]["table"] <= 256))
    base = 0x808080
    near = np.array([base] + [base ^ (1 << (8 * c + b)) for c in range(3) for b in (0, 2, 3, 7)], np.uint32)
    near_frame = near[np.random.default_rng(4).integers(0, len(near), (9, 13))]
    near_frame.reshape(-1)[:len(near)] = near
    out.append(_case("one_bit_apart_exact", near_frame[None], lambda i: i[0]["exact"] and i[0]["table"] == 13))
    out.append(_case("one_bit_apart_cut", near_frame[None], lambda i: not i[0]["exact"] and i[0]["cells"] > 4 and i[0]["boxes"] == 4, colours="quantise", max_colours=4))
    out.append(_case("flat_192x192", np.full((1, 192, 192), 0x123456, np.uint32), lambda i: i[0]["longest"] > 256 and i[0]["segments"] == 1, segment_pixels=0))
    out.append(_case("flat_192x192_segments", np.full((1, 192, 192), 0x123456, np.uint32), lambda i: i[0]["longest"] > 64 and i[0]["segments"] == 3, segment_pixels=16384))
    x = np.arange(70 * 70)
    for p in (2, 3):
        out.append(_case("stripes_70x70_period%d" % p, PAL256[(x % p == 0).astype(np.uint8)].reshape(1, 70, 70), lambda i, p=p: i[0]["longest"] > (64 if p == 2 else 48), segment_pixels=0))
    out.append(_case("noise_96x96", PAL256[noise(5, 96 * 96, 256)].reshape(1, 96, 96), lambda i: i[0]["table"] == 256 and i[0]["clears"] >= 3 and i[0]["segments"] == 1, segment_pixels=16384))
    out.append(_case("noise_96x96_segments", PAL256[noise(5, 96 * 96, 256)].reshape(1, 96, 96), lambda i: i[0]["segments"] == 36, segment_pixels=256))
    n = 1024
    seg = PAL256[noise(8, n + 1, 16)]
    for k, at in ((n, 1), (n - 1, 1), (n + 1, 2)):
        out.append(_case("segment_of_%d_for_%d" % (n, k), seg[:k].reshape(1, 1, k), lambda i, at=at: i[0]["segments"] == at, segment_pixels=n))
    out.append(_case("one_segment", seg[:n].reshape(1, 1, n), lambda i: i[0]["segments"] == 1, segment_pixels=0))
    for target, (px, seed) in PAYLOADS.items():
        out.append(_case("payload_of_%d" % target, _row(seed, px), lambda i, t=target: i[0]["payload_bytes"] == t))
    clip = diff_clip()
    out.append(_case("clip_diff", clip, lambda i: [f["rect"] for f in i] == DIFF_RECTS, chunks=(1, 2, 3, 0)))
    out.append(_case("clip_whole_frames", clip, lambda i: all(f["rect"] == (0, 0, 12, 10) for f in i), chunks=(1, 2, 3, 0), diff=False))
    out.append(_case("clip_loop_3_delay_7", clip[:3], loop=3, delay_cs=7))
    out.append(_case("clip_no_loop_30fps", clip[:3], fps=30.0, loop=-1))
    # the quantiser
    out.append(_case("cut_192x192_all_distinct", distinct(192 * 192).reshape(1, 192, 192), lambda i: not i[0]["exact"] and i[0]["cells"] > 256 and i[0]["boxes"] == 256))
    cells10 = np.array([(r << 19 | g << 11 | b << 3) for r, g, b in ((1, 2, 3), (1, 2, 4), (9, 9, 9), (30, 1, 1), (1, 30, 1), (1, 1, 30), (31, 31, 31), (0, 0, 0), (16, 16, 16), (16, 17, 16))])
    inside = np.array([(r << 16 | g << 8 | b) for r in range(5) for g in range(3) for b in range(2)])
    c300 = (cells10[:, None] + inside[None, :]).reshape(-1).astype(np.uint32)
    out.append(_case("cut_300_colours_in_10_cells", np.tile(c300, 2).reshape(1, 20, 30), lambda i: not i[0]["exact"] and i[0]["colours"] == 300 and i[0]["cells"] == 10 and i[0]["boxes"] == 10))
    grid = np.array([((4 * r + 1) << 19 | (4 * g + 1) << 11 | (4 * b + 1) << 3) for r in range(4) for g in range(4) for b in range(4)], np.uint32)
    out.append(_case("cut_equal_counts", np.repeat(grid, 4).reshape(1, 16, 16), lambda i: {"box", "axis"} <= i[0]["ties"] and i[0]["boxes"] == 16, colours="quantise", max_colours=16))
    heavy = np.array([0x101010, 0xF0F0F0, 0xF0F0F0, 0xF0F0F0], np.uint32)
    out.append(_case("cut_moved_down", heavy.reshape(1, 2, 2), lambda i: "cut moved" in i[0]["ties"] and i[0]["boxes"] == 2, colours="quantise", max_colours=2))
    rgb = np.random.default_rng(9).integers(0, 1 << 24, (1, 64, 64)).astype(np.uint32)
    out.append(_case("cut_max_colours_2", rgb, lambda i: i[0]["boxes"] == 2 and i[0]["min_code"] == 2, max_colours=2))
    out.append(_case("cut_max_colours_17", rgb, lambda i: i[0]["boxes"] == 17 and i[0]["min_code"] == 5, max_colours=17))
    two = np.concatenate([rgb, _all_used(2, 64, 64, 16)])
    out.append(_case("clip_cut_then_exact", two, lambda i: [f["exact"] for f in i] == [False, True], chunks=(1, 0)))
    return out


@functools.lru_cache(maxsize=None)
def streams():
    out = [("one_index", np.zeros(1, np.uint8), 2, 0, lambda m: m["codes"] == 3)]
    out.append(("fills_on_the_last_index", noise(5, FILLS_ON_LAST + 300, 256), 8, FILLS_ON_LAST, lambda m: m["fills_on_last"] and m["segments"] == 2))
    out.append(("widens_on_the_last_code", noise(6, 2000, 16), 4, WIDENS_ON_LAST, lambda m: m["widen_last"]))
    out.append(("segment_bits_multiple_of_32", noise(4, 1200, 16), 4, 300, lambda m: any(b % 32 == 0 for b in m["seg_bits"][:-1])))
    out.append(("segment_bits_multiple_of_8", noise(0, 1200, 16), 4, 300, lambda m: any(b % 8 == 0 and b % 32 for b in m["seg_bits"][:-1]) and any(b % 8 for b in m["seg_bits"])))
    out.append(("flat_36864", np.full(192 * 192, 5, np.uint8), 8, 0, lambda m: m["codes"] < 300))
    out.append(("noise_9216_min8", noise(5, 96 * 96, 256), 8, 4096, lambda m: m["segments"] == 3 and m["clears"] >= 4))
    for mn in range(2, 9):
        out.append(("noise_700_min%d" % mn, noise(mn, 700, 1 << mn), mn, 256, lambda m: m["segments"] == 3))
    return out


@functools.lru_cache(maxsize=None)
def refused():
    one = np.zeros((1, 2, 2), np.uint32)
    many = distinct(257).reshape(1, 1, 257)
    out = [("257_colours_exact", many, FPS, dict(colours="exact"), R.UNSUPPORTED), ("17_colours_exact_16", _all_used(2, 17, 33, 17), FPS, dict(colours="exact", max_colours=16), R.UNSUPPORTED)]
    for name, opt in (("max_colours_1", dict(max_colours=1)), ("max_colours_257", dict(max_colours=257)), ("segment_255", dict(segment_pixels=255)), ("loop_below", dict(loop=-2)),
                      ("loop_above", dict(loop=65536)), ("delay_1", dict(delay_cs=1)), ("delay_above", dict(delay_cs=65536))):
        out.append((name, one, FPS, opt, R.INVAL))
    out.append(("rate_too_slow", one, 0.001, {}, R.INVAL))
    out.append(("rate_zero", one, 0.0, {}, R.INVAL))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's (file, canvas, info) of a clip, computed once"""
    c = next(c for c in clips() if c["name"] == name)
    return R.encode(c["frames"], c["fps"], **c["opt"])


def check_claims():
    for c in clips():
        assert c["claim"](expected(c["name"])[2]), c["name"]
    for name, idx, mn, seg, claim in streams():
        assert claim(R.payload(idx, mn, seg)[1]), name
    for name, frames, fps, opt, code in refused():
        try:
            R.encode(frames, fps, **opt)
        except R.Refused as e:
            assert e.code == code, name
        else:
            raise AssertionError(name)


def write(path):
    """for tests/c/gif_encode.c: per clip nf, w, h (u32), fps (f64), the six options (i32), the frames, the file's size (u32), the file"""
    with open(path, "wb") as f:
        cs = clips()
        f.write(struct.pack("<I", len(cs)))
        for c in cs:
            o = R.options(**c["opt"])
            nf, h, w = c["frames"].shape
            f.write(struct.pack("<IIId6i", nf, w, h, c["fps"], R.COLOURS[o["colours"]], o["max_colours"], int(o["diff"]), o["segment_pixels"], o["loop"], o["delay_cs"]))
            f.write(c["frames"].tobytes())
            file = expected(c["name"])[0]
            f.write(struct.pack("<I", len(file)) + file)


if __name__ == "__main__":
    check_claims()
    write(sys.argv[1])
