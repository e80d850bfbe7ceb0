"""The cases of the WebP writer's tests, with what each one reaches; the claims are asserted on the restatement
(tests/webp_out_ref.py) alone, by check_claims().  `python tests/webp_out_cases.py FILE` writes them, with the restatement's files, for
tests/c/webp_encode.c (tools/asan_webp_out.sh).

  clips()   [dict(name, frames uint32 [F][h][w], fps, opt, claim(info), chunks)]: info: webp_out_ref.encode's, a dict per frame; chunks: the
            chunk_frames the device form is run at (every byte stays equal)
  refused() [(name, frames, fps, opt, code)]
The seeds of the searched cases were found with the restatement; the claims hold them to what they were found for."""
import functools
import struct
import sys

import numpy as np

try:
    from tests import webp_out_ref as R
except ImportError:  # run as a script
    sys.path.insert(0, __file__.rsplit("/", 2)[0])
    from tests import webp_out_ref as R

PAL256 = np.array(sorted((i * 0x9E3779 + 0x050000) & 0xFFFFFF for i in range(256)), np.uint32)
FPS = 25.0
BITS_32_SEED, BITS_8_SEED = 1, 6  # noise_bits(seed): a segment but the last of a multiple of 32 bits; of 8 and not 32, beside one of neither


def distinct(n):
    return ((np.arange(n, dtype=np.uint64) * 0x9E3779 + 12345) & 0xFFFFFF).astype(np.uint32)


def _all_used(seed, w, h, colours):
    """a frame of w x h in which each of the first `colours` entries of PAL256 occurs (where there is room)"""
    idx = np.random.default_rng(seed).integers(0, colours, w * h)
    idx[:colours] = np.arange(colours)[:w * h]
    return PAL256[idx].reshape(1, h, w)


def noise_bits(seed):
    return PAL256[np.random.default_rng(seed).integers(0, 16, 1200)].reshape(1, 24, 50)


def fibonacci_frame():
    """18 colours whose counts are 1, 1, 2, 3, 5 ...: an unlimited Huffman code of the green alphabet is 17 deep"""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    idx = np.repeat(np.arange(18), fib)
    np.random.default_rng(7).shuffle(idx)
    assert len(idx) == 89 * 76
    return PAL256[idx * 9].reshape(1, 76, 89)


def run_row(run, tail):
    """one row: run + 1 pixels of one colour, then `tail` pixels each of another"""
    return np.concatenate([np.full(run + 1, PAL256[200], np.uint32), distinct(tail)]).reshape(1, 1, run + 1 + tail)


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


# the even rule: a changed pixel at an odd x or y pulls its rectangle's corner one back
DIFF_RECTS = [(0, 0, 12, 10), (0, 0, 1, 1), (0, 0, 1, 1), (10, 0, 2, 1), (0, 8, 1, 2), (10, 8, 2, 2), (0, 0, 12, 10), (2, 0, 6, 5)]


def tiles_64():
    tile = np.random.default_rng(11).integers(0, 16, (8, 8))
    tile.reshape(-1)[:16] = np.arange(16)
    return PAL256[np.tile(tile, (8, 8))][None]


@functools.lru_cache(maxsize=None)
def clips():
    out = []
    for w, h, colours in ((1, 1, 1), (2, 1, 2), (3, 5, 3), (17, 33, 5)):
        out.append(_case("size_%dx%d" % (w, h), _all_used(1, w, h, colours), lambda i, c=colours: i[0]["colours"] == c))
    out.append(_case("size_1x1_green", _all_used(1, 1, 1, 1), lambda i: i[0]["colours"] == 0 and i[0]["tokens"] == 1, palette="off"))
    for colours, per in ((1, 8), (2, 8), (3, 4), (4, 4), (5, 2), (16, 2), (17, 1), (256, 1)):
        out.append(_case("table_of_%d" % colours, _all_used(2, 17, 33, colours),
                         lambda i, c=colours, p=per: i[0]["colours"] == c and i[0]["per"] == p and i[0]["symbols"] == 33 * ((17 + p - 1) // p)))
    out.append(_case("table_of_16_green", _all_used(2, 17, 33, 16), lambda i: i[0]["colours"] == 0 and i[0]["symbols"] == 17 * 33, palette="off"))
    out.append(_case("257_colours_auto", distinct(257).reshape(1, 1, 257), lambda i: i[0]["colours"] == 0 and i[0]["per"] == 1))
    # one literal and matches: the green alphabet's two used symbols, one of them a length, need a normal code
    out.append(_case("flat_17x33", np.full((1, 33, 17), 0x123456, np.uint32), lambda i: i[0]["tokens"] == 2 and i[0]["matches"] == 1 and i[0]["kinds"][0] == "normal"))
    out.append(_case("no_match_3x5", distinct(15).reshape(1, 5, 3), lambda i: i[0]["matches"] == 0 and i[0]["kinds"][4] == "simple0"))
    out.append(_case("fibonacci_counts", fibonacci_frame(), lambda i: i[0]["deepest"][0] > 15 and i[0]["kinds"][0] == "normal", lz77=False))
    out.append(_case("tiles_64x64", tiles_64(), lambda i: i[0]["matches"] >= 5 and {4, 256} <= set(i[0]["distances"]), segment_pixels=0))  # the tile to the left, the tile above
    out.append(_case("tiles_64x64_literals", tiles_64(), lambda i: i[0]["matches"] == 0, segment_pixels=0, lz77=False))
    out.append(_case("tiles_64x64_borders", tiles_64(), lambda i: i[0]["segments"] == 5 and i[0]["reaches_back"] > 0 and i[0]["ends_at_border"] > 0, segment_pixels=500))
    out.append(_case("run_of_4096", run_row(4096, 10), lambda i: i[0]["longest"] == 4096 and i[0]["tokens"] == 12 and i[0]["matches"] == 1, segment_pixels=0, palette="off"))
    out.append(_case("run_of_5000", run_row(5000, 10), lambda i: i[0]["longest"] == 4096 and i[0]["tokens"] == 13 and i[0]["matches"] == 2, segment_pixels=0, palette="off"))
    seg = _all_used(8, 32, 32, 16)  # 512 coded pixels
    for k, at in ((512, 1), (511, 2), (513, 1), (0, 1)):
        out.append(_case("segment_of_%d_for_512" % k, seg, lambda i, at=at: i[0]["symbols"] == 512 and i[0]["segments"] == at, segment_pixels=k))
    out.append(_case("segment_bits_multiple_of_32", noise_bits(BITS_32_SEED), lambda i: any(b % 32 == 0 for b in i[0]["seg_bits"][:-1]), segment_pixels=100))
    out.append(_case("segment_bits_multiple_of_8", noise_bits(BITS_8_SEED),
                     lambda i: any(b % 8 == 0 and b % 32 for b in i[0]["seg_bits"][:-1]) and any(b % 8 for b in i[0]["seg_bits"][:-1]), segment_pixels=100))
    clip = diff_clip()
    out.append(_case("clip_diff", clip, lambda i: [f["rect"] for f in i] == DIFF_RECTS, chunks=(1, 2, 3, 0)))
    out.append(_case("clip_whole_frames", clip, lambda i: all(f["rect"] == (0, 0, 12, 10) for f in i), chunks=(1, 2, 3, 0), diff=False))
    out.append(_case("clip_loop_3_duration_70", clip[:3], loop=3, duration_ms=70))
    out.append(_case("clip_30fps_green", clip[:3], fps=30.0, palette="off"))
    rgb = np.random.default_rng(9).integers(0, 1 << 24, (1, 64, 64)).astype(np.uint32)
    out.append(_case("clip_green_then_indexed", np.concatenate([rgb, _all_used(2, 64, 64, 16)]), lambda i: [f["colours"] for f in i] == [0, 16], chunks=(1, 0)))
    return out


@functools.lru_cache(maxsize=None)
def device_clips():
    """what only the device test adds: one frame that spans several workgroups of every kernel"""
    big = PAL256[np.random.default_rng(12).integers(0, 16, (192, 192)) * (np.arange(192) % 48 < 40)][None]
    return [_case("noise_192x192", big, lambda i: i[0]["segments"] == 5 and i[0]["matches"] > 100, segment_pixels=4096)]


@functools.lru_cache(maxsize=None)
def refused():
    one = np.zeros((1, 2, 2), np.uint32)
    out = []
    for name, opt in (("diff_2", dict(diff=2)), ("lz77_2", dict(lz77=2)), ("segment_below", dict(segment_pixels=-1)), ("loop_below", dict(loop=-1)), ("loop_above", dict(loop=65536)),
                      ("duration_below", dict(duration_ms=-1)), ("duration_above", dict(duration_ms=1 << 24))):
        out.append((name, one, FPS, opt, R.INVAL))
    out.append(("rate_too_slow", one, 0.00001, {}, R.INVAL))
    out.append(("rate_zero", one, 0.0, {}, R.INVAL))
    out.append(("side_above", np.zeros((1, 1, 16385), np.uint32), FPS, {}, R.UNSUPPORTED))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's (file, canvas, info) of a clip, computed once"""
    c = next(c for c in clips() + device_clips() if c["name"] == name)
    return R.encode(c["frames"], c["fps"], **c["opt"])


def check_claims():
    for c in clips() + device_clips():
        assert c["claim"](expected(c["name"])[2]), c["name"]
    assert len(expected("tiles_64x64")[0]) < len(expected("tiles_64x64_literals")[0])
    assert len(expected("table_of_16")[0]) < len(expected("table_of_16_green")[0])
    for name, frames, fps, opt, code in refused():
        try:
            R.encode(frames, fps, **opt)
        except R.Refused as e:
            assert e.code == code, name
        else:
            raise AssertionError(name)


def write(path):
    """for tests/c/webp_encode.c: per clip nf, w, h (u32), fps (f64), the six options (i32), the frames, the file's size (u32), the file"""
    with open(path, "wb") as f:
        cs = clips()
        f.write(struct.pack("<I", len(cs)))
        for c in cs:
            o = R.options(**c["opt"])
            nf, h, w = c["frames"].shape
            f.write(struct.pack("<IIId6i", nf, w, h, c["fps"], int(o["diff"]), R.PALETTE[o["palette"]], int(o["lz77"]), o["segment_pixels"], o["loop"], o["duration_ms"]))
            f.write(c["frames"].tobytes())
            file = expected(c["name"])[0]
            f.write(struct.pack("<I", len(file)) + file)


if __name__ == "__main__":
    check_claims()
    write(sys.argv[1])
