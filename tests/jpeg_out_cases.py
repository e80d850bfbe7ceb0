"""The pictures of the JPEG writer's tests, seeded, with what each one is there to reach.  `python
tests/jpeg_out_cases.py FILE` writes them with the restatement's files for tests/c/jpeg_encode.c (tools/asan_jpeg_out.sh).

  cases()      [(name, rgb uint8 [h][w][3], reaches)]
  by_size()    {(w, h): [names]}: the pictures of one size go through the device form as the frames of one call, in one launch
  REACHED      [(property, case, sampling, quality, restart_rows)]: where the restatement alone must show a property
  strided / stack32   the pictures of one size as padded frames, the store and a view of it
  rgb32(rgb)   the picture as the library takes it, uint32 [h][w] of 0x00RRGGBB

The device form codes a lane per block in workgroups of 256 lanes over all blocks of a call: 520x24 at 4:4:4 has 195 blocks in an MCU
row, so a workgroup's span ends inside the second row, and a call's second frame starts inside a workgroup.  24x520 at 4:4:4 with a
restart interval of one row has 65 segments: more than a wave's lanes and more than the eight RSTn numbers."""
import functools
import struct
import sys

import numpy as np

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 49), (72, 64), (520, 24), (24, 520)]


def _grey(v):
    return np.repeat(np.asarray(v, np.uint8)[..., None], 3, -1)


def flat(w, h, colour=(200, 30, 90)):
    return np.tile(np.array(colour, np.uint8), (h, w, 1))


def smooth(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 3 + yy) % 256, (yy * 5 + 20) % 256, (xx + yy * 2) % 256], -1).astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def checker(w, h, cell=1):
    yy, xx = np.mgrid[0:h, 0:w]
    return _grey(((xx // cell + yy // cell) % 2) * 255)


def steps(w, h):
    """8x8 blocks that alternate between 0 and 255: the largest DC differences"""
    return checker(w, h, 8)


def mixed(w, h, seed):
    """smooth with a noisy quarter and a hard edge"""
    p = smooth(w, h)
    n = noise(w, h, seed)
    p[:h // 2 + 1, :w // 2 + 1] = n[:h // 2 + 1, :w // 2 + 1]
    p[:, w - 1 - w // 5:] = 255 - p[:, w - 1 - w // 5:]
    return p


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, rgb, reaches):
        out.append((name, np.ascontiguousarray(rgb, np.uint8), reaches))
    add("flat_1x1", flat(1, 1), "one pixel: every sample of every block is an edge repeat; EOB only")
    add("noise_1x1", noise(1, 1, 1), "one pixel of another colour, the second frame of the 1x1 call")
    add("smooth_7x9", smooth(7, 9), "less than a block across, two partial blocks down")
    add("noise_7x9", noise(7, 9, 2), "the same with noise")
    add("flat_8x8", flat(8, 8), "EOB only; at 4:2:0 and 4:2:2 dummy blocks to the right and (4:2:0) below")
    add("checker_8x8", checker(8, 8), "a 0/255 checkerboard: coefficient 63 set (no EOB) and, at low quality, runs above 15 (ZRL)")
    add("rows_8x8", _grey(np.repeat((np.arange(8) % 2 * 255)[:, None], 8, 1)), "8 rows at 4:2:0: the shrunk plane repeats its own last row")
    add("smooth_16x16", smooth(16, 16), "one MCU of 4:2:0")
    add("noise_16x16", noise(16, 16, 3), "noise at quality 100: the most bits, FF bytes")
    add("mixed_17x23", mixed(17, 23, 4), "partial MCUs on both axes, odd chroma sizes, dummy blocks right and below")
    add("checker_17x23", checker(17, 23), "the checkerboard over partial blocks")
    add("mixed_33x49", mixed(33, 49, 5), "more than one block per row, partial MCUs")
    add("noise_33x49", noise(33, 49, 6), "noise over several MCU rows")
    add("smooth_72x64", smooth(72, 64), "whole MCUs")
    add("steps_72x64", steps(72, 64), "blocks of 0 and 255 in turn: DC category 11")
    add("mixed_520x24", mixed(520, 24, 7), "crosses a workgroup's span of blocks")
    add("noise_520x24", noise(520, 24, 8), "the same with noise: long blocks across the span's end")
    add("mixed_24x520", mixed(24, 520, 9), "65 segments at 4:4:4 with a restart interval of one row")
    add("steps_24x520", steps(24, 520), "the largest DC differences down 65 segments")
    return out


def by_size():
    out = {}
    for name, rgb, _ in cases():
        out.setdefault((rgb.shape[1], rgb.shape[0]), []).append(name)
    return out


def case(name):
    return {n: p for n, p, _ in cases()}[name]


def rgb32(rgb):
    p = np.asarray(rgb).astype(np.uint32)
    return p[..., 0] << 16 | p[..., 1] << 8 | p[..., 2]


def strided(names, row_pad=0, frame_pad=0):
    """the named pictures (of one size) in a store uint32 [F][frame_px] whose rows are row_pad and whose frames frame_pad pixels longer than
    the pictures, the padding filled with a colour the files must not show -> (store, row stride, frame stride in pixels, h, w)"""
    pics = [rgb32(case(n)) for n in names]
    h, w = pics[0].shape
    store = np.full((len(pics), h * (w + row_pad) + frame_pad), 0x00fe01fd, np.uint32)
    for f, p in enumerate(pics):
        store[f, :h * (w + row_pad)].reshape(h, w + row_pad)[:, :w] = p
    return store, w + row_pad, store.shape[1], h, w


def stack32(names, row_pad=0, frame_pad=0):
    """the same as a view uint32 [F][H][W] of that store"""
    store, stride, frame_px, h, w = strided(names, row_pad, frame_pad)
    return np.lib.stride_tricks.as_strided(store, (len(names), h, w), (frame_px * 4, stride * 4, 4))


# where the restatement must show each property (tests/test_jpeg_out_host.py asserts them on the restatement alone)
REACHED = [
    ("ff00", "noise_16x16", "444", 100, 1),
    ("zrl", "checker_8x8", "grey", 1, 0),
    ("no_eob", "checker_8x8", "grey", 100, 0),
    ("dc_cat_11", "steps_72x64", "444", 100, 0),
    ("ac_cat_10", "checker_8x8", "grey", 100, 0),
    ("dummy_right", "mixed_17x23", "422", 90, 1),
    ("dummy_below", "flat_8x8", "420", 90, 1),
    ("segments_65", "mixed_24x520", "444", 90, 1),
]


def dump(path):
    """for tests/c/jpeg_encode.c: count, then per item w, h, quality, sampling, restart_rows, the file's size, the pixels (uint32), the file"""
    try:
        from tests import jpeg_out_ref
    except ImportError:
        import jpeg_out_ref
    sampling_id = {"420": 0, "422": 1, "444": 2, "grey": 3}
    items = []
    for name, rgb, _ in cases():
        if rgb.shape[0] * rgb.shape[1] > 72 * 64:
            continue
        for k, sampling in enumerate(jpeg_out_ref.SAMPLINGS):
            q, r = (1, 50, 90, 100)[(k + len(items)) % 4], (0, 1, 2)[len(items) % 3]
            items.append((rgb, q, sampling_id[sampling], r, jpeg_out_ref.encode(rgb, q, sampling, r)[0]))
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(items)))
        for rgb, q, s, r, f in items:
            fh.write(struct.pack("<6I", rgb.shape[1], rgb.shape[0], q, s, r, len(f)) + rgb32(rgb).astype("<u4").tobytes() + f)


if __name__ == "__main__":
    dump(sys.argv[1])
