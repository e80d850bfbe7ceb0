"""Inputs of the Load and window-feature comparisons past one chunk, batch, strip and grid (tests/test_gpu_load_front.py), each with what it
claims to reach.  tests/test_load_cases_host.py asserts those claims on the oracle's output alone; the GPU tests compare the library with
the oracle on the same inputs.  Everything is a pure function of the case's name: both files see the same arrays.  numpy only.

Sizes are read against the kernels' constants: k_pearson_frames stages PC values per chunk and adds them in groups of 32 (the mean's
doubles) and 64 (the Singles), then one by one; a wave of k_load_tiles converts LT_BATCH consecutive tiles and a workgroup (four waves) takes
a second batch past LOAD_GRID workgroups; a workgroup of k_window_dcts takes strips of WD_RY x WD_CX windows, a second one past WD_GRID."""
import functools
import importlib.util
import os

import numpy as np

PC, PC_GROUP_F64, PC_GROUP_F32 = 2048, 32, 64
LT_BATCH, LOAD_GRID = 8, 2048
WD_RY, WD_CX, WD_GRID = 8, 32, 1024
MM_LIMIT6 = 10922  # the matrix form of the motion search holds |coefficient| <= this in every block


def _synth():
    """tiler_amd/synth.py on its own (numpy only): importing the package would bring the device plumbing with it"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiler_amd", "synth.py")
    spec = importlib.util.spec_from_file_location("_load_cases_synth", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


synth = _synth()


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _seed(*parts):
    """a seed from a case's name: the same in every process (no hash())"""
    s = 0x42381337
    for p in parts:
        for ch in str(p).encode():
            s = (s * 1000003 + ch) & 0xFFFFFFFFFFFF
    return s


def swap_rb(c):
    c = np.asarray(c, np.uint32)
    return ((c & 0xFF) << 16) | ((c >> 16) & 0xFF) | (c & 0xFF00) | (c & np.uint32(0xFF000000))


# ---- Pearson ----------------------------------------------------------------------------------------------------------------------------
# one value (no variance at all), the groups of 32 and 64 and their neighbours, one value short of a chunk, a chunk, one past; a chunk plus
# 32 / 63 / 64 (the second chunk's groups), two chunks, one past, three chunks and one; Load's own size at 720p (22 chunks, the last partial)
PEARSON_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 192, 2047, 2048, 2049, 2080, 2111, 2112, 4096, 4097, 6145, 43200)
PEARSON_FRAMES = (1, 2, 7)
PEARSON_KINDS = ("near", "indep", "same", "const-one", "const-both", "one-off", "large", "tiny")


def pearson_chunks(per):
    return (per + PC - 1) // PC


def _lab_like(rng, per):
    """L uniform in 0..100, a and b uniform in +-100, interleaved as the tile means are, cut to per"""
    n = (per + 2) // 3
    v = np.stack([rng.uniform(0.0, 100.0, n), rng.uniform(-100.0, 100.0, n), rng.uniform(-100.0, 100.0, n)], axis=1)
    return v.reshape(-1)[:per].astype(np.float32)


@functools.lru_cache(maxsize=None)
def pearson_case(kind, per, nframes):
    """float32 [nframes][per]: frame f + 1 is made from frame f by the kind's rule"""
    rng = np.random.default_rng(_seed("pearson", kind, per, nframes))
    out = np.empty((nframes, per), np.float32)
    out[0] = _lab_like(rng, per)
    if kind == "const-both":
        out[0] = np.float32(rng.uniform(-100.0, 100.0))
    for f in range(1, nframes):
        x = out[f - 1]
        if kind in ("near", "large", "tiny"):
            y = x + rng.normal(0.0, 2.0, per).astype(np.float32)
        elif kind == "indep":
            y = rng.permutation(x)
        elif kind == "same":
            y = x
        elif kind == "const-one":  # odd frames are constant: (x, c) and (c, x) both occur
            y = np.full(per, rng.uniform(-100.0, 100.0), np.float32) if f % 2 else _lab_like(rng, per)
        elif kind == "const-both":
            y = np.full(per, rng.uniform(-100.0, 100.0), np.float32)
        elif kind == "one-off":
            y = x.copy()
            y[int(rng.integers(per))] += np.float32(rng.choice([-7.5, 0.25, 31.0]))
        else:
            raise ValueError(kind)
        out[f] = y
    if kind == "large":
        out *= np.float32(300.0)
    if kind == "tiny":  # |value| <= 1e-18: the products are at most 1e-36, a good part of them subnormal Singles
        out *= np.float32(1e-20)
    return _frozen(out)


def pearson_sums(x, y, pairwise=False):
    """(num, sum dx^2, sum dy^2) as Singles: the mean's sum sequential in double, everything else Single; the three sums sequential (the
    reference's order) or, pairwise=True, as numpy's pairwise summation adds them (another order: the discriminating twin)"""
    n = x.size
    mx = np.float32(np.cumsum(x.astype(np.float64))[-1] / n)
    my = np.float32(np.cumsum(y.astype(np.float64))[-1] / n)
    dx, dy = x - mx, y - my
    prods = (dx * dy, dx * dx, dy * dy)
    if pairwise:
        return np.array([np.sum(p, dtype=np.float32) for p in prods], np.float32)
    return np.array([np.cumsum(p, dtype=np.float32)[-1] for p in prods], np.float32)


def pearson_finish(sums):
    """the correlation's last lines on one triple of sums, in Single arithmetic"""
    den = np.sqrt(np.float32(sums[1])) * np.sqrt(np.float32(sums[2]))
    return np.float32(sums[0]) / den if den != 0 else np.float32(1.0)


# ---- Load -------------------------------------------------------------------------------------------------------------------------------
LOAD_SHAPES = (  # (frames, height, width, tm_w, tm_h)
    (1, 1, 1, 1, 1),          # the smallest input
    (2, 7, 5, 1, 1),          # an image smaller than one tile
    (3, 60, 100, 13, 8),      # 104 tiles a frame: a multiple of LT_BATCH
    (3, 100, 52, 7, 13),      # 91 tiles a frame: batches cross frames
    (5, 24, 24, 3, 3),        # 9 tiles a frame: every batch crosses a frame
    (2, 64, 64, 10, 10),      # whole tiles beyond the image stay zero
    (2, 64, 64, 5, 6),        # a tile map smaller than the image
    (8, 2000, 264, 33, 250),  # 66 000 tiles: the second batch of a workgroup
)
LOAD_CONTENTS = ("synth", "noise", "synth-alpha", "noise-alpha", "mirror-ties")


def load_batches(shape):
    f, _, _, tm_w, tm_h = shape
    return (f * tm_w * tm_h + 4 * LT_BATCH - 1) // (4 * LT_BATCH)


def _luma_unit_step():
    """the smallest (dr, dg, db) with 299 dr + 587 dg + 114 db = 1: one luma unit of GetTileZoneSum"""
    best = None
    for dr in range(-60, 61):
        for dg in range(-60, 61):
            rest = 1 - 299 * dr - 587 * dg
            if rest % 114 == 0 and abs(rest // 114) <= 60:
                cand = (abs(dr) + abs(dg) + abs(rest // 114), dr, dg, rest // 114)
                if best is None or cand < best:
                    best = cand
    return best[1:]


@functools.lru_cache(maxsize=None)
def mirror_tie_tiles():
    """(tiles uint32 [n][8][8] 0x00RRGGBB, flags uint8 [n]: what the mirror rule must give them).  Flat tiles, tiles symmetric left-right,
    top-bottom or both -- their half sums tie: flag 0 --, and tiles symmetric both ways but for one pixel that is one luma unit heavier or
    lighter: the quadrant it sits in decides (bit 0: the right half is heavier, bit 1: the bottom half)"""
    rng = np.random.default_rng(_seed("mirror-ties"))
    dr, dg, db = _luma_unit_step()
    tiles, flags = [], []

    def pack(rgb):
        return (rgb[..., 0].astype(np.uint32) << 16) | (rgb[..., 1].astype(np.uint32) << 8) | rgb[..., 2].astype(np.uint32)

    for _ in range(6):  # flat
        tiles.append(pack(np.broadcast_to(rng.integers(0, 256, 3), (8, 8, 3))))
        flags.append(0)
    for _ in range(6):  # left-right symmetric with equal top and bottom sums (rows mirrored too), or only one of the two ...
        q = rng.integers(0, 256, (4, 4, 3))
        top = np.concatenate([q, q[:, ::-1]], axis=1)
        tiles.append(pack(np.concatenate([top, top[::-1]], axis=0)))
        flags.append(0)
    for _ in range(6):  # ... left-right symmetric, the top half heavier: no flag either way
        half = np.sort(rng.integers(0, 256, (8, 4, 3)), axis=0)[::-1]
        half[4:] = half[4:] // 2
        tiles.append(pack(np.concatenate([half, half[:, ::-1]], axis=1)))
        flags.append(0)
    for _ in range(6):  # ... top-bottom symmetric, the left half heavier
        half = np.sort(rng.integers(0, 256, (4, 8, 3)), axis=1)[:, ::-1]
        half[:, 4:] = half[:, 4:] // 2
        tiles.append(pack(np.concatenate([half, half[::-1]], axis=0)))
        flags.append(0)
    for sign in (1, -1):  # one luma unit, in either direction, in each quadrant
        for qy in (0, 1):
            for qx in (0, 1):
                for _ in range(3):
                    q = rng.integers(64, 192, (4, 4, 3))
                    top = np.concatenate([q, q[:, ::-1]], axis=1)
                    t = np.concatenate([top, top[::-1]], axis=0)
                    t[qy * 4 + int(rng.integers(4)), qx * 4 + int(rng.integers(4))] += sign * np.array([dr, dg, db])
                    tiles.append(pack(t))
                    right_heavier = (qx == 1) == (sign == 1)
                    bottom_heavier = (qy == 1) == (sign == 1)
                    flags.append((1 if right_heavier else 0) | (2 if bottom_heavier else 0))
    return _frozen(np.stack(tiles).astype(np.uint32)), _frozen(np.array(flags, np.uint8))


def tiles_to_image(tiles, rows, cols):
    """uint32 [rows*cols][8][8] -> [rows*8][cols*8]"""
    return np.ascontiguousarray(tiles.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))


@functools.lru_cache(maxsize=4)
def load_case(content, shape):
    """uint32 [F][H][W] RGB32 (0xAARRGGBB)"""
    f, h, w, _, _ = shape
    rng = np.random.default_rng(_seed("load", content.replace("-alpha", ""), shape))
    if content.startswith("synth"):
        out = synth.video(f, w, h, cut=2) & np.uint32(0xFFFFFF)
    elif content.startswith("noise"):
        out = rng.integers(0, 1 << 24, (f, h, w), dtype=np.uint32)
    elif content == "mirror-ties":
        tiles, _ = mirror_tie_tiles()
        rows, cols = (h + 7) // 8, (w + 7) // 8
        pick = rng.integers(0, tiles.shape[0], (f, rows * cols))
        out = np.stack([tiles_to_image(tiles[pick[i]], rows, cols)[:h, :w] for i in range(f)])
    else:
        raise ValueError(content)
    if content.endswith("-alpha"):
        out = out | (np.random.default_rng(_seed("load-alpha", shape)).integers(0, 256, (f, h, w), dtype=np.uint32) << 24)
    return _frozen(out.astype(np.uint32))


# ---- window features --------------------------------------------------------------------------------------------------------------------
WINDOW_BUFFERS = (  # (width, height)
    (8, 8),      # one window
    (9, 8),      # two windows in a row
    (8, 9),      # two windows in a column
    (15, 15),    # 8 x 8 windows: less than one strip both ways
    (39, 15),    # 32 x 8 windows: one full strip
    (40, 16),    # a full strip plus strips of one column and one row
    (47, 23),    # 40 x 16 windows: ragged strips both ways
    (71, 8),     # two full strips in a row
    (72, 9),     # ragged strips past two full ones
    (104, 64),   # a 13 x 8 tile frame
)
WINDOW_BUFFERS_LARGE = (
    (8, 8207),   # 1025 strips of one column: a workgroup's second strip
    (72, 2759),  # 3 x 344 = 1032 strips, 178 880 windows
)
WINDOW_CONTENTS = ("synth", "noise", "checker", "flat", "two-level", "ramps", "periodic", "noise-alpha")
WINDOW_CONTENTS_LARGE = ("noise", "two-level")
WINDOW_CASES = tuple((c, b) for b in WINDOW_BUFFERS for c in WINDOW_CONTENTS) + tuple((c, b) for b in WINDOW_BUFFERS_LARGE for c in WINDOW_CONTENTS_LARGE)


def window_strips(buf):
    w, h = buf
    return ((w - 7 + WD_CX - 1) // WD_CX) * ((h - 7 + WD_RY - 1) // WD_RY)


def _bgr(r, g, b):
    return (np.asarray(b, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(r, np.uint32)


@functools.lru_cache(maxsize=4)
def frame_buffer(content, buf):
    """uint32 [height][width] 0x00BBGGRR, the layout of the encoder's frame buffers (the top byte is random for noise-alpha)"""
    w, h = buf
    rng = np.random.default_rng(_seed("window", content.replace("-alpha", ""), buf))
    y, x = np.mgrid[0:h, 0:w]
    if content == "synth":
        # the top left quarter of a synthetic frame of twice the size: its gradients stay in the darker half, where no window's DC term
        # leaves the range of the search's matrix form (a window of near-white pixels does: 13 214)
        out = swap_rb(synth.frame(1, 2 * w, 2 * h, np.random.default_rng(_seed("synth", buf)))[:h, :w]) & np.uint32(0xFFFFFF)
    elif content in ("noise", "noise-alpha"):
        out = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
        if content == "noise-alpha":
            out = out | (np.random.default_rng(_seed("alpha", buf)).integers(0, 256, (h, w), dtype=np.uint32) << 24)
    elif content == "checker":  # one-pixel black and white squares, their phase flipped on every other 8 x 8 block of a grid offset by 3 pixels
        v = (((x + y) ^ ((x + 3) >> 3) ^ ((y + 3) >> 3)) & 1) * 255
        out = _bgr(v, v, v)
    elif content == "flat":
        r, g, b = rng.integers(0, 200, 3)  # (dark enough for the matrix form's range, like two-level)
        out = np.full((h, w), _bgr(r, g, b), np.uint32)
    elif content == "two-level":  # green one step up on a random half of the pixels
        r, g, b = rng.integers(1, 200, 3)
        out = _bgr(np.full((h, w), r), g + rng.integers(0, 2, (h, w)), np.full((h, w), b))
    elif content == "ramps":
        # 0..200 along x, 0..150 along y, 0..100 along x + y, whatever the size: no window is bright enough to leave the matrix form's range
        out = _bgr(200 * x // max(w - 1, 1), 150 * y // max(h - 1, 1), 100 * (x + y) // max(w + h - 2, 1))
    elif content == "periodic":
        tile = rng.integers(0, 1 << 24, (8, 8), dtype=np.uint32)
        out = tile[y & 7, x & 7]
    else:
        raise ValueError(content)
    return _frozen(out.astype(np.uint32))


# ---- motion search from a frame buffer -------------------------------------------------------------------------------------------------
MOTION_GRIDS = ((1, 1), (4, 1), (5, 2), (13, 8), (33, 9), (29, 18))  # (tm_w, tm_h)
MOTION_RADII = (1, 8, 32, 128)
MOTION_FORMS = (None, "TM_MOTION_PACK_SEPARATE", "TM_MOTION_FORCE_FLAG", "TM_MOTION_VALU")
MOTION_CASES = tuple((c, g, r) for g in MOTION_GRIDS for r in MOTION_RADII if g != (29, 18) or r == 32 for c in WINDOW_CONTENTS)


def motion_frame_buffer(content, grid):
    return frame_buffer(content, (grid[0] * 8, grid[1] * 8))


@functools.lru_cache(maxsize=4)
def motion_second_frame(content, grid):
    """the frame whose tiles are searched: the buffer's picture moved by (+3, -2) pixels with its edge repeated, noise of +-2 per channel on a
    quarter of the tiles -> uint32 [tm_h*8][tm_w*8] 0x00BBGGRR"""
    fb = motion_frame_buffer(content, grid)
    h, w = fb.shape
    rng = np.random.default_rng(_seed("second", content, grid))
    y, x = np.mgrid[0:h, 0:w]
    moved = fb[np.clip(y + 2, 0, h - 1), np.clip(x - 3, 0, w - 1)]
    noisy = np.repeat(np.repeat(rng.random((grid[1], grid[0])) < 0.25, 8, axis=0), 8, axis=1)
    out = np.zeros((h, w), np.uint32)
    for shift in (0, 8, 16):
        ch = ((moved >> shift) & 0xFF).astype(np.int64) + rng.integers(-2, 3, (h, w)) * noisy
        out |= np.clip(ch, 0, 255).astype(np.uint32) << shift
    return _frozen(out)


def screen_to_tiles(screen):
    """[tm_h*8][tm_w*8] -> [tm_h*tm_w][64], the tiles in their original orientation"""
    h, w = screen.shape
    return np.ascontiguousarray(screen.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64))


# ---- the Load step -----------------------------------------------------------------------------------------------------------------------
STEP_CLIPS = {  # name -> (frames, width, height, cut, values a frame, the oracle's key frames at ShotTransMinSecondsPerKF = 0.05)
    "264x256": (6, 264, 256, 3, 3168, [0, 3]),
    "1000x200": (5, 1000, 200, 2, 9375, [0, 2, 4]),
}
STEP_FPS = 24.0
STEP_MIN_SECONDS = (0.05, None)  # None: the default (1 s: only frame 0 is a key frame)


@functools.lru_cache(maxsize=2)
def step_clip(name):
    n, w, h, cut = STEP_CLIPS[name][:4]
    return _frozen(synth.video(n, w, h, cut=cut))
