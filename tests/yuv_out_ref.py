"""Frames delivered as YUV (include/tilemotion.h, tm_yuv_out) restated in numpy from the rule's description, not from
the kernel.

    constants   round(k 65536) of the forward matrix of Kr, Kb; the G coefficient absorbs the rounding so that the Y row sums to
                round(ys 65536) and the U and V rows to 0
    a sample    ((c . S + half) >> s) + off, clamped to 0 .. 2^d - 1;  s = 16 - (d - 8) + lw,  half = 1 << (s - 1)
    footprints  the pixel (luma, 4:4:4);  the 2 x 2 block (420jpeg);  columns 2k - 1, 2k, 2k + 1 weighted 1, 2, 1 (422), on rows 2j and
                2j + 1 (420mpeg2);  coordinates outside the picture repeat the edge pixel
"""
import numpy as np

AUTO, BT601_LIMITED, BT601_FULL, TILER, BT709_LIMITED, BT709_FULL = range(6)
C444, C422, C420JPEG, C420MPEG2, MONO = range(5)
U8, U16_LOW, U16_HIGH = range(3)
KRKB = {BT601_LIMITED: (0.299, 0.114), BT601_FULL: (0.299, 0.114), BT709_LIMITED: (0.2126, 0.0722), BT709_FULL: (0.2126, 0.0722)}
INTEGER_MODES = (BT601_LIMITED, BT601_FULL, BT709_LIMITED, BT709_FULL)
LIMITED = (BT601_LIMITED, BT709_LIMITED)

# name -> (chroma, samples, depth, pairs), as tiler_amd.yuv_out names them, plus the deep planar layout the tests ask for
LAYOUTS = {"444": (C444, U8, 8, False), "422": (C422, U8, 8, False), "420jpeg": (C420JPEG, U8, 8, False), "420mpeg2": (C420MPEG2, U8, 8, False),
           "mono": (MONO, U8, 8, False), "nv12": (C420JPEG, U8, 8, True), "p010": (C420JPEG, U16_HIGH, 10, True),
           "420p10": (C420JPEG, U16_LOW, 10, False)}


def float_matrix(mode):
    """rows Y, U, V; columns R, G, B"""
    kr, kb = KRKB[mode]
    kg = 1.0 - kr - kb
    ys, cs = (219.0 / 255.0, 224.0 / 255.0) if mode in LIMITED else (1.0, 1.0)
    return np.array([[kr * ys, kg * ys, kb * ys],
                     [-kr / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, (1 - kb) / (2 * (1 - kb)) * cs],
                     [(1 - kr) / (2 * (1 - kr)) * cs, -kg / (2 * (1 - kr)) * cs, -kb / (2 * (1 - kr)) * cs]])


def int_matrix(mode):
    m = float_matrix(mode)
    c = np.rint(m * 65536.0).astype(np.int64)
    ys = 219.0 / 255.0 if mode in LIMITED else 1.0
    want = [int(np.rint(ys * 65536.0)), 0, 0]
    for r in range(3):
        c[r, 1] += want[r] - c[r].sum()
    return c


def offsets(mode, depth):
    return (16 << (depth - 8)) if mode in LIMITED else 0, 128 << (depth - 8)


def sample(c, sr, sg, sb, lw, depth, off):
    s = 16 - (depth - 8) + lw
    v = ((int(c[0]) * sr + int(c[1]) * sg + int(c[2]) * sb + (1 << (s - 1))) >> s) + off
    return np.clip(v, 0, (1 << depth) - 1)


def channels(rgb):
    a = np.asarray(rgb).astype(np.int64) & 0xffffffff
    return (a >> 16) & 255, (a >> 8) & 255, a & 255


def tiler_pixels(rgb):
    """GenerateY4M's loop: double products narrowed once to Single, + 128 in Single, round half to even, clamp"""
    r, g, b = (c.astype(np.float64) for c in channels(rgb))
    yy = (r * (299.0 / 1000) + g * (587.0 / 1000) + b * (114.0 / 1000)).astype(np.float32)
    uu = ((b - yy.astype(np.float64)) * 0.492).astype(np.float32)
    vv = ((r - yy.astype(np.float64)) * 0.877).astype(np.float32)
    rnd = lambda v: np.clip(np.rint(v.astype(np.float64)), 0, 255).astype(np.int64)  # noqa: E731
    return rnd(yy + np.float32(0.0)), rnd(uu + np.float32(128.0)), rnd(vv + np.float32(128.0))


def pixels(rgb, mode, depth=8):
    """every pixel through the one-pixel footprint -> (Y, U, V) int64 arrays of rgb's shape, d-bit values"""
    if mode == AUTO:
        mode = BT601_LIMITED
    if mode == TILER:
        assert depth == 8
        return tiler_pixels(rgb)
    c = int_matrix(mode)
    yo, co = offsets(mode, depth)
    r, g, b = channels(rgb)
    return sample(c[0], r, g, b, 0, depth, yo), sample(c[1], r, g, b, 0, depth, co), sample(c[2], r, g, b, 0, depth, co)


def _edge(a, ys, xs):
    """a [..., H, W] at rows ys and columns xs, clamped to the picture"""
    h, w = a.shape[-2:]
    return a[..., np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]


def footprint_sums(ch, chroma):
    """one channel [..., H, W] -> (sums over every chroma sample's footprint, lw)"""
    h, w = ch.shape[-2:]
    if chroma == C444:
        return ch, 0
    cw = (w + 1) // 2
    k = np.arange(cw)
    if chroma == C422:
        ys = np.arange(h)
        return _edge(ch, ys, 2 * k - 1) + 2 * _edge(ch, ys, 2 * k) + _edge(ch, ys, 2 * k + 1), 2
    j = np.arange((h + 1) // 2)
    if chroma == C420JPEG:
        return sum(_edge(ch, 2 * j + dy, 2 * k + dx) for dy in (0, 1) for dx in (0, 1)), 2
    assert chroma == C420MPEG2
    return sum(_edge(ch, 2 * j + dy, 2 * k - 1) + 2 * _edge(ch, 2 * j + dy, 2 * k) + _edge(ch, 2 * j + dy, 2 * k + 1) for dy in (0, 1)), 3


def planes(rgb, layout, mode):
    """frames [F][H][W] 0x00RRGGBB -> (y, u, v) as they are stored: uint8, or uint16 words (U16_HIGH: shifted left by 16 - depth); u, v None
    for mono; v None and u [F][ch][2 cw] where U and V alternate"""
    chroma, samples, depth, pairs = LAYOUTS[layout] if isinstance(layout, str) else layout
    if mode == AUTO:
        mode = BT601_LIMITED
    dt = np.uint8 if samples == U8 else np.uint16
    sh = 16 - depth if samples == U16_HIGH else 0
    if mode == TILER:
        assert chroma in (C444, MONO) and samples == U8
        y, u, v = tiler_pixels(rgb)
    else:
        c = int_matrix(mode)
        yo, co = offsets(mode, depth)
        r, g, b = channels(rgb)
        y = sample(c[0], r, g, b, 0, depth, yo)
        if chroma != MONO:
            (sr, lw), (sg, _), (sb, _) = (footprint_sums(x, chroma) for x in (r, g, b))
            u, v = sample(c[1], sr, sg, sb, lw, depth, co), sample(c[2], sr, sg, sb, lw, depth, co)
    y = (y << sh).astype(dt)
    if chroma == MONO:
        return y, None, None
    u, v = (u << sh).astype(dt), (v << sh).astype(dt)
    if pairs:
        return y, np.stack([u, v], axis=-1).reshape(u.shape[:-1] + (2 * u.shape[-1],)), None
    return y, u, v


def all_colours():
    """all 2^24 triples as 0x00RRGGBB"""
    return np.arange(1 << 24, dtype=np.uint32)
