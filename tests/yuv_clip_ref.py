"""A YUV clip lent in memory (include/tilemotion.h, tm_yuv_clip) in numpy, from its description: deep samples become bytes where they are
fetched, interleaved chroma is split into two planes, and from there on the clip goes through the existing restatements unchanged
(resample_ref.resample_yuv, yuv_ref.to_rgb32).  The two BT.709 colour rules are held here.

    U16_LOW:  p_d = word & (2^d - 1)        U16_HIGH:  p_d = word >> (16 - d)        p = min(255, (p_d + 2^(d-9)) >> (d - 8))
"""
import numpy as np

from tests import resample_ref, yuv_ref

U8, U16_LOW, U16_HIGH = 0, 1, 2
BT709_LIMITED, BT709_FULL = 4, 5
KR, KB = 0.2126, 0.0722


def narrow(words, samples, depth):
    """samples as stored (bytes, or 16-bit words of either signedness) -> bytes"""
    if samples == U8:
        assert depth == 8
        return np.asarray(words).astype(np.uint8)
    assert 9 <= depth <= 16
    w = np.asarray(words).astype(np.int64) & 0xffff  # (the word's bits, whatever integer type carried them)
    pd = (w & ((1 << depth) - 1)) if samples == U16_LOW else (w >> (16 - depth))
    return np.minimum(255, (pd + (1 << (depth - 9))) >> (depth - 8)).astype(np.uint8)


def split_pairs(uv):
    """a plane [..., ch, 2 cw] of (U, V) pairs, U first -> u, v [..., ch, cw]"""
    return uv[..., 0::2], uv[..., 1::2]


def bt709_matrix(limited):
    """rows R, G, B; columns the factors of (Y - 16 or Y), D = U - 128, E = V - 128; from Kr and Kb"""
    kg = 1.0 - KR - KB
    ys, cs = (255.0 / 219.0, 255.0 / 224.0) if limited else (1.0, 1.0)
    return np.array([[ys, 0.0, 2.0 * (1.0 - KR) * cs],
                     [ys, -2.0 * KB * (1.0 - KB) / kg * cs, -2.0 * KR * (1.0 - KR) / kg * cs],
                     [ys, 2.0 * (1.0 - KB) * cs, 0.0]])


BT709_INT = {BT709_LIMITED: (8, 16, [[298, 0, 459], [298, -55, -136], [298, 541, 0]]),
             BT709_FULL: (16, 0, [[65536, 0, 103206], [65536, -12276, -30679], [65536, 121609, 0]])}  # fractional bits, luma offset, rows R G B


def rgb_channels(y, u, v, mode):
    if mode not in BT709_INT:
        return yuv_ref.rgb_channels(y, u, v, mode)
    bits, y0, m = BT709_INT[mode]
    C = np.asarray(y).astype(np.int64) - y0
    D = np.asarray(u).astype(np.int64) - 128
    E = np.asarray(v).astype(np.int64) - 128
    return tuple(np.clip((r[0] * C + r[1] * D + r[2] * E + (1 << (bits - 1))) >> bits, 0, 255) for r in m)


def to_rgb32(y, u, v, mode):
    if mode not in BT709_INT:
        return yuv_ref.to_rgb32(y, u, v, mode)
    R, G, B = rgb_channels(y, u, v, mode)
    return ((R << 16) | (G << 8) | B).astype(np.uint32)


def narrowed_planes(y, u, v, layout, samples, depth):
    """the clip as three planes of bytes (u, v None for "mono"): v None means u holds pairs"""
    if layout == "mono":
        return narrow(y, samples, depth), None, None
    if v is None:
        u, v = split_pairs(u)
    return narrow(y, samples, depth), narrow(u, samples, depth), narrow(v, samples, depth)


def clip_to_rgb32(y, u, v, layout, samples, depth, dst_w, dst_h, mode):
    """the RGB32 frames [F][dst_h][dst_w] Load makes of a lent clip"""
    Y, U, V = narrowed_planes(y, u, v, layout, samples, depth)
    return to_rgb32(*resample_ref.resample_yuv(Y, U, V, layout, dst_w, dst_h), mode)
