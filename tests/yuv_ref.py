"""The three colour rules of Load's input path (include/tilemotion.h, TM_YUV_*) in numpy, from their description.  Bytes Y, U, V in, pixels
0x00RRGGBB out; D = U - 128, E = V - 128, every channel clamped to 0..255."""
import numpy as np

AUTO, BT601_LIMITED, BT601_FULL, TILER = 0, 1, 2, 3


def rgb_channels(y, u, v, mode):
    Y = np.asarray(y).astype(np.int64)
    D = np.asarray(u).astype(np.int64) - 128
    E = np.asarray(v).astype(np.int64) - 128
    if mode in (AUTO, BT601_LIMITED):  # (AUTO without a header: limited range)
        C = Y - 16
        R = (298 * C + 409 * E + 128) >> 8
        G = (298 * C - 100 * D - 208 * E + 128) >> 8
        B = (298 * C + 516 * D + 128) >> 8
    elif mode == BT601_FULL:  # libjpeg's constants
        R = (65536 * Y + 91881 * E + 32768) >> 16
        G = (65536 * Y - 22554 * D - 46802 * E + 32768) >> 16
        B = (65536 * Y + 116130 * D + 32768) >> 16
    elif mode == TILER:
        # YUVToRGB (utils.pas:492-509): Single operands, each right-hand side evaluated in double and narrowed once to Single, Round
        # (half to even), EnsureRange
        yd, ud, vd = (a.astype(np.float32).astype(np.float64) for a in (Y, D, E))
        r = (yd + vd * 1.13983).astype(np.float32)
        g = (yd - ud * 0.39465 - vd * 0.58060).astype(np.float32)
        b = (yd + ud * 2.03211).astype(np.float32)
        R, G, B = (np.rint(c).astype(np.int64) for c in (r, g, b))
    else:
        raise ValueError(mode)
    return np.clip(R, 0, 255), np.clip(G, 0, 255), np.clip(B, 0, 255)


def to_rgb32(y, u, v, mode):
    R, G, B = rgb_channels(y, u, v, mode)
    return ((R << 16) | (G << 8) | B).astype(np.uint32)
