"""The resampling rule of Load's input path (include/tilemotion.h, tm_stage_yuv_to_rgb32), restated in numpy from
its description -- not from the C++.  Separable, horizontal pass first, integer throughout:

    r = n / m;  f = max(1, r / s);  x_j = (j + 0.5) r - 0.5;  u_j = (x_j - o) / s
    taps k = max(0, ceil(u_j - 3f)) .. min(np - 1, floor(u_j + 3f))
    w_k = L((k - u_j) / f),  L(t) = sinc(t) sinc(t / 3) for |t| < 3
    c_k = RoundHalfEven(16384 w_k / sum w); the remainder 16384 - sum c goes to the tap of largest w (lowest k on a tie)
    horizontal: h = (sum c_k p_k + 64) >> 7;   vertical: v = clamp((sum c_k h_k + 2^20) >> 21, 0, 255)

`sin` is the C library's (math.sin), as on the other side, so that the rounded coefficients cannot differ."""
import math

import numpy as np

MAX_TAPS = 64

# chroma layout -> (sx, sy, ox, oy): the plane's samples sit at luma positions s k + o
LAYOUTS = {"444": (1, 1, 0.0, 0.0), "422": (2, 1, 0.0, 0.0), "420jpeg": (2, 2, 0.5, 0.5), "420mpeg2": (2, 2, 0.0, 0.5), "mono": None}
CHROMA_ID = {"444": 0, "422": 1, "420jpeg": 2, "420mpeg2": 3, "mono": 4}


def lanczos(t):
    t = abs(t)
    if t >= 3.0:
        return 0.0
    if t == 0.0:
        return 1.0
    x = math.pi * t
    return (math.sin(x) / x) * (math.sin(x / 3.0) / (x / 3.0))


def taps(n, m, n_plane, s, o):
    """[(first tap, [coefficients])] for the m output samples of one axis"""
    r = n / m
    if r / s > 8:
        raise ValueError("more than 64 taps")
    f = max(1.0, r / s)
    out = []
    for j in range(m):
        x = (j + 0.5) * r - 0.5
        u = (x - o) / s
        k0 = max(0, math.ceil(u - 3.0 * f))
        k1 = min(n_plane - 1, math.floor(u + 3.0 * f))
        w = [lanczos((k - u) / f) for k in range(k0, k1 + 1)]
        tot = 0.0
        for v in w:
            tot += v
        c = [int(np.rint(v / tot * 16384.0)) for v in w]
        best = max(range(len(w)), key=lambda i: (w[i], -i))
        c[best] += 16384 - sum(c)
        out.append((k0, c))
    return out


def chroma_shape(layout, w, h):
    sx, sy, _, _ = LAYOUTS[layout]
    return ((h + 1) // 2 if sy == 2 else h, (w + 1) // 2 if sx == 2 else w)


def resample(plane, src_w, src_h, dst_w, dst_h, sx=1, sy=1, ox=0.0, oy=0.0):
    """plane uint8 [..., ph, pw] (leading axes: frames) -> uint8 [..., dst_h, dst_w]"""
    ph, pw = plane.shape[-2:]
    tx, ty = taps(src_w, dst_w, pw, sx, ox), taps(src_h, dst_h, ph, sy, oy)
    p = plane.astype(np.int64)
    h = np.zeros(plane.shape[:-1] + (dst_w,), np.int64)
    for j, (k0, c) in enumerate(tx):
        h[..., j] = (p[..., k0:k0 + len(c)] @ np.array(c, np.int64) + 64) >> 7
    assert np.abs(h).max() < 2 ** 31
    out = np.zeros(plane.shape[:-2] + (dst_h, dst_w), np.int64)
    for i, (k0, c) in enumerate(ty):
        s2 = np.tensordot(np.array(c, np.int64), h[..., k0:k0 + len(c), :], axes=([0], [-2]))
        assert np.abs(s2).max() < 2 ** 31
        out[..., i, :] = (s2 + (1 << 20)) >> 21
    return np.clip(out, 0, 255).astype(np.uint8)


def resample_yuv(y, u, v, layout, dst_w, dst_h):
    """the three planes of a clip at the output size: y [..., H, W]; u, v as chroma_shape says (ignored for "mono")"""
    src_h, src_w = y.shape[-2:]
    Y = resample(y, src_w, src_h, dst_w, dst_h)
    if layout == "mono":
        half = np.full_like(Y, 128)
        return Y, half, half
    sx, sy, ox, oy = LAYOUTS[layout]
    return Y, resample(u, src_w, src_h, dst_w, dst_h, sx, sy, ox, oy), resample(v, src_w, src_h, dst_w, dst_h, sx, sy, ox, oy)
