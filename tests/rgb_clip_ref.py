"""An RGB clip lent in memory (include/tilemotion.h, tm_rgb_clip) in numpy, from its description: every layout's samples are picked out of
the array, deep samples become bytes by the YUV clips' rule (yuv_clip_ref.narrow), the pixel is R << 16 | G << 8 | B, and a clip at another
size is scale_ref.scale(..., "lanczos") of those pixels.  Test infrastructure (no test in here)."""
import numpy as np

from tests import scale_ref, yuv_clip_ref
from tests.yuv_clip_ref import U8, U16_LOW, U16_HIGH

# the packed layouts: channels per pixel, and where R, G, B sit among them; [N,H,W,C]
PACKED = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)), "argb": (4, (1, 2, 3)), "abgr": (4, (3, 2, 1)),
          "rgb48": (3, (0, 1, 2)), "bgr48": (3, (2, 1, 0)), "rgba64": (4, (0, 1, 2)), "bgra64": (4, (2, 1, 0))}
PACKED8 = ("rgb24", "bgr24", "rgba", "bgra", "argb", "abgr")
PACKED16 = ("rgb48", "bgr48", "rgba64", "bgra64")
# the planar layouts: which plane holds R, G, B; [N,3,H,W]
PLANAR = {"rgbp": (0, 1, 2), "gbrp": (2, 0, 1)}


def channels(buf, layout):
    """the R, G, B samples [N,H,W] of an array in the layout's shape, as stored"""
    buf = np.asarray(buf)
    if layout in PACKED:
        assert buf.ndim == 4 and buf.shape[3] == PACKED[layout][0]
        return tuple(buf[..., i] for i in PACKED[layout][1])
    if layout in PLANAR:
        assert buf.ndim == 4 and buf.shape[1] == 3
        return tuple(buf[:, i] for i in PLANAR[layout])
    assert layout == "gray" and buf.ndim == 3
    return buf, buf, buf


def unpack(buf, layout, samples=U8, depth=8):
    """the unscaled pixels: uint32 [N,H,W] 0x00RRGGBB"""
    r, g, b = (yuv_clip_ref.narrow(c, samples, depth).astype(np.uint32) for c in channels(buf, layout))
    return (r << np.uint32(16)) | (g << np.uint32(8)) | b


def to_rgb32(buf, layout, samples, depth, dst_w, dst_h):
    """the RGB32 frames [N][dst_h][dst_w] Load makes of a lent clip"""
    px = unpack(buf, layout, samples, depth)
    return px if px.shape[-2:] == (dst_h, dst_w) else scale_ref.scale(px, dst_w, dst_h, "lanczos")


def pack(rgb32, layout, samples=U8, depth=8, rng=None):
    """an array in the layout's shape whose pixels unpack to rgb32 & 0xffffff exactly (deep samples: the byte in the sample's high bits, noise
    below it that the rule rounds away); alpha, and with rng every bit the rule ignores, is noise.  "gray" takes the green channel."""
    rgb32 = np.asarray(rgb32, np.uint32)
    rng = rng or np.random.default_rng(0)
    ch = [((rgb32 >> np.uint32(s)) & np.uint32(255)).astype(np.uint16) for s in (16, 8, 0)]
    if samples == U8:
        dt, store = np.uint8, [c.astype(np.uint8) for c in ch]
    else:
        dt = np.uint16
        # p_d = byte << (d - 8) plus less than half a step: (p_d + 2^(d-9)) >> (d - 8) gives the byte back
        deep = [(c << (depth - 8)) + rng.integers(0, 1 << (depth - 9), c.shape).astype(np.uint16) for c in ch]
        junk = [rng.integers(0, 1 << (16 - depth), c.shape).astype(np.uint16) if depth < 16 else np.zeros(c.shape, np.uint16) for c in ch]
        store = [(d | (j << depth)) if samples == U16_LOW else ((d << (16 - depth)) | j) for d, j in zip(deep, junk)]
    n, h, w = rgb32.shape
    if layout in PACKED:
        nch, idx = PACKED[layout]
        out = rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), (n, h, w, nch)).astype(dt)
        for c, i in zip(store, idx):
            out[..., i] = c
        return out
    if layout in PLANAR:
        out = np.zeros((n, 3, h, w), dt)
        for c, i in zip(store, PLANAR[layout]):
            out[:, i] = c
        return out
    assert layout == "gray"
    return store[1].astype(dt)


def random_clip(rng, layout, n, h, w, samples=U8, depth=8):
    """noise in every byte of the layout's array, alpha included; deep samples in their own bits only (dirty() sets the others)"""
    if layout in PACKED:
        shape = (n, h, w, PACKED[layout][0])
    elif layout in PLANAR:
        shape = (n, 3, h, w)
    else:
        shape = (n, h, w)
    if samples == U8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    p = rng.integers(0, 1 << depth, shape).astype(np.uint16)
    return p << (16 - depth) if samples == U16_HIGH else p


def padded(a, layout, pad, extra_rows, lead=0):
    """the array's bytes inside a flat buffer of 0xFF whose rows are `pad` bytes longer and whose frames (planes) `extra_rows` rows longer,
    starting `lead` bytes into it: (a view of the array's own shape and type, the flat uint8 buffer that holds it)"""
    a = np.ascontiguousarray(a)
    hax = 2 if layout in PLANAR else 1
    row_bytes = int(np.prod(a.shape[hax + 1:])) * a.itemsize
    big_shape = a.shape[:hax] + (a.shape[hax] + extra_rows, row_bytes + pad)
    flat = np.full(lead + int(np.prod(big_shape)), 0xFF, np.uint8)
    big = flat[lead:].reshape(big_shape)
    big[..., :a.shape[hax], :row_bytes] = a.view(np.uint8).reshape(a.shape[:hax + 1] + (row_bytes,))
    return np.ndarray(a.shape, a.dtype, buffer=flat, offset=lead, strides=big.strides[:hax + 1] + a.strides[hax + 1:]), flat


def dirty(rng, buf, samples, depth):
    """the same clip with the bits outside the depth set at random: above it for U16_LOW, below it for U16_HIGH"""
    if samples == U8 or depth == 16:
        return buf
    junk = rng.integers(0, 1 << (16 - depth), buf.shape).astype(np.uint16)
    return buf | (junk << depth if samples == U16_LOW else junk)
