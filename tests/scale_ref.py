"""The RGB32 scaling rule (include/tilemotion.h, tm_stage_scale_rgb32), restated in numpy on top of
tests/resample_ref.py: a frame is uint32 0x00RRGGBB, its R, G and B are three planes at luma positions (s = 1, o = 0), each resampled by the
rule of section 17 and packed with a top byte of 0.  "nearest": output sample j of m takes source sample ((2 j + 1) n) // (2 m), per axis.
Test infrastructure (no test in here)."""
import numpy as np

from tests import resample_ref

LANCZOS3, NEAREST = 0, 1
FILTERS = {"lanczos": LANCZOS3, "nearest": NEAREST}

# source (w, h) -> destination (w, h): enlarging by 2 and 1.5, shrinking by 2, by a little more than 2 (odd sizes), one axis only, by exactly 8
# (48 taps), the identity, and a source smaller than one tile enlarged by 2.5 and 8 and shrunk by 8
SHAPES = [((264, 136), (528, 272)), ((264, 136), (396, 204)), ((264, 136), (132, 68)), ((264, 136), (131, 67)), ((264, 136), (199, 136)),
          ((264, 136), (33, 17)), ((264, 136), (264, 136)), ((40, 24), (100, 60)), ((40, 24), (320, 192)), ((40, 24), (5, 3))]


def scale(frames, dst_w, dst_h, filter="lanczos"):
    """frames uint32 [..., H, W] -> uint32 [..., dst_h, dst_w], top byte 0"""
    frames = np.asarray(frames, np.uint32)
    src_h, src_w = frames.shape[-2:]
    if FILTERS.get(filter, filter) == NEAREST:
        ys = ((2 * np.arange(dst_h, dtype=np.int64) + 1) * src_h) // (2 * dst_h)
        xs = ((2 * np.arange(dst_w, dtype=np.int64) + 1) * src_w) // (2 * dst_w)
        return frames[..., ys[:, None], xs[None, :]] & np.uint32(0xFFFFFF)
    out = np.zeros(frames.shape[:-2] + (dst_h, dst_w), np.uint32)
    for shift in (16, 8, 0):
        plane = ((frames >> np.uint32(shift)) & np.uint32(255)).astype(np.uint8)
        out |= resample_ref.resample(plane, src_w, src_h, dst_w, dst_h).astype(np.uint32) << np.uint32(shift)
    return out


def random_frames(seed, nf, h, w):
    """noise in all four bytes: the top byte must not matter"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (nf, h, w), dtype=np.uint64).astype(np.uint32)


def edge_frames(nf, h, w):
    """halves of 0 and 255 per channel, split along another line in each frame and channel: the Lanczos lobes overshoot on both sides of a
    hard edge, so the clamp bites at 0 and at 255"""
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((nf, h, w), np.uint32)
    for f in range(nf):
        r = np.where(x < w // 2 + f, 0, 255)
        g = np.where(y < h // 2 - f, 255, 0)
        b = np.where(x * h + (f + 1) * y * w // 2 < w * h, 0, 255)
        out[f] = (r.astype(np.uint32) << 16) | (g.astype(np.uint32) << 8) | b.astype(np.uint32) | np.uint32(0xA5000000)
    return out
