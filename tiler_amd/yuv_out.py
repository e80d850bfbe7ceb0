"""YUV destinations (tm_yuv_out, include/tilemotion.h): the layouts decoded frames can leave in, the arrays that take
them and the descriptor the library reads.  Shared by GtmPlayer.ReadYUV, TilingEncoder.RenderFramesYUV and stages.rgb32_to_yuv; the ctypes
struct is SetFramesYUV's (the field layout is the same, the pointers are written instead of read)."""
import ctypes

import numpy as np

from ._lib import YuvClip, lib, check

YuvOut = YuvClip  # tm_yuv_out

C444, C422, C420JPEG, C420MPEG2, MONO = range(5)      # TM_CHROMA_*
U8, U16_LOW, U16_HIGH = range(3)                      # TM_SAMPLES_*
YUV_MODES = {"auto": 0, "bt601-limited": 1, "bt601-full": 2, "tiler": 3, "bt709-limited": 4, "bt709-full": 5}  # TM_YUV_*

# name -> (chroma, samples, depth, pairs)
LAYOUTS = {"444": (C444, U8, 8, False), "422": (C422, U8, 8, False), "420": (C420JPEG, U8, 8, False), "420jpeg": (C420JPEG, U8, 8, False),
           "420mpeg2": (C420MPEG2, U8, 8, False), "mono": (MONO, U8, 8, False), "nv12": (C420JPEG, U8, 8, True),
           "p010": (C420JPEG, U16_HIGH, 10, True)}


def layout_of(layout):
    """a name of LAYOUTS, or (chroma, samples, depth, pairs) -> that tuple"""
    if isinstance(layout, str):
        if layout not in LAYOUTS:
            raise ValueError("unknown YUV layout %r (one of %s, or (chroma, samples, depth, pairs))" % (layout, " ".join(LAYOUTS)))
        return LAYOUTS[layout]
    chroma, samples, depth, pairs = layout
    return int(chroma), int(samples), int(depth), bool(pairs)


def mode_of(yuv):
    if isinstance(yuv, str):
        if yuv not in YUV_MODES:
            raise ValueError("unknown YUV rule %r (one of %s)" % (yuv, " ".join(YUV_MODES)))
        return YUV_MODES[yuv]
    return int(yuv)


def plane_shapes(layout, frames, height, width):
    """shapes of (y, u, v); None for a plane the layout does not have; with pairs u is [F][ch][2 cw]"""
    chroma, _, _, pairs = layout_of(layout)
    if chroma == MONO:
        return (frames, height, width), None, None
    cw = width if chroma == C444 else (width + 1) // 2
    ch = (height + 1) // 2 if chroma in (C420JPEG, C420MPEG2) else height
    if pairs:
        return (frames, height, width), (frames, ch, 2 * cw), None
    return (frames, height, width), (frames, ch, cw), (frames, ch, cw)


def alloc(layout, frames, height, width, device=None):
    """planes (y, u, v) for `frames` frames: torch tensors on `device` (uint8, or int16 holding the words), or numpy arrays (uint8 / uint16)
    when device is None"""
    _, samples, _, _ = layout_of(layout)
    out = []
    for shape in plane_shapes(layout, frames, height, width):
        if shape is None:
            out.append(None)
        elif device is None:
            out.append(np.zeros(shape, np.uint8 if samples == U8 else np.uint16))
        else:
            import torch
            out.append(torch.zeros(shape, dtype=torch.uint8 if samples == U8 else torch.int16, device=device))
    return tuple(out)


def descriptor(planes, layout, full_range=False):
    """the tm_yuv_out of planes (y, u, v): size, capacity, pointers and strides are taken from the arrays, whose last axis must be dense; a
    chroma plane smaller than the layout makes of y's size is refused here (the library cannot see an array's extent)"""
    chroma, samples, depth, pairs = layout_of(layout)
    y, u, v = planes
    d = YuvOut()
    frames, height, width = (int(n) for n in y.shape)
    need = plane_shapes(layout, frames, height, width)
    on_device = bool(getattr(y, "is_cuda", False))
    item = 1 if samples == U8 else 2
    for name, a in zip("yuv", (y, u, v)):
        if a is None:
            continue
        torch_like = hasattr(a, "data_ptr")
        if bool(getattr(a, "is_cuda", False)) != on_device or (a.element_size() if torch_like else a.itemsize) != item:
            raise ValueError("YUV destination: the planes must share their memory kind and fit the sample type")
        st = [s * item for s in a.stride()] if torch_like else list(a.strides)
        if len(st) != 3 or st[2] != item:
            raise ValueError("YUV destination: plane %s must be [F][rows][samples] with a dense last axis" % name)
        if not torch_like and not a.flags.writeable:
            raise ValueError("YUV destination: plane %s is read-only" % name)
        want = need["yuv".index(name)]
        if want is not None and any(int(have) < n for have, n in zip(a.shape, want)):
            raise ValueError("YUV destination: plane %s is %s, the layout needs %s" % (name, tuple(a.shape), want))
        setattr(d, name, a.data_ptr() if torch_like else a.ctypes.data)
        setattr(d, name + "_row", st[1])
        setattr(d, name + "_frame", st[0])
    d.frames, d.height, d.width = frames, height, width
    d.fps, d.chroma, d.samples, d.depth = 1.0, chroma, samples, depth
    d.full_range, d.memory = int(bool(full_range)), 1 if on_device else 0
    return d


def destination(layout, frames, height, width, device, out, full_range=False):
    """(planes, descriptor) for a read of `frames` frames: `out` -- (y, u, v) to fill -- or fresh arrays"""
    planes = tuple(out) + (None,) * (3 - len(out)) if out is not None else alloc(layout, max(frames, 1), height, width, device)
    return planes, descriptor(planes, layout, full_range)


def probe(d, width, height, yuv="auto"):
    """tm_probe_yuv_out_host: every check the entry points make of the descriptor d for frames of width x height, without a device.  Raises
    TileMotionError as they do."""
    check(lib().tm_probe_yuv_out_host(ctypes.byref(d), int(width), int(height), mode_of(yuv)))


def first(planes, n):
    """the planes' first n frames"""
    return tuple(None if a is None else a[:n] for a in planes)
