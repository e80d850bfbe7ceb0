"""RGB clips in memory as tm_rgb_clip describes them (include/tilemotion.h): the layout names SetFramesRGB and
stages.rgb_to_rgb32 take, and the descriptor of a numpy array or torch tensor, with step, row and frame taken from its own strides."""
from ._lib import RgbClip, TileMotionError

U8, U16_LOW, U16_HIGH = 0, 1, 2  # TM_SAMPLES_*

# name -> (shape kind, channels in the packed axis, index of R, G, B along the channel axis, bytes per sample; None: 1 or 2, by the array)
LAYOUTS = {
    "rgb24": ("packed", 3, (0, 1, 2), 1), "bgr24": ("packed", 3, (2, 1, 0), 1),
    "rgba": ("packed", 4, (0, 1, 2), 1), "bgra": ("packed", 4, (2, 1, 0), 1), "argb": ("packed", 4, (1, 2, 3), 1), "abgr": ("packed", 4, (3, 2, 1), 1),
    "rgb48": ("packed", 3, (0, 1, 2), 2), "bgr48": ("packed", 3, (2, 1, 0), 2), "rgba64": ("packed", 4, (0, 1, 2), 2), "bgra64": ("packed", 4, (2, 1, 0), 2),
    "rgbp": ("planar", 3, (0, 1, 2), None), "gbrp": ("planar", 3, (2, 0, 1), None),
    "gray": ("gray", 1, (0, 0, 0), None),
}


def _refuse(msg):
    raise TileMotionError(-1, "rgb clip: " + msg)  # TM_E_INVAL, as the library's own checks answer


def describe(frames, layout="rgb24", depth=None, samples=None, fps=1.0):
    """The tm_rgb_clip of `frames`: a numpy array, or a torch tensor on the CPU (lent as host memory) or on a device (device memory).
    [N,H,W,C] for the packed layouts, [N,3,H,W] for rgbp / gbrp, [N,H,W] for gray; 8-bit integers, or 16-bit ones holding words of `depth`
    bits (default 16; samples: U16_LOW, the default, or U16_HIGH).  Views with padding or skipped columns are described as they are;
    a negative stride is TM_E_INVAL."""
    if layout not in LAYOUTS:
        raise ValueError("unknown RGB layout %r (one of %s)" % (layout, " ".join(LAYOUTS)))
    kind, nch, idx, want_item = LAYOUTS[layout]
    torch_like = hasattr(frames, "data_ptr")
    item = frames.element_size() if torch_like else frames.itemsize
    if str(frames.dtype).split(".")[-1] not in ("uint8", "int8", "uint16", "int16") or (want_item is not None and item != want_item):
        raise ValueError("layout %s takes %s integers, not %s" % (layout, {1: "8-bit", 2: "16-bit", None: "8- or 16-bit"}[want_item], frames.dtype))
    shape = tuple(int(n) for n in frames.shape)
    st = [int(s) * item for s in frames.stride()] if torch_like else [int(s) for s in frames.strides]
    if kind == "packed":
        ok = len(shape) == 4 and shape[3] == nch
        (n, h, w), (frame, row, step), chan = (shape[:3], st[:3], st[3]) if ok else ((0, 0, 0), (0, 0, 0), 0)
    elif kind == "planar":
        ok = len(shape) == 4 and shape[1] == 3
        (n, h, w), (frame, row, step), chan = ((shape[0], shape[2], shape[3]), (st[0], st[2], st[3]), st[1]) if ok else ((0, 0, 0), (0, 0, 0), 0)
    else:
        ok = len(shape) == 3
        (n, h, w), (frame, row, step), chan = (shape, st, 0) if ok else ((0, 0, 0), (0, 0, 0), 0)
    if not ok:
        raise ValueError("layout %s takes %s, not an array of shape %s" % (layout, {"packed": "[N,H,W,%d]" % nch, "planar": "[N,3,H,W]", "gray": "[N,H,W]"}[kind], shape))
    if min(frame, row, step, chan) < 0:
        _refuse("a negative stride (%d, %d, %d, %d bytes per frame, row, pixel, channel) is not described" % (frame, row, step, chan))
    if samples is None:
        samples = U8 if item == 1 else U16_LOW
    if (int(samples) == U8) != (item == 1):
        raise ValueError("samples=%r does not fit %d-byte elements" % (samples, item))
    if depth is None:
        depth = 8 * item
    base = frames.data_ptr() if torch_like else frames.ctypes.data
    clip = RgbClip()
    clip.r, clip.g, clip.b = (base + i * chan for i in idx)
    clip.step, clip.row, clip.frame = step, row, frame
    clip.width, clip.height, clip.frames, clip.fps = w, h, n, float(fps)
    clip.samples, clip.depth, clip.memory = int(samples), int(depth), 1 if bool(getattr(frames, "is_cuda", False)) else 0
    return clip
