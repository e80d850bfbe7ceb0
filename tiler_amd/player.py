"""GtmPlayer: the frames of an existing .gtm stream, played on the device frame by frame (tm_player_*, include/tilemotion.h; DESIGN.md
section 19).  No encoder stands behind it: open a file, read frames in order, seek.  Host-only helpers (probe, parse_keyframe) need no GPU.
"""
import ctypes

import numpy as np

from ._lib import lib, check, scale_filter_of, SCALE_FILTERS, c_void_p, c_int, c_int64, c_double, c_char_p
from . import yuv_out


class GtmInfo(ctypes.Structure):  # tm_gtm_info
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("tm_w", ctypes.c_int32), ("tm_h", ctypes.c_int32), ("frames", ctypes.c_int32),
                ("keyframes", ctypes.c_int32), ("tile_count", ctypes.c_int32), ("tileset_tiles", ctypes.c_int32), ("pal_size", ctypes.c_int32),
                ("pal_count", ctypes.c_int32), ("encoder_version", ctypes.c_int32), ("avg_bytes_per_s", ctypes.c_uint32),
                ("kf_max_bytes_per_s", ctypes.c_uint32), ("fps", c_double), ("host_bytes", c_int64), ("device_bytes", c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# one tile-map item as the player's kernel reads it (tm_player_parse_host)
PLAY_RECORD = np.dtype([("a", "<u4"), ("pal", "<u2"), ("flags", "u1"), ("zero", "u1")])
REC_MIRROR_H, REC_MIRROR_V, REC_PREDICTED, REC_INTRA = 1, 2, 4, 8
assert PLAY_RECORD.itemsize == 8

_SIGS = {
    "tm_player_open": (c_int, [c_char_p, c_int, ctypes.POINTER(c_void_p)]),
    "tm_player_info": (c_int, [c_void_p, ctypes.POINTER(GtmInfo)]),
    "tm_player_keyframes": (c_int, [c_void_p, c_void_p]),
    "tm_player_settings_text": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "tm_player_read": (c_int, [c_void_p, c_int, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "tm_player_read_yuv": (c_int, [c_void_p, c_int, ctypes.POINTER(yuv_out.YuvOut), c_int, ctypes.POINTER(c_int)]),
    "tm_player_seek": (c_int, [c_void_p, c_int]),
    "tm_player_set_output": (c_int, [c_void_p, c_int, c_int, c_int]),
    "tm_player_get_output": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_player_tell": (c_int, [c_void_p]),
    "tm_player_timings": (c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_double)]),
    "tm_player_close": (None, [c_void_p]),
    "tm_player_probe_host": (c_int, [c_char_p, ctypes.POINTER(GtmInfo), c_void_p, c_int, ctypes.POINTER(c_int)]),
    "tm_player_parse_host": (c_int, [c_void_p, ctypes.c_size_t, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p,
                                     ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "tm_stage_play_frame": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p]),
}


def _bind():
    L = lib()
    if not getattr(L, "_player_bound", False):
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        L._player_bound = True
    return L


def probe(path):
    """header and index of a .gtm file as tm_player_open checks them, without a device: (info dict, key frames as dicts of frame / raw /
    comp / ms).  The stream's own fields (tm_w, pal_size, ...) are 0 here: they lie in the first key frame's compressed stream."""
    L = _bind()
    info, n = GtmInfo(), c_int()
    check(L.tm_player_probe_host(str(path).encode(), ctypes.byref(info), None, 0, ctypes.byref(n)))
    kf = np.zeros((n.value, 4), np.int32)
    check(L.tm_player_probe_host(str(path).encode(), None, kf.ctypes.data_as(c_void_p), n.value, None))
    k = kf.view(np.uint32)
    return info.as_dict(), [dict(frame=int(k[i, 0]), raw=int(k[i, 1]), comp=int(k[i, 2]), ms=int(k[i, 3])) for i in range(n.value)]


def parse_keyframe(raw, tm_w, tm_h, tile_count=0, sized=True):
    """one key frame's decoded command bytes -> (records [frames][tm_h*tm_w] PLAY_RECORD, intra [n][64] uint8, intra_first [frames+1]);
    tm_w / tm_h / tile_count as the first key frame's SetDimensions gave them.  sized=False: only walk the bytes, with the stream's own
    SetDimensions when tm_w and tm_h are 0 -> (frames, intra tiles)"""
    if sized and (tm_w <= 0 or tm_h <= 0):
        raise ValueError("parse_keyframe: pass tm_w and tm_h (the record array is sized by them)")
    L = _bind()
    buf = np.frombuffer(bytes(raw), np.uint8)
    nf, ni = c_int(), c_int64()
    check(L.tm_player_parse_host(buf.ctypes.data_as(c_void_p), buf.size, tm_w, tm_h, tile_count, None, 0, None, 0, None, ctypes.byref(nf), ctypes.byref(ni)))
    if not sized:
        return nf.value, ni.value
    intra = np.zeros((ni.value, 64), np.uint8)
    first = np.zeros(nf.value + 1, np.int64)
    per = tm_w * tm_h
    recs = np.zeros((nf.value, per), PLAY_RECORD)
    check(L.tm_player_parse_host(buf.ctypes.data_as(c_void_p), buf.size, tm_w, tm_h, tile_count, recs.ctypes.data_as(c_void_p), nf.value,
                                 intra.ctypes.data_as(c_void_p), ni.value, first.ctypes.data_as(c_void_p), ctypes.byref(nf), ctypes.byref(ni)))
    return recs, intra, first


def play_frame(records, intra, tiles, palettes, prev, tm_w, tm_h, stream=None):
    """tm_stage_play_frame on torch CUDA tensors: records uint8 [tm_h*tm_w*8] (PLAY_RECORD bytes), intra uint8 [n][64], tiles uint8 [t][64],
    palettes int32 [p][pal_size], prev int32 [tm_h*8][tm_w*8] or None -> int32 [tm_h*8][tm_w*8] 0x00RRGGBB"""
    import torch
    L = _bind()
    out = torch.empty((tm_h * 8, tm_w * 8), dtype=torch.int32, device=records.device)
    ptr = lambda t: c_void_p(t.data_ptr() if t is not None and t.numel() else 0)  # noqa: E731
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(L.tm_stage_play_frame(ptr(records), ptr(intra), intra.shape[0], ptr(tiles), ptr(palettes), ptr(prev), ptr(out), tm_w, tm_h,
                                palettes.shape[1] if palettes.dim() == 2 else 0, tiles.shape[0], palettes.shape[0], c_void_p(s)))
    return out


class GtmPlayer:
    """with GtmPlayer(path) as p: p.info(); p.Read(10); p.Seek(120); p.Read(1, device=False)"""

    def __init__(self, path, device=0):
        self._L = _bind()
        h = c_void_p()
        check(self._L.tm_player_open(str(path).encode(), int(device), ctypes.byref(h)))
        self._h = h.value
        self._device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.tm_player_close(c_void_p(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def info(self):
        i = GtmInfo()
        check(self._L.tm_player_info(c_void_p(self._h), ctypes.byref(i)))
        return i.as_dict()

    def KeyFrames(self):
        out = np.zeros(self.info()["keyframes"], np.int32)
        check(self._L.tm_player_keyframes(c_void_p(self._h), out.ctypes.data_as(c_void_p)))
        return out

    def SettingsText(self):
        n = ctypes.c_size_t()
        check(self._L.tm_player_settings_text(c_void_p(self._h), None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        check(self._L.tm_player_settings_text(c_void_p(self._h), buf, n.value, ctypes.byref(n)))
        return buf.raw[:n.value].decode("latin-1")

    def Tell(self):
        return self._L.tm_player_tell(c_void_p(self._h))

    def Seek(self, frame):
        check(self._L.tm_player_seek(c_void_p(self._h), int(frame)))

    def SetOutput(self, width, height, filter="lanczos"):
        """the size Read and ReadYUV deliver at from now on (tm_player_set_output): scaled on the device behind the frames; filter "lanczos"
        or "nearest".  (0, 0): the stream's own size again.  A refused size leaves the setting as it was"""
        check(self._L.tm_player_set_output(c_void_p(self._h), int(width), int(height), scale_filter_of(filter)))

    def Output(self):
        """(width, height, filter) as SetOutput left them; (0, 0, "lanczos"): the stream's own size"""
        w, h, f = c_int(), c_int(), c_int()
        check(self._L.tm_player_get_output(c_void_p(self._h), ctypes.byref(w), ctypes.byref(h), ctypes.byref(f)))
        return w.value, h.value, {v: k for k, v in SCALE_FILTERS.items()}[f.value]

    def _size(self, i):
        """(height, width) of a delivered frame"""
        w, h, _ = self.Output()
        return (h, w) if w > 0 else (i["tm_h"] * 8, i["tm_w"] * 8)

    def Read(self, count=None, device=True, out=None):
        """the next `count` frames (None: to the end) as [got][height][width] 0x00RRGGBB -- tm_h*8 x tm_w*8, or the size SetOutput set: a
        torch int32 CUDA tensor (device=True) or a numpy uint32 array; fewer than count only at the end of the stream.  out: a tensor /
        array of at least that size to fill instead"""
        i = self.info()
        count = i["frames"] - self.Tell() if count is None else int(count)
        shape = (max(count, 0),) + self._size(i)
        got = c_int()
        if device:
            import torch
            if out is None:
                out = torch.empty(shape, dtype=torch.int32, device="cuda:%d" % self._device)
            check(self._L.tm_player_read(c_void_p(self._h), count, c_void_p(out.data_ptr()), 1, ctypes.byref(got)))
        else:
            if out is None:
                out = np.empty(shape, np.uint32)
            check(self._L.tm_player_read(c_void_p(self._h), count, out.ctypes.data_as(c_void_p), 0, ctypes.byref(got)))
        return out[:got.value]

    def ReadYUV(self, count=None, layout="nv12", yuv="auto", device=True, out=None, full_range=False):
        """the next `count` frames (None: to the end) as YUV planes (tm_player_read_yuv), converted on the device: (y, u, v) of [got][rows]
        [samples], torch tensors on the player's device (uint8, or int16 holding the words) or numpy arrays (uint8 / uint16); u is None for
        "mono", v is None where u holds (U, V) pairs ([got][ch][2 cw]).  layout: 444 422 420 420mpeg2 mono nv12 p010, or (chroma, samples,
        depth, pairs); yuv: auto bt601-limited bt601-full tiler bt709-limited bt709-full (auto: bt601-full when full_range, else
        bt601-limited).  out: (y, u, v) of at least that size to fill instead (strides are taken from the arrays)"""
        i = self.info()
        count = i["frames"] - self.Tell() if count is None else int(count)
        height, width = self._size(i)
        planes, d = yuv_out.destination(layout, count, height, width, "cuda:%d" % self._device if device else None, out, full_range)
        got = c_int()
        check(self._L.tm_player_read_yuv(c_void_p(self._h), count, ctypes.byref(d), yuv_out.mode_of(yuv), ctypes.byref(got)))
        return yuv_out.first(planes, got.value)

    def Timings(self):
        ms = (c_double * 5)()
        first = c_double()
        check(self._L.tm_player_timings(c_void_p(self._h), ms, ctypes.byref(first)))
        return dict(decode_ms=ms[0], parse_ms=ms[1], upload_ms=ms[2], worker_wait_ms=ms[3], launch_ms=ms[4], first_frame_ms=first.value)
