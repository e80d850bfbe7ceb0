"""Host-side mirror of the reference's TTilingEncoder (tilingencoder.pas:308-568) over the coarse C ABI.

Same names and argument meaning as the Pascal class: LoadDefaultSettings / LoadSettings, the settings properties
(INI key names, tilingencoder.pas:3745-3770), Run(step) with TEncoderStep values, Tiles / TileMap / Palettes views.
Errors that the reference raises as exceptions/assertions surface as TileMotionError.
"""
import ctypes
import os
import enum

import numpy as np

from ._lib import lib, check, TileMotionError, YuvClip, RgbClip, RenderViewDesc, c_void_p, c_int, c_int64, c_double, c_char_p


class TEncoderStep(enum.IntEnum):  # tilingencoder.pas:18
    esAll = -1
    esLoad = 0
    esPredictMotion = 1
    esReduce = 2
    esPreparePalettes = 3
    esDither = 4
    esReconstruct = 5
    esReindex = 6
    esSave = 7


class TPsyVisMode(enum.IntEnum):  # tilingencoder.pas:21
    pvsDCT = 0
    pvsWeightedDCT = 1
    pvsWavelets = 2
    pvsSpeDCT = 3
    pvsWeightedSpeDCT = 4


class TInputYUV(enum.IntEnum):  # tm_set_input_yuv: how a Y4M clip's samples become RGB
    yuvAuto = 0
    yuvBT601Limited = 1
    yuvBT601Full = 2
    yuvTiler = 3
    yuvBT709Limited = 4
    yuvBT709Full = 5


class TChroma(enum.IntEnum):  # TM_CHROMA_*: where the U / V samples sit among the luma samples
    c444 = 0
    c422 = 1
    c420jpeg = 2
    c420mpeg2 = 3
    mono = 4


class TSamples(enum.IntEnum):  # TM_SAMPLES_*: bytes, or little-endian words with the sample in the low (yuv420p10le) or the high bits (P010)
    u8 = 0
    u16Low = 1
    u16High = 2


TILE_HDR = np.dtype([("UseCount", "<u4"), ("TmpIndex", "<i4"), ("MergeIndex", "<i4"), ("PalIdx_Initial", "<i4"), ("Flags", "<u4")])
TILEMAP_ITEM = np.dtype([("TileIdx", "<i4"), ("PalIdx", "<i4"), ("PredictedX", "i1"), ("PredictedY", "i1"), ("PSNR", "<f4"),
                         ("Flags", "<u4")])  # packed, 18 bytes (tilingencoder.pas:178-184)
assert TILE_HDR.itemsize == 20 and TILEMAP_ITEM.itemsize == 18

_ENC_SIGS = {
    "tm_create": (c_void_p, []),
    "tm_destroy": (None, [c_void_p]),
    "tm_set_device": (c_int, [c_void_p, c_int]),
    "tm_set_device_mask": (c_int, [c_void_p, ctypes.c_uint32]),
    "tm_set_devices": (c_int, [c_void_p, ctypes.POINTER(c_int), c_int]),
    "tm_load_default_settings": (c_int, [c_void_p]),
    "tm_load_settings_ini": (c_int, [c_void_p, c_char_p]),
    "tm_set_int": (c_int, [c_void_p, c_char_p, c_int64]),
    "tm_set_float": (c_int, [c_void_p, c_char_p, c_double]),
    "tm_set_bool": (c_int, [c_void_p, c_char_p, c_int]),
    "tm_set_str": (c_int, [c_void_p, c_char_p, c_char_p]),
    "tm_get_int": (c_int, [c_void_p, c_char_p, ctypes.POINTER(c_int64)]),
    "tm_get_float": (c_int, [c_void_p, c_char_p, ctypes.POINTER(c_double)]),
    "tm_set_progress_cb": (c_int, [c_void_p, c_void_p, c_void_p]),
    "tm_set_video": (c_int, [c_void_p, c_int, c_int, c_double, c_int]),
    "tm_push_frame_rgb32": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "tm_set_frames_device": (c_int, [c_void_p, c_void_p]),
    "tm_set_frames_host": (c_int, [c_void_p, c_void_p]),
    "tm_prefetch_frames_host": (c_int, [c_void_p, c_void_p]),
    "tm_set_frames_yuv": (c_int, [c_void_p, ctypes.POINTER(YuvClip)]),
    "tm_set_frames_rgb": (c_int, [c_void_p, ctypes.POINTER(RgbClip)]),
    "tm_open_input": (c_int, [c_void_p]),
    "tm_get_video": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_double), ctypes.POINTER(c_int)]),
    "tm_set_input_yuv": (c_int, [c_void_p, c_int]),
    "tm_run": (c_int, [c_void_p, c_int]),
    "tm_get_counts": (c_int, [c_void_p, ctypes.POINTER(c_int64)] + [ctypes.POINTER(c_int)] * 5),
    "tm_get_tile": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "tm_get_tiles": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "tm_get_tilemap": (c_int, [c_void_p, c_int, c_void_p]),
    "tm_get_tilemaps": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "tm_get_palette": (c_int, [c_void_p, c_int, c_void_p]),
    "tm_get_keyframes": (c_int, [c_void_p, c_void_p]),
    "tm_get_frame_correlations": (c_int, [c_void_p, c_void_p]),
    "tm_get_stage_ms": (c_int, [c_void_p, c_void_p]),
    "tm_get_psnr": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_double)]),
    "tm_save_gtm": (c_int, [c_void_p, c_char_p]),
    "tm_reload_gtm": (c_int, [c_void_p, c_char_p]),
    "tm_generate_y4m": (c_int, [c_void_p, c_char_p, c_int]),
    "tm_generate_pngs": (c_int, [c_void_p, c_int]),
    "tm_render_frames": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int]),
    "tm_render_frames_yuv": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(YuvClip), c_int]),
    "tm_render_frames_scaled": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int]),
    "tm_render_frames_yuv_scaled": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(YuvClip), c_int, c_int]),
    "tm_get_frame_quality": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_double)]),
    "tm_render_view_frames": (c_int, [c_void_p, ctypes.POINTER(RenderViewDesc), c_int, c_int, c_void_p, c_int]),
    "tm_render_tile_pages": (c_int, [c_void_p, ctypes.POINTER(RenderViewDesc), c_int, c_int, c_void_p, c_int]),
    "tm_get_tile_page_count": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "tm_set_query_shard": (c_int, [c_void_p, c_int, c_int]),
    "tm_set_dither_shard": (c_int, [c_void_p, c_int, c_int]),
    "tm_set_collective": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_get_stream": (c_void_p, [c_void_p]),
    "tm_set_collective_mode": (c_int, [c_void_p, c_int]),
    "tm_get_device_array": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "tm_sync_tilemap": (c_int, [c_void_p]),
    "tm_get_knn_kernel_split": (c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int64)]),
    "tm_get_knn_stats": (c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                         ctypes.POINTER(c_int64)]),
}

_INT_KEYS = ["StartFrame", "FrameCount", "MotionPredictRadius", "GlobalTilingTileCount", "PaletteSize", "PaletteCount", "DitheringMode",
             "DitheringYliluoma2MixedColors", "MaxThreadCount"]
_BOOL_KEYS = ["GlobalTilingUseTargetPSNR", "DitheringUseThomasKnoll", "FrameTilingExtendedPaletteUsage"]
_FLOAT_KEYS = ["Scaling", "GlobalTilingTargetPSNR", "GlobalTilingQualityBasedTileCount", "ShotTransMaxSecondsPerKF",
               "ShotTransMinSecondsPerKF", "ShotTransCorrelLoThres"]


def _bind():
    L = lib()
    if not getattr(L, "_enc_bound", False):
        for name, (res, args) in _ENC_SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        L._enc_bound = True
    return L


class TilingEncoder:
    """TTilingEncoder: Create -> settings -> SetVideo/PushFrame (the FFMPEG callback's contract) -> Run(step)."""

    def __init__(self):
        self._L = _bind()
        self._h = self._L.tm_create()
        if not self._h:
            check(-2)
        self._frames_ref = None

    _h = None  # class-level default: close() / __del__ are safe on an instance whose __init__ failed early
    _L = None

    def close(self):
        h = self.__dict__.get("_h")
        if h:
            self._L.tm_destroy(c_void_p(h))
            object.__setattr__(self, "_h", None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass

    # -- settings (properties named like the Pascal ones)
    def __getattr__(self, name):
        if name in _INT_KEYS or name in _BOOL_KEYS:
            v = c_int64()
            check(self._L.tm_get_int(c_void_p(self._h), name.encode(), ctypes.byref(v)))
            return bool(v.value) if name in _BOOL_KEYS else v.value
        if name in _FLOAT_KEYS:
            v = c_double()
            check(self._L.tm_get_float(c_void_p(self._h), name.encode(), ctypes.byref(v)))
            return v.value
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _INT_KEYS:
            check(self._L.tm_set_int(c_void_p(self._h), name.encode(), int(value)))
        elif name in _BOOL_KEYS:
            check(self._L.tm_set_bool(c_void_p(self._h), name.encode(), int(bool(value))))
        elif name in _FLOAT_KEYS:
            check(self._L.tm_set_float(c_void_p(self._h), name.encode(), float(value)))
        elif name in ("InputFileName", "OutputFileName"):
            check(self._L.tm_set_str(c_void_p(self._h), name.encode(), str(value).encode()))
        elif name == "InputYUV":  # not a settings key (the INI text is the reference's): TInputYUV
            check(self._L.tm_set_input_yuv(c_void_p(self._h), int(value)))
            object.__setattr__(self, "_input_yuv", TInputYUV(int(value)))
        else:
            object.__setattr__(self, name, value)

    def LoadDefaultSettings(self):
        check(self._L.tm_load_default_settings(c_void_p(self._h)))

    def LoadSettings(self, path):
        check(self._L.tm_load_settings_ini(c_void_p(self._h), str(path).encode()))

    # -- video
    def SetDeviceMask(self, mask):
        """One process, several devices (tm_set_device_mask): bit d = HIP device d; before SetVideo."""
        check(self._L.tm_set_device_mask(c_void_p(self._h), ctypes.c_uint32(int(mask))))

    def SetDevices(self, devices):
        """The same with a list of devices, which may repeat (several shards on one device)."""
        devs = [int(d) for d in devices]
        arr = (c_int * max(1, len(devs)))(*devs)
        check(self._L.tm_set_devices(c_void_p(self._h), arr, len(devs)))

    def SetVideo(self, width, height, fps, frame_count):
        check(self._L.tm_set_video(c_void_p(self._h), width, height, float(fps), frame_count))

    def OpenInput(self):
        """The probe half of Load (tilingencoder.pas:1764-1820): InputFileName -- a Y4M file, a .gtm stream (played on the device), or a Format pattern naming a PNG sequence --
        with StartFrame, FrameCount and Scaling becomes the video (as SetVideo) and the frame source of the next Run(esLoad).  Run calls
        it by itself when no video has been described yet.  Returns VideoInfo()."""
        check(self._L.tm_open_input(c_void_p(self._h)))
        return self.VideoInfo()

    def VideoInfo(self):
        """width, height, fps, frames as SetVideo / OpenInput left them (tm_get_video)"""
        w, h, n, fps = c_int(), c_int(), c_int(), c_double()
        check(self._L.tm_get_video(c_void_p(self._h), ctypes.byref(w), ctypes.byref(h), ctypes.byref(fps), ctypes.byref(n)))
        return dict(width=w.value, height=h.value, fps=fps.value, frames=n.value)

    @property
    def InputYUV(self):
        return self.__dict__.get("_input_yuv", TInputYUV.yuvAuto)

    def PushFrame(self, index, pixels):
        """pixels: numpy uint32 [height][width] RGB32 (AV_PIX_FMT_RGB32), host memory, read during the call only"""
        a = np.ascontiguousarray(pixels, dtype=np.uint32)
        check(self._L.tm_push_frame_rgb32(c_void_p(self._h), index, a.ctypes.data_as(c_void_p), a.shape[1]))

    def SetFramesDevice(self, frames):
        """frames: torch int32 CUDA tensor [F][H][W] holding RGB32; borrowed until the encoder is closed"""
        self._frames_ref = frames
        check(self._L.tm_set_frames_device(c_void_p(self._h), c_void_p(frames.data_ptr())))

    def SetFramesHost(self, frames):
        """frames: torch int32 CPU tensor (ideally pinned) or numpy uint32 array [F][H][W] holding RGB32; borrowed: Load copies it to
        the device in chunks beside its own kernel"""
        self._frames_ref = frames
        ptr = frames.data_ptr() if hasattr(frames, "data_ptr") else frames.ctypes.data
        check(self._L.tm_set_frames_host(c_void_p(self._h), c_void_p(ptr)))

    def SetFramesYUV(self, y, u, v=None, *, chroma, fps, samples=None, depth=8, full_range=False):
        """A YUV clip lent in memory as a decoder leaves it (tm_set_frames_yuv): what OpenInput does for a file.  y [F][H][W]; u, v [F][ch][cw]
        planes, or v=None and u [F][ch][2 cw] (or [F][ch][cw][2]) holding (U, V) pairs as in NV12 / P010; u=None for TChroma.mono.  torch
        tensors on the device or the CPU (ideally pinned), or numpy arrays, of 8- or 16-bit integers; the last axis must be dense, the row
        and frame strides are taken from the arrays.  samples: TSamples (default: u8 for bytes, u16Low for words), depth: bits per sample;
        full_range feeds TInputYUV.yuvAuto.  Scaling applies as for a file.  The arrays are borrowed (and kept alive here) until the
        Run that loads them has returned.  Returns VideoInfo()."""
        planes = [y, u, v]
        given = [a for a in planes if a is not None]
        on_device = bool(getattr(y, "is_cuda", False))
        item = y.element_size() if hasattr(y, "element_size") else y.itemsize
        if item not in (1, 2):
            raise ValueError("SetFramesYUV: samples must be 8- or 16-bit integers")
        if samples is None:
            samples = TSamples.u8 if item == 1 else TSamples.u16Low
        if (int(samples) == TSamples.u8) != (item == 1):
            raise ValueError("SetFramesYUV: samples=%r does not fit %d-byte elements" % (samples, item))
        clip = YuvClip()
        for name, a in zip("yuv", planes):
            if a is None:
                continue
            torch_like = hasattr(a, "data_ptr")
            if bool(getattr(a, "is_cuda", False)) != on_device or (a.element_size() if torch_like else a.itemsize) != item:
                raise ValueError("SetFramesYUV: the planes must share their memory kind and sample type")
            st = [s * item for s in a.stride()] if torch_like else list(a.strides)
            dense = len(st) >= 3 and st[-1] == item and (len(st) == 3 or (len(st) == 4 and name == "u" and v is None and a.shape[3] == 2 and st[2] == 2 * item))
            if not dense:
                raise ValueError("SetFramesYUV: plane %s must be [F][rows][samples] with a dense last axis" % name)
            setattr(clip, name, a.data_ptr() if torch_like else a.ctypes.data)
            setattr(clip, name + "_row", st[1])
            setattr(clip, name + "_frame", st[0])
        clip.frames, clip.height, clip.width = (int(n) for n in y.shape[:3])
        clip.fps, clip.chroma, clip.samples, clip.depth = float(fps), int(chroma), int(samples), int(depth)
        clip.full_range, clip.memory = int(bool(full_range)), 1 if on_device else 0
        check(self._L.tm_set_frames_yuv(c_void_p(self._h), ctypes.byref(clip)))
        self._yuv_ref = given
        return self.VideoInfo()

    def SetFramesRGB(self, frames, layout="rgb24", *, fps, depth=None, samples=None):
        """An RGB clip lent in memory as its producer leaves it (tm_set_frames_rgb): SetFramesYUV's twin for RGB sources.  frames: a numpy
        array or a torch tensor (CPU tensors are lent as host memory, cuda tensors as device memory); layout: rgb24, bgr24, rgba, bgra, argb,
        abgr ([N,H,W,C] uint8), rgb48, bgr48, rgba64, bgra64 ([N,H,W,C] uint16), rgbp ([N,3,H,W] in R, G, B order), gbrp (the same shape in
        G, B, R order; both uint8, or uint16 with depth), gray ([N,H,W]).  Step, row and frame are the array's own strides, so sliced and
        padded views work; depth: bits per 16-bit sample (default 16; samples: TSamples, default u16Low).  Scaling applies as for a file.
        The array is borrowed (and kept alive here) until the Run that loads it has returned.  Returns VideoInfo()."""
        from . import rgb_in
        clip = rgb_in.describe(frames, layout, depth, samples, fps)
        check(self._L.tm_set_frames_rgb(c_void_p(self._h), ctypes.byref(clip)))
        self._yuv_ref = [frames]
        return self.VideoInfo()

    def SetFramesPNG(self, files, fps):
        """PNG files lent in memory (tm_set_frames_png): files = a list of bytes objects, one per frame -- an archive's members, a capture, a
        socket.  The size is the first file's (Scaling is ignored, as for a PNG sequence); a file of another size fails the Load.  The key
        frames follow the automatic rule.  Decoded where SetPngDecode says.  The files are borrowed (and kept alive here) until the Run that
        loads them has returned.  Returns VideoInfo()."""
        from ._lib import file_list
        files = [bytes(f) for f in files]
        ptrs, sizes, keep = file_list(files)
        check(self._L.tm_set_frames_png(c_void_p(self._h), ptrs, sizes, len(files), float(fps)))
        self._yuv_ref = [ptrs, sizes, keep]
        return self.VideoInfo()

    def SetFramesJPEG(self, files, fps):
        """JPEG files lent in memory (tm_set_frames_jpeg): files = a list of bytes objects, one per frame -- camera stills, the frames of an
        MJPEG capture.  Baseline files only (include/tilemotion.h lists what is read).  The size and the sampling are the first file's
        (Scaling is ignored); a file of another size or sampling fails the Load.  The key frames follow the automatic rule.  Decoded where
        SetJpegDecode says, converted by the InputYUV rule (auto: full-range BT.601).  The files are borrowed (and kept alive here) until
        the Run that loads them has returned.  Returns VideoInfo()."""
        from ._lib import file_list
        files = [bytes(f) for f in files]
        ptrs, sizes, keep = file_list(files)
        check(self._L.tm_set_frames_jpeg(c_void_p(self._h), ptrs, sizes, len(files), float(fps)))
        self._yuv_ref = [ptrs, sizes, keep]
        return self.VideoInfo()

    def SetJpegDecode(self, where="auto"):
        """Where the Load of a JPEG sequence or of lent JPEG files decodes (tm_set_jpeg_decode): "host" (the host form of the decoder on
        the reader threads, the planes uploaded), "device" (the files' bytes uploaded, k_jpeg_decode), "auto" (the device when the first file has
        four restart segments or more, else the host: DESIGN.md section 39.3 has the measurement).  The environment variable TM_JPEG_DECODE=host|device overrides."""
        from ._lib import PNG_DECODE
        if isinstance(where, str):
            if where not in PNG_DECODE:
                raise ValueError("unknown JPEG decode place %r (one of %s)" % (where, " ".join(PNG_DECODE)))
            where = PNG_DECODE[where]
        check(self._L.tm_set_jpeg_decode(c_void_p(self._h), int(where)))

    def JpegDecode(self):
        from ._lib import PNG_DECODE
        v = c_int()
        check(self._L.tm_get_jpeg_decode(c_void_p(self._h), ctypes.byref(v)))
        return {n: k for k, n in PNG_DECODE.items()}[v.value]

    def SetFramesGIF(self, data, fps=None):
        """One animated GIF file lent in memory (tm_set_frames_gif): data = the file's bytes.  The size is the logical screen's, every
        image is a frame (drawn over what the frames before it left, under its disposal rule), the rate is the file's unless fps is given.
        Scaling, StartFrame and FrameCount do not apply; the key frames follow the automatic rule.  Decoded where SetGifDecode says.  The
        file is borrowed (and kept alive here) until the Run that loads it has returned.  Returns VideoInfo()."""
        data = bytes(data)
        check(self._L.tm_set_frames_gif(c_void_p(self._h), data, len(data), float(fps) if fps else 0.0))
        self._yuv_ref = [data]
        return self.VideoInfo()

    def SetGifDecode(self, where="auto"):
        """Where the Load of a GIF file decodes (tm_set_gif_decode): "host" (the LZW on the reader threads, the frames composited on the
        host, the RGB32 clip uploaded), "device" (the file's bytes uploaded, k_gif_lzw and k_gif_compose), "auto" (the device: DESIGN.md
        section 42.3 has the measurement).  The environment variable TM_GIF_DECODE=host|device overrides."""
        from ._lib import PNG_DECODE
        if isinstance(where, str):
            if where not in PNG_DECODE:
                raise ValueError("unknown GIF decode place %r (one of %s)" % (where, " ".join(PNG_DECODE)))
            where = PNG_DECODE[where]
        check(self._L.tm_set_gif_decode(c_void_p(self._h), int(where)))

    def GifDecode(self):
        from ._lib import PNG_DECODE
        v = c_int()
        check(self._L.tm_get_gif_decode(c_void_p(self._h), ctypes.byref(v)))
        return {n: k for k, n in PNG_DECODE.items()}[v.value]

    def SetGifBackground(self, colour=None):
        """The colour a GIF's canvas starts with and disposal 2 restores (tm_set_gif_background): 0x00RRGGBB, or None for the file's (the
        global table's entry at the background index, else black)"""
        check(self._L.tm_set_gif_background(c_void_p(self._h), -1 if colour is None else int(colour)))

    def GifBackground(self):
        v = c_int()
        check(self._L.tm_get_gif_background(c_void_p(self._h), ctypes.byref(v)))
        return None if v.value < 0 else v.value

    def SetPngDecode(self, where="auto"):
        """Where the Load of a PNG sequence or of lent PNG files decodes (tm_set_png_decode): "host" (the reader on host threads, the RGB32
        clip uploaded), "device" (the files' bytes uploaded, inflate and unfilter in kernels), "auto" (the device: DESIGN.md section 35 has the
        measurement).  The environment variable TM_PNG_DECODE=host|device overrides."""
        from ._lib import PNG_DECODE
        if isinstance(where, str):
            if where not in PNG_DECODE:
                raise ValueError("unknown PNG decode place %r (one of %s)" % (where, " ".join(PNG_DECODE)))
            where = PNG_DECODE[where]
        check(self._L.tm_set_png_decode(c_void_p(self._h), int(where)))

    def PngDecode(self):
        from ._lib import PNG_DECODE
        v = c_int()
        check(self._L.tm_get_png_decode(c_void_p(self._h), ctypes.byref(v)))
        return {n: k for k, n in PNG_DECODE.items()}[v.value]

    def InputStats(self):
        """What the last Load of a PNG or JPEG input did (tm_get_input_stats): frames, the files' bytes, the bytes uploaded for them, where they
        were decoded ("host" / "device"), and its milliseconds: reading (host: reading and decoding), the device, the wall clock"""
        from ._lib import PNG_DECODE, InputStatsDesc
        st = InputStatsDesc()
        check(self._L.tm_get_input_stats(c_void_p(self._h), ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in InputStatsDesc._fields_}
        out["where"] = {n: k for k, n in PNG_DECODE.items()}[st.where]
        return out

    def SaveSettings(self, path):
        self._L.tm_save_settings_ini.restype = c_int
        self._L.tm_save_settings_ini.argtypes = [c_void_p, c_char_p]
        check(self._L.tm_save_settings_ini(c_void_p(self._h), str(path).encode()))

    def PrefetchFramesHost(self, frames):
        """queues the upload of the clip the NEXT Load will read (same argument forms as SetFramesHost) beside the current clip's steps;
        call SetFramesHost with the same clip before the Run that is to adopt it.  Borrowed until that Load has returned."""
        self._prefetch_ref = frames
        ptr = frames.data_ptr() if hasattr(frames, "data_ptr") else frames.ctypes.data
        check(self._L.tm_prefetch_frames_host(c_void_p(self._h), c_void_p(ptr)))

    def Run(self, step=TEncoderStep.esAll):
        check(self._L.tm_run(c_void_p(self._h), int(step)))
        if int(step) in (TEncoderStep.esAll, TEncoderStep.esLoad):
            self._yuv_ref = None  # a clip lent with SetFramesYUV / SetFramesRGB is the caller's again once Load has returned

    # -- read-back
    def counts(self):
        t = c_int64()
        v = [c_int() for _ in range(5)]
        check(self._L.tm_get_counts(c_void_p(self._h), ctypes.byref(t), *[ctypes.byref(x) for x in v]))
        return dict(tiles=t.value, frames=v[0].value, palettes=v[1].value, tm_w=v[2].value, tm_h=v[3].value, keyframes=v[4].value)

    def Tiles(self, first=0, count=None):
        n = self.counts()["tiles"]
        count = n - first if count is None else count
        hdr = np.zeros(count, TILE_HDR)
        pal = np.zeros((count, 64), np.uint8)
        rgb = np.zeros((count, 64), np.uint32)
        check(self._L.tm_get_tiles(c_void_p(self._h), first, count, hdr.ctypes.data_as(c_void_p), pal.ctypes.data_as(c_void_p),
                                   rgb.ctypes.data_as(c_void_p)))
        return hdr, pal, rgb

    def TileMap(self, frame):
        c = self.counts()
        items = np.zeros(c["tm_w"] * c["tm_h"], TILEMAP_ITEM)
        check(self._L.tm_get_tilemap(c_void_p(self._h), frame, items.ctypes.data_as(c_void_p)))
        return items

    def TileMaps(self, first=0, count=None, out=None):
        """Frames[first .. first+count-1].TileMap in one read-back; `out` (optional) = a uint8 array / tensor of count*tm_w*tm_h*18 bytes to
        fill (page-locked memory makes the copy one DMA)"""
        c = self.counts()
        count = c["frames"] - first if count is None else count
        per = c["tm_w"] * c["tm_h"]
        if out is None:
            items = np.zeros(count * per, TILEMAP_ITEM)
            check(self._L.tm_get_tilemaps(c_void_p(self._h), first, count, items.ctypes.data_as(c_void_p)))
            return items.reshape(count, per)
        ptr = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
        check(self._L.tm_get_tilemaps(c_void_p(self._h), first, count, c_void_p(ptr)))
        return out

    def Palettes(self):
        c = self.counts()
        out = np.zeros((c["palettes"], self.PaletteSize), np.int32)
        for i in range(c["palettes"]):
            check(self._L.tm_get_palette(c_void_p(self._h), i, out[i].ctypes.data_as(c_void_p)))
        return out

    def KeyFrames(self):
        n = self.counts()["keyframes"]
        out = np.zeros(n, np.int32)
        check(self._L.tm_get_keyframes(c_void_p(self._h), out.ctypes.data_as(c_void_p)))
        return out

    def FrameCorrelations(self):
        out = np.zeros(self.counts()["frames"], np.float32)
        check(self._L.tm_get_frame_correlations(c_void_p(self._h), out.ctypes.data_as(c_void_p)))
        return out

    def PSNR(self):
        """TKeyFrame.LogPSNR (tilingencoder.pas:1006-1028): {"per_keyframe": [...], "global": mean PSNR-HVS by tile}"""
        n = self.counts()["keyframes"]
        per = np.zeros(max(n, 1), np.float64)
        g = c_double()
        check(self._L.tm_get_psnr(c_void_p(self._h), per.ctypes.data_as(c_void_p), ctypes.byref(g)))
        return {"per_keyframe": [float(v) for v in per[:n]], "global": g.value, "unit": "dB, PSNR-HVS by tile (LogPSNR)"}

    def StageMs(self):
        out = np.zeros(8, np.float64)
        check(self._L.tm_get_stage_ms(c_void_p(self._h), out.ctypes.data_as(c_void_p)))
        return out

    # -- multi-GPU plumbing (one process per GPU; collectives stay in the host, see tiler_amd/distributed.py)
    def SetQueryShard(self, first_frame, frame_count):
        check(self._L.tm_set_query_shard(c_void_p(self._h), first_frame, frame_count))

    # -- the native multi-process path: RCCL inside the library (tm_comm_*)
    @staticmethod
    def CommUniqueId():
        """128 bytes from ncclGetUniqueId: one process makes them, every process of the job passes them to CommInit"""
        from ._lib import lib
        buf = (ctypes.c_uint8 * 128)()
        L = lib()
        L.tm_comm_unique_id.restype = c_int
        L.tm_comm_unique_id.argtypes = [c_void_p]
        check(L.tm_comm_unique_id(buf))
        return bytes(buf)

    def CommInit(self, comm_id, rank, world):
        """collective: returns once all `world` processes have called it.  From then on Run(step) shards and merges by itself."""
        assert len(comm_id) == 128
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(comm_id)
        self._L.tm_comm_init.restype = c_int
        self._L.tm_comm_init.argtypes = [c_void_p, c_void_p, c_int, c_int]
        check(self._L.tm_comm_init(c_void_p(self._h), buf, int(rank), int(world)))
        self._native_comm = (int(rank), int(world))

    def CommDestroy(self):
        self._L.tm_comm_destroy.restype = c_int
        self._L.tm_comm_destroy.argtypes = [c_void_p]
        check(self._L.tm_comm_destroy(c_void_p(self._h)))
        self._native_comm = None

    def CollectiveStats(self, reset=False):
        calls = (c_int64 * 4)()
        nbytes = c_int64()
        self._L.tm_get_collective_stats.restype = c_int
        self._L.tm_get_collective_stats.argtypes = [c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int]
        check(self._L.tm_get_collective_stats(c_void_p(self._h), calls, ctypes.byref(nbytes), 1 if reset else 0))
        return dict(all_reduce_sum_i32=calls[0], all_reduce_max_i32=calls[1], all_reduce_sum_i64=calls[2], all_gather=calls[3], bytes=nbytes.value)

    def SetCollective(self, rank, world, coll):
        """one process per GPU: `coll` (tiler_amd.distributed.Collective) runs the collectives the steps ask for; world == 1 clears it"""
        self._coll_ref = coll  # the ctypes callback must outlive the encoder's use of it
        cb = ctypes.cast(coll.callback, c_void_p) if (coll is not None and world > 1) else None
        check(self._L.tm_set_collective(c_void_p(self._h), int(rank), int(world), cb, None))
        # a communicator that can queue its work on the encoder's own stream (RCCL through torch.distributed) is used stream-ordered
        ordered = bool(coll is not None and world > 1 and getattr(coll, "bind_stream", None) and coll.bind_stream(self._L.tm_get_stream(c_void_p(self._h))))
        check(self._L.tm_set_collective_mode(c_void_p(self._h), 1 if ordered else 0))

    def SetDitherShard(self, rank, world):
        """Dither only tiles [T * rank / world, T * (rank + 1) / world); the others stay 0 in DeviceArray(7) for an all-reduce(SUM)"""
        check(self._L.tm_set_dither_shard(c_void_p(self._h), rank, world))

    def DeviceArray(self, which):
        """torch view of an encoder-owned device array, no copy: 0 TileIdx, 1 error, 2 PalIdx (int32); with motion
        prediction 3 IsPredicted (uint8), 4/5 PredictedX/Y (int8), 6 PredictMotion's best error (int32); 7 the dithered
        tiles' palette indices, seen as int32 words (64 bytes = 16 words per tile) so that any backend can add them"""
        import torch
        ptr, cnt = c_void_p(), c_int64()
        check(self._L.tm_get_device_array(c_void_p(self._h), which, ctypes.byref(ptr), ctypes.byref(cnt)))
        typestr = {3: "|u1", 4: "|i1", 5: "|i1"}.get(int(which), "<i4")
        n = cnt.value // 4 if int(which) == 7 else cnt.value

        class _View:
            __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr.value, False), "version": 2}

        return torch.as_tensor(_View(), device="cuda")

    def Save(self, path=None):
        """Save (tilingencoder.pas:2040) -> SaveStream (:5177): writes the .gtm; path defaults to OutputFileName"""
        if path is None:
            self.Run(TEncoderStep.esSave)
        else:
            check(self._L.tm_save_gtm(c_void_p(self._h), os.fsencode(path)))

    def SaveStats(self):
        """What the last Save did (tm_get_save_stats): raw and compressed bytes, key frames, the parser threads and the match finder
        ("host" or "device") that ran, and its milliseconds: the command bytes, the device finder, the parse summed over threads, the wall clock"""
        class _Stats(ctypes.Structure):  # tm_save_stats
            _fields_ = [("raw_bytes", c_int64), ("comp_bytes", c_int64), ("key_frames", ctypes.c_int32), ("threads", ctypes.c_int32),
                        ("finder", ctypes.c_int32), ("reserved", ctypes.c_int32), ("ms_commands", c_double), ("ms_finder", c_double),
                        ("ms_parse", c_double), ("ms_wall", c_double)]
        st = _Stats()
        self._L.tm_get_save_stats.restype = c_int
        self._L.tm_get_save_stats.argtypes = [c_void_p, c_void_p]
        check(self._L.tm_get_save_stats(c_void_p(self._h), ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in _Stats._fields_ if name != "reserved"}
        out["finder"] = "device" if st.finder == 1 else "host"
        return out

    def GenerateY4M(self, path, input=False):
        """GenerateY4M (tilingencoder.pas:2126): the rendered output frames (or the source frames) as a C444 .y4m"""
        check(self._L.tm_generate_y4m(c_void_p(self._h), os.fsencode(path), int(bool(input))))

    def GeneratePNGs(self, input=False):
        """GeneratePNGs (tilingencoder.pas:2075): <OutputFileName>_NNNN.png per frame + the palettes as <OutputFileName>.txt"""
        check(self._L.tm_generate_pngs(c_void_p(self._h), int(bool(input))))

    def GenerateJPEGs(self, input=False):
        """<OutputFileName>_NNNN.jpg per frame (tm_generate_jpegs): the frames GeneratePNGs writes, coded on the device as SetJpegOptions says"""
        check(self._L.tm_generate_jpegs(c_void_p(self._h), int(bool(input))))

    def GenerateMJPEG(self, path, input=False):
        """The same files one behind another in `path` (tm_generate_mjpeg)"""
        check(self._L.tm_generate_mjpeg(c_void_p(self._h), os.fsencode(path), int(bool(input))))

    def GenerateGIF(self, path, input=False):
        """One animated GIF of the frames GeneratePNGs writes (tm_generate_gif), coded on the device as SetGifOptions says: lossless when
        the frames hold at most 256 colours (PaletteCount x PaletteSize <= 256), quantised per frame otherwise"""
        check(self._L.tm_generate_gif(c_void_p(self._h), os.fsencode(path), int(bool(input))))

    def SetGifOptions(self, colours="auto", max_colours=256, diff=True, segment_pixels=4096, loop=0, delay_cs=0):
        """How GenerateGIF writes from now on (tm_set_gif_options): colours "auto" (exact tables where a frame's colours fit, a median cut
        where they do not), "exact" (refuse such a frame) or "quantise" (cut every frame); max_colours 2 .. 256; diff: code only the
        rectangle that changed; segment_pixels: indices per separately coded LZW segment (0: one per image); loop: -1 none, 0 for ever, n
        times; delay_cs: 1/100 s per frame (0: from the rate)"""
        from ._lib import gif_options
        check(self._L.tm_set_gif_options(c_void_p(self._h), ctypes.byref(gif_options(colours, max_colours, diff, segment_pixels, loop, delay_cs))))

    def GifOptions(self):
        from ._lib import GIF_COLOURS, GifOptions
        opt = GifOptions()
        check(self._L.tm_get_gif_options(c_void_p(self._h), ctypes.byref(opt)))
        out = {name: getattr(opt, name) for name, _ in GifOptions._fields_}
        out["colours"] = {v: k for k, v in GIF_COLOURS.items()}[opt.colours]
        out["diff"] = bool(opt.diff)
        return out

    def GenerateWebP(self, path, input=False):
        """One animated lossless WebP of the frames GeneratePNGs writes (tm_generate_webp), coded on the device as SetWebpOptions says:
        exact at any PaletteCount x PaletteSize.  The file carries the clip's rate.  input=True: the Input tab's frames."""
        check(self._L.tm_generate_webp(c_void_p(self._h), os.fsencode(path), int(bool(input))))

    def SetWebpOptions(self, diff=True, palette="auto", lz77=True, segment_pixels=4096, loop=0, duration_ms=0):
        """How GenerateWebP writes from now on (tm_set_webp_options): diff (the changed rectangle, not the whole frame), palette "auto" (a
        colour-indexing transform where a frame holds at most 256 colours, subtract-green otherwise) or "off", lz77, segment_pixels (coded
        pixels per separately parsed segment; 0: one per image), loop (0: for ever), duration_ms (0: from the clip's rate)."""
        from ._lib import webp_options
        check(self._L.tm_set_webp_options(c_void_p(self._h), ctypes.byref(webp_options(diff, palette, lz77, segment_pixels, loop, duration_ms))))

    def WebpOptions(self):
        from ._lib import WEBP_PALETTE, WebpOptions
        opt = WebpOptions()
        check(self._L.tm_get_webp_options(c_void_p(self._h), ctypes.byref(opt)))
        out = {name: getattr(opt, name) for name, _ in WebpOptions._fields_}
        out["palette"] = {v: k for k, v in WEBP_PALETTE.items()}[opt.palette]
        return out

    def WebpExportStats(self):
        """What the last GenerateWebP did (tm_get_webp_export_stats): frames, how many were colour-indexed, segments, tokens, matches, the
        file's bytes and ms per stage."""
        from ._lib import WebpExportStatsDesc
        st = WebpExportStatsDesc()
        check(self._L.tm_get_webp_export_stats(c_void_p(self._h), ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in WebpExportStatsDesc._fields_}

    def GifExportStats(self):
        """What the last GenerateGIF did (tm_get_gif_export_stats): frames, how many were coded exact and quantised, LZW segments, the
        file's bytes, and milliseconds per stage"""
        from ._lib import GifExportStatsDesc
        st = GifExportStatsDesc()
        check(self._L.tm_get_gif_export_stats(c_void_p(self._h), ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in GifExportStatsDesc._fields_}

    def SetJpegOptions(self, quality=90, sampling="420", restart_rows=1):
        """How GenerateJPEGs / GenerateMJPEG write from now on (tm_set_jpeg_options): quality 1 .. 100; sampling "420", "422", "444" or
        "grey"; restart_rows: 0 = no restart markers, n = one every n MCU rows (1, the default, is the file Load decodes on the device)"""
        from ._lib import jpeg_options
        check(self._L.tm_set_jpeg_options(c_void_p(self._h), ctypes.byref(jpeg_options(quality, sampling, restart_rows))))

    def JpegOptions(self):
        from ._lib import JPEG_SAMPLINGS, JpegOptions
        opt = JpegOptions()
        check(self._L.tm_get_jpeg_options(c_void_p(self._h), ctypes.byref(opt)))
        return {"quality": opt.quality, "sampling": {v: k for k, v in JPEG_SAMPLINGS.items()}[opt.sampling], "restart_rows": opt.restart_rows}

    def JpegExportStats(self):
        """What the last GenerateJPEGs / GenerateMJPEG did (tm_get_jpeg_export_stats): frames, the files' bytes, the options that held, and
        its times in ms (ms_device, ms_write, ms_wall, as ExportStats has them)"""
        from ._lib import JPEG_SAMPLINGS, JpegExportStatsDesc
        st = JpegExportStatsDesc()
        check(self._L.tm_get_jpeg_export_stats(c_void_p(self._h), ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in JpegExportStatsDesc._fields_ if name != "reserved"}
        out["sampling"] = {v: k for k, v in JPEG_SAMPLINGS.items()}[st.sampling]
        return out

    def SetPngOptions(self, level=1, filter="auto"):
        """How GeneratePNGs writes from now on (tm_set_png_options): level 0 = stored blocks (the default), level 1 = filtered, matched
        and Huffman-coded on the device; filter: "auto" (none for the output frames, adaptive for the source frames), "none", "adaptive",
        "smaller" (both coded, the shorter file kept)"""
        from ._lib import png_options
        check(self._L.tm_set_png_options(c_void_p(self._h), ctypes.byref(png_options(level, filter))))

    def PngOptions(self):
        from ._lib import PNG_FILTERS, PngOptions
        opt = PngOptions()
        check(self._L.tm_get_png_options(c_void_p(self._h), ctypes.byref(opt)))
        return {"level": opt.level, "filter": {v: k for k, v in PNG_FILTERS.items()}[opt.filter]}

    def ExportStats(self):
        """What the last GeneratePNGs did (tm_get_export_stats): frames, the files' bytes, the level and the filter that held, and its
        milliseconds: on the device (render, coding, read-back), writing the files, the wall clock"""
        from ._lib import PNG_FILTERS, ExportStatsDesc
        st = ExportStatsDesc()
        check(self._L.tm_get_export_stats(c_void_p(self._h), ctypes.byref(st)))
        out = {name: getattr(st, name) for name, _ in ExportStatsDesc._fields_}
        out["filter"] = {v: k for k, v in PNG_FILTERS.items()}[st.filter]
        return out

    def RenderFrames(self, first=0, count=None, input=False, device=True, size=None, filter="lanczos"):
        """The decoded frames [first, first+count) as Render (tilingencoder.pas:3455-3640) draws them with the constructor's defaults -- or
        the source frames (input=True) -- rendered on the device: [count][tm_h*8][tm_w*8] 0x00RRGGBB (the pushed frames' format, alpha 0),
        as a torch int32 CUDA tensor (device=True) or a numpy uint32 array.  size=(width, height): the frames resampled on the device to
        [count][height][width] (tm_render_frames_scaled); filter: "lanczos" or "nearest", as GtmPlayer.SetOutput takes it"""
        c = self.counts()
        count = c["frames"] - first if count is None else count
        if size is not None:
            from ._lib import scale_filter_of
            w, h, flt = int(size[0]), int(size[1]), scale_filter_of(filter)
            shape = (max(count, 0), max(h, 0), max(w, 0))
            if device:
                import torch
                out = torch.empty(shape, dtype=torch.int32, device="cuda")
            else:
                out = np.empty(shape, np.uint32)
            ptr = c_void_p(out.data_ptr()) if device else out.ctypes.data_as(c_void_p)
            check(self._L.tm_render_frames_scaled(c_void_p(self._h), first, count, int(bool(input)), w, h, flt, ptr, int(bool(device))))
            return out
        shape = (max(count, 0), c["tm_h"] * 8, c["tm_w"] * 8)
        if device:
            import torch
            out = torch.empty(shape, dtype=torch.int32, device="cuda")
            check(self._L.tm_render_frames(c_void_p(self._h), first, count, int(bool(input)), c_void_p(out.data_ptr()), 1))
            return out
        out = np.empty(shape, np.uint32)
        check(self._L.tm_render_frames(c_void_p(self._h), first, count, int(bool(input)), out.ctypes.data_as(c_void_p), 0))
        return out

    def _view_pictures(self, fn, view, first, count, device):
        c = self.counts()
        shape = (max(count, 0), c["tm_h"] * 8, c["tm_w"] * 8)
        if device:
            import torch
            out = torch.empty(shape, dtype=torch.int32, device="cuda")
            check(fn(c_void_p(self._h), ctypes.byref(view), first, count, c_void_p(out.data_ptr()), 1))
            return out
        out = np.empty(shape, np.uint32)
        check(fn(c_void_p(self._h), ctypes.byref(view), first, count, out.ctypes.data_as(c_void_p), 0))
        return out

    def RenderView(self, first=0, count=None, page="output", predicted=True, mirrored=True, dithered=True, gamma=None, palette=-1, device=False):
        """Frames [first, first+count) as Render (tilingencoder.pas:3455-3736) draws its Output or Input page (page="output" / "input") under
        its switches (tm_render_view_frames; the rule: include/tilemotion.h): predicted = FRenderPredicted, mirrored = FRenderMirrored,
        dithered = FRenderOutputDithered, gamma = RenderGammaValue with FRenderUseGamma on (None: off), palette = FRenderPaletteIndex
        (-1: every palette).  [count][tm_h*8][tm_w*8] 0x00RRGGBB, a numpy uint32 array or (device=True) a torch int32 CUDA tensor; the
        defaults give RenderFrames' pictures"""
        from ._lib import render_view_desc
        count = self.counts()["frames"] - first if count is None else count
        view = render_view_desc(page, predicted, mirrored, dithered, gamma, palette)
        return self._view_pictures(self._L.tm_render_view_frames, view, first, count, device)

    def TilePageCount(self):
        """pages of the Tiles page: ceil(tiles / (tm_w * tm_h)); the tiles must exist (after Reduce or ReloadGTM)"""
        n = c_int()
        check(self._L.tm_get_tile_page_count(c_void_p(self._h), ctypes.byref(n)))
        return n.value

    def RenderTilePages(self, first=0, count=None, mirrored=True, dithered=True, gamma=None, palette=-1, device=False):
        """Pages [first, first+count) of Render's Tiles page (tm_render_tile_pages): cell (sy, sx) of page p shows tile
        tm_w*sy + sx + tm_w*tm_h*p through palette `palette`, or its own first palette (-1), or as RGB pixels (dithered=False); aqua
        beyond the last tile.  Shapes and switches as RenderView"""
        from ._lib import render_view_desc
        count = self.TilePageCount() - first if count is None else count
        view = render_view_desc("tiles", True, mirrored, dithered, gamma, palette)
        return self._view_pictures(self._L.tm_render_tile_pages, view, first, count, device)

    def RenderFramesYUV(self, first=0, count=None, input=False, layout="nv12", yuv="auto", device=True, out=None, full_range=False, size=None,
                        filter="lanczos"):
        """RenderFrames' frames as YUV planes (tm_render_frames_yuv), converted on the device behind the render: (y, u, v) as
        GtmPlayer.ReadYUV returns them (layout, yuv, out and full_range as there).  size=(width, height): the frames resampled on the device
        before the conversion (tm_render_frames_yuv_scaled; with `out`, its planes must have that size); filter: "lanczos" or "nearest", as GtmPlayer.SetOutput takes it"""
        from . import yuv_out
        c = self.counts()
        count = c["frames"] - first if count is None else count
        if size is not None:
            from ._lib import scale_filter_of
            planes, d = yuv_out.destination(layout, count, int(size[1]), int(size[0]), "cuda" if device else None, out, full_range)
            check(self._L.tm_render_frames_yuv_scaled(c_void_p(self._h), first, count, int(bool(input)), ctypes.byref(d), yuv_out.mode_of(yuv),
                                                      scale_filter_of(filter)))
            return yuv_out.first(planes, max(count, 0))
        planes, d = yuv_out.destination(layout, count, c["tm_h"] * 8, c["tm_w"] * 8, "cuda" if device else None, out, full_range)
        check(self._L.tm_render_frames_yuv(c_void_p(self._h), first, count, int(bool(input)), ctypes.byref(d), yuv_out.mode_of(yuv)))
        return yuv_out.first(planes, max(count, 0))

    def FrameQuality(self, first=0, count=None):
        """Pixel-domain quality of the decoded frames [first, first+count) against the source (tm_get_frame_quality): sse uint64 [count][3]
        (R, G, B), psnr [count] (dB, inf where SSE is 0), ssim_y [count] (SSIM of the .y4m luma, 8x8 windows on a 4-pixel grid), clip_psnr
        (from the summed SSE), clip_ssim_y (mean of the frames')"""
        count = self.counts()["frames"] - first if count is None else count
        sse = np.zeros((max(count, 0), 3), np.uint64)
        psnr = np.zeros(max(count, 0), np.float64)
        ssim = np.zeros(max(count, 0), np.float64)
        cp, cs = c_double(), c_double()
        check(self._L.tm_get_frame_quality(c_void_p(self._h), first, count, sse.ctypes.data_as(c_void_p), psnr.ctypes.data_as(c_void_p),
                                           ssim.ctypes.data_as(c_void_p), ctypes.byref(cp), ctypes.byref(cs)))
        return dict(sse=sse, psnr=psnr, ssim_y=ssim, clip_psnr=cp.value, clip_ssim_y=cs.value)

    def ReloadGTM(self, path):
        """ReloadGTM (tilingencoder.pas:2059) -> LoadStream (:4880): tiles, palettes, tile maps, key frames from a .gtm"""
        check(self._L.tm_reload_gtm(c_void_p(self._h), os.fsencode(path)))

    def SyncTileMap(self):
        check(self._L.tm_sync_tilemap(c_void_p(self._h)))

    def KmeansIters(self):
        """iterations and points of the last PreparePalettes' two clusterings (tm_get_kmeans_iters)"""
        ti, pi = c_int(), c_int()
        tp, pc, px, pci = c_int64(), c_int64(), c_int64(), c_int64()
        self._L.tm_get_kmeans_iters.restype = c_int
        self._L.tm_get_kmeans_iters.argtypes = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                                ctypes.POINTER(c_int64)]
        check(self._L.tm_get_kmeans_iters(c_void_p(self._h), ctypes.byref(ti), ctypes.byref(tp), ctypes.byref(pi), ctypes.byref(pc), ctypes.byref(px), ctypes.byref(pci)))
        return dict(tile_iters=ti.value, tile_points=tp.value, pixel_iters=pi.value, pixel_colours=pc.value, pixel_points=px.value, pixel_colour_iters=pci.value)

    def DitherPairs(self):
        """distinct (palette, colour) pairs the last Dither planned once each; 0 = every pixel planned on its own"""
        self._L.tm_get_dither_pairs.restype = c_int64
        self._L.tm_get_dither_pairs.argtypes = [c_void_p]
        return int(self._L.tm_get_dither_pairs(c_void_p(self._h)))

    def KnnStats(self):
        ms, pairs, launches, kb, rows = c_double(), c_int64(), c_int(), c_int(), c_int64()
        check(self._L.tm_get_knn_stats(c_void_p(self._h), ctypes.byref(ms), ctypes.byref(pairs), ctypes.byref(launches), ctypes.byref(kb),
                                       ctypes.byref(rows)))
        self._L.tm_get_knn_queries.restype = c_int64
        self._L.tm_get_knn_queries.argtypes = [c_void_p]
        sm, sp = (c_double * 3)(), (c_int64 * 3)()
        check(self._L.tm_get_knn_kernel_split(c_void_p(self._h), sm, sp))
        return dict(kernel_ms=ms.value, pairs=pairs.value, launches=launches.value, k_bytes=kb.value, db_rows=rows.value,
                    queries=int(self._L.tm_get_knn_queries(c_void_p(self._h))),
                    seed_ms=sm[0], lists_ms=sm[1], consume_ms=sm[2], seed_pairs=sp[0], consume_pairs=sp[1], consume_mfma=sp[2])
