"""ctypes binding of libtilemotion.so (include/tilemotion.h).  Fails loudly when the library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    variant = os.environ.get("TM_LIB_VARIANT")  # development builds of tools/build_variant.sh
    if variant:
        return os.path.join(_HERE, "lib", "variants", "libtilemotion_%s.so" % variant)
    return os.path.join(_HERE, "lib", "libtilemotion.so")


class TileMotionError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libtilemotion error {code}: {msg}")
        self.code = code


_lib = None

c_void_p, c_int, c_int64, c_double, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_char_p


class YuvClip(ctypes.Structure):  # tm_yuv_clip: a YUV clip lent in memory (tm_set_frames_yuv); tm_yuv_out has the same fields (yuv_out.py)
    _fields_ = [("y", c_void_p), ("u", c_void_p), ("v", c_void_p),
                ("y_row", c_int64), ("y_frame", c_int64), ("u_row", c_int64), ("u_frame", c_int64), ("v_row", c_int64), ("v_frame", c_int64),
                ("width", c_int), ("height", c_int), ("frames", c_int), ("fps", c_double),
                ("chroma", c_int), ("samples", c_int), ("depth", c_int), ("full_range", c_int), ("memory", c_int)]


class RgbClip(ctypes.Structure):  # tm_rgb_clip: an RGB clip lent in memory (tm_set_frames_rgb; rgb_in.py describes arrays with it), 88 bytes
    _fields_ = [("r", c_void_p), ("g", c_void_p), ("b", c_void_p), ("step", c_int64), ("row", c_int64), ("frame", c_int64),
                ("width", c_int), ("height", c_int), ("frames", c_int), ("fps", c_double), ("samples", c_int), ("depth", c_int), ("memory", c_int)]


class RenderViewDesc(ctypes.Structure):  # tm_render_view: Render's switches (32 bytes)
    _fields_ = [("page", ctypes.c_int32), ("predicted", ctypes.c_int32), ("mirrored", ctypes.c_int32), ("dithered", ctypes.c_int32),
                ("use_gamma", ctypes.c_int32), ("palette_index", ctypes.c_int32), ("gamma", c_double)]


class PngOptions(ctypes.Structure):  # tm_png_options
    _fields_ = [("level", ctypes.c_int32), ("filter", ctypes.c_int32)]


class ExportStatsDesc(ctypes.Structure):  # tm_export_stats
    _fields_ = [("frames", c_int64), ("file_bytes", c_int64), ("level", ctypes.c_int32), ("filter", ctypes.c_int32),
                ("ms_device", c_double), ("ms_write", c_double), ("ms_wall", c_double)]


class InflateSpan(ctypes.Structure):  # tm_inflate_span: bytes [off, off + len) of a blob
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class InflateStream(ctypes.Structure):  # tm_inflate_stream: where a stream's output goes and which spans are its input
    _fields_ = [("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint32), ("first_span", ctypes.c_uint32), ("span_count", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class InflateStatus(ctypes.Structure):  # tm_inflate_status
    _fields_ = [("code", ctypes.c_int32), ("in_pos", ctypes.c_uint32), ("out_n", ctypes.c_uint32)]


class InputStatsDesc(ctypes.Structure):  # tm_input_stats
    _fields_ = [("frames", c_int64), ("file_bytes", c_int64), ("bytes_uploaded", c_int64), ("where", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("ms_read", c_double), ("ms_device", c_double), ("ms_wall", c_double)]


class JpegInfoDesc(ctypes.Structure):  # tm_jpeg_info
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "components", "h_samp", "v_samp", "restart_interval", "segments", "sof", "chroma", "status")]


class JpegOptions(ctypes.Structure):  # tm_jpeg_options
    _fields_ = [("quality", ctypes.c_int32), ("sampling", ctypes.c_int32), ("restart_rows", ctypes.c_int32)]


class JpegExportStatsDesc(ctypes.Structure):  # tm_jpeg_export_stats
    _fields_ = [("frames", c_int64), ("file_bytes", c_int64), ("quality", ctypes.c_int32), ("sampling", ctypes.c_int32), ("restart_rows", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("ms_device", c_double), ("ms_write", c_double), ("ms_wall", c_double)]


class GifInfoDesc(ctypes.Structure):  # tm_gif_info
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "frames", "uniform_delay", "loop_count", "global_table_size", "background_index", "version")] + [
        ("background", ctypes.c_uint32), ("reserved", ctypes.c_int32), ("fps", c_double)]


class GifFrameDesc(ctypes.Structure):  # tm_gif_frame
    _fields_ = [(n, ctypes.c_int32) for n in ("left", "top", "width", "height", "delay", "disposal", "transparent", "interlaced", "table_size", "local_table",
                                              "min_code_size", "reserved")] + [("data_off", ctypes.c_uint64), ("data_bytes", ctypes.c_uint64)]


class GifStreamDesc(ctypes.Structure):  # tm_gif_stream
    _fields_ = [("src_off", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("src_bytes", ctypes.c_uint32), ("npix", ctypes.c_uint32), ("min_code_size", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class GifStatusDesc(ctypes.Structure):  # tm_gif_status
    _fields_ = [("code", ctypes.c_int32), ("in_pos", ctypes.c_uint32), ("out_n", ctypes.c_uint32)]


class GifOptions(ctypes.Structure):  # tm_gif_options
    _fields_ = [(n, ctypes.c_int32) for n in ("colours", "max_colours", "diff", "segment_pixels", "loop", "delay_cs")]


class GifExportStatsDesc(ctypes.Structure):  # tm_gif_export_stats
    _fields_ = [(n, c_int64) for n in ("frames", "frames_exact", "frames_quantised", "segments", "file_bytes")] + [
        (n, c_double) for n in ("ms_colours", "ms_tables", "ms_lzw", "ms_emit", "ms_device", "ms_write", "ms_wall")]


GIF_COLOURS = {"auto": 0, "exact": 1, "quantise": 2}  # TM_GIF_COLOURS_*


def gif_options(colours="auto", max_colours=256, diff=True, segment_pixels=4096, loop=0, delay_cs=0):
    """tm_gif_options from the keywords SetGifOptions / stages.gif_encode take"""
    if isinstance(colours, str):
        if colours not in GIF_COLOURS:
            raise ValueError("unknown GIF colours %r (one of %s)" % (colours, " ".join(GIF_COLOURS)))
        colours = GIF_COLOURS[colours]
    return GifOptions(int(colours), int(max_colours), int(diff), int(segment_pixels), int(loop), int(delay_cs))


class WebpOptions(ctypes.Structure):  # tm_webp_options
    _fields_ = [(n, ctypes.c_int32) for n in ("diff", "palette", "lz77", "segment_pixels", "loop", "duration_ms")]


class WebpExportStatsDesc(ctypes.Structure):  # tm_webp_export_stats
    _fields_ = [(n, c_int64) for n in ("frames", "frames_indexed", "segments", "tokens", "matches", "file_bytes")] + [
        (n, c_double) for n in ("ms_colours", "ms_match", "ms_parse", "ms_codes", "ms_emit", "ms_device", "ms_write", "ms_wall")]


WEBP_PALETTE = {"auto": 0, "off": 1}  # TM_WEBP_PALETTE_*


def webp_options(diff=True, palette="auto", lz77=True, segment_pixels=4096, loop=0, duration_ms=0):
    """tm_webp_options from the keywords SetWebpOptions / stages.webp_encode take"""
    if isinstance(palette, str):
        if palette not in WEBP_PALETTE:
            raise ValueError("unknown WebP palette %r (one of %s)" % (palette, " ".join(WEBP_PALETTE)))
        palette = WEBP_PALETTE[palette]
    return WebpOptions(int(diff), int(palette), int(lz77), int(segment_pixels), int(loop), int(duration_ms))


PNG_DECODE = {"auto": 0, "host": 1, "device": 2}  # TM_PNG_DECODE_*

RENDER_PAGES = {"input": 0, "output": 1, "tiles": 2}  # TM_RENDER_PAGE_*


def render_view_desc(page="output", predicted=True, mirrored=True, dithered=True, gamma=None, palette=-1):
    """tm_render_view from the keywords RenderView / stages.render_view take; gamma=None: off (the value stays the constructor's 0.6)"""
    if isinstance(page, str):
        if page not in RENDER_PAGES:
            raise ValueError("unknown render page %r (one of %s)" % (page, " ".join(RENDER_PAGES)))
        page = RENDER_PAGES[page]
    return RenderViewDesc(int(page), int(bool(predicted)), int(bool(mirrored)), int(bool(dithered)), int(gamma is not None), int(palette),
                          0.6 if gamma is None else float(gamma))


# name -> (restype, argtypes); mirrors include/tilemotion.h one to one
SIGNATURES = {
    "tm_last_error": (c_char_p, []),
    "tm_device_count": (c_int, []),
    "tm_version": (c_char_p, []),
    "tm_probe_mfma_i8": (c_int, [c_double, ctypes.POINTER(c_double)]),
    "tm_probe_hbm_triad": (c_int, [c_int64, ctypes.POINTER(c_double)]),
    "tm_probe_group_allreduce": (c_int, [ctypes.POINTER(c_int), c_int, c_int64, c_int, ctypes.POINTER(c_double)]),
    "tm_set_device_mask": (c_int, [c_void_p, ctypes.c_uint32]),
    "tm_set_devices": (c_int, [c_void_p, ctypes.POINTER(c_int), c_int]),
    "tm_stage_load": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tm_pearson_finish_host": (c_int, [c_void_p, c_int, c_void_p]),
    "tm_stage_pearson": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_features_rgb": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_features_rgb_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tm_stage_features_pal": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_features_cluster": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "tm_stage_window_dcts": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_motion_search": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tm_stage_motion_search_fb": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tm_stage_knn_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "tm_stage_epu_rerank": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "tm_stage_knn": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "tm_knn_index_create": (c_void_p, [c_void_p, c_int64, c_void_p]),
    "tm_knn_index_destroy": (None, [c_void_p]),
    "tm_knn_index_search": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "tm_knn_index_last_stats": (c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "tm_knn_index_last_list_counts": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "tm_knn_index_last_chunk_counts": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "tm_knn_index_last_survivor_counts": (c_int, [c_void_p] + [ctypes.POINTER(c_int64)] * 6),
    "tm_knn_index_row_order": (c_int, [c_void_p, c_void_p, c_void_p]),
    "tm_stage_knn_tile_order": (c_int, [c_void_p, c_int64, c_void_p]),
    "tm_stage_curve_keys": (c_int, [c_void_p, c_int64, ctypes.POINTER(c_int), c_int, c_void_p, c_void_p]),
    "tm_knn_last_plan": (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "tm_stage_dedup": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "tm_stage_dedup_by_index": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "tm_host_waits": (ctypes.c_longlong, []),
    "tm_stage_kmeans": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int),
                                ctypes.POINTER(c_int), c_void_p]),
    "tm_stage_kmeans_seeded": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int),
                                       ctypes.POINTER(c_int), c_void_p]),
    "tm_stage_quantize_palettes": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_palettize": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "tm_kmeans_last_resident": (c_int, []),
    "tm_kmeans_last_first_look": (None, [ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "tm_stage_pp_seeds": (c_int, [c_void_p, c_void_p, c_int64, c_int, ctypes.POINTER(c_int64), ctypes.POINTER(c_int), c_void_p]),
    "tm_stage_kmodes": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(c_int), c_void_p]),
    "tm_stage_dither": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_render": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int, c_int,
                                c_void_p, c_void_p]),
    "tm_stage_frame_quality": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "tm_render_view_default": (c_int, [ctypes.POINTER(RenderViewDesc)]),
    "tm_probe_render_view_host": (c_int, [ctypes.POINTER(RenderViewDesc), c_int]),
    "tm_render_gamma_lut_host": (c_int, [c_double, c_void_p]),
    "tm_stage_render_view": (c_int, [ctypes.POINTER(RenderViewDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_yuv_to_rgb32": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "tm_stage_yuv_to_rgb32_fmt": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                          c_void_p]),
    "tm_stage_rgb32_to_yuv_fmt": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int,
                                          c_void_p]),
    "tm_probe_yuv_out_host": (c_int, [ctypes.POINTER(YuvClip), c_int, c_int, c_int]),
    "tm_yuv_out_matrix_host": (c_int, [c_int, ctypes.POINTER(ctypes.c_int32)]),
    "tm_rgb32_to_yuv_host": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tm_probe_yuv_clip_host": (c_int, [ctypes.POINTER(YuvClip), c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_probe_rgb_clip_host": (c_int, [ctypes.POINTER(RgbClip), c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_rgb_to_rgb32_host": (c_int, [ctypes.POINTER(RgbClip), c_int, c_int, c_int, c_int, c_void_p]),
    "tm_stage_rgb_to_rgb32": (c_int, [ctypes.POINTER(RgbClip), c_int, c_int, c_void_p, c_void_p]),
    "tm_probe_input_host": (c_int, [c_char_p, c_int, c_int, c_double] + [ctypes.POINTER(c_int)] * 5 + [ctypes.POINTER(c_double)] + [ctypes.POINTER(c_int)] * 2),
    "tm_read_png_host": (c_int, [c_char_p, c_void_p, c_int64, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_inflate_host": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "tm_resample_taps_host": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tm_probe_scale_host": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "tm_scale_rgb32_host": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_int]),
    "tm_lz_matches_host": (c_int, [c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "tm_lz_compress_from_matches_host": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "tm_stage_lz_matches": (c_int, [c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                    c_void_p]),
    "tm_stage_lz_compress": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "tm_stage_scale_rgb32": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "tm_set_png_options": (c_int, [c_void_p, ctypes.POINTER(PngOptions)]),
    "tm_get_png_options": (c_int, [c_void_p, ctypes.POINTER(PngOptions)]),
    "tm_get_export_stats": (c_int, [c_void_p, ctypes.POINTER(ExportStatsDesc)]),
    "tm_png_bound_host": (c_int, [c_int, c_int, ctypes.POINTER(c_int64)]),
    "tm_stage_png_encode": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, ctypes.POINTER(PngOptions), c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "tm_png_encode_host": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, ctypes.POINTER(PngOptions), c_void_p, c_int64, ctypes.POINTER(c_int64)]),
    "tm_stage_zlib_compress": (c_int, [c_void_p, c_int64, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "tm_zlib_compress_host": (c_int, [c_void_p, c_int64, c_void_p, c_int64, ctypes.POINTER(c_int64)]),
    "tm_png_filter_rows_host": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "tm_deflate_code_lengths_host": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "tm_inflate_streams_host": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tm_stage_inflate": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p]),
    "tm_png_decode_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "tm_stage_png_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "tm_set_png_decode": (c_int, [c_void_p, c_int]),
    "tm_get_png_decode": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "tm_set_frames_png": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double]),
    "tm_probe_png_clip_host": (c_int, [c_void_p, c_void_p, c_int, c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_get_input_stats": (c_int, [c_void_p, ctypes.POINTER(InputStatsDesc)]),
    "tm_probe_jpeg_host": (c_int, [c_void_p, ctypes.c_size_t, ctypes.POINTER(JpegInfoDesc)]),
    "tm_jpeg_decode_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tm_stage_jpeg_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tm_set_jpeg_decode": (c_int, [c_void_p, c_int]),
    "tm_get_jpeg_decode": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "tm_set_frames_jpeg": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_double]),
    "tm_probe_jpeg_clip_host": (c_int, [c_void_p, c_void_p, c_int, c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "tm_probe_gif_host": (c_int, [c_void_p, ctypes.c_size_t, ctypes.POINTER(GifInfoDesc)]),
    "tm_gif_frames_host": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_int, ctypes.POINTER(c_int)]),
    "tm_gif_lzw_streams_host": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tm_stage_gif_lzw": (c_int, [c_void_p, ctypes.c_size_t, c_void_p, c_int, c_void_p, ctypes.c_size_t, c_void_p, c_void_p]),
    "tm_gif_decode_host": (c_int, [c_void_p, ctypes.c_size_t, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p]),
    "tm_stage_gif_decode": (c_int, [c_void_p, ctypes.c_size_t, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p]),
    "tm_set_gif_decode": (c_int, [c_void_p, c_int]),
    "tm_get_gif_decode": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "tm_set_gif_background": (c_int, [c_void_p, c_int]),
    "tm_get_gif_background": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "tm_set_frames_gif": (c_int, [c_void_p, c_void_p, ctypes.c_size_t, c_double]),
    "tm_probe_gif_clip_host": (c_int, [c_void_p, ctypes.c_size_t, c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_double)]),
    "tm_generate_jpegs": (c_int, [c_void_p, c_int]),
    "tm_generate_mjpeg": (c_int, [c_void_p, c_char_p, c_int]),
    "tm_set_jpeg_options": (c_int, [c_void_p, ctypes.POINTER(JpegOptions)]),
    "tm_get_jpeg_options": (c_int, [c_void_p, ctypes.POINTER(JpegOptions)]),
    "tm_get_jpeg_export_stats": (c_int, [c_void_p, ctypes.POINTER(JpegExportStatsDesc)]),
    "tm_jpeg_bound_host": (c_int, [c_int, c_int, ctypes.POINTER(JpegOptions), ctypes.POINTER(c_int64)]),
    "tm_jpeg_quant_tables_host": (c_int, [c_int, c_void_p, c_void_p]),
    "tm_stage_jpeg_encode": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, ctypes.POINTER(JpegOptions), c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "tm_set_gif_options": (c_int, [c_void_p, ctypes.POINTER(GifOptions)]),
    "tm_get_gif_options": (c_int, [c_void_p, ctypes.POINTER(GifOptions)]),
    "tm_generate_gif": (c_int, [c_void_p, c_char_p, c_int]),
    "tm_get_gif_export_stats": (c_int, [c_void_p, ctypes.POINTER(GifExportStatsDesc)]),
    "tm_gif_bound_host": (c_int, [c_int, c_int, c_int, ctypes.POINTER(GifOptions), ctypes.POINTER(c_int64)]),
    "tm_stage_gif_encode": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, ctypes.POINTER(GifOptions), c_int, c_void_p, c_int64,
                                    ctypes.POINTER(c_int64), ctypes.POINTER(GifExportStatsDesc), c_void_p]),
    "tm_gif_encode_host": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, ctypes.POINTER(GifOptions), c_void_p, c_int64, ctypes.POINTER(c_int64),
                                   c_void_p, ctypes.POINTER(GifExportStatsDesc)]),
    "tm_set_webp_options": (c_int, [c_void_p, ctypes.POINTER(WebpOptions)]),
    "tm_get_webp_options": (c_int, [c_void_p, ctypes.POINTER(WebpOptions)]),
    "tm_generate_webp": (c_int, [c_void_p, c_char_p, c_int]),
    "tm_get_webp_export_stats": (c_int, [c_void_p, ctypes.POINTER(WebpExportStatsDesc)]),
    "tm_webp_bound_host": (c_int, [c_int, c_int, c_int, ctypes.POINTER(WebpOptions), ctypes.POINTER(c_int64)]),
    "tm_stage_webp_encode": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, ctypes.POINTER(WebpOptions), c_int, c_void_p, c_int64,
                                     ctypes.POINTER(c_int64), ctypes.POINTER(WebpExportStatsDesc), c_void_p]),
    "tm_webp_encode_host": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_double, ctypes.POINTER(WebpOptions), c_void_p, c_int64, ctypes.POINTER(c_int64),
                                    c_void_p, ctypes.POINTER(WebpExportStatsDesc)]),
    "tm_stage_gif_lzw_pack": (c_int, [c_void_p, ctypes.c_uint32, c_int, c_int, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "tm_gif_lzw_pack_host": (c_int, [c_void_p, ctypes.c_uint32, c_int, c_int, c_void_p, c_int64, ctypes.POINTER(c_int64)]),
    "tm_stage_gif_palettise": (c_int, [c_void_p, c_int64, c_int, c_int, ctypes.POINTER(GifOptions), c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p,
                                       c_void_p]),
    "tm_gif_palettise_host": (c_int, [c_void_p, c_int64, c_int, c_int, ctypes.POINTER(GifOptions), c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p]),
    "tm_jpeg_encode_host": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, ctypes.POINTER(JpegOptions), c_void_p, c_int64, ctypes.POINTER(c_int64)]),
}


PNG_FILTERS = {"auto": 0, "none": 1, "adaptive": 2, "smaller": 3}  # TM_PNG_FILTER_*


def png_options(level=1, filter="auto"):
    """tm_png_options from the keywords SetPngOptions / stages.png_encode take"""
    if isinstance(filter, str):
        if filter not in PNG_FILTERS:
            raise ValueError("unknown PNG filter strategy %r (one of %s)" % (filter, " ".join(PNG_FILTERS)))
        filter = PNG_FILTERS[filter]
    return PngOptions(int(level), int(filter))


JPEG_SAMPLINGS = {"420": 0, "422": 1, "444": 2, "grey": 3}  # TM_JPEG_*


def jpeg_options(quality=90, sampling="420", restart_rows=1):
    """tm_jpeg_options from the keywords SetJpegOptions / stages.jpeg_encode take"""
    if isinstance(sampling, str):
        if sampling not in JPEG_SAMPLINGS:
            raise ValueError("unknown JPEG sampling %r (one of %s)" % (sampling, " ".join(JPEG_SAMPLINGS)))
        sampling = JPEG_SAMPLINGS[sampling]
    return JpegOptions(int(quality), int(sampling), int(restart_rows))


def inflate_batch(streams, caps=None, dst_offs=None, src_offs=None):
    """The arguments tm_inflate_streams_host / tm_stage_inflate take for a batch.  streams: a list whose items are bytes (one span) or a
    list of bytes (the spans of one stream, in order; empty ones allowed); caps: the most each may write; dst_offs: where each one's
    output starts (default: one behind the other, 16 bytes apart at least); src_offs: where each span starts in the blob (default: one
    behind the other) -> (blob uint8 array, spans, streams, dst_bytes), the last two ctypes arrays"""
    import numpy as np
    lists = [[s] if isinstance(s, (bytes, bytearray)) else list(s) for s in streams]
    flat = [bytes(p) for l in lists for p in l]
    if src_offs is None:
        src_offs, at = [], 0
        for p in flat:
            src_offs.append(at)
            at += len(p)
    blob = np.zeros(max([o + len(p) for o, p in zip(src_offs, flat)] + [1]), np.uint8)
    spans = (InflateSpan * max(len(flat), 1))()
    for j, (o, p) in enumerate(zip(src_offs, flat)):
        blob[o:o + len(p)] = np.frombuffer(p, np.uint8)
        spans[j] = InflateSpan(o, len(p), 0)
    descs = (InflateStream * max(len(lists), 1))()
    first, at = 0, 0
    for i, l in enumerate(lists):
        cap = int(caps[i])
        off = int(dst_offs[i]) if dst_offs is not None else at
        descs[i] = InflateStream(off, cap, first, len(l), 0)
        first += len(l)
        at = off + ((cap + 15) & ~15) + 16
    dst_bytes = max([d.dst_off + d.dst_cap for d in descs[:len(lists)]] + [0])
    return blob, spans, descs, dst_bytes, len(flat)


def file_list(files):
    """(pointer array, size array, keep-alive) of a list of bytes objects, as tm_png_decode_host and tm_set_frames_png take them"""
    bufs = [ctypes.create_string_buffer(bytes(f), len(f)) if len(f) else ctypes.create_string_buffer(1) for f in files]
    ptrs = (c_void_p * max(len(files), 1))(*[ctypes.addressof(b) for b in bufs])
    sizes = (ctypes.c_size_t * max(len(files), 1))(*[len(f) for f in files])
    return ptrs, sizes, bufs


def jpeg_plane_sizes(w, h, components, h_samp, v_samp):
    """[(width, height)] of the planes a JPEG of this geometry decodes to: chroma is ceil(w / h_samp) x ceil(h / v_samp)"""
    if components == 1:
        return [(w, h)]
    c = ((w + h_samp - 1) // h_samp, (h + v_samp - 1) // v_samp)
    return [(w, h), c, c]


SCALE_FILTERS = {"lanczos": 0, "nearest": 1}  # TM_SCALE_*


def scale_filter_of(filter):
    if isinstance(filter, str):
        if filter not in SCALE_FILTERS:
            raise ValueError("unknown scaling filter %r (one of %s)" % (filter, " ".join(SCALE_FILTERS)))
        return SCALE_FILTERS[filter]
    return int(filter)


def lib():
    """The loaded library; raises if it has not been built (python __graft_entry__.py / tiler_amd/csrc/build.sh)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise TileMotionError(-2, f"{p} not found: build it with tiler_amd/csrc/build.sh (no CPU fallback exists)")
        L = ctypes.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:
                continue  # declared-but-not-yet-built symbols are caught by tests/test_abi.py
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise TileMotionError(rc, lib().tm_last_error().decode("utf-8", "replace"))
