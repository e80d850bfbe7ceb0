"""Stage-level host wrappers over the C ABI for torch device tensors (tm_stage_*, include/tilemotion.h).

Each function names the reference routine it stands for; tensors must live on the current CUDA(HIP) device.
"""
import ctypes

import numpy as np
import torch

from ._lib import lib, check, scale_filter_of


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def load(frames, tm_w, tm_h):
    """TFrame.LoadFromImage + PrepareInterFrameData + mirror canonicalisation (tilingencoder.pas:1293-1411).
    frames: uint32-as-int32 [F][H][W] RGB32 -> (tiles int32 [F*tm_w*tm_h][64], flags uint8, lab_means float32 [.,3])"""
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.is_contiguous()
    f, h, w = frames.shape
    n = f * tm_w * tm_h
    tiles = torch.empty((n, 64), dtype=torch.int32, device=frames.device)
    flags = torch.empty((n,), dtype=torch.uint8, device=frames.device)
    lab = torch.empty((n, 3), dtype=torch.float32, device=frames.device)
    check(lib().tm_stage_load(_p(frames), f, w, h, tm_w, tm_h, _p(tiles), _p(flags), _p(lab), _stream()))
    return tiles, flags, lab


def pearson(lab):
    """PearsonCorrelation (tilingencoder.pas:2201-2228) of consecutive rows, as Load runs it on the frames' Lab tile means: lab float32
    [nframes][per] on the device -> numpy float32 [nframes] (entry 0 is 0)"""
    assert lab.is_cuda and lab.dtype == torch.float32 and lab.is_contiguous() and lab.dim() == 2
    nframes, per = lab.shape
    out = np.zeros((nframes,), np.float32)
    check(lib().tm_stage_pearson(_p(lab), nframes, per, out.ctypes.data_as(ctypes.c_void_p), _stream()))
    return out


def yuv_to_rgb32(y, u, v, chroma, dst_w, dst_h, yuv_mode=0):
    """Planes of a Y4M clip -> RGB32 frames (tm_stage_yuv_to_rgb32): chroma upsampling, the Lanczos-3 resize and the colour conversion in
    one kernel.  y uint8 [F][H][W]; u, v uint8 [F][ch][cw] (None for chroma 4 = mono); chroma: TM_CHROMA_* (0 444, 1 422, 2 420jpeg,
    3 420mpeg2, 4 mono); yuv_mode: TM_YUV_* -> int32 [F][dst_h][dst_w] 0x00RRGGBB"""
    assert y.is_cuda and y.dtype == torch.uint8 and y.dim() == 3 and y.stride(2) == 1
    f, h, w = y.shape
    strides = [y.stride(1), y.stride(0)]
    for c in (u, v):
        assert c is None or (c.is_cuda and c.dtype == torch.uint8 and c.dim() == 3 and c.stride(2) == 1 and c.shape[0] == f)
        strides += [c.stride(1), c.stride(0)] if c is not None else [0, 0]
    out = torch.empty((f, dst_h, dst_w), dtype=torch.int32, device=y.device)
    check(lib().tm_stage_yuv_to_rgb32(_p(y), _p(u), _p(v), (ctypes.c_int64 * 6)(*strides), f, w, h, int(chroma), dst_w, dst_h, int(yuv_mode), _p(out), _stream()))
    return out


def yuv_to_rgb32_fmt(y, u, v, chroma, dst_w, dst_h, yuv_mode=0, samples=0, depth=8):
    """The same for every sample format of a lent clip (tm_stage_yuv_to_rgb32_fmt): uint8 planes, or int16 / uint16 planes holding little-endian
    words of `depth` bits (samples: TM_SAMPLES_* -- 0 bytes, 1 the sample in the low bits, 2 in the high bits as P010 has it); v=None: u
    [F][ch][2 cw] holds (U, V) pairs as NV12 / P010 do.  Strides are taken from the tensors -> int32 [F][dst_h][dst_w] 0x00RRGGBB"""
    item = y.element_size()
    assert y.is_cuda and item in (1, 2) and y.dim() == 3 and y.stride(2) == 1
    f, h, w = y.shape
    strides = [y.stride(1) * item, y.stride(0) * item]
    for c in (u, v):
        assert c is None or (c.is_cuda and c.element_size() == item and c.dim() == 3 and c.stride(2) == 1 and c.shape[0] == f)
        strides += [c.stride(1) * item, c.stride(0) * item] if c is not None else [0, 0]
    out = torch.empty((f, dst_h, dst_w), dtype=torch.int32, device=y.device)
    check(lib().tm_stage_yuv_to_rgb32_fmt(_p(y), _p(u), _p(v), (ctypes.c_int64 * 6)(*strides), f, w, h, int(chroma), int(samples), int(depth), dst_w, dst_h,
                                          int(yuv_mode), _p(out), _stream()))
    return out


def scale_rgb32(frames, size, filter="lanczos", out=None):
    """RGB32 frames at another size (tm_stage_scale_rgb32, the kernel behind GtmPlayer.SetOutput and RenderFrames(size=...)): frames int32
    [F][H][W'] 0x00RRGGBB with a dense last axis; size (width, height); filter "lanczos" (the Lanczos-3 rule of yuv_to_rgb32, per channel) or
    "nearest".  out: an int32 CUDA tensor [F][height][width'] to fill (strides are taken from it) -> int32 [F][height][width], top byte 0"""
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 3 and frames.stride(2) == 1
    f, h, w = frames.shape
    dw, dh = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((f, max(dh, 0), max(dw, 0)), dtype=torch.int32, device=frames.device)
    if not (out.is_cuda and out.dtype == torch.int32 and out.dim() == 3 and out.stride(2) == 1 and tuple(out.shape) == (f, dh, dw)):
        raise ValueError("scale_rgb32: out must be an int32 CUDA tensor of %d frames of %d x %d with a dense last axis" % (f, dw, dh))
    check(lib().tm_stage_scale_rgb32(_p(frames), frames.stride(1), frames.stride(0), f, w, h, _p(out), out.stride(1), out.stride(0), dw, dh, scale_filter_of(filter),
                                     _stream()))
    return out


def rgb_to_rgb32(frames, layout="rgb24", size=None, depth=None, out=None, samples=None):
    """An RGB clip in device memory -> RGB32 frames (tm_stage_rgb_to_rgb32, the kernels behind SetFramesRGB's Load): frames and layout as
    SetFramesRGB takes them (a CUDA tensor; strides are its own); size (width, height): the output's, default the clip's (a pure unpack;
    otherwise the Lanczos-3 rule of scale_rgb32 on the unpacked pixels).  out: a contiguous int32 CUDA tensor [N][height][width] to fill
    -> int32 [N][height][width] 0x00RRGGBB"""
    from . import rgb_in
    assert frames.is_cuda
    clip = rgb_in.describe(frames, layout, depth, samples)
    dw, dh = (clip.width, clip.height) if size is None else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty((clip.frames, max(dh, 0), max(dw, 0)), dtype=torch.int32, device=frames.device)
    if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (clip.frames, dh, dw)):
        raise ValueError("rgb_to_rgb32: out must be a contiguous int32 CUDA tensor of %d frames of %d x %d" % (clip.frames, dw, dh))
    check(lib().tm_stage_rgb_to_rgb32(ctypes.byref(clip), dw, dh, _p(out), _stream()))
    return out


def rgb32_to_yuv(rgb, layout="nv12", yuv="auto", out=None, width=None):
    """RGB32 frames -> YUV planes (tm_stage_rgb32_to_yuv_fmt, the kernel behind GtmPlayer.ReadYUV): rgb int32 [F][H][W'] 0x00RRGGBB with a
    dense last axis, of which `width` columns (default: all) are converted; layout and yuv as ReadYUV takes them (auto = bt601-limited).
    out: (y, u, v) CUDA tensors to fill (strides are taken from them) -> (y, u, v), u None for mono, v None where u holds pairs"""
    from . import yuv_out
    assert rgb.is_cuda and rgb.dtype == torch.int32 and rgb.dim() == 3 and rgb.stride(2) == 1 and rgb.stride(0) == rgb.stride(1) * rgb.shape[1]
    f, h = rgb.shape[0], rgb.shape[1]
    w = rgb.shape[2] if width is None else int(width)
    planes, d = yuv_out.destination(layout, f, h, w, rgb.device, out)
    if (d.width, d.height) != (w, h) or d.frames < f or not d.memory:
        raise ValueError("rgb32_to_yuv: out must be CUDA planes of %d frames of %d x %d" % (f, w, h))
    strides = (ctypes.c_int64 * 6)(d.y_row, d.y_frame, d.u_row, d.u_frame, d.v_row, d.v_frame)
    check(lib().tm_stage_rgb32_to_yuv_fmt(_p(rgb), rgb.stride(1), f, w, h, ctypes.c_void_p(d.y), ctypes.c_void_p(d.u), ctypes.c_void_p(d.v), strides, d.chroma,
                                          d.samples, d.depth, yuv_out.mode_of(yuv), _stream()))
    return yuv_out.first(planes, f)


def rgb_to_lab(rgb):
    """RGBToLAB (utils.pas:374-410) of colours 0x00RRGGBB (int32 [n]) -> float32 [n][3]"""
    assert rgb.is_cuda and rgb.dtype == torch.int32 and rgb.is_contiguous()
    out = torch.empty((rgb.shape[0], 3), dtype=torch.float32, device=rgb.device)
    check(lib().tm_stage_rgb_to_lab(_p(rgb), rgb.shape[0], _p(out), _stream()))
    return out


def features_rgb(tiles, mirror_flags=None, mode=1, use_lab=False):
    """ConvertToCpnPixels + ComputeCpnPixelsPsyVisFeatures (tilingencoder.pas:3049-3131) -> int16 [n][192]"""
    assert tiles.is_cuda and tiles.dtype == torch.int32 and tiles.is_contiguous()
    n = tiles.shape[0]
    out = torch.empty((n, 192), dtype=torch.int16, device=tiles.device)
    check(lib().tm_stage_features_rgb(_p(tiles), n, _p(mirror_flags), mode, int(use_lab), _p(out), _stream()))
    return out


def features_rgb_rows(tiles, rows, mode=1, use_lab=False, with_colmm=True):
    """features_rgb of tiles[rows] without the gather (Reconstruct's queries: rows int32 [n], repeats allowed) -> int16 [n][192] and, with_colmm,
    int32 [2][192]: the minimum and the maximum of every output column, folded in by the kernel (None otherwise)"""
    assert tiles.is_cuda and tiles.dtype == torch.int32 and tiles.is_contiguous()
    assert rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous()
    n = rows.shape[0]
    out = torch.empty((n, 192), dtype=torch.int16, device=tiles.device)
    colmm = None
    if with_colmm:  # the kernel's atomics start from the empty range
        info = torch.iinfo(torch.int32)
        colmm = torch.tensor([[info.max], [info.min]], dtype=torch.int32, device=tiles.device).repeat(1, 192)
    check(lib().tm_stage_features_rgb_rows(_p(tiles), _p(rows), n, mode, int(use_lab), _p(out), _p(colmm), _stream()))
    return out, colmm


def features_pal(pal_px, pal_idx, palettes, mode=1):
    """PrepareReconstruct.DoPsyV (tilingencoder.pas:4570-4583) -> int16 [n][192]"""
    n = pal_px.shape[0]
    out = torch.empty((n, 192), dtype=torch.int16, device=pal_px.device)
    check(lib().tm_stage_features_pal(_p(pal_px), _p(pal_idx), n, _p(palettes), palettes.shape[1], mode, _p(out), _stream()))
    return out


def features_cluster(tiles, mode=4):
    """ComputeTilePsyVisFeatures as DoPalettization calls it (tilingencoder.pas:4126), Round()ed -> int32 [n][192]; mode 2 =
    pvsWavelets, the Haar branch of its double path (3150-3157)"""
    n = tiles.shape[0]
    out = torch.empty((n, 192), dtype=torch.int32, device=tiles.device)
    check(lib().tm_stage_features_cluster(_p(tiles), n, mode, _p(out), _stream()))
    return out


def window_dcts(frame_buffer):
    """PredictMotion.DoDCTs / Reconstruct.DoDCTs (tilingencoder.pas:1157-1182): int32 [H][W] 0x00BBGGRR -> int16 [(H-7)*(W-7)][192]"""
    h, w = frame_buffer.shape
    out = torch.empty(((h - 7) * (w - 7), 192), dtype=torch.int16, device=frame_buffer.device)
    check(lib().tm_stage_window_dcts(_p(frame_buffer), w, h, _p(out), _stream()))
    return out


def motion_search(cur, tm_w, tm_h, win, radius):
    """PredictMotion.DoXY search (tilingencoder.pas:1209-1253) -> (err int32-as-uint32, px int8, py int8), one per tile"""
    n = tm_w * tm_h
    err = torch.empty((n,), dtype=torch.int32, device=cur.device)
    px = torch.empty((n,), dtype=torch.int8, device=cur.device)
    py = torch.empty((n,), dtype=torch.int8, device=cur.device)
    check(lib().tm_stage_motion_search(_p(cur), tm_w, tm_h, _p(win), radius, _p(err), _p(px), _p(py), _stream()))
    return err, px, py


def motion_search_fb(cur, tm_w, tm_h, fb, radius):
    """the same search in a frame buffer (int32 [tm_h*8][tm_w*8] 0x00BBGGRR), whose window features are made in the search's own layout:
    what PredictMotion runs per frame (tm_stage_motion_search_fb) -> (err int32-as-uint32, px int8, py int8), one per tile"""
    assert fb.is_cuda and fb.dtype == torch.int32 and fb.is_contiguous() and tuple(fb.shape) == (tm_h * 8, tm_w * 8)
    assert cur.is_cuda and cur.dtype == torch.int16 and cur.is_contiguous() and tuple(cur.shape) == (tm_w * tm_h, 192)
    n = tm_w * tm_h
    err = torch.empty((n,), dtype=torch.int32, device=cur.device)
    px = torch.empty((n,), dtype=torch.int8, device=cur.device)
    py = torch.empty((n,), dtype=torch.int8, device=cur.device)
    check(lib().tm_stage_motion_search_fb(_p(cur), tm_w, tm_h, _p(fb), radius, _p(err), _p(px), _p(py), _stream()))
    return err, px, py


def knn_topk(queries, db, k=64):
    """ann_kdtree_short_search_multi (tilingencoder.pas:1563) for every query -> (idx int32 [nq][k], err int32-as-uint32 [nq][k])"""
    nq = queries.shape[0]
    idx = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    err = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    check(lib().tm_stage_knn_topk(_p(queries), nq, _p(db), db.shape[0], k, _p(idx), _p(err), _stream()))
    return idx, err


def epu_rerank(queries, knn_idx, pal_px, tile_pal_idx, palettes):
    """FrameTilingExtendedPaletteUsage re-rank (tilingencoder.pas:1576-1610) -> (tile int32, pal int32, err int32-as-uint32)"""
    nq = queries.shape[0]
    t = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    p = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    e = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    check(lib().tm_stage_epu_rerank(_p(queries), nq, _p(knn_idx), knn_idx.shape[1], _p(pal_px), _p(tile_pal_idx), pal_px.shape[0],
                                    _p(palettes), palettes.shape[0], palettes.shape[1], _p(t), _p(p), _p(e), _stream()))
    return t, p, e


def knn(queries, db):
    """ann_kdtree_short_search(eps=0) for every query (tilingencoder.pas:1547) -> (idx int32, err int32-as-uint32)"""
    nq, nt = queries.shape[0], db.shape[0]
    idx = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    err = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    check(lib().tm_stage_knn(_p(queries), nq, _p(db), nt, _p(idx), _p(err), _stream()))
    return idx, err


def knn_tile_order(perm):
    """every run of 32 entries of perm (int32 / uint32 bit patterns on the device) into ascending unsigned order, in place"""
    check(lib().tm_stage_knn_tile_order(_p(perm), perm.shape[0], _stream()))
    return perm


def curve_keys(coords, bits, kind):
    """the KNN searches' curve key of every cell of coords (int32 / uint32 bit patterns [n][4] on the device, coordinate d below 2^bits[d]) ->
    int32 [n] holding uint32 bit patterns.  kind 0: Morton order (the bits interleaved), 1: Hilbert order"""
    n = coords.shape[0]
    keys = torch.empty((n,), dtype=torch.int32, device=coords.device)
    check(lib().tm_stage_curve_keys(_p(coords), n, (ctypes.c_int * 4)(*[int(b) for b in bits]), kind, _p(keys), _stream()))
    return keys


def knn_last_plan():
    """(ht, hq, topk, arena_retries): the digit plan and mode of this thread's last scan, and the process's count of repeated scans (tests)"""
    ht, hq, tk, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    check(lib().tm_knn_last_plan(ctypes.byref(ht), ctypes.byref(hq), ctypes.byref(tk), ctypes.byref(r)))
    return ht.value, hq.value, tk.value, r.value


class KnnIndex:
    """ann_kdtree_short_create analogue: the database is packed once and searched by many query batches."""

    def __init__(self, db):
        self.db = db  # borrowed for the index lifetime, like the reference's DS.Dataset (tilingencoder.pas:4600)
        self.h = lib().tm_knn_index_create(_p(db), db.shape[0], _stream())
        if not self.h:
            check(-3)

    def search(self, queries):
        nq = queries.shape[0]
        idx = torch.empty((nq,), dtype=torch.int32, device=queries.device)
        err = torch.empty((nq,), dtype=torch.int32, device=queries.device)
        check(lib().tm_knn_index_search(ctypes.c_void_p(self.h), _p(queries), nq, _p(idx), _p(err), _stream()))
        return idx, err

    def last_stats(self):
        ms, kb, pairs = ctypes.c_double(), ctypes.c_int(), ctypes.c_int64()
        check(lib().tm_knn_index_last_stats(ctypes.c_void_p(self.h), ctypes.byref(ms), ctypes.byref(kb), ctypes.byref(pairs)))
        return ms.value, kb.value, pairs.value

    def last_list_counts(self):
        """(entries listed, entries popped) of the last search's tile lists"""
        listed, popped = ctypes.c_int64(), ctypes.c_int64()
        check(lib().tm_knn_index_last_list_counts(ctypes.c_void_p(self.h), ctypes.byref(listed), ctypes.byref(popped)))
        return listed.value, popped.value

    def last_chunk_counts(self):
        """(listed blocks judged on their first chunk, blocks that ended there) of the last search"""
        looked, stopped = ctypes.c_int64(), ctypes.c_int64()
        check(lib().tm_knn_index_last_chunk_counts(ctypes.c_void_p(self.h), ctypes.byref(looked), ctypes.byref(stopped)))
        return looked.value, stopped.value

    def last_survivor_counts(self):
        """(tiles popped, those with no block past its look, survivor entries queued, entries the full queue turned away, tiles loaded
        whole, blocks run to completion) of the last search's consume kernel"""
        v = [ctypes.c_int64() for _ in range(6)]
        check(lib().tm_knn_index_last_survivor_counts(ctypes.c_void_p(self.h), *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def row_order(self):
        """the database's row order as the scan sees it (numpy uint32 [nt]; tile t = rows [32 t, 32 t + 32)), after a search"""
        out = np.empty((self.db.shape[0],), dtype=np.uint32)
        check(lib().tm_knn_index_row_order(ctypes.c_void_p(self.h), out.ctypes.data_as(ctypes.c_void_p), _stream()))
        return out

    def close(self):
        if self.h:
            lib().tm_knn_index_destroy(ctypes.c_void_p(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dither(tiles, flags, pal_idx, palettes, use_thomas_knoll=True, y2_mixed=4):
    """Dither = PreparePlan + DitherTile per tile (tilingencoder.pas:1873-1907) -> uint8 [n][64]"""
    n = tiles.shape[0]
    out = torch.empty((n, 64), dtype=torch.uint8, device=tiles.device)
    check(lib().tm_stage_dither(_p(tiles), _p(flags), _p(pal_idx), n, _p(palettes), palettes.shape[0], palettes.shape[1],
                                int(use_thomas_knoll), y2_mixed, _p(out), _stream()))
    return out


def dedup(rows, use_in=None):
    """MakeTilesUnique + ReindexTiles (tilingencoder.pas:4720-4781, 4626-4700).  rows: int32 [n][64] (RGB tiles) or
    uint8 [n][64] (palette-index tiles).  -> (n_unique, remap int32 [n], order int32 [n_unique], use uint32-as-int32 [n_unique])"""
    n = rows.shape[0]
    row_bytes = rows.shape[1] * rows.element_size()
    remap = torch.empty((n,), dtype=torch.int32, device=rows.device)
    order = torch.empty((n,), dtype=torch.int32, device=rows.device)
    use = torch.empty((n,), dtype=torch.int32, device=rows.device)
    nu = ctypes.c_int64()
    check(lib().tm_stage_dedup(_p(rows), n, row_bytes, _p(use_in), _p(remap), _p(order), _p(use), ctypes.byref(nu), _stream()))
    return nu.value, remap, order[: nu.value], use[: nu.value]


def dedup_by_index(rows):
    """the grouping Reconstruct puts its database rows through: rows [n][row_bytes a multiple of 16] -> (n_unique, remap int32 [n] (position
    of each row's first occurrence in order), order int32 [n_unique] (the first occurrences, ascending), use int32 [n_unique] (rows per group))"""
    n = rows.shape[0]
    row_bytes = rows.shape[1] * rows.element_size()
    remap = torch.empty((n,), dtype=torch.int32, device=rows.device)
    order = torch.empty((n,), dtype=torch.int32, device=rows.device)
    use = torch.empty((n,), dtype=torch.int32, device=rows.device)
    nu = ctypes.c_int64()
    check(lib().tm_stage_dedup_by_index(_p(rows), n, row_bytes, _p(remap), _p(order), _p(use), ctypes.byref(nu), _stream()))
    return nu.value, remap, order[: nu.value], use[: nu.value]


def host_waits():
    """how often the library has made the host wait for a stream so far in PreparePalettes and the dedup (small read-backs and the stream
    synchronisations of those stages), over all threads"""
    return int(lib().tm_host_waits())


def kmeans(pts, weights, k, max_iter=300):
    """the build's deterministic k-means: pts int32 [n][d] -> (live_k, assign int32 [n], centroids float64 [k][d], iters)"""
    n, d = pts.shape
    assign = torch.empty((n,), dtype=torch.int32, device=pts.device)
    cent = torch.zeros((k, d), dtype=torch.float64, device=pts.device)
    hk, hi = ctypes.c_int(), ctypes.c_int()
    check(lib().tm_stage_kmeans(_p(pts), _p(weights), n, d, k, max_iter, _p(assign), _p(cent), ctypes.byref(hk), ctypes.byref(hi), _stream()))
    return hk.value, assign, cent, hi.value


def kmeans_seeded(pts, weights, k, init_idx, max_iter=300):
    """the same Lloyd iterations from the caller's own initial centres (init_idx: k point indices, -1 = none)"""
    import numpy as np
    n, d = pts.shape
    assign = torch.empty((n,), dtype=torch.int32, device=pts.device)
    cent = torch.zeros((k, d), dtype=torch.float64, device=pts.device)
    idx = np.full(k, -1, np.int64)
    idx[: len(init_idx)] = np.asarray(init_idx, np.int64)[:k]
    hk, hi = ctypes.c_int(), ctypes.c_int()
    check(lib().tm_stage_kmeans_seeded(_p(pts), _p(weights), n, d, k, idx.ctypes.data_as(ctypes.c_void_p), max_iter, _p(assign), _p(cent),
                                       ctypes.byref(hk), ctypes.byref(hi), _stream()))
    return hk.value, assign, cent, hi.value


def quantize_palettes(tiles, pal_idx, npal, pal_size, max_iter=300):
    """QuantizeUsingYakmo + DoQuantization for every palette (tilingencoder.pas:4434-4564) -> int32 [npal][pal_size]"""
    out = torch.empty((npal, pal_size), dtype=torch.int32, device=tiles.device)
    check(lib().tm_stage_quantize_palettes(_p(tiles), _p(pal_idx), tiles.shape[0], npal, pal_size, max_iter, _p(out), _stream()))
    return out


def palettize(feat, use, npal, max_iter=300):
    """DoPalettization (tilingencoder.pas:4105-4245): cluster features -> PalIdx_Initial int32 [n], palettes ranked by tile count"""
    out = torch.empty((feat.shape[0],), dtype=torch.int32, device=feat.device)
    check(lib().tm_stage_palettize(_p(feat), _p(use), feat.shape[0], npal, max_iter, _p(out), _stream()))
    return out


def kmeans_last_resident():
    """did this thread's last k-means (kmeans, kmeans_seeded, or the one inside palettize / quantize_palettes) run through a resident launch
    to its end?  False: one launch per step -- by shape, by TM_KM_LAUNCHES, or after a barrier of the resident launch gave up"""
    return bool(lib().tm_kmeans_last_resident())


def kmeans_last_first_look():
    """the first look of this thread's last tile k-means (D = 192): (point-scorings looked at in single precision, those of them that went
    to the double-precision chain); (0, 0) under TM_KM_FIRST_LOOK=0"""
    looked, exact = ctypes.c_int64(0), ctypes.c_int64(0)
    lib().tm_kmeans_last_first_look(ctypes.byref(looked), ctypes.byref(exact))
    return int(looked.value), int(exact.value)


def pp_seeds(feat, use, k):
    """the D^2 seeding of palettize alone (test seam): feat int32 [n][192], use uint32-as-int32 [n] or None ->
    (centres found, numpy int64 [k]: the picked point indices in pick order, -1 beyond the centres found)"""
    import numpy as np
    assert feat.is_cuda and feat.dtype == torch.int32 and feat.is_contiguous() and feat.dim() == 2 and feat.shape[1] == 192
    assert use is None or (use.is_cuda and use.dtype == torch.int32 and use.is_contiguous() and use.numel() == feat.shape[0])
    seeds = np.full(k, -1, np.int64)
    kk = ctypes.c_int()
    check(lib().tm_stage_pp_seeds(_p(feat), _p(use), feat.shape[0], k, seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(kk), _stream()))
    return kk.value, seeds


def kmodes(rows, num_clusters, num_init=0, num_modalities=256, max_iter=-1):
    """TKModes.ComputeKModes (kmodes.pas:923-1094): rows uint8 numpy [n][80] (host, like the Pascal arrays) ->
    (labels int32 [n], centroids uint8 [k][80], cost, iterations of the best run)"""
    import numpy as np
    rows = np.ascontiguousarray(rows, np.uint8)
    assert rows.ndim == 2 and rows.shape[1] == 80
    labels = np.zeros(rows.shape[0], np.int32)
    cent = np.zeros((num_clusters, 80), np.uint8)
    cost, iters = ctypes.c_uint64(), ctypes.c_int()
    check(lib().tm_stage_kmodes(rows.ctypes.data_as(ctypes.c_void_p), rows.shape[0], num_clusters, num_init, num_modalities, max_iter,
                                labels.ctypes.data_as(ctypes.c_void_p), cent.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cost), ctypes.byref(iters), _stream()))
    return labels, cent, cost.value, iters.value


def dl3quant(rgb, quant_to, lookup_bpc):
    """dl3quant (dlquant/quantizer.c:437-455): rgb = torch uint8 CUDA tensor [n][3] (R, G, B) -> (palette uint8 CUDA [3][quant_to] planar,
    number of colours left)"""
    import torch
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.ndim == 2 and rgb.shape[1] == 3
    rgb = rgb.contiguous()
    pal = torch.zeros((3, quant_to), dtype=torch.uint8, device=rgb.device)
    n = ctypes.c_int()
    L = lib()
    L.tm_stage_dl3quant.restype = ctypes.c_int
    L.tm_stage_dl3quant.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    check(L.tm_stage_dl3quant(ctypes.c_void_p(rgb.data_ptr()), rgb.shape[0], int(quant_to), int(lookup_bpc), ctypes.c_void_p(pal.data_ptr()), ctypes.byref(n), _stream()))
    return pal, n.value


def kmodes_dev(rows, num_clusters, num_init=0, num_modalities=256, max_iter=-1):
    """TKModes.ComputeKModes on device memory: rows torch uint8 CUDA [n][80] -> (labels int32 CUDA [n], centroids uint8 CUDA [k][80], cost,
    iterations of the best run, points x iterations of all runs)"""
    import torch
    assert rows.is_cuda and rows.dtype == torch.uint8 and rows.ndim == 2 and rows.shape[1] == 80
    rows = rows.contiguous()
    labels = torch.zeros(rows.shape[0], dtype=torch.int32, device=rows.device)
    cent = torch.zeros((num_clusters, 80), dtype=torch.uint8, device=rows.device)
    cost, iters, pit = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int64()
    L = lib()
    L.tm_stage_kmodes_dev.restype = ctypes.c_int
    L.tm_stage_kmodes_dev.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    check(L.tm_stage_kmodes_dev(ctypes.c_void_p(rows.data_ptr()), rows.shape[0], num_clusters, num_init, num_modalities, max_iter, ctypes.c_void_p(labels.data_ptr()),
                                ctypes.c_void_p(cent.data_ptr()), ctypes.byref(cost), ctypes.byref(iters), ctypes.byref(pit), _stream()))
    return labels, cent, cost.value, iters.value, pit.value


def render(tile_idx, pal_idx, item_flags, px, py, tm_w, tm_h, pal_px, palettes):
    """Render (tilingencoder.pas:3455-3640, the constructor's defaults) of F frames from their tile maps: tile_idx / pal_idx int32 [F][tm_h*tm_w],
    item_flags uint8 (bit 0 H mirror, bit 1 V mirror, bit 2 predicted), px / py int8 (PredictedX / PredictedY), pal_px uint8 [T][64],
    palettes int32 [npal][pal_size] 0x00BBGGRR -> int32 [F][tm_h*8][tm_w*8] 0x00RRGGBB; predicted items copy frame f-1's output (black before frame 0)"""
    per = tm_w * tm_h
    for t, dt in ((tile_idx, torch.int32), (pal_idx, torch.int32), (item_flags, torch.uint8), (px, torch.int8), (py, torch.int8), (pal_px, torch.uint8),
                  (palettes, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    n = tile_idx.numel()
    assert n % per == 0 and all(t.numel() == n for t in (pal_idx, item_flags, px, py))
    nf = n // per
    out = torch.empty((nf, tm_h * 8, tm_w * 8), dtype=torch.int32, device=tile_idx.device)
    check(lib().tm_stage_render(_p(tile_idx), _p(pal_idx), _p(item_flags), _p(px), _p(py), tm_w, tm_h, nf, _p(pal_px), pal_px.numel() // 64, _p(palettes),
                                palettes.shape[0], palettes.shape[1], _p(out), _stream()))
    return out


def render_view(tile_idx, pal_idx, item_flags, px, py, tm_w, tm_h, pal_px, rgb_px, tile_flags, pal_idx_initial, palettes, page="output", predicted=True,
                mirrored=True, dithered=True, gamma=None, palette=-1, pages=None):
    """Render's Output or Tiles page under its switches (tm_stage_render_view; the rule: include/tilemotion.h) from caller-held tables: those of
    render(), plus rgb_px int32 [T][64] 0x00BBGGRR, tile_flags int32 [T] (the tm_tile_hdr Flags bits: 0 Active, 1 HasRGBPixels, 2 HasPalPixels,
    3 / 4 H / VMirror_Initial) and pal_idx_initial int32 [T].  page="output": the F frames of the tile maps; page="tiles": `pages` pages from page 0
    (default: all, ceil(T / (tm_w*tm_h)); the tile-map tensors may be None).  Switches as TilingEncoder.RenderView -> int32 [F][tm_h*8][tm_w*8]"""
    from ._lib import render_view_desc
    per = tm_w * tm_h
    for t, dt in ((pal_px, torch.uint8), (rgb_px, torch.int32), (tile_flags, torch.int32), (pal_idx_initial, torch.int32), (palettes, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    ntiles = tile_flags.numel()
    assert pal_px.numel() == ntiles * 64 and rgb_px.numel() == ntiles * 64 and pal_idx_initial.numel() == ntiles
    view = render_view_desc(page, predicted, mirrored, dithered, gamma, palette)
    if view.page == 2:
        nf = -(-ntiles // per) if pages is None else int(pages)
        maps = [None] * 5
    else:
        maps = [tile_idx, pal_idx, item_flags, px, py]
        for t, dt in zip(maps, (torch.int32, torch.int32, torch.uint8, torch.int8, torch.int8)):
            assert t.is_cuda and t.dtype == dt and t.is_contiguous()
        n = tile_idx.numel()
        assert n % per == 0 and all(t.numel() == n for t in maps)
        nf = n // per
    out = torch.empty((nf, tm_h * 8, tm_w * 8), dtype=torch.int32, device=pal_px.device)
    check(lib().tm_stage_render_view(view, *[None if t is None else _p(t) for t in maps], tm_w, tm_h, nf, _p(pal_px), _p(rgb_px), _p(tile_flags),
                                     _p(pal_idx_initial), ntiles, _p(palettes), palettes.shape[0], palettes.shape[1], _p(out), _stream()))
    return out


def _mean_in_order(v):
    acc = 0.0
    for x in v.tolist():  # frame order, as tm_get_frame_quality sums
        acc += x
    return acc / len(v) if len(v) else float("nan")


def frame_quality(a, b):
    """Quality of frames b (decoded) against a (source), int32 [F][H][W] 0x00RRGGBB (H, W multiples of 4, rows may be padded): the sums of
    tm_get_frame_quality.  -> dict: sse int64 [F][3] (R, G, B) and ssim_y float64 [F] on the device; psnr (numpy [F], inf where SSE is 0),
    clip_psnr (from the summed SSE) and clip_ssim_y (mean of the frames') on the host"""
    import numpy as np
    assert a.is_cuda and b.is_cuda and a.dtype == torch.int32 and b.dtype == torch.int32 and a.shape == b.shape and a.dim() == 3
    assert a.stride() == b.stride() and a.stride(2) == 1 and a.stride(0) == a.shape[1] * a.stride(1)
    f, h, w = a.shape
    sse = torch.empty((f, 3), dtype=torch.int64, device=a.device)
    ssim = torch.empty((f,), dtype=torch.float64, device=a.device)
    check(lib().tm_stage_frame_quality(_p(a), _p(b), f, w, h, a.stride(1), _p(sse), _p(ssim), _stream()))
    e = sse.cpu().numpy().astype(np.uint64)
    s = ssim.cpu().numpy()
    peak = 3.0 * w * h * 255.0 * 255.0
    tot = e.sum(axis=1)
    with np.errstate(divide="ignore"):
        psnr = np.where(tot > 0, 10.0 * np.log10(peak / np.maximum(tot, 1).astype(np.float64)), np.inf)
    allsum = int(tot.sum())
    clip_psnr = 10.0 * np.log10(peak * f / allsum) if allsum else float("inf")
    return dict(sse=sse, ssim_y=ssim, psnr=psnr, clip_psnr=float(clip_psnr), clip_ssim_y=_mean_in_order(s))


LZ_PAIR = np.dtype([("len", "<u2"), ("zero", "<u2"), ("dist", "<u4")])  # tm_lz_pair: a match of `len` bytes at distance `dist` + 1


def lz_matches(src, first=0, count=None):
    """The LZMA coder's match lists of positions [first, first + count) of a stream, found on the device (tm_stage_lz_matches; the rule:
    include/tilemotion.h): src = torch uint8 CUDA tensor [n] -> (counts uint8 CUDA [count], pairs numpy LZ_PAIR [sum of counts], position
    order), pair for pair what tm_lz_matches_host returns"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()
    n = src.numel()
    count = n - first if count is None else count
    counts = torch.zeros((max(count, 1),), dtype=torch.uint8, device=src.device)
    need = ctypes.c_size_t()
    rc = lib().tm_stage_lz_matches(_p(src), n, first, count, _p(counts), None, 0, ctypes.byref(need), _stream())
    if rc == 0:  # no pairs at all
        return counts[:count], np.zeros(0, LZ_PAIR)
    if need.value == 0:
        check(rc)
    pairs = torch.zeros((need.value, 2), dtype=torch.int32, device=src.device)
    check(lib().tm_stage_lz_matches(_p(src), n, first, count, _p(counts), _p(pairs), need.value, ctypes.byref(need), _stream()))
    return counts[:count], pairs.cpu().numpy().view(LZ_PAIR).reshape(-1)


def lz_compress(data):
    """LZCompress (extern.pas:420-439) with the match lists from the device finder and the host parser behind it (tm_stage_lz_compress):
    bytes -> bytes, exactly tm_lz_compress_host's"""
    src = np.frombuffer(bytes(data), np.uint8)
    cap = src.size + src.size // 4 + 64
    dst = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t()
    check(lib().tm_stage_lz_compress(src.ctypes.data_as(ctypes.c_void_p) if src.size else None, src.size, dst.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)))
    return dst[:n.value].tobytes()


def png_encode(frames, level=1, filter="none"):
    """RGB32 frames on the device as PNG files (tm_stage_png_encode; the rule: include/tilemotion.h): frames = torch
    int32 CUDA tensor [F][H][W] of 0x00RRGGBB, rows and frames at any stride -> list of F bytes objects, byte for byte what
    tm_png_encode_host writes.  level 0: stored blocks; level 1: filtered rows (filter: "none", "adaptive", "smaller"; "auto" = "none"
    here), matched, parsed, coded and packed on the device -- only the files' bytes come to the host"""
    from ._lib import png_options
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 3 and (frames.shape[2] <= 1 or frames.stride(2) == 1)
    nf, h, w = frames.shape
    opt = png_options(level, filter)
    bound = ctypes.c_int64()
    check(lib().tm_png_bound_host(w, h, ctypes.byref(bound)))
    out = np.empty(bound.value * max(nf, 1), np.uint8)
    offs = (ctypes.c_int64 * (nf + 1))()
    check(lib().tm_stage_png_encode(_p(frames), frames.stride(1), frames.stride(0), nf, w, h, ctypes.byref(opt), out.ctypes.data_as(ctypes.c_void_p), out.size, offs,
                                    _stream()))
    return [out[offs[f]:offs[f + 1]].tobytes() for f in range(nf)]


def zlib_compress(data):
    """The PNG writer's stream coder alone (tm_stage_zlib_compress): data = bytes, or a torch uint8 CUDA tensor [n] -> one zlib stream,
    exactly tm_zlib_compress_host's"""
    if not torch.is_tensor(data):
        raw = np.frombuffer(bytes(data), np.uint8)
        data = torch.from_numpy(raw.copy()).cuda() if raw.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
    n = data.numel()
    cap = n + 10 * (n // 32768 + 1) + 6
    out = np.empty(cap, np.uint8)
    got = ctypes.c_int64()
    check(lib().tm_stage_zlib_compress(_p(data) if n else None, n, out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(got), _stream()))
    return out[:got.value].tobytes()


def inflate(streams, caps, dst_offs=None, src_offs=None, guard=0):
    """A batch of zlib streams in host memory inflated on the device in one launch (tm_stage_inflate; the rule: tm_inflate.h, DESIGN.md
    section 35).  streams: a list whose items are bytes or a list of bytes (a stream's spans); caps: the most each may write; dst_offs:
    where each one's output starts in the destination (default: one behind the other); src_offs: where each span starts in the blob;
    guard: bytes of 0xA5 kept behind the last destination -> (dst uint8 CUDA tensor, filled with 0xA5 before the launch, [(code, in_pos,
    out_n)] per stream)"""
    from ._lib import InflateStatus, inflate_batch
    blob, spans, descs, dst_bytes, nspans = inflate_batch(streams, caps, dst_offs, src_offs)
    dst = torch.full((dst_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    status = (InflateStatus * max(len(streams), 1))()
    check(lib().tm_stage_inflate(blob.ctypes.data_as(ctypes.c_void_p), blob.size if nspans else 0, spans, nspans, descs, len(streams), _p(dst), dst_bytes, status, _stream()))
    return dst, [(s.code, s.in_pos, s.out_n) for s in status[:len(streams)]]


def png_decode(files, w, h, frame_px=None):
    """A batch of PNG file images in host memory decoded on the device (tm_stage_png_decode: k_inflate, k_png_unfilter).  files: a list of
    bytes, every one a w x h picture; frame_px: pixels from one frame of the destination to the next (default w h) -> (int32 CUDA tensor
    [len(files)][frame_px] filled with -1 before the launch: frame f's pixels are its first w h entries, 0x00RRGGBB; status per file)"""
    from ._lib import file_list
    frame_px = w * h if frame_px is None else int(frame_px)
    ptrs, sizes, keep = file_list(files)
    out = torch.full((max(len(files), 1), frame_px), -1, dtype=torch.int32, device="cuda")
    status = (ctypes.c_int32 * max(len(files), 1))()
    check(lib().tm_stage_png_decode(ptrs, sizes, len(files), w, h, _p(out), frame_px, status, _stream()))
    del keep
    return out[:len(files)], list(status[:len(files)])


def jpeg_probe(file):
    """What the container walk finds of one JPEG file, with no device (tm_probe_jpeg_host): a dict of width, height, components, h_samp,
    v_samp (the luma sampling factors), restart_interval, segments, sof, chroma (TM_CHROMA_*) and status (0, or TM_JPG_BAD_RESTART).  The
    walk's refusals raise."""
    from ._lib import JpegInfoDesc
    info = JpegInfoDesc()
    buf = bytes(file)
    check(lib().tm_probe_jpeg_host(buf, len(buf), ctypes.byref(info)))
    return {name: getattr(info, name) for name, _ in JpegInfoDesc._fields_}


def _jpeg_decode(files, w, h, guard, host):
    import numpy as np
    from ._lib import file_list
    files = [bytes(f) for f in files]
    n = len(files)
    ptrs, sizes, keep = file_list(files)
    # every plane's slot holds w x h samples on rows of w rounded up to 8 bytes, with `guard` bytes of 0xA5 before, between and behind
    row = (w + 7) & ~7
    frame = (row * h + guard + 7) & ~7
    total = guard + frame * max(n, 1)
    if host:
        planes = [np.full(total, 0xA5, np.uint8) for _ in range(3)]
        base = [p.ctypes.data + guard for p in planes]
    else:
        planes = [torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
        base = [p.data_ptr() + guard for p in planes]
    strides = (ctypes.c_int64 * 6)(row, frame, row, frame, row, frame)
    status = (ctypes.c_int32 * max(n, 1))()
    if host:
        check(lib().tm_jpeg_decode_host(ptrs, sizes, n, w, h, base[0], base[1], base[2], strides, status))
    else:
        check(lib().tm_stage_jpeg_decode(ptrs, sizes, n, w, h, base[0], base[1], base[2], strides, status, _stream()))
    del keep
    return planes, list(status[:n]), {"row": row, "frame": frame, "first": guard}


def jpeg_decode(files, w=None, h=None, guard=64):
    """A batch of JPEG file images in host memory decoded on the device (tm_stage_jpeg_decode: k_jpeg_decode).  files: a list of bytes;
    w, h: the size of a plane's slot (default: the largest file's) -> ([Y, U, V] uint8 CUDA tensors filled with 0xA5 before the launch,
    status per file, layout): file i's plane starts at layout["first"] + i layout["frame"], rows layout["row"] apart, at the file's own
    size; `guard` bytes lie before the first slot and behind every slot's h rows."""
    if w is None or h is None:
        infos = [jpeg_probe(f) for f in files]
        w = max([i["width"] for i in infos] + [1])
        h = max([i["height"] for i in infos] + [1])
    return _jpeg_decode(files, int(w), int(h), int(guard), False)


def jpeg_decode_host(files, w=None, h=None, guard=64):
    """jpeg_decode's host twin (tm_jpeg_decode_host), no device: the same arguments and layout, numpy arrays"""
    if w is None or h is None:
        infos = [jpeg_probe(f) for f in files]
        w = max([i["width"] for i in infos] + [1])
        h = max([i["height"] for i in infos] + [1])
    return _jpeg_decode(files, int(w), int(h), int(guard), True)


def jpeg_bound(w, h, quality=90, sampling="420", restart_rows=1):
    """An upper bound of one JPEG file's size for any pixels (tm_jpeg_bound_host), no device"""
    from ._lib import jpeg_options
    opt = jpeg_options(quality, sampling, restart_rows)
    bound = ctypes.c_int64()
    check(lib().tm_jpeg_bound_host(int(w), int(h), ctypes.byref(opt), ctypes.byref(bound)))
    return bound.value


def jpeg_quant_tables(quality):
    """The luma and chroma quantisers of a quality in natural order (tm_jpeg_quant_tables_host), no device -> two uint16 arrays [64]"""
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    check(lib().tm_jpeg_quant_tables_host(int(quality), luma.ctypes.data_as(ctypes.c_void_p), chroma.ctypes.data_as(ctypes.c_void_p)))
    return luma, chroma


def _jpeg_encode(call, ptr, stride_px, frame_px, nf, w, h, opt, cap, guard, full, extra):
    if cap is None:
        bound = ctypes.c_int64()
        check(lib().tm_jpeg_bound_host(w, h, ctypes.byref(opt), ctypes.byref(bound)))
        cap = bound.value * max(nf, 1)
    buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
    offs = (ctypes.c_int64 * (nf + 1))(*([-1] * (nf + 1)))
    rc = call(ptr, stride_px, frame_px, nf, w, h, ctypes.byref(opt), ctypes.c_void_p(buf.ctypes.data + guard) if cap else None, cap, offs, *extra)
    if not full:
        check(rc)
    files = [buf[guard + offs[f]:guard + offs[f + 1]].tobytes() for f in range(nf)] if rc == 0 else None
    return dict(rc=rc, files=files, buffer=buf, offsets=list(offs), guard=guard) if full else files


def jpeg_encode(frames, quality=90, sampling="420", restart_rows=1, cap=None, guard=0, full=False):
    """RGB32 frames on the device as baseline JPEG files (tm_stage_jpeg_encode; the rule: include/tilemotion.h):
    frames = torch int32 CUDA tensor [F][H][W] of 0x00RRGGBB, rows and frames at any stride -> list of F bytes objects, byte for byte what
    tm_jpeg_encode_host (and libjpeg) writes; only the files' bytes come to the host.  cap: the room given (default: F times
    jpeg_bound); guard: bytes of 0xA5 kept before and behind that room; full=True: nothing raises, and the result is a dict of rc, files
    (None when refused), buffer (guards included), offsets and guard"""
    from ._lib import jpeg_options
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 3 and (frames.shape[2] <= 1 or frames.stride(2) == 1)
    nf, h, w = frames.shape
    return _jpeg_encode(lib().tm_stage_jpeg_encode, _p(frames), frames.stride(1), frames.stride(0), nf, w, h, jpeg_options(quality, sampling, restart_rows), cap,
                        guard, full, (_stream(),))


def jpeg_encode_host(frames, quality=90, sampling="420", restart_rows=1, cap=None, guard=0, full=False):
    """jpeg_encode's host twin (tm_jpeg_encode_host), no device: frames = numpy uint32 or int32 array [F][H][W], rows and frames at any
    stride (a multiple of 4 bytes; pixels contiguous)"""
    from ._lib import jpeg_options
    assert frames.dtype in (np.uint32, np.int32) and frames.ndim == 3 and (frames.shape[2] <= 1 or frames.strides[2] == 4)
    nf, h, w = frames.shape
    return _jpeg_encode(lib().tm_jpeg_encode_host, ctypes.c_void_p(frames.ctypes.data), frames.strides[1] // 4, frames.strides[0] // 4, nf, w, h,
                        jpeg_options(quality, sampling, restart_rows), cap, guard, full, ())


def probe_gif(file):
    """What the container walk finds of one GIF file, with no device (tm_probe_gif_host): a dict of width, height, frames, uniform_delay,
    loop_count (-1: none), global_table_size, background_index, version (87 / 89), background (resolved, 0x00RRGGBB) and fps.  The walk's
    refusals raise."""
    from ._lib import GifInfoDesc
    info = GifInfoDesc()
    buf = bytes(file)
    check(lib().tm_probe_gif_host(buf, len(buf), ctypes.byref(info)))
    return {name: getattr(info, name) for name, _ in GifInfoDesc._fields_ if name != "reserved"}


def gif_frames(file):
    """The images of one GIF file, with no device (tm_gif_frames_host): a list of dicts of left, top, width, height, delay (1/100 s, as
    stored), disposal, transparent (index or -1), interlaced, table_size, local_table, min_code_size, data_off and data_bytes (the sub-block
    chain in the file, terminator included)"""
    from ._lib import GifFrameDesc
    buf = bytes(file)
    n = ctypes.c_int()
    check(lib().tm_gif_frames_host(buf, len(buf), None, 0, ctypes.byref(n)))
    out = (GifFrameDesc * max(n.value, 1))()
    check(lib().tm_gif_frames_host(buf, len(buf), out, n.value, ctypes.byref(n)))
    return [{name: getattr(out[i], name) for name, _ in GifFrameDesc._fields_ if name != "reserved"} for i in range(n.value)]


def _gif_lzw(blob, streams, guard, host):
    from ._lib import GifStreamDesc, GifStatusDesc
    blob = bytes(blob)
    n = len(streams)
    desc = (GifStreamDesc * max(n, 1))()
    at = guard
    offs = []
    for i, (src_off, src_bytes, min_code, npix) in enumerate(streams):
        desc[i] = GifStreamDesc(int(src_off), at, int(src_bytes), int(npix), int(min_code), 0)
        offs.append(at)
        at += int(npix) + guard
    total = max(at, 1)
    status = (GifStatusDesc * max(n, 1))()
    if host:
        dst = np.full(total, 0xA5, np.uint8)
        check(lib().tm_gif_lzw_streams_host(blob, len(blob), desc, n, dst.ctypes.data, total, status))
    else:
        dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        check(lib().tm_stage_gif_lzw(blob, len(blob), desc, n, _p(dst), total, status, _stream()))
    return dst, [(status[i].code, status[i].in_pos, status[i].out_n) for i in range(n)], offs


def gif_lzw(blob, streams, guard=64):
    """A batch of GIF image data decoded on the device (tm_stage_gif_lzw: k_gif_lzw, a wave per stream, one launch).  blob: bytes; streams:
    a list of (src_off, src_bytes, min_code_size, npix), the sub-block chain of each with its length bytes -> (a uint8 CUDA tensor filled
    with 0xA5 before the launch, [(code, in_pos, out_n)] per stream, [dst_off] per stream): stream i's indices start at its dst_off, with
    `guard` bytes before the first stream and behind every stream's npix."""
    return _gif_lzw(blob, streams, int(guard), False)


def gif_lzw_host(blob, streams, guard=64):
    """gif_lzw's host twin (tm_gif_lzw_streams_host), no device: the same arguments and layout, a numpy array"""
    return _gif_lzw(blob, streams, int(guard), True)


def _gif_decode(file, first, count, background, frame_px, fill, host):
    buf = bytes(file)
    info = probe_gif(buf)
    if count is None:
        count = info["frames"] - first
    px = info["width"] * info["height"]
    frame_px = px if frame_px is None else int(frame_px)
    status = (ctypes.c_int32 * max(first + count, 1))()
    bg = -1 if background is None else int(background)
    if host:
        out = np.full((max(count, 1), frame_px), fill, np.uint32)
        check(lib().tm_gif_decode_host(buf, len(buf), first, count, bg, out.ctypes.data, frame_px, status))
    else:
        out = torch.full((max(count, 1), frame_px), fill, dtype=torch.int32, device="cuda")
        check(lib().tm_stage_gif_decode(buf, len(buf), first, count, bg, _p(out), frame_px, status, _stream()))
    return out[:count, :px].reshape(count, info["height"], info["width"]), list(status[:first + count])


def gif_decode(file, first=0, count=None, background=None, frame_px=None, fill=0x5A5A5A5A):
    """Frames [first, first + count) of a GIF file in host memory decoded and composited on the device (tm_stage_gif_decode: k_gif_lzw and
    k_gif_compose per chunk of images) -> (int32 CUDA tensor [count][height][width] of 0x00RRGGBB, filled with `fill` before the call, status
    per image 0 .. first + count - 1).  background: None (the file's) or 0x00RRGGBB."""
    return _gif_decode(file, int(first), count, background, frame_px, int(fill), False)


def gif_decode_host(file, first=0, count=None, background=None, frame_px=None, fill=0x5A5A5A5A):
    """gif_decode's host twin (tm_gif_decode_host), no device: the same arguments, a numpy uint32 array"""
    return _gif_decode(file, int(first), count, background, frame_px, int(fill), True)


def _gif_stats(st):
    from ._lib import GifExportStatsDesc
    return {name: getattr(st, name) for name, _ in GifExportStatsDesc._fields_}


def gif_bound(w, h, nframes, **options):
    """An upper bound of a GIF file's size for any pixels (tm_gif_bound_host), no device; options: as gif_encode takes them"""
    from ._lib import gif_options
    opt = gif_options(**options)
    bound = ctypes.c_int64()
    check(lib().tm_gif_bound_host(int(w), int(h), int(nframes), ctypes.byref(opt), ctypes.byref(bound)))
    return bound.value


def _gif_encode(call, ptr, stride_px, frame_px, nf, w, h, fps, opt, cap, guard, full, extra_before, extra_after):
    from ._lib import GifExportStatsDesc
    if cap is None:
        bound = ctypes.c_int64()
        rc = lib().tm_gif_bound_host(w, h, max(nf, 1), ctypes.byref(opt), ctypes.byref(bound))
        if rc != 0 and not full:
            check(rc)
        cap = bound.value if rc == 0 else 4096  # (what the bound refuses the call refuses too: any room will do)
    buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
    need = ctypes.c_int64(-1)
    st = GifExportStatsDesc()
    rc = call(ptr, stride_px, frame_px, nf, w, h, float(fps), ctypes.byref(opt), *extra_before, ctypes.c_void_p(buf.ctypes.data + guard) if cap else None, cap,
              ctypes.byref(need), *extra_after(st))
    if not full:
        check(rc)
    file = buf[guard:guard + need.value].tobytes() if rc == 0 else None
    return dict(rc=rc, file=file, buffer=buf, bytes=need.value, guard=guard, stats=_gif_stats(st)) if full else file


def gif_encode(frames, fps, chunk_frames=0, cap=None, guard=0, full=False, **options):
    """RGB32 frames on the device as one animated GIF (tm_stage_gif_encode; the rule: include/tilemotion.h): frames =
    torch int32 CUDA tensor [F][H][W] of 0x00RRGGBB, rows and frames at any stride -> the file's bytes, byte for byte what
    tm_gif_encode_host writes; only file bytes come to the host.  options: colours ("auto", "exact", "quantise"), max_colours, diff,
    segment_pixels, loop, delay_cs.  chunk_frames: frames per trip through the device stages (0: the writer's own; no byte depends on
    it).  cap: the room given (default: gif_bound); guard: bytes of 0xA5 kept before and behind that room; full=True: nothing raises, and the
    result is a dict of rc, file (None when refused), buffer (guards included), bytes (the size, or the size needed), guard and stats."""
    from ._lib import gif_options
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 3 and (frames.shape[2] <= 1 or frames.stride(2) == 1)
    nf, h, w = frames.shape
    return _gif_encode(lib().tm_stage_gif_encode, _p(frames), frames.stride(1), frames.stride(0), nf, w, h, fps, gif_options(**options), cap, guard, full,
                       (int(chunk_frames),), lambda st: (ctypes.byref(st), _stream()))


def gif_encode_host(frames, fps, cap=None, guard=0, full=False, canvas=False, **options):
    """gif_encode's host twin (tm_gif_encode_host), no device: frames = numpy uint32 or int32 array [F][H][W], rows and frames at any
    stride (a multiple of 4 bytes; pixels contiguous).  canvas=True: -> (file, uint32 array [F][H][W] of what a reader shows)"""
    from ._lib import gif_options
    assert frames.dtype in (np.uint32, np.int32) and frames.ndim == 3 and (frames.shape[2] <= 1 or frames.strides[2] == 4)
    nf, h, w = frames.shape
    shown = np.zeros((max(nf, 1), h, w), np.uint32) if canvas else None
    out = _gif_encode(lib().tm_gif_encode_host, ctypes.c_void_p(frames.ctypes.data), frames.strides[1] // 4, frames.strides[0] // 4, nf, w, h, fps, gif_options(**options),
                      cap, guard, full, (), lambda st: (ctypes.c_void_p(shown.ctypes.data) if canvas else None, ctypes.byref(st)))
    return (out, shown[:nf]) if canvas else out


def webp_bound(w, h, nframes, **options):
    """An upper bound of a WebP file's size for any pixels (tm_webp_bound_host), no device; options: as webp_encode takes them"""
    from ._lib import webp_options
    opt = webp_options(**options)
    bound = ctypes.c_int64()
    check(lib().tm_webp_bound_host(int(w), int(h), int(nframes), ctypes.byref(opt), ctypes.byref(bound)))
    return bound.value


def _webp_encode(call, ptr, stride_px, frame_px, nf, w, h, fps, opt, cap, guard, full, extra_before, extra_after):
    from ._lib import WebpExportStatsDesc
    if cap is None:
        bound = ctypes.c_int64()
        rc = lib().tm_webp_bound_host(w, h, max(nf, 1), ctypes.byref(opt), ctypes.byref(bound))
        if rc != 0 and not full:
            check(rc)
        cap = bound.value if rc == 0 else 4096  # (what the bound refuses the call refuses too: any room will do)
    buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
    need = ctypes.c_int64(-1)
    st = WebpExportStatsDesc()
    rc = call(ptr, stride_px, frame_px, nf, w, h, float(fps), ctypes.byref(opt), *extra_before, ctypes.c_void_p(buf.ctypes.data + guard) if cap else None, cap,
              ctypes.byref(need), *extra_after(st))
    if not full:
        check(rc)
    file = buf[guard:guard + need.value].tobytes() if rc == 0 else None
    stats = {name: getattr(st, name) for name, _ in WebpExportStatsDesc._fields_}
    return dict(rc=rc, file=file, buffer=buf, bytes=need.value, guard=guard, stats=stats) if full else file


def webp_encode(frames, fps, chunk_frames=0, cap=None, guard=0, full=False, **options):
    """RGB32 frames on the device as one animated lossless WebP (tm_stage_webp_encode; the rule: include/tilemotion.h, DESIGN.md section
    44): frames = torch int32 CUDA tensor [F][H][W] of 0x00RRGGBB, rows and frames at any stride -> the file's bytes, byte for byte what
    tm_webp_encode_host writes; only file bytes come to the host.  options: diff, palette ("auto", "off"), lz77, segment_pixels, loop,
    duration_ms.  chunk_frames: frames per trip through the device stages (0: the writer's own; no byte depends on it).  cap: the room
    given (default: webp_bound); guard: bytes of 0xA5 kept before and behind that room; full=True: nothing raises, and the result is a dict
    of rc, file (None when refused), buffer (guards included), bytes (the size, or the size needed), guard and stats."""
    from ._lib import webp_options
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 3 and (frames.shape[2] <= 1 or frames.stride(2) == 1)
    nf, h, w = frames.shape
    return _webp_encode(lib().tm_stage_webp_encode, _p(frames), frames.stride(1), frames.stride(0), nf, w, h, fps, webp_options(**options), cap, guard, full,
                        (int(chunk_frames),), lambda st: (ctypes.byref(st), _stream()))


def webp_encode_host(frames, fps, cap=None, guard=0, full=False, canvas=False, **options):
    """webp_encode's host twin (tm_webp_encode_host), no device: frames = numpy uint32 or int32 array [F][H][W], rows and frames at any
    stride (a multiple of 4 bytes; pixels contiguous).  canvas=True: -> (file, uint32 array [F][H][W] of what a reader shows)"""
    from ._lib import webp_options
    assert frames.dtype in (np.uint32, np.int32) and frames.ndim == 3 and (frames.shape[2] <= 1 or frames.strides[2] == 4)
    nf, h, w = frames.shape
    shown = np.zeros((max(nf, 1), h, w), np.uint32) if canvas else None
    out = _webp_encode(lib().tm_webp_encode_host, ctypes.c_void_p(frames.ctypes.data), frames.strides[1] // 4, frames.strides[0] // 4, nf, w, h, fps, webp_options(**options),
                       cap, guard, full, (), lambda st: (ctypes.c_void_p(shown.ctypes.data) if canvas else None, ctypes.byref(st)))
    return (out, shown[:nf]) if canvas else out


def _gif_lzw_pack(call, ptr, n, min_code, segment_pixels, extra):
    nseg = -(-n // segment_pixels) if segment_pixels else 1
    cap = 12 * (n + n // 4094 + 3 * nseg + 1) // 8 + 8  # every segment's bound (tm_gif_out.h)
    buf = np.full(cap + 128, 0xA5, np.uint8)
    need = ctypes.c_int64(-1)
    check(call(ptr, n, int(min_code), int(segment_pixels), ctypes.c_void_p(buf.ctypes.data + 64), cap, ctypes.byref(need), *extra))
    assert (buf[:64] == 0xA5).all() and (buf[64 + need.value:] == 0xA5).all()
    return buf[64:64 + need.value].tobytes()


def gif_lzw_pack(indices, min_code, segment_pixels=0):
    """Indices on the device (a torch uint8 CUDA tensor, each below 1 << min_code) as GIF image data before sub-blocks
    (tm_stage_gif_lzw_pack: k_gif_lzw_pack, a wave per segment, and k_gif_emit) -> bytes"""
    assert indices.is_cuda and indices.dtype == torch.uint8 and indices.dim() == 1 and indices.is_contiguous()
    return _gif_lzw_pack(lib().tm_stage_gif_lzw_pack, _p(indices), indices.numel(), min_code, segment_pixels, (_stream(),))


def gif_lzw_pack_host(indices, min_code, segment_pixels=0):
    """gif_lzw_pack's host twin (tm_gif_lzw_pack_host), no device: indices = a numpy uint8 array"""
    indices = np.ascontiguousarray(indices, np.uint8).reshape(-1)
    return _gif_lzw_pack(lib().tm_gif_lzw_pack_host, ctypes.c_void_p(indices.ctypes.data), indices.size, min_code, segment_pixels, ())


def _gif_palettise(call, ptr, stride_px, w, h, opt, extra):
    table = np.zeros(256, np.uint32)
    idx = np.zeros((h, w), np.uint8)
    ncol, exact = ctypes.c_int(), ctypes.c_int()
    check(call(ptr, stride_px, w, h, ctypes.byref(opt), ctypes.c_void_p(table.ctypes.data), ctypes.byref(ncol), ctypes.byref(exact), ctypes.c_void_p(idx.ctypes.data), *extra))
    return table[:ncol.value].copy(), bool(exact.value), idx


def gif_palettise(frame, **options):
    """One RGB32 frame on the device (torch int32 CUDA tensor [H][W], rows at any stride) as a colour table and indices
    (tm_stage_gif_palettise: k_gif_colours, k_gif_hist for a frame to quantise, k_gif_map) -> (table uint32 [colours], exact, uint8 [H][W])"""
    from ._lib import gif_options
    assert frame.is_cuda and frame.dtype == torch.int32 and frame.dim() == 2 and (frame.shape[1] <= 1 or frame.stride(1) == 1)
    h, w = frame.shape
    return _gif_palettise(lib().tm_stage_gif_palettise, _p(frame), frame.stride(0), w, h, gif_options(**options), (_stream(),))


def gif_palettise_host(frame, **options):
    """gif_palettise's host twin (tm_gif_palettise_host), no device: frame = numpy uint32 or int32 array [H][W]"""
    from ._lib import gif_options
    assert frame.dtype in (np.uint32, np.int32) and frame.ndim == 2 and (frame.shape[1] <= 1 or frame.strides[1] == 4)
    h, w = frame.shape
    return _gif_palettise(lib().tm_gif_palettise_host, ctypes.c_void_p(frame.ctypes.data), frame.strides[0] // 4, w, h, gif_options(**options), ())
