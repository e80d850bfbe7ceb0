"""Hand-made .gtm streams for the player's tests: arrays made so that tm_write_gtm_host emits every item command -- ShortShort, LongShort
(more than 65 536 tiles), LongLong (more than 1 024 palettes), Intra (use-count-1 tiles), PredictedShort / PredictedLong (offsets inside and
beyond +-31), SkipBlock (runs of >= 4 zero offsets) -- with both mirror flags, and what the player's records must be for them.
Test infrastructure (no test in here)."""
import ctypes
import os

import numpy as np

from tests import gtm_reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMI = np.dtype([("TileIdx", "<i4"), ("PalIdx", "<i4"), ("PredictedX", "i1"), ("PredictedY", "i1"), ("PSNR", "<f4"), ("Flags", "<u4")])
RECORD = np.dtype([("a", "<u4"), ("pal", "<u2"), ("flags", "u1"), ("zero", "u1")])
ITEM_KINDS = {"ss", "ls", "ll", "intra", "ps", "pl", "skip"}

N_SHARED = 65536 + 24     # tiles with UseCount 2: they go into the TileSet; the last 24 need LongShort
N_TILES = N_SHARED + 1600 # the rest have UseCount 1: they travel as Intra items
N_PAL = 1030              # palettes 1024.. need LongLong


def write_lib():
    L = ctypes.CDLL(os.path.join(ROOT, "tiler_amd", "lib", "libtilemotion.so"))
    L.tm_write_gtm_host.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.c_char_p]
    L.tm_lz_compress_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.tm_lz_decompress_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.tm_last_error.restype = ctypes.c_char_p
    return L


def tables(pal_size, n_shared=N_SHARED, seed=7):
    """tiles (61 patterns in turn, so that the 4 MB TileSet compresses at once and to little; 65 536 is no multiple of 61, so a tile index cut
    to 16 bits shows), use counts, palettes"""
    rng = np.random.default_rng(seed)
    k, j = np.mgrid[0:61, 0:64]
    v = k * 7 + j * (1 + k % 3) + (j // 8) * 5  # no pattern is its own mirror image
    patterns = ((v >> (0 if pal_size > 2 else 2)) % pal_size).astype(np.uint8)
    n_tiles = n_shared + N_TILES - N_SHARED
    t = np.arange(n_tiles)
    pal_px = patterns[t % 61].copy()
    pal_px[n_shared:] = rng.integers(0, pal_size, (n_tiles - n_shared, 64), dtype=np.uint8)  # intra tiles: each its own
    use = np.where(t < n_shared, 2, 1).astype(np.uint32)
    palettes = rng.integers(0, 1 << 24, (N_PAL, pal_size)).astype(np.int32)
    return pal_px, use, palettes


def tilemaps(tm_w, tm_h, nframes, kf, mode, n_shared=N_SHARED, seed=11):
    """mode "inside": predicted offsets keep the source block inside the picture (the JavaScript player's domain); "border": items along the
    four borders and in the corners point outward (the clamp's domain); a key frame's first frame (but frame 0) holds drawn items only"""
    rng = np.random.default_rng(seed)
    per = tm_w * tm_h
    W, H = tm_w * 8, tm_h * 8
    tm = np.zeros((nframes, per), TMI)
    tm["TileIdx"] = -1
    tm["PalIdx"] = -1
    next_intra = n_shared
    for f in range(nframes):
        drawn_only = f in kf and f > 0
        i = 0
        while i < per:
            kind = ["ss", "ls", "ll", "intra", "pred", "pred", "run"][int(rng.integers(0, 7))]
            if drawn_only and kind in ("pred", "run"):
                kind = "ss"
            if kind == "run":  # zero offsets: >= 4 in a row become a SkipBlock, fewer stay PredictedShort(0, 0)
                n = min(int(rng.choice([2, 4, 5, 9])), per - i)
                tm["Flags"][f, i:i + n] = 4
                i += n
                continue
            it = tm[f, i]
            if kind == "pred":
                ty, tx = divmod(i, tm_w)
                y, x = ty * 8, tx * 8
                lo_x, hi_x, lo_y, hi_y = max(-x, -128), min(W - 8 - x, 127), max(-y, -128), min(H - 8 - y, 127)
                if mode == "border":  # outward at the borders, anywhere else
                    lo_x, hi_x, lo_y, hi_y = -128, 127, -128, 127
                    if tx == 0: hi_x = -1           # noqa: E701
                    if tx == tm_w - 1: lo_x = 1     # noqa: E701
                    if ty == 0: hi_y = -1           # noqa: E701
                    if ty == tm_h - 1: lo_y = 1     # noqa: E701
                if rng.integers(0, 2):  # the short form where the range allows it
                    lo_x, hi_x, lo_y, hi_y = max(lo_x, -32), min(hi_x, 31), max(lo_y, -32), min(hi_y, 31)
                it["PredictedX"], it["PredictedY"] = int(rng.integers(lo_x, hi_x + 1)), int(rng.integers(lo_y, hi_y + 1))
                it["Flags"] = 4
            else:
                it["Flags"] = int(rng.integers(0, 4))
                it["PalIdx"] = int(rng.integers(1024, N_PAL)) if kind == "ll" else int(rng.integers(0, 1024))
                if kind == "intra":
                    it["TileIdx"] = next_intra
                    next_intra += 1
                    if rng.integers(0, 2):
                        it["PalIdx"] = int(rng.integers(1024, N_PAL))
                else:
                    it["TileIdx"] = int(rng.integers(n_shared - 24, n_shared)) if kind == "ls" else int(rng.integers(0, min(65536, n_shared)))
            tm[f, i] = it
            i += 1
    assert next_intra <= n_shared + N_TILES - N_SHARED
    return tm


_made = {}


def write_stream(L, path, tm_w, tm_h, pal_size, nframes=5, kf=(0, 3), mode="inside", fps=25.0, settings="[Load]\r\nInputFileName=made.y4m\r\n",
                 n_shared=N_SHARED):
    """-> dict(data, pal_px, use, palettes, tilemaps, kf); n_shared: tiles of the TileSet (the default needs LongShort); a stream is made once per process and written out again from memory"""
    key = (tm_w, tm_h, pal_size, nframes, tuple(kf), mode, fps, settings, n_shared)
    if key in _made:
        with open(path, "wb") as f:
            f.write(_made[key]["data"])
        return _made[key]
    _made[key] = _write_stream(L, path, tm_w, tm_h, pal_size, nframes, kf, mode, fps, settings, n_shared)
    return _made[key]


def _write_stream(L, path, tm_w, tm_h, pal_size, nframes, kf, mode, fps, settings, n_shared):
    return write_arrays(L, path, tm_w, tm_h, pal_size, tilemaps(tm_w, tm_h, nframes, kf, mode, n_shared), kf, fps, settings, n_shared)


def write_arrays(L, path, tm_w, tm_h, pal_size, tm, kf, fps=25.0, settings="[Load]\r\n", n_shared=N_SHARED, n_tiles=None):
    """the stream of the tile maps tm [nframes][tm_w * tm_h] over tables(pal_size, n_shared)"""
    pal_px, use, palettes = tables(pal_size, n_shared)
    if n_tiles is not None:  # (a table cut short: with n_tiles <= n_shared no tile is left that is used once)
        pal_px, use = np.ascontiguousarray(pal_px[:n_tiles]), np.ascontiguousarray(use[:n_tiles])
    nframes = tm.shape[0]
    kfa = np.ascontiguousarray(kf, np.int32)
    rc = L.tm_write_gtm_host(os.fsencode(str(path)), tm_w, tm_h, nframes, fps, kfa.ctypes.data, kfa.size, pal_px.ctypes.data, use.ctypes.data, use.size,
                             palettes.ctypes.data, palettes.shape[0], palettes.shape[1], tm.ctypes.data, settings.encode())
    assert rc == 0, L.tm_last_error()
    return dict(data=open(path, "rb").read(), pal_px=pal_px, use=use, palettes=palettes, tilemaps=tm, kf=list(kf), settings=settings, n_tiles=int(use.size))


def lz_decode(L, blob, cap):
    src = np.frombuffer(blob, np.uint8)
    dst = np.zeros(max(cap, 1), np.uint8)
    n, used = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.tm_lz_decompress_host(src.ctypes.data, src.size, dst.ctypes.data, cap, ctypes.byref(n), ctypes.byref(used))
    assert rc == 0, L.tm_last_error()
    return dst[:n.value].tobytes(), used.value


def lz_encode(L, data):
    src = np.frombuffer(data, np.uint8)
    cap = len(data) + len(data) // 4 + 64
    dst = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t()
    rc = L.tm_lz_compress_host(src.ctypes.data, src.size, dst.ctypes.data, cap, ctypes.byref(n))
    assert rc == 0, L.tm_last_error()
    return dst[:n.value].tobytes()


def raw_keyframes(L, data):
    """-> header, [decoded command bytes per key frame]"""
    hdr = gtm_reader.read_header(data)
    pos, raws = hdr["whole"], []
    for k in hdr["kf"]:
        raw, used = lz_decode(L, data[pos:pos + k["comp"]], k["raw"] + 16)
        assert used == k["comp"] and len(raw) == k["raw"]
        raws.append(raw)
        pos += k["comp"]
    return hdr, raws


def expected_records(items, per):
    """gtm_reader.Player's item tuples of one frame -> (records [per], intra [n][64])"""
    recs = np.zeros(per, RECORD)
    intra = []
    i = 0
    for it in items:
        if it[0] == "skip":
            recs["flags"][i:i + it[1]] = 4
            i += it[1]
            continue
        if it[0] in ("ss", "ls", "ll"):
            recs[i] = (it[1], it[2], it[3], 0)
        elif it[0] in ("ps", "pl"):
            recs[i] = ((it[1] & 255) | ((it[2] & 255) << 8), 0, 4, 0)
        else:
            recs[i] = (len(intra), it[2], it[3] | 8, 0)
            intra.append(np.frombuffer(it[1], np.uint8))
        i += 1
    assert i == per
    return recs, (np.stack(intra) if intra else np.zeros((0, 64), np.uint8))
