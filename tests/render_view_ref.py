"""Render's views in plain numpy (the rule of include/tilemotion.h, tm_render_view): DrawTile, the Output page drawn frame after frame with a
back buffer as the Pascal does (tilingencoder.pas:3455-3736), the Input page and the Tiles page.  Pixels 0x00RRGGBB, background 0.
Test infrastructure (no test in here)."""
import functools

import numpy as np

MAGENTA, AQUA = 0x00FF00FF, 0x0000FFFF
ACTIVE, HAS_RGB, HAS_PAL, HMIR, VMIR = 1, 2, 4, 8, 16  # tm_tile_hdr.Flags


class View:
    def __init__(self, page="output", predicted=True, mirrored=True, dithered=True, gamma=None, palette=-1):
        self.page, self.predicted, self.mirrored, self.dithered, self.gamma, self.palette = page, predicted, mirrored, dithered, gamma, palette

    def kwargs(self):
        return dict(predicted=self.predicted, mirrored=self.mirrored, dithered=self.dithered, gamma=self.gamma, palette=self.palette)


@functools.lru_cache(maxsize=None)
def gamma_lut(g):
    """lut[i] = round half to even of pow(i / 255, max(0, g)) * 255, in double"""
    return np.array([round(pow(i / 255.0, max(0.0, g)) * 255.0) for i in range(256)], np.uint32)


def swap_rb(a):
    a = np.asarray(a).astype(np.uint32)
    return ((a & 0xFF) << 16) | (a & 0xFF00) | ((a >> 16) & 0xFF)


def draw_tile(view, flags, pal_px, rgb_px, pal, hmir, vmir, force_active):
    """DrawTile: one tile's [8][8] picture.  pal_px uint8 [64], rgb_px uint32 [64] 0x00BBGGRR, pal: the palette's colours or None"""
    c = np.full((8, 8), MAGENTA, np.uint32)
    if (flags & ACTIVE) or force_active:
        if pal is not None:
            if flags & HAS_PAL:
                k = pal_px.reshape(8, 8).astype(np.int64)
                inside = k < len(pal)
                c = np.where(inside, swap_rb(np.asarray(pal)[np.where(inside, k, 0)]), 0).astype(np.uint32)
        elif flags & HAS_RGB:
            c = swap_rb(rgb_px.reshape(8, 8))
    if hmir:
        c = c[:, ::-1]
    if vmir:
        c = c[::-1, :]
    if view.gamma is not None:
        lut = gamma_lut(view.gamma)
        c = (lut[(c >> 16) & 0xFF] << 16) | (lut[(c >> 8) & 0xFF] << 8) | lut[c & 0xFF]
    return c.astype(np.uint32)


def render_output(view, maps, tm_w, tm_h, pal_px, rgb_px, tile_flags, palettes):
    """every frame of the tile maps (structured array [F][tm_h*tm_w]: TileIdx, PalIdx, PredictedX, PredictedY, Flags), from frame 0 on"""
    nf, H, W = maps.shape[0], tm_h * 8, tm_w * 8
    ntiles, npal = len(tile_flags), len(palettes)
    out = np.zeros((nf, H, W), np.uint32)
    back = np.zeros((H, W), np.uint32)
    yy, xx = np.mgrid[0:8, 0:8]
    for f in range(nf):
        for i in range(tm_w * tm_h):
            it = maps[f, i]
            y0, x0 = (i // tm_w) * 8, (i % tm_w) * 8
            fl = int(it["Flags"])
            if (fl & 4) and view.predicted:
                sy = np.clip(y0 + yy + int(it["PredictedY"]), 0, H - 1)
                sx = np.clip(x0 + xx + int(it["PredictedX"]), 0, W - 1)
                out[f, y0:y0 + 8, x0:x0 + 8] = back[sy, sx]
                continue
            t, p = int(it["TileIdx"]), int(it["PalIdx"])
            if not 0 <= t < ntiles:
                continue
            pal = None
            if view.dithered:
                if view.palette < 0:
                    if not 0 <= p < npal:
                        continue
                    pal = palettes[p]
                else:
                    if p != view.palette:
                        continue
                    pal = palettes[view.palette]
            hm, vm = (fl & 1, fl & 2) if view.mirrored else (0, 0)
            out[f, y0:y0 + 8, x0:x0 + 8] = draw_tile(view, int(tile_flags[t]), pal_px[t], rgb_px[t], pal, hm, vm, True)
        back = out[f]
    return out


def render_input(view, frame_tiles, frame_flags, tm_w, tm_h):
    """frame_tiles uint32 [F][tm_h*tm_w][64] 0x00BBGGRR in their stored orientation, frame_flags [F][tm_h*tm_w] (bit 0 H, bit 1 V mirror)"""
    nf = frame_tiles.shape[0]
    out = np.zeros((nf, tm_h * 8, tm_w * 8), np.uint32)
    plain = View(gamma=view.gamma)
    for f in range(nf):
        for i in range(tm_w * tm_h):
            fl = int(frame_flags[f, i]) if view.mirrored else 0
            y0, x0 = (i // tm_w) * 8, (i % tm_w) * 8
            out[f, y0:y0 + 8, x0:x0 + 8] = draw_tile(plain, HAS_RGB, None, frame_tiles[f, i], None, fl & 1, fl & 2, True)
    return out


def tile_page_count(ntiles, tm_w, tm_h):
    return -(-ntiles // (tm_w * tm_h))


def render_tiles(view, tm_w, tm_h, pal_px, rgb_px, tile_flags, pal_idx_initial, palettes):
    """every page of the Tiles page"""
    ntiles, npal, per = len(tile_flags), len(palettes), tm_w * tm_h
    pages = tile_page_count(ntiles, tm_w, tm_h)
    out = np.full((pages, tm_h * 8, tm_w * 8), AQUA, np.uint32)
    for pg in range(pages):
        for i in range(per):
            t = i + per * pg
            if t >= ntiles:
                continue
            y0, x0 = (i // tm_w) * 8, (i % tm_w) * 8
            fl = int(tile_flags[t])
            pal = None
            if view.dithered and npal > 0:
                p = view.palette if view.palette >= 0 else max(0, int(pal_idx_initial[t]))
                if p >= npal:  # the reference would index past FPalettes: background
                    out[pg, y0:y0 + 8, x0:x0 + 8] = 0
                    continue
                pal = palettes[p]
            hm, vm = (fl & HMIR, fl & VMIR) if view.mirrored else (0, 0)
            out[pg, y0:y0 + 8, x0:x0 + 8] = draw_tile(view, fl, pal_px[t], rgb_px[t], pal, hm, vm, False)
    return out
