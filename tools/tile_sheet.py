"""The tile sheet of a .gtm stream -- Render's Tiles page (tilingencoder.pas:3678-3707) and its palette strip (FPaletteBitmap, 3659-3676):
python tools/tile_sheet.py IN.gtm OUT_%d.png [--palette N] [--no-mirror] [--gamma G] [--pages A:B]

The stream's header is probed on the host (tm_player_probe_host), the video is described to an encoder, ReloadGTM brings tiles, palettes
and tile maps, and the pages are drawn on the device (RenderTilePages): page p is a picture of the frame's size whose cell (sy, sx) shows
tile tm_w*sy + sx + tm_w*tm_h*p, aqua beyond the last tile.  --palette N shows every tile through palette N (default: a reloaded tile has
no first palette of its own, so palette 0); --no-mirror drops the tiles' initial mirror flags (a stream's tiles carry none); --gamma G
applies Render's gamma table; --pages A:B writes pages A .. B-1 (default: all).  OUT_%d.png takes the page number; the palette strip --
[palettes][pal_size] pixels, one row a palette -- goes to OUT_palettes.png (the name with %d replaced).  Written through Pillow where it
imports, as raw RGB24 (.rgb, size in the printed line) otherwise."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tiler_amd import player  # noqa: E402
from tiler_amd.encoder import TilingEncoder  # noqa: E402


def rgb24(img):
    """0x00RRGGBB [h][w] -> uint8 [h][w][3]"""
    img = np.asarray(img, np.uint32)
    return np.stack([(img >> 16) & 0xFF, (img >> 8) & 0xFF, img & 0xFF], axis=-1).astype(np.uint8)


def write_picture(path, img):
    """-> the name written: `path` through Pillow, or path with .rgb (raw RGB24) where Pillow does not import"""
    px = rgb24(img)
    try:
        from PIL import Image
    except ImportError:
        path = os.path.splitext(path)[0] + ".rgb"
        px.tofile(path)
        return path
    Image.fromarray(px, "RGB").save(path)
    return path


def palette_strip(palettes):
    """FPaletteBitmap: [palettes][pal_size], SwapRB of PaletteRGB (0x00BBGGRR -> 0x00RRGGBB)"""
    p = np.asarray(palettes).astype(np.uint32)
    return ((p & 0xFF) << 16) | (p & 0xFF00) | ((p >> 16) & 0xFF)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output", help="page pictures, with %%d for the page number")
    ap.add_argument("--palette", type=int, default=-1)
    ap.add_argument("--no-mirror", action="store_true")
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--pages", default=None, help="A:B")
    a = ap.parse_args()
    if "%d" not in a.output:
        ap.error("the output name needs %d for the page number")
    info, _ = player.probe(a.input)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.SetVideo(info["width"], info["height"], info["fps"], info["frames"])
    enc.ReloadGTM(a.input)
    pages = enc.TilePageCount()
    first, end = 0, pages
    if a.pages:
        try:
            first, end = (int(v) if v else d for v, d in zip(a.pages.split(":"), (0, pages)))
        except ValueError:
            ap.error("--pages takes A:B")
    pics = enc.RenderTilePages(first, end - first, mirrored=not a.no_mirror, gamma=a.gamma, palette=a.palette)
    names = [write_picture(a.output % (first + i), pics[i]) for i in range(pics.shape[0])]
    strip = palette_strip(enc.Palettes())
    names.append(write_picture(a.output.replace("%d", "palettes"), strip))
    c = enc.counts()
    print(json.dumps(dict(tiles=c["tiles"], pages=pages, written=names, page_size=[c["tm_w"] * 8, c["tm_h"] * 8], palette_strip=list(strip.shape[::-1]))))
    enc.close()


if __name__ == "__main__":
    main()
