"""Render's other views on the device (tm_render_view_frames / RenderView, tm_render_tile_pages / RenderTilePages, tm_stage_render_view /
stages.render_view): every switch against the numpy restatement of the rule (tests/render_view_ref.py), bit for bit -- on hand-made tables
through the stage seam, and on a small panning clip with motion prediction through the encoder.  The stage seam takes no first frame: the
range that starts inside a chain (first = 2) goes through the encoder."""
import itertools

import numpy as np
import pytest

from tests import gtm_reader, render_view_ref as ref
from tests import player_streams as ps

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TMI = np.dtype([("TileIdx", "<i4"), ("PalIdx", "<i4"), ("PredictedX", "i1"), ("PredictedY", "i1"), ("PSNR", "<f4"), ("Flags", "<u4")])
GAMMA = 0.6


def _tables(tm_w, tm_h, nframes, ntiles, npal, pal_size, seed):
    """tiles of every kind and tile maps with out-of-range indices, random predicted items and two corner chains"""
    rng = np.random.default_rng(seed)
    per = tm_w * tm_h
    pal_px = rng.integers(0, 16, (ntiles, 64)).astype(np.uint8)  # (with pal_size 5: indices at and above the palette size)
    pal_px[0] %= pal_size  # (tile 0, where the corner chain lands, shows colours)
    rgb_px = rng.integers(0, 1 << 24, (ntiles, 64)).astype(np.uint32)
    flags = (ref.ACTIVE | ref.HAS_RGB | ref.HAS_PAL | (rng.integers(0, 4, ntiles) << 3)).astype(np.uint32)
    for t in (3, 11):
        if t < ntiles:
            flags[t] &= ~np.uint32(ref.HAS_RGB)
    for t in (5, 17):
        if t < ntiles:
            flags[t] &= ~np.uint32(ref.HAS_PAL)
    if ntiles > 7:
        flags[7] &= ~np.uint32(ref.ACTIVE)
    initial = rng.integers(-1, npal, ntiles).astype(np.int32)
    if ntiles > 20:
        initial[20] = npal + 2  # beyond the palettes: background on the Tiles page
    palettes = rng.integers(0, 1 << 24, (npal, pal_size)).astype(np.int32)
    tm = np.zeros((nframes, per), TMI)
    tm["TileIdx"] = rng.integers(0, ntiles, (nframes, per))
    tm["PalIdx"] = rng.integers(0, npal, (nframes, per))
    tm["Flags"] = rng.integers(0, 4, (nframes, per))
    if per > 8:
        tm["TileIdx"][0, :min(per, ntiles)] = rng.permutation(ntiles)[:min(per, ntiles)]  # frame 0 shows many kinds of tiles
        for k, t in enumerate((3, 5, 7, 11)):
            tm["TileIdx"][0, 1 + k] = t
        tm["TileIdx"][0, 6], tm["TileIdx"][1, 6] = -1, ntiles          # tiles out of range
        tm["PalIdx"][0, 7], tm["PalIdx"][1, 7] = -1, npal              # palettes out of range
        for f in range(1, nframes):                                    # random predicted items; offsets reach across items and edges
            for i in rng.choice(per, per // 3, replace=False):
                tm["Flags"][f, i] |= 4
                tm["PredictedX"][f, i], tm["PredictedY"][f, i] = rng.integers(-9, 10), rng.integers(-9, 10)
        tm["Flags"][0, 9] |= 4                                         # predicted in frame 0: reads before the clip
        tm["PredictedX"][0, 9] = 3
        # a chain three frames deep in the top-left corner, clamped at the left and the top edge, that lands on an item of palette 1 (which
        # the filters 0 and 2 skip); its twin in the bottom-right corner lands on palette 0
        for corner, (ox, oy), pal in ((0, (-3, -5), 1), (per - 1, (6, 4), 0)):
            tm[0, corner] = (corner % ntiles, pal, 0, 0, 0.0, 1)
            for f in range(1, nframes):
                tm[f, corner] = (0, 0, ox, oy, 0.0, 4)
    else:  # a single item: drawn, then predicted onto itself with offsets that clamp everywhere
        tm[0, 0] = (1, 1, 0, 0, 0.0, 2)
        for f in range(1, nframes):
            tm[f, 0] = (0, 0, -2, 3, 0.0, 4)
    return dict(pal_px=pal_px, rgb_px=rgb_px, flags=flags, initial=initial, palettes=palettes, maps=tm)


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def _stage(tb, tm_w, tm_h, **kw):
    from tiler_amd import stages
    m = tb["maps"]
    if "dev" not in tb:
        tb["dev"] = dict(tile=_cuda(m["TileIdx"], np.int32), pal=_cuda(m["PalIdx"], np.int32), fl=_cuda(m["Flags"] & 7, np.uint8),
                         px=_cuda(m["PredictedX"], np.int8), py=_cuda(m["PredictedY"], np.int8), pal_px=_cuda(tb["pal_px"], np.uint8),
                         rgb=_cuda(tb["rgb_px"].view(np.int32), np.int32), tf=_cuda(tb["flags"].view(np.int32), np.int32),
                         ini=_cuda(tb["initial"], np.int32), pals=_cuda(tb["palettes"], np.int32))
    d = tb["dev"]
    out = stages.render_view(d["tile"], d["pal"], d["fl"], d["px"], d["py"], tm_w, tm_h, d["pal_px"], d["rgb"], d["tf"], d["ini"], d["pals"], **kw)
    return out.cpu().numpy().view(np.uint32)


def _want(tb, tm_w, tm_h, view):
    if view.page == "tiles":
        return ref.render_tiles(view, tm_w, tm_h, tb["pal_px"], tb["rgb_px"], tb["flags"], tb["initial"], tb["palettes"])
    return ref.render_output(view, tb["maps"], tm_w, tm_h, tb["pal_px"], tb["rgb_px"], tb["flags"], tb["palettes"])


SWEEP = [ref.View(page, bool(p), bool(m), bool(d), GAMMA if g else None, pal)
         for page in ("output", "tiles") for p, m, d, g in itertools.product((1, 0), repeat=4) for pal in (-1, 0, 2)]


@pytest.mark.parametrize("pal_size", [16, 5])
def test_stage_seam_every_switch(pal_size):
    """5 x 3 tile map, 4 frames, 23 tiles (page 1: 8 tiles and 7 aqua cells), 3 palettes: all 16 combinations of predicted / mirrored /
    dithered / use_gamma, times palette_index -1, 0, 2, times pages OUTPUT and TILES, bit for bit against the numpy reference"""
    tm_w, tm_h = 5, 3
    tb = _tables(tm_w, tm_h, 4, 23, 3, pal_size, seed=20261019 + pal_size)
    pred = (tb["maps"]["Flags"] >> 2) & 1
    assert pred[1:, 0].all() and pred[1:, 14].all() and not pred[0, 0]
    seen = {}
    for v in SWEEP:
        got = _stage(tb, tm_w, tm_h, page=v.page, **v.kwargs())
        want = _want(tb, tm_w, tm_h, v)
        assert got.shape == want.shape == ((2 if v.page == "tiles" else 4), 24, 40)
        assert np.array_equal(got, want), vars(v)
        seen[(v.page, v.predicted, v.mirrored, v.dithered, v.gamma, v.palette)] = want
    # the cases really differ: each switch changes the Output page, the chain in the corner shows the filter, page 1 ends in aqua
    base = seen[("output", True, True, True, None, -1)]
    for key in (("output", False, True, True, None, -1), ("output", True, False, True, None, -1), ("output", True, True, False, None, -1),
                ("output", True, True, True, GAMMA, -1), ("output", True, True, True, None, 0), ("output", True, True, True, None, 2)):
        assert not np.array_equal(seen[key], base), key
    assert (seen[("output", True, True, True, None, 0)][3, :3, :3] == 0).all() and (base[3, :3, :3] != 0).any()  # landed on a skipped item
    assert (base[0, 8:16, 32:40] == 0).all()  # the item predicted in frame 0
    page1 = seen[("tiles", True, True, True, None, -1)][1]
    assert (page1[8:, 24:] == ref.AQUA).all() and (page1[16:, :] == ref.AQUA).all() and (page1[:8] != ref.AQUA).any()
    assert (seen[("tiles", True, True, False, None, -1)][0, 8:16, 16:24] == ref.MAGENTA).all()  # tile 7 is inactive
    # default switches: the stage render's frames
    from tiler_amd import stages
    d = tb["dev"]
    plain = stages.render(d["tile"], d["pal"], d["fl"], d["px"], d["py"], tm_w, tm_h, d["pal_px"], d["pals"]).cpu().numpy().view(np.uint32)
    if pal_size == 16:  # (tm_stage_render ignores HasPalPixels: equal where every tile has palette pixels)
        tb["dev"]["tf"] = _cuda((tb["flags"] | ref.HAS_PAL).view(np.int32), np.int32)
        assert np.array_equal(_stage(tb, tm_w, tm_h), plain)


def test_stage_seam_one_item():
    """a 1 x 1 tile map: one group of pixels per row pair, chains that clamp on every side; and the seam's refusals"""
    from tiler_amd._lib import TileMotionError
    tb = _tables(1, 1, 3, 2, 2, 16, seed=5)
    for v in SWEEP:
        if v.palette == 2:
            continue
        got = _stage(tb, 1, 1, page=v.page, **v.kwargs())
        assert np.array_equal(got, _want(tb, 1, 1, v)), vars(v)
    for kw in (dict(palette=2), dict(page="input"), dict(gamma=float("nan")), dict(page="tiles", pages=3)):
        with pytest.raises(TileMotionError) as ei:
            _stage(tb, 1, 1, **kw)
        assert ei.value.code == -1, kw


def _pan_clip(nf, w, h, every):
    """a smooth textured scene that moves one pixel to the left every `every` frames"""
    y, x = np.mgrid[0:h, 0:w + nf].astype(np.int64)
    r = (128 + 90 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.int64)
    g = (128 + 80 * np.cos(x / 17.0 + y / 11.0)).astype(np.int64)
    b = (x * 2 + y) % 256
    img = (0xFF << 24) | (np.clip(r, 0, 255) << 16) | (np.clip(g, 0, 255) << 8) | b
    return np.stack([img[:, f // every:f // every + w] for f in range(nf)]).astype(np.uint32)


NF, W, H = 10, 64, 48
SETTINGS = dict(PaletteCount=3, GlobalTilingTileCount=100, MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=False, ShotTransMaxSecondsPerKF=1000.0,
                ShotTransMinSecondsPerKF=1000.0)


def _encoder(devices=None, **settings):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    if devices is not None:
        enc.SetDevices(devices)
    enc.LoadDefaultSettings()
    for k, v in {**SETTINGS, **settings}.items():
        setattr(enc, k, v)
    enc.SetVideo(W, H, 24.0, NF)
    frames = _pan_clip(NF, W, H, 2)
    for f in range(NF):
        enc.PushFrame(f, frames[f])
    return enc, frames


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """the encoded pan clip, its tables read back, and the .gtm it saved"""
    out = str(tmp_path_factory.mktemp("view") / "pan.gtm")
    enc, frames = _encoder(OutputFileName=out)
    enc.Run()
    c = enc.counts()
    hdr, pal_px, rgb = enc.Tiles()
    maps = enc.TileMaps()
    assert ((maps["Flags"] >> 2) & 1)[2:].any(), "no predicted items"
    yield dict(enc=enc, frames=frames, c=c, hdr=hdr, pal_px=pal_px, rgb=rgb, maps=maps, palettes=enc.Palettes(), gtm=out)
    enc.close()


VIEWS = [dict(predicted=False), dict(mirrored=False), dict(dithered=False), dict(gamma=GAMMA), dict(palette=1), dict(palette=0, predicted=False),
         dict(gamma=2.2, palette=2, mirrored=False), dict(dithered=False, gamma=0.0, predicted=False, mirrored=False), dict(dithered=False, palette=1)]


def test_encoder_default_view_is_render_frames(clip):
    """RenderView() = RenderFrames(), page input = RenderFrames(input=True), for the clip and for a range that starts inside a chain; host and
    device destinations agree"""
    enc = clip["enc"]
    out, src = enc.RenderFrames(device=False), enc.RenderFrames(input=True, device=False)
    assert np.array_equal(enc.RenderView(), out)
    assert np.array_equal(enc.RenderView(page="input"), src)
    assert np.array_equal(enc.RenderView(2, 5), out[2:7]) and np.array_equal(enc.RenderView(2, 5, page="input"), src[2:7])
    assert np.array_equal(enc.RenderView(device=True).cpu().numpy().view(np.uint32), out)
    assert np.array_equal(enc.RenderView(page="input", device=True).cpu().numpy().view(np.uint32), src)
    assert enc.RenderView(3, 0).shape == (0, H, W)


@pytest.mark.parametrize("kw", VIEWS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_encoder_views_against_the_reference(clip, kw):
    """every non-default view = the numpy reference fed with Tiles(), TileMaps() and Palettes() read back: frames, a range from frame 2,
    the tile pages; host and device destinations agree"""
    enc, c = clip["enc"], clip["c"]
    v = ref.View(**kw)
    want = ref.render_output(v, clip["maps"], c["tm_w"], c["tm_h"], clip["pal_px"], clip["rgb"], clip["hdr"]["Flags"], clip["palettes"])
    got = enc.RenderView(**kw)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, enc.RenderFrames(device=False))
    assert np.array_equal(enc.RenderView(2, 3, **kw), want[2:5])
    assert np.array_equal(enc.RenderView(device=True, **kw).cpu().numpy().view(np.uint32), want)
    tkw = {k: x for k, x in kw.items() if k != "predicted"}
    pages = ref.render_tiles(ref.View("tiles", **tkw), c["tm_w"], c["tm_h"], clip["pal_px"], clip["rgb"], clip["hdr"]["Flags"],
                             clip["hdr"]["PalIdx_Initial"], clip["palettes"])
    assert np.array_equal(enc.RenderTilePages(**tkw), pages)
    assert np.array_equal(enc.RenderTilePages(1, 1, device=True, **tkw).cpu().numpy().view(np.uint32), pages[1:2])


def test_encoder_tile_pages_and_input_page(clip):
    """TilePageCount = ceil(tiles / items); the last page ends in aqua; the Input page with mirrored=False shows the stored frame tiles,
    with gamma the reference's table"""
    from tiler_amd import stages
    enc, c = clip["enc"], clip["c"]
    per = c["tm_w"] * c["tm_h"]
    assert c["tiles"] > per and enc.TilePageCount() == -(-c["tiles"] // per)
    pages = enc.RenderTilePages()
    assert pages.shape == (enc.TilePageCount(), H, W)
    assert np.array_equal(pages, ref.render_tiles(ref.View("tiles"), c["tm_w"], c["tm_h"], clip["pal_px"], clip["rgb"], clip["hdr"]["Flags"],
                                                  clip["hdr"]["PalIdx_Initial"], clip["palettes"]))
    if c["tiles"] % per:
        assert (pages[-1, -8:, -8:] == ref.AQUA).all()
    tiles, flags, _ = stages.load(torch.from_numpy(clip["frames"].view(np.int32)).cuda(), c["tm_w"], c["tm_h"])
    tiles = (tiles.cpu().numpy().view(np.uint32) & 0xFFFFFF).reshape(NF, per, 64)
    flags = flags.cpu().numpy().reshape(NF, per)
    assert flags.any()
    stored = ref.render_input(ref.View(mirrored=False), tiles, flags, c["tm_w"], c["tm_h"])
    assert np.array_equal(enc.RenderView(page="input", mirrored=False), stored)
    assert not np.array_equal(stored, enc.RenderFrames(input=True, device=False))
    for kw in (dict(gamma=GAMMA), dict(gamma=2.2, mirrored=False), dict(predicted=False, dithered=False, palette=1)):  # (the last: ignored switches)
        assert np.array_equal(enc.RenderView(page="input", **kw), ref.render_input(ref.View(**kw), tiles, flags, c["tm_w"], c["tm_h"])), kw


def test_reloaded_stream_has_no_rgb_pixels(clip):
    """after ReloadGTM the tiles carry no RGB pixels: the undithered view is magenta on drawn items (through gamma: the table's magenta), the
    dithered one is the player's frames of the file (gtm_reader.Player) and the encoder's own output"""
    from tiler_amd.encoder import TilingEncoder
    enc, c = clip["enc"], clip["c"]
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.SetVideo(W, H, 24.0, NF)
    fresh.ReloadGTM(clip["gtm"])
    L = ps.write_lib()
    _, raws = ps.raw_keyframes(L, open(clip["gtm"], "rb").read())
    pl = gtm_reader.Player()
    for raw in raws:
        pl.feed(raw)
    dithered = fresh.RenderView()
    assert len(pl.frames) == NF
    for f in range(NF):
        assert np.array_equal(dithered[f], ref.swap_rb(np.asarray(pl.frames[f]) & 0xFFFFFF)), f
    assert np.array_equal(dithered, enc.RenderFrames(device=False))
    maps = fresh.TileMaps()
    drawn = np.repeat(np.repeat((maps["TileIdx"] >= 0).reshape(NF, c["tm_h"], c["tm_w"]), 8, 1), 8, 2)
    assert drawn.any()
    assert np.array_equal(fresh.RenderView(dithered=False, predicted=False), np.where(drawn, ref.MAGENTA, 0))
    lut = ref.gamma_lut(GAMMA)
    mg = (int(lut[255]) << 16) | (int(lut[0]) << 8) | int(lut[255])
    assert np.array_equal(fresh.RenderView(dithered=False, predicted=False, gamma=GAMMA), np.where(drawn, mg, 0))
    und = fresh.RenderView(dithered=False)
    assert set(np.unique(und).tolist()) <= {0, ref.MAGENTA}
    assert fresh.TilePageCount() == -(-fresh.counts()["tiles"] // (c["tm_w"] * c["tm_h"]))
    pg = fresh.RenderTilePages(dithered=False)
    assert set(np.unique(pg).tolist()) <= {ref.MAGENTA, ref.AQUA}
    hdr, pal_px, rgb = fresh.Tiles()
    flags = hdr["Flags"] & ~np.uint32(ref.HAS_RGB)
    assert np.array_equal(fresh.RenderTilePages(), ref.render_tiles(ref.View("tiles"), c["tm_w"], c["tm_h"], pal_px, rgb, flags, hdr["PalIdx_Initial"],
                                                                    fresh.Palettes()))
    fresh.close()


def test_refusals_leave_the_buffer_untouched(clip):
    """before Reduce, a page range out of bounds, a palette out of range, the Tiles page through the frames call, a frame range out of
    bounds: TM_E_INVAL, and a poisoned output buffer keeps every byte"""
    import ctypes
    from tiler_amd._lib import render_view_desc
    enc, c = clip["enc"], clip["c"]
    L, h = enc._L, ctypes.c_void_p(enc._h)
    npages = enc.TilePageCount()
    host = np.full((2, H, W), 0x5A5A5A5A, np.uint32)
    dev = torch.full((2, H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    calls = [(L.tm_render_view_frames, render_view_desc("tiles"), 0, 2), (L.tm_render_view_frames, render_view_desc(palette=3), 0, 2),
             (L.tm_render_view_frames, render_view_desc(7), 0, 2), (L.tm_render_view_frames, render_view_desc(gamma=float("nan")), 0, 2),
             (L.tm_render_view_frames, render_view_desc(), NF - 1, 2), (L.tm_render_view_frames, render_view_desc(), -1, 2),
             (L.tm_render_tile_pages, render_view_desc("tiles"), npages - 1, 2), (L.tm_render_tile_pages, render_view_desc("tiles"), -1, 1),
             (L.tm_render_tile_pages, render_view_desc("tiles", palette=3), 0, 1), (L.tm_render_view_frames, None, 0, 2)]
    for fn, view, first, count in calls:
        ptr = None if view is None else ctypes.byref(view)
        assert fn(h, ptr, first, count, host.ctypes.data_as(ctypes.c_void_p), 0) == -1
        assert fn(h, ptr, first, count, ctypes.c_void_p(dev.data_ptr()), 1) == -1
    # an encoder that has loaded but not reduced: no tiles yet, no output yet
    early, _ = _encoder()
    early.Run(0)
    eh = ctypes.c_void_p(early._h)
    n = ctypes.c_int(-7)
    assert L.tm_get_tile_page_count(eh, ctypes.byref(n)) == -1 and n.value == -7
    for fn, view in ((L.tm_render_tile_pages, render_view_desc("tiles")), (L.tm_render_view_frames, render_view_desc())):
        assert fn(eh, ctypes.byref(view), 0, 1, host.ctypes.data_as(ctypes.c_void_p), 0) == -1
        assert fn(eh, ctypes.byref(view), 0, 1, ctypes.c_void_p(dev.data_ptr()), 1) == -1
    assert np.array_equal(early.RenderView(page="input"), early.RenderFrames(input=True, device=False))  # (the Input page needs Load only)
    early.close()
    torch.cuda.synchronize()
    assert (host == 0x5A5A5A5A).all() and int((dev != 0x5A5A5A5A).sum()) == 0


def test_device_group_reads_shard_0(clip):
    """two shards on one device: the views and the tile pages are the single encoder's; after a sharded Load (motion prediction off) an Input
    range that shard 0 did not load is refused"""
    from tiler_amd._lib import TileMotionError
    one = clip["enc"]
    enc, _ = _encoder([0, 0])
    enc.Run()
    assert np.array_equal(enc.TileMaps(), clip["maps"])
    for kw in (dict(), dict(predicted=False, gamma=GAMMA), dict(dithered=False, mirrored=False), dict(palette=1)):
        assert np.array_equal(enc.RenderView(**kw), one.RenderView(**kw)), kw
        assert np.array_equal(enc.RenderView(device=True, **kw).cpu().numpy(), one.RenderView(device=True, **kw).cpu().numpy()), kw
        tkw = {k: x for k, x in kw.items() if k != "predicted"}
        assert np.array_equal(enc.RenderTilePages(**tkw), one.RenderTilePages(**tkw)), kw
    assert enc.TilePageCount() == one.TilePageCount()
    assert np.array_equal(enc.RenderView(1, 3, page="input", mirrored=False), one.RenderView(1, 3, page="input", mirrored=False))
    enc.close()
    # motion prediction off: Load is sharded, shard 0 holds the source of the first half of the clip only
    enc, _ = _encoder([0, 0], MotionPredictRadius=0)
    enc.Run()
    src = enc.RenderFrames(input=True, device=False)  # (gathered from both shards)
    assert np.array_equal(enc.RenderView(1, 3, page="input"), src[1:4])
    assert np.array_equal(enc.RenderView(), enc.RenderFrames(device=False))
    with pytest.raises(TileMotionError) as ei:
        enc.RenderView(NF - 2, 2, page="input")
    assert ei.value.code == -1
    enc.close()


def test_tile_sheet_tool(clip, tmp_path):
    """tools/tile_sheet.py writes the reloaded stream's tile pages and its palette strip"""
    import json
    import os
    import subprocess
    import sys
    from tiler_amd.encoder import TilingEncoder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output([sys.executable, os.path.join(root, "tools", "tile_sheet.py"), clip["gtm"], str(tmp_path / "sheet_%d.png"), "--palette", "1",
                                   "--pages", "1:2"], text=True)
    info = json.loads(out.strip().splitlines()[-1])
    c = clip["c"]
    assert info["pages"] == -(-info["tiles"] // (c["tm_w"] * c["tm_h"])) and len(info["written"]) == 2 and info["page_size"] == [W, H]
    fresh = TilingEncoder()
    fresh.LoadDefaultSettings()
    fresh.SetVideo(W, H, 24.0, NF)
    fresh.ReloadGTM(clip["gtm"])
    want = fresh.RenderTilePages(1, 1, palette=1)[0]
    pals = fresh.Palettes()
    fresh.close()

    def read(path, h, w):
        if path.endswith(".rgb"):
            px = np.fromfile(path, np.uint8).reshape(h, w, 3).astype(np.uint32)
        else:
            from PIL import Image
            px = np.asarray(Image.open(path).convert("RGB")).astype(np.uint32)
        return (px[:, :, 0] << 16) | (px[:, :, 1] << 8) | px[:, :, 2]

    assert os.path.basename(info["written"][0]).startswith("sheet_1.")
    assert np.array_equal(read(info["written"][0], H, W), want)
    assert np.array_equal(read(info["written"][1], pals.shape[0], pals.shape[1]), ref.swap_rb(pals))
