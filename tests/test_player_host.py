"""The .gtm player's host side (tm_player_probe_host, tm_player_parse_host, and tm_player_open's refusals, which are decided before any
device call): records against tests/gtm_reader.Player on the reference's own bytes and on hand-made streams that hold every item command.
No GPU needed."""
import collections
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from tests import gtm_reader, player_streams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TM_E_IO, TM_E_UNSUPPORTED = -5, -6


@pytest.fixture(scope="module")
def L():
    return ps.write_lib()


def _walk(raw, tm_w, tm_h, tile_count):
    w = gtm_reader.Player(render=False)
    w.w, w.h, w.tile_count = tm_w, tm_h, tile_count
    w.feed(raw)
    return w


def _check_records(raw, tm_w, tm_h, tile_count):
    """tm_player_parse_host's records of one key frame = what gtm_reader.Player walks; -> the walker"""
    from tiler_amd import player
    recs, intra, first = player.parse_keyframe(raw, tm_w, tm_h, tile_count)
    w = _walk(raw, tm_w, tm_h, tile_count)
    assert recs.shape == (len(w.items), tm_w * tm_h) and first.shape == (len(w.items) + 1,) and first[0] == 0
    for f, items in enumerate(w.items):
        want, want_intra = ps.expected_records(items, tm_w * tm_h)
        assert np.array_equal(recs[f].view(np.uint64), want.view(np.uint64)), f
        assert np.array_equal(intra[first[f]:first[f + 1]], want_intra), f
    assert first[-1] == intra.shape[0]
    return w, recs


def test_reference_keyframe_records(L):
    """football_cif.gtm's second key frame (verbatim reference bytes): 33 frames, the pinned per-kind item counts, every record's fields"""
    pins = json.load(open(os.path.join(GOLDEN, "gtm_demo_pins.json")))["football_cif"]
    blob = open(os.path.join(GOLDEN, "football_cif_kf1.lzma"), "rb").read()
    raw, used = ps.lz_decode(L, blob, pins["kf"][1]["raw"] + 16)
    assert used == len(blob) and len(raw) == pins["kf"][1]["raw"]
    w, recs = _check_records(raw, pins["tm_w"], pins["tm_h"], pins["tile_count"])
    assert recs.shape[0] == pins["kf1_walk"]["frames"] == 33
    hist = pins["kf1_walk"]["item_histogram"]
    assert hist == {"intra": 8188, "ps": 26581, "ss": 17503}
    fl = recs["flags"]
    got = {"intra": int(((fl & 8) != 0).sum()), "ps": int(((fl & 4) != 0).sum()), "ss": int(((fl & 12) == 0).sum())}
    assert got == hist
    assert dict(collections.Counter(it[0] for fr in w.items for it in fr)) == hist


@pytest.mark.parametrize("pal_size", [2, 64])
def test_every_command_form(L, tmp_path, pal_size):
    """a 5 x 3 tile map written by tm_write_gtm_host with > 65 536 tiles, > 1 024 palettes, use-count-1 tiles, short and long offsets, runs
    of zero offsets, both mirror flags: all seven item commands occur, and the records are gtm_reader.Player's items"""
    s = ps.write_stream(L, tmp_path / "made.gtm", 5, 3, pal_size, nframes=9, kf=(0, 4), mode="border")
    hdr, raws = ps.raw_keyframes(L, s["data"])
    assert [k["frame"] for k in hdr["kf"]] == [0, 4]
    kinds, mirrors = set(), set()
    for raw in raws:
        w, recs = _check_records(raw, 5, 3, ps.N_TILES)
        for fr in w.items:
            kinds |= {it[0] for it in fr}
            mirrors |= {it[3] for it in fr if it[0] in ("ss", "ls", "ll", "intra")}
        assert w.pal_size in (0, pal_size)
    assert kinds == ps.ITEM_KINDS, kinds  # a stream without a SkipBlock proves nothing about SkipBlocks
    assert mirrors == {0, 1, 2, 3}
    pred = s["tilemaps"][(s["tilemaps"]["Flags"] & 4) != 0]
    assert (np.abs(pred["PredictedX"].astype(int)) > 32).any() and (np.abs(pred["PredictedX"].astype(int)) < 31).any()


def _probe(path):
    from tiler_amd import player
    from tiler_amd._lib import TileMotionError
    try:
        return player.probe(path), None
    except TileMotionError as e:
        return None, e


def _open_refused(path):
    """tm_player_open of a file that must be refused: -> the error (the refusal comes before any device call, so this needs no GPU)"""
    from tiler_amd import player
    from tiler_amd._lib import TileMotionError
    with pytest.raises(TileMotionError) as ei:
        player.GtmPlayer(path).close()
    assert len(str(ei.value)) > 30  # a message, not only a code
    return ei.value


def test_probe_and_refusals(L, tmp_path):
    """the probe against gtm_reader.read_header; wrong magic, cuts of the header and of the first stream, a GTMk raw size off by one, a damaged
    stream behind an intact index, a frame that ends early: TM_E_IO or TM_E_UNSUPPORTED with a message, never a crash"""
    s = ps.write_stream(L, tmp_path / "made.gtm", 5, 3, 2, nframes=9, kf=(0, 4), mode="border", n_shared=48)  # (a small TileSet: few cuts)
    data = s["data"]
    hdr = gtm_reader.read_header(data)
    (info, kf), err = _probe(tmp_path / "made.gtm")
    assert err is None
    assert (info["width"], info["height"], info["frames"], info["keyframes"], info["encoder_version"]) == (hdr["width"], hdr["height"], hdr["frame_count"], hdr["kf_count"], hdr["version"])
    assert (info["avg_bytes_per_s"], info["kf_max_bytes_per_s"]) == (hdr["avg_bps"], hdr["kf_max_bps"])
    assert kf == hdr["kf"]

    def variant(blob, name="bad.gtm"):
        p = tmp_path / name
        p.write_bytes(blob)
        return p

    # wrong magic: a headerless stream is tm_reload_gtm's to read
    e = _open_refused(variant(data[hdr["whole"]:]))
    assert e.code == TM_E_UNSUPPORTED and "tm_reload_gtm" in str(e)
    assert _probe(variant(b"GTMx" + data[4:]))[1].code == TM_E_UNSUPPORTED
    # cut at every 97th byte of the header and of the first stream
    first_end = hdr["whole"] + hdr["kf"][0]["comp"]
    cuts = list(range(0, first_end, 97))
    assert len(cuts) > 10 and cuts[0] < hdr["whole"] < cuts[-1]
    for cut in cuts:
        p = variant(data[:cut])
        assert _probe(p)[1].code in (TM_E_IO, TM_E_UNSUPPORTED), cut
        assert _open_refused(p).code in (TM_E_IO, TM_E_UNSUPPORTED), cut
    # the same cuts of the first stream behind an index that still describes a whole file: the LZMA decoder or the command walk refuses
    s1 = ps.write_stream(L, tmp_path / "one.gtm", 5, 3, 2, nframes=4, kf=(0,), n_shared=48)
    one = s1["data"]
    h1 = gtm_reader.read_header(one)
    for cut in range(h1["whole"] + 18, len(one), 97):
        blob = bytearray(one[:cut])
        struct.pack_into("<I", blob, 40 + 20, cut - h1["whole"])
        assert _open_refused(variant(bytes(blob))).code == TM_E_IO, cut
    # a GTMk raw size off by one
    for d in (-1, 1):
        blob = bytearray(data)
        struct.pack_into("<I", blob, 40 + 16, hdr["kf"][0]["raw"] + d)
        e = _open_refused(variant(bytes(blob)))
        assert e.code == TM_E_IO and "GTMk" in str(e)
    # a frame that ends early: the first FrameEnd moved one item forward
    _, raws = ps.raw_keyframes(L, one)
    raw = raws[0]
    w = gtm_reader.Player(render=False)
    w.feed(raw)
    from tiler_amd import player
    from tiler_amd._lib import TileMotionError
    cmds = struct.pack("<H", 2 | (0 << 4)) + struct.pack("<H", 7) + struct.pack("<H", 11)  # one ShortShort, then FrameEnd
    head_end = raw.index(struct.pack("<HHH", (0 << 4) | 14, 5, 3)) + 14  # SetDimensions and its 12 operand bytes
    with pytest.raises(TileMotionError) as ei:
        player.parse_keyframe(raw[:head_end] + cmds, 5, 3, s1["n_tiles"])
    assert ei.value.code == TM_E_IO and "incomplete tile map" in str(ei.value)
    short = raw[:head_end] + cmds
    blob = bytearray(one[:h1["whole"]]) + ps.lz_encode(L, short)
    struct.pack_into("<I", blob, 40 + 16, len(short))
    struct.pack_into("<I", blob, 40 + 20, len(blob) - h1["whole"])
    e = _open_refused(variant(bytes(blob)))
    assert e.code == TM_E_IO and "incomplete tile map" in str(e)
    # a tile set beyond the declared tile count
    bad = bytearray(raw)
    struct.pack_into("<I", bad, head_end - 4, 47)  # SetDimensions' tile count, below the TileSet's last tile
    with pytest.raises(TileMotionError) as ei:
        player.parse_keyframe(bytes(bad), 5, 3, 47)
    assert ei.value.code == TM_E_IO and "tile count" in str(ei.value)

    def refile(raw_bytes):
        """`one` with its only key frame's commands replaced"""
        blob = bytearray(one[:h1["whole"]]) + ps.lz_encode(L, bytes(raw_bytes))
        struct.pack_into("<I", blob, 40 + 16, len(raw_bytes))
        struct.pack_into("<I", blob, 40 + 20, len(blob) - h1["whole"])
        return variant(bytes(blob))

    e = _open_refused(refile(bad))
    assert e.code == TM_E_IO and "tile count" in str(e)
    # a SetDimensions that is not the header's picture: two damaged bytes must not size the records (65535 x 32768 items would be 17 GB)
    for tw, th in ((6, 3), (5, 4), (65535, 32768), (65535, 65535)):
        bad = bytearray(raw)
        struct.pack_into("<HH", bad, head_end - 12, tw, th)
        e = _open_refused(refile(bad))
        assert e.code == TM_E_IO and "GTMv header" in str(e), (tw, th)
        with pytest.raises(TileMotionError) as ei:  # without a header at hand: the bound on a frame's items
            player.parse_keyframe(bytes(bad), 0 if tw > 6 else 5, 0 if tw > 6 else 3, s1["n_tiles"], sized=False)
        assert ei.value.code == TM_E_IO and ("items a frame" in str(ei.value) or "SetDimensions" in str(ei.value)), (tw, th)
    # a stream that decodes to far more than its GTMk entry says is stopped there, not decoded to its end
    big = raw[:head_end] + struct.pack("<HI", 15 | (1 << 4), 1 << 22) + bytes(1 << 22) + raw[head_end:]  # an ExtendedCommand of 4 MB
    blob = bytearray(refile(big).read_bytes())
    struct.pack_into("<I", blob, 40 + 16, len(raw))
    e = _open_refused(variant(bytes(blob)))
    assert e.code == TM_E_IO and "more than" in str(e)


def test_stream_without_a_tile_set(L, tmp_path):
    """no tile used twice: tm_write_gtm_host writes no TileSet (as SaveStream, tilingencoder.pas:5307), so nothing in the commands says how
    many colours a LoadPalette carries.  The parser takes the settings text's PaletteSize= line, and the records are gtm_reader.Player's
    items when it is given that size; without the line the stream cannot be read, and that is TM_E_IO, not a crash"""
    from tiler_amd import player
    from tiler_amd._lib import TileMotionError
    per = 15
    tm = np.zeros((5, per), ps.TMI)
    tm["TileIdx"], tm["PalIdx"] = -1, -1
    tm["Flags"] = 4
    tm["PredictedX"][1:] = (np.arange(4 * per).reshape(4, per) % 7) - 3
    tm["PredictedY"][1:] = (np.arange(4 * per).reshape(4, per) % 5) - 2
    tm["PredictedX"][3, :6] = tm["PredictedY"][3, :6] = 0  # a SkipBlock
    nxt = 0
    for f, items in ((0, range(per)), (1, (2, 9)), (2, range(per)), (4, (0, 14))):  # frame 2 opens the second key frame
        for i in items:
            tm[f, i] = (nxt, nxt % 1030, 0, 0, 0.0, nxt % 4)
            nxt += 1
    for name, settings, ok in (("with.gtm", "[Load]\r\nStartFrame=0\r\n\r\n[Dither]\r\nPaletteSize=16\r\nPaletteCount=1030\r\n", True),
                               ("without.gtm", "[Load]\r\nStartFrame=0\r\nTilePaletteSize=16\r\n", False)):
        s = ps.write_arrays(L, tmp_path / name, 5, 3, 16, tm, (0, 2), settings=settings, n_shared=0)
        hdr, raws = ps.raw_keyframes(L, s["data"])
        if not ok:
            with pytest.raises(TileMotionError) as ei:
                player.parse_keyframe(raws[0], 5, 3, s["n_tiles"])
            assert ei.value.code == TM_E_IO
            continue
        kinds = set()
        for k, raw in enumerate(raws):
            recs, intra, first = player.parse_keyframe(raw, 5, 3, s["n_tiles"])
            w = gtm_reader.Player(render=False)
            w.w, w.h, w.tile_count, w.pal_size = 5, 3, s["n_tiles"], 16
            w.feed(raw)
            assert w.tileset_ranges == [] and (len(w.palettes) == 1030) == (k == 0)
            assert recs.shape[0] == len(w.items) == (2, 3)[k]
            for f, items in enumerate(w.items):
                want, want_intra = ps.expected_records(items, per)
                assert np.array_equal(recs[f].view(np.uint64), want.view(np.uint64)), (k, f)
                assert np.array_equal(intra[first[f]:first[f + 1]], want_intra), (k, f)
                kinds |= {it[0] for it in items}
        assert kinds == {"intra", "ps", "skip"}


def test_table_without_a_single_use_tile(L, tmp_path):
    """every tile used twice or more: the whole table travels in the TileSet (SaveStream's count of reused tiles starts at 0 and stays there
    when no tile has UseCount 1, tilingencoder.pas:5296-5307, which leaves every item naming a tile the stream never carries)"""
    per = 15
    tm = np.zeros((2, per), ps.TMI)
    tm["TileIdx"] = np.arange(2 * per).reshape(2, per) % 12
    tm["PalIdx"] = np.arange(2 * per).reshape(2, per) % 5
    tm["Flags"] = np.arange(2 * per).reshape(2, per) % 4
    s = ps.write_arrays(L, tmp_path / "all_shared.gtm", 5, 3, 16, tm, (0,), n_shared=48, n_tiles=12)
    assert (s["use"] >= 2).all() and s["n_tiles"] == 12
    hdr, raws = ps.raw_keyframes(L, s["data"])
    w, recs = _check_records(raws[0], 5, 3, 12)
    assert w.tileset_ranges == [(0, 11)] and w.pal_size == 16
    assert np.array_equal(w.tiles[:12].reshape(12, 64), s["pal_px"])
    assert np.array_equal(recs["a"], tm["TileIdx"]) and not (recs["flags"] & 12).any()
