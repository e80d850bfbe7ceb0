"""Render's views, the host side (no GPU): tm_render_view's layout and defaults, the gamma table, the probe's refusals, and the numpy
reference of the rule (tests/render_view_ref.py) against the player-semantics renderer the render tests use."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import gtm_reader, render_view_ref as ref
from tests import player_streams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TM_E_INVAL = -1


@pytest.fixture(scope="module")
def L():
    from tiler_amd._lib import lib
    lib_ = lib()
    lib_.tm_last_error.restype = ctypes.c_char_p
    return lib_


def test_view_layout_as_the_c_compiler_sees_it(tmp_path):
    """sizeof and offsetof of tm_render_view from a C program, against the header's comment and the ctypes mirror"""
    from tiler_amd._lib import RenderViewDesc
    want = dict(page=0, predicted=4, mirrored=8, dithered=12, use_gamma=16, palette_index=20, gamma=24)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tilemotion.h"\nint main(void) {\n  printf("%zu", sizeof(tm_render_view));\n'
                   + "".join('  printf(" %%zu", offsetof(tm_render_view, %s));\n' % n for n in want)
                   + '  printf(" %d %d %d", TM_RENDER_PAGE_INPUT, TM_RENDER_PAGE_OUTPUT, TM_RENDER_PAGE_TILES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(t) for t in subprocess.check_output([str(exe)], text=True).split()] == [32] + list(want.values()) + [0, 1, 2]
    assert ctypes.sizeof(RenderViewDesc) == 32
    assert {n: getattr(RenderViewDesc, n).offset for n in want} == want


def test_default_view(L):
    """tm_render_view_default: the constructor's switches (tilingencoder.pas:5495-5509); the Python keywords build the same struct"""
    from tiler_amd._lib import RenderViewDesc, render_view_desc
    v = RenderViewDesc(9, 9, 9, 9, 9, 9, 9.0)
    assert L.tm_render_view_default(ctypes.byref(v)) == 0
    got = (v.page, v.predicted, v.mirrored, v.dithered, v.use_gamma, v.palette_index, v.gamma)
    assert got == (1, 1, 1, 1, 0, -1, 0.6)
    assert bytes(render_view_desc()) == bytes(v)
    assert L.tm_render_view_default(None) == TM_E_INVAL


@pytest.mark.parametrize("g", [0.0, 0.6, 1.0, 2.2, -1.0])
def test_gamma_table(L, g):
    """lut[i] = round(pow(i / 255, max(0, g)) * 255), half to even, in double; identity at 1, 255 everywhere at 0 (and at a clamped -1)"""
    lut = np.zeros(256, np.uint8)
    assert L.tm_render_gamma_lut_host(g, lut.ctypes.data_as(ctypes.c_void_p)) == 0
    want = [round(pow(i / 255.0, max(0.0, g)) * 255.0) for i in range(256)]
    assert lut.tolist() == want
    assert np.array_equal(ref.gamma_lut(g), lut)
    if g == 1.0:
        assert lut.tolist() == list(range(256))
    if g <= 0.0:
        assert (lut == 255).all()
    if g == 0.6:
        assert lut[0] == 0 and lut[255] == 255 and (np.diff(lut.astype(int)) >= 0).all() and lut[64] > 64


def test_gamma_table_refusals(L):
    lut = np.full(256, 7, np.uint8)
    assert L.tm_render_gamma_lut_host(float("nan"), lut.ctypes.data_as(ctypes.c_void_p)) == TM_E_INVAL
    assert (lut == 7).all()
    assert L.tm_render_gamma_lut_host(1.0, None) == TM_E_INVAL


def test_probe_refusals(L):
    """a null struct, an unknown page, a NaN gamma and palette_index >= pal_count are TM_E_INVAL with a message; a negative gamma is not"""
    from tiler_amd._lib import render_view_desc
    probe = L.tm_probe_render_view_host
    assert probe(None, 4) == TM_E_INVAL and b"null" in L.tm_last_error()
    for page in (0, 1, 2):
        assert probe(render_view_desc(page), 4) == 0
    for page in (-1, 3, 77):
        assert probe(render_view_desc(page), 4) == TM_E_INVAL and b"page" in L.tm_last_error()
    assert probe(render_view_desc(gamma=float("nan")), 4) == TM_E_INVAL and b"gamma" in L.tm_last_error()
    v = render_view_desc()
    v.gamma = float("nan")  # refused with gamma off too: the struct is checked, not its use
    assert probe(v, 4) == TM_E_INVAL
    for g in (-1.0, -1e300, 0.0, 1e300, float("inf")):
        assert probe(render_view_desc(gamma=g), 4) == 0, g
    for pal, count, ok in ((-1, 0, True), (-5, 4, True), (0, 4, True), (3, 4, True), (4, 4, False), (0, 0, False), (1 << 30, 4, False)):
        rc = probe(render_view_desc(palette=pal), count)
        assert rc == (0 if ok else TM_E_INVAL), (pal, count)
        if not ok:
            assert b"palette" in L.tm_last_error()
    with pytest.raises(ValueError):
        render_view_desc("sideways")


def test_reference_with_default_switches_is_the_player(tmp_path):
    """the numpy reference under the default view = gtm_reader.Player's frames (R and B swapped) of a hand-made stream with predicted
    chains, both mirror flags, use-count-1 tiles and more than 1 024 palettes"""
    tm_w, tm_h, pal_size = 6, 4, 16
    L = ps.write_lib()
    s = ps.write_stream(L, tmp_path / "made.gtm", tm_w, tm_h, pal_size, nframes=6, kf=(0, 4), mode="inside", n_shared=48)
    maps = s["tilemaps"]
    pred = (maps["Flags"] >> 2) & 1
    assert pred[1].any() and pred[2].any() and pred[3].any() and not pred[4].any()  # chains up to three frames deep
    _, raws = ps.raw_keyframes(L, s["data"])
    pl = gtm_reader.Player()
    for raw in raws:
        pl.feed(raw)
    nt = s["pal_px"].shape[0]
    flags = np.full(nt, ref.ACTIVE | ref.HAS_PAL, np.uint32)  # what a stream's tiles carry: no RGB pixels
    rgb = np.zeros((nt, 64), np.uint32)
    got = ref.render_output(ref.View(), maps, tm_w, tm_h, s["pal_px"], rgb, flags, s["palettes"])
    assert len(pl.frames) == got.shape[0] == 6
    for f in range(6):
        assert np.array_equal(got[f], ref.swap_rb(np.asarray(pl.frames[f]) & 0xFFFFFF)), f
    # and the reference's other switches change what they should: undithered tiles without RGB pixels are magenta where drawn
    und = ref.render_output(ref.View(dithered=False, predicted=False), maps, tm_w, tm_h, s["pal_px"], rgb, flags, s["palettes"])
    drawn = np.repeat(np.repeat((maps["TileIdx"] >= 0).reshape(6, tm_h, tm_w), 8, 1), 8, 2)
    assert np.array_equal(und, np.where(drawn, ref.MAGENTA, 0))
