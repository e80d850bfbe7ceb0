"""Frames delivered as YUV, the host side (no GPU): the forward colour rules of tm_rgb32_to_yuv_host against the numpy restatement
(tests/yuv_out_ref.py) and against their description over all 2^24 colours, and the checks of a destination through tm_probe_yuv_out_host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import quality_ref, yuv_clip_ref
from tests import yuv_out_ref as ref
from tests.yuv_out_ref import BT601_LIMITED, BT601_FULL, TILER, BT709_LIMITED, BT709_FULL, INTEGER_MODES, LIMITED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVAL, E_UNSUPPORTED = -1, -6

# the issue's table: rows Y, U, V; columns R, G, B
TABLE = {BT601_LIMITED: [[16829, 33039, 6416], [-9714, -19070, 28784], [28784, -24103, -4681]],
         BT601_FULL: [[19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329]],
         BT709_LIMITED: [[11966, 40254, 4064], [-6596, -22188, 28784], [28784, -26145, -2639]],
         BT709_FULL: [[13933, 46871, 4732], [-7509, -25259, 32768], [32768, -29763, -3005]]}


@pytest.fixture(scope="module")
def L():
    from tiler_amd import lib
    return lib()


@pytest.fixture(scope="module")
def colours():
    a = ref.all_colours()
    a.setflags(write=False)
    return a


def host_pixels(L, rgb, mode, depth):
    rgb = np.ascontiguousarray(rgb, np.uint32)
    out = [np.zeros(rgb.size, np.uint16) for _ in range(3)]
    rc = L.tm_rgb32_to_yuv_host(rgb.ctypes.data_as(ctypes.c_void_p), rgb.size, mode, depth, *(o.ctypes.data_as(ctypes.c_void_p) for o in out))
    assert rc == 0, L.tm_last_error()
    return out


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "tilemotion.h")).read()
    assert "TM_E_INVAL = %d" % E_INVAL in hdr and "TM_E_UNSUPPORTED = %d" % E_UNSUPPORTED in hdr


# ---- 1. the constants
@pytest.mark.parametrize("mode", INTEGER_MODES)
def test_constants_follow_from_kr_kb(L, mode):
    c = ref.int_matrix(mode)
    got = (ctypes.c_int32 * 9)()
    assert L.tm_yuv_out_matrix_host(mode, got) == 0
    assert np.array_equal(np.array(got[:]).reshape(3, 3), c)
    assert c.tolist() == TABLE[mode]
    assert c[0].sum() == int(np.rint((219.0 / 255.0 if mode in LIMITED else 1.0) * 65536)) and c[1].sum() == 0 and c[2].sum() == 0
    plain = np.rint(ref.float_matrix(mode) * 65536).astype(np.int64)
    delta = c - plain  # the correction: +1 on the U row's G for the two limited rules, otherwise nothing
    want = np.zeros((3, 3), np.int64)
    if mode in LIMITED:
        want[1, 1] = 1
    assert np.array_equal(delta, want)
    for m in (0, TILER, 6):
        assert L.tm_yuv_out_matrix_host(m, got) == E_INVAL


@pytest.mark.parametrize("mode,depth", [(m, 8) for m in INTEGER_MODES] + [(m, 10) for m in LIMITED])
def test_host_rule_is_the_restatement_over_all_colours(L, colours, mode, depth):
    got = host_pixels(L, colours, mode, depth)
    exp = ref.pixels(colours, mode, depth)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("mode,depth", [(m, 8) for m in INTEGER_MODES] + [(m, d) for m in LIMITED for d in (9, 10, 11, 12)])
def test_samples_lie_within_one_of_the_float_matrix(L, colours, mode, depth):
    got = host_pixels(L, colours, mode, depth)
    r, g, b = (c.astype(np.float64) for c in ref.channels(colours))
    m = ref.float_matrix(mode) * float(1 << (depth - 8))
    yo, co = ref.offsets(mode, depth)
    worst = 0.0
    for row, off, have in zip(m, (yo, co, co), got):
        exact = np.clip(row[0] * r + row[1] * g + row[2] * b + off, 0, (1 << depth) - 1)
        worst = max(worst, float(np.abs(have.astype(np.float64) - exact).max()))
    print("mode %d depth %d: worst distance from the float matrix %.4f" % (mode, depth, worst))
    assert worst <= 1.0


# ---- 2. grey stays grey
@pytest.mark.parametrize("mode,depth", [(m, 8) for m in INTEGER_MODES] + [(m, d) for m in LIMITED for d in (10, 12, 16)])
def test_grey_stays_grey(L, mode, depth):
    v = np.arange(256, dtype=np.uint32)
    y, u, w = host_pixels(L, v << 16 | v << 8 | v, mode, depth)
    assert np.all(u == 128 << (depth - 8)) and np.all(w == 128 << (depth - 8))
    if mode in LIMITED:
        assert y[0] == 16 << (depth - 8) and y[255] == 235 << (depth - 8)
    else:
        assert y[0] == 0 and y[255] == 255
    assert np.all(np.diff(y.astype(np.int64)) >= 0)


# ---- 3. the round trip through the input side's inverse
@pytest.mark.parametrize("mode", INTEGER_MODES)
def test_round_trip_through_the_inverse(L, colours, mode):
    y, u, v = host_pixels(L, colours, mode, 8)
    back = yuv_clip_ref.rgb_channels(y, u, v, mode)
    worst = [int(np.abs(np.asarray(b).astype(np.int64) - c).max()) for b, c in zip(back, ref.channels(colours))]
    print("mode %d: worst round-trip error R %d G %d B %d" % (mode, *worst))
    assert max(worst) <= (2 if mode in LIMITED else 1)


# ---- 4. TM_YUV_TILER is GenerateY4M's loop
def test_tiler_is_generate_y4m_over_all_colours(L, colours):
    y, u, v = host_pixels(L, colours, TILER, 8)
    ey, eu, ev = ref.tiler_pixels(colours)
    assert np.array_equal(y, ey) and np.array_equal(u, eu) and np.array_equal(v, ev)
    assert np.array_equal(y, quality_ref.luma(colours))


def test_host_seam_refusals(L):
    px = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint16)
    call = lambda mode, depth: L.tm_rgb32_to_yuv_host(px.ctypes.data_as(ctypes.c_void_p), 4, mode, depth, out.ctypes.data_as(ctypes.c_void_p), None, None)  # noqa: E731
    assert call(BT601_LIMITED, 8) == 0 and call(BT709_LIMITED, 16) == 0 and call(0, 8) == 0
    assert call(BT601_FULL, 10) == E_UNSUPPORTED and call(BT709_FULL, 9) == E_UNSUPPORTED
    assert call(TILER, 10) == E_INVAL and call(6, 8) == E_INVAL and call(-1, 8) == E_INVAL and call(1, 7) == E_INVAL and call(1, 17) == E_INVAL


# ---- 5. the destination: layout and checks
def test_struct_layout_is_the_clips(tmp_path):
    from tiler_amd.yuv_out import YuvOut
    want = dict(y=0, u=8, v=16, y_row=24, y_frame=32, u_row=40, u_frame=48, v_row=56, v_frame=64, width=72, height=76, frames=80, fps=88, chroma=96,
                samples=100, depth=104, full_range=108, memory=112)
    assert ctypes.sizeof(YuvOut) == 120
    assert {n: getattr(YuvOut, n).offset for n, _ in YuvOut._fields_} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tilemotion.h"\nint main(void) {\n  printf("%zu %zu", sizeof(tm_yuv_out), sizeof(tm_yuv_clip));\n'
                   + "".join('  printf(" %%zu %%zu", offsetof(tm_yuv_out, %s), offsetof(tm_yuv_clip, %s));\n' % (n, n) for n in want) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(t) for t in subprocess.check_output([str(exe)], text=True).split()] == [120, 120] + [o for o in want.values() for _ in range(2)]


W, H = 17, 9
CW, CH = 9, 5


def good(layout="420jpeg", memory=0):
    from tiler_amd.yuv_out import YuvOut
    chroma, samples, depth, pairs = ref.LAYOUTS[layout]
    b = 1 if samples == ref.U8 else 2
    d = YuvOut()
    d.y, d.u, d.v = 0x10000, (0x20000 if chroma != ref.MONO else 0), (0x30000 if chroma != ref.MONO and not pairs else 0)
    cw = W if chroma == ref.C444 else CW
    ch = CH if chroma in (ref.C420JPEG, ref.C420MPEG2) else H
    d.y_row, d.y_frame = W * b, W * b * H
    d.u_row, d.u_frame = cw * b * (2 if pairs else 1), cw * b * (2 if pairs else 1) * ch
    d.v_row, d.v_frame = cw * b, cw * b * ch
    d.width, d.height, d.frames, d.fps = W, H, 3, 0.0
    d.chroma, d.samples, d.depth, d.full_range, d.memory = chroma, samples, depth, 0, memory
    return d


def probe(L, d, mode=0, w=W, h=H):
    return L.tm_probe_yuv_out_host(ctypes.byref(d) if d is not None else None, w, h, mode)


@pytest.mark.parametrize("layout", sorted(ref.LAYOUTS))
def test_probe_accepts_every_layout(L, layout):
    for memory in (0, 1):
        assert probe(L, good(layout, memory), BT601_LIMITED) == 0
        assert probe(L, good(layout, memory), BT709_LIMITED) == 0
        assert probe(L, good(layout, memory), 0) == 0


def test_probe_takes_odd_byte_addresses_and_padding(L):
    d = good("420jpeg")
    d.y, d.u, d.v = 0x10001, 0x20003, 0x30005
    d.y_row, d.u_row, d.v_row = W + 3, CW + 1, CW + 7
    d.y_frame, d.u_frame, d.v_frame = (W + 3) * H + 5, 0, (CW + 7) * CH + 1
    assert probe(L, d, BT601_FULL) == 0


def test_probe_refusals(L):
    def bad(change, mode=BT601_LIMITED, layout="420jpeg", w=W, h=H):
        d = good(layout)
        change(d)
        return probe(L, d, mode, w, h)

    def setter(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    assert probe(L, None) == E_INVAL                                         # a null struct
    assert bad(setter(y=0)) == E_INVAL                                       # ... or y
    assert bad(setter(u=0, v=0)) == E_INVAL                                  # chroma missing for a layout that has it
    assert bad(setter(u=0)) == E_INVAL                                       # v without u
    assert bad(setter(u=0, v=0), layout="nv12") == E_INVAL
    assert bad(setter(u=0, v=0), layout="mono") == 0                         # (mono has none)
    assert bad(setter(width=W + 1)) == E_INVAL and bad(setter(height=H - 1)) == E_INVAL   # a size that differs from the frames'
    assert bad(setter(), w=W - 1) == E_INVAL and bad(setter(), h=H + 1) == E_INVAL
    assert bad(setter(frames=0)) == E_INVAL
    for field in ("chroma", "samples", "memory"):                           # unknown enum values
        assert bad(setter(**{field: -1})) == E_INVAL and bad(setter(**{field: 5 if field == "chroma" else 3 if field == "samples" else 2})) == E_INVAL
    assert bad(setter(), mode=-1) == E_INVAL and bad(setter(), mode=6) == E_INVAL
    assert bad(setter(depth=10)) == E_INVAL and bad(setter(depth=7)) == E_INVAL            # a depth that does not fit the sample type
    assert bad(setter(depth=8), layout="p010") == E_INVAL and bad(setter(depth=17), layout="p010") == E_INVAL
    assert bad(setter(depth=9), layout="p010") == 0 and bad(setter(depth=16), layout="420p10") == 0
    assert bad(setter(y_row=W - 1)) == E_INVAL and bad(setter(u_row=CW - 1)) == E_INVAL and bad(setter(v_row=CW - 1)) == E_INVAL   # a row stride shorter than the row
    assert bad(setter(u_row=2 * CW - 1), layout="nv12") == E_INVAL           # (interleaved rows are twice as long)
    assert bad(setter(u_row=4 * CW - 2), layout="p010") == E_INVAL
    assert bad(setter(y_row=2 * W - 2), layout="420p10") == E_INVAL
    assert bad(setter(y=0x10001), layout="p010") == E_INVAL and bad(setter(u=0x20001), layout="p010") == E_INVAL           # odd pointers or strides with words
    assert bad(setter(y_row=2 * W + 1), layout="420p10") == E_INVAL and bad(setter(v_frame=2 * CW * CH + 1), layout="420p10") == E_INVAL
    assert bad(setter(v=0x30001), layout="420p10") == E_INVAL
    assert bad(setter(y_frame=-1)) == E_INVAL and bad(setter(u_frame=-2)) == E_INVAL and bad(setter(v_frame=-16)) == E_INVAL   # negative frame strides
    # the mode refusals
    for layout in ("p010", "420p10"):
        assert bad(setter(), mode=BT601_FULL, layout=layout) == E_UNSUPPORTED and bad(setter(), mode=BT709_FULL, layout=layout) == E_UNSUPPORTED
        assert bad(setter(full_range=1), mode=0, layout=layout) == E_UNSUPPORTED     # AUTO: BT601_FULL when full_range is set
        assert bad(setter(full_range=0), mode=0, layout=layout) == 0
    assert bad(setter(), mode=TILER, layout="444") == 0 and bad(setter(), mode=TILER, layout="mono") == 0
    for layout in ("422", "420jpeg", "420mpeg2", "nv12", "p010", "420p10"):
        assert bad(setter(), mode=TILER, layout=layout) == E_INVAL
    assert bad(setter(samples=1, depth=10, y_row=2 * W, u_row=2 * W, v_row=2 * W), mode=TILER, layout="444") == E_INVAL


def test_python_layout_names():
    from tiler_amd import yuv_out
    for name in ("444", "422", "420", "420mpeg2", "mono", "nv12", "p010"):
        assert yuv_out.layout_of(name) == ref.LAYOUTS["420jpeg" if name == "420" else name]
    assert yuv_out.layout_of((2, 1, 10, False)) == ref.LAYOUTS["420p10"]
    assert yuv_out.plane_shapes("nv12", 3, 9, 17) == ((3, 9, 17), (3, 5, 18), None)
    assert yuv_out.plane_shapes("422", 2, 9, 17) == ((2, 9, 17), (2, 9, 9), (2, 9, 9))
    assert yuv_out.plane_shapes("mono", 1, 9, 17) == ((1, 9, 17), None, None)
    with pytest.raises(ValueError):
        yuv_out.layout_of("411")
    with pytest.raises(ValueError):
        yuv_out.mode_of("bt2020")
    y, u, v = yuv_out.alloc("p010", 2, 9, 17)
    assert y.dtype == np.uint16 and u.shape == (2, 5, 18) and v is None
    d = yuv_out.descriptor((y, u, v), "p010")
    assert (d.y_row, d.y_frame, d.u_row, d.u_frame, d.frames, d.memory, d.samples, d.depth) == (34, 34 * 9, 36, 36 * 5, 2, 0, 2, 10)
    assert (d.width, d.height) == (17, 9)
    yuv_out.probe(d, 17, 9, yuv="bt709-limited")
    from tiler_amd._lib import TileMotionError
    with pytest.raises(TileMotionError) as ei:
        yuv_out.probe(d, 17, 10)
    assert ei.value.code == E_INVAL
    with pytest.raises(ValueError):  # a chroma plane too small for the layout never reaches the library
        yuv_out.descriptor((y, u[:, :4], None), "p010")
    with pytest.raises(ValueError):
        yuv_out.descriptor((y, u[:, :, :17], None), "p010")
