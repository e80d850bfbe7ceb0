"""The JPEG writer's rule on the host (tm_jpeg_out.h through tm_jpeg_encode_host), no GPU: the host twin against the
Python restatement (tests/jpeg_out_ref.py) byte for byte, both against Pillow (libjpeg) where it is installed, the quantisers, the bound,
the refusals, strides, and the files back through the reader's host form."""
import ctypes
import functools
import io

import numpy as np
import pytest

from tests import jpeg_out_cases as C
from tests import jpeg_out_ref as R
from tiler_amd import stages
from tiler_amd._lib import JpegOptions, jpeg_options, lib

QUALITIES = (1, 50, 90, 100)
RESTARTS = (0, 1, 2)
INVAL = -1


@functools.lru_cache(maxsize=None)
def ref(name, quality, sampling, restart_rows):
    return R.encode(C.case(name), quality, sampling, restart_rows)


def twin(name, quality, sampling, restart_rows):
    return stages.jpeg_encode_host(C.rgb32(C.case(name))[None].copy(), quality, sampling, restart_rows)[0]


def test_the_cases_reach_what_they_are_there_for():
    """on the restatement alone"""
    for prop, name, sampling, q, r in C.REACHED:
        reached = ref(name, q, sampling, r)[1]
        if prop in ("ff00", "zrl", "no_eob", "dummy_right", "dummy_below"):
            assert reached[prop] >= 1, (prop, name, reached)
        elif prop == "dc_cat_11":
            assert reached["dc_cat"] == 11, reached
        elif prop == "ac_cat_10":
            assert reached["ac_cat"] == 10, reached
        elif prop == "segments_65":
            assert reached["segments"] == 65, reached
        else:
            raise AssertionError(prop)
    # flat pictures code EOB only
    reached = ref("flat_8x8", 90, "444", 0)[1]
    assert reached["ac_cat"] == 0 and reached["no_eob"] == 0 and reached["zrl"] == 0
    # no picture, at any setting of the matrix, passes the categories 8-bit samples can make
    for name, _, _ in C.cases():
        for sampling in R.SAMPLINGS:
            reached = ref(name, 100, sampling, 0)[1]
            assert reached["dc_cat"] <= 11 and reached["ac_cat"] <= 10


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_twin_equals_the_restatement(sampling):
    for name, _, _ in C.cases():
        for q in QUALITIES:
            for r in RESTARTS:
                assert twin(name, q, sampling, r) == ref(name, q, sampling, r)[0], (name, q, sampling, r)


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_both_equal_pillow(sampling):
    Image = pytest.importorskip("PIL.Image")
    for name, rgb, _ in C.cases():
        for q in QUALITIES:
            for r in RESTARTS:
                if sampling == "grey":
                    im, kw = Image.fromarray(R.y_plane(rgb), "L"), {}
                else:
                    im, kw = Image.fromarray(rgb, "RGB"), {"subsampling": {"444": 0, "422": 1, "420": 2}[sampling]}
                out = io.BytesIO()
                im.save(out, "JPEG", quality=q, restart_marker_rows=r, **kw)
                assert out.getvalue() == ref(name, q, sampling, r)[0], (name, q, sampling, r)
                assert out.getvalue() == twin(name, q, sampling, r), (name, q, sampling, r)


def test_quant_tables_equal_the_restatement_and_pillow():
    for q in range(1, 101):
        luma, chroma = stages.jpeg_quant_tables(q)
        assert (luma.tolist(), chroma.tolist()) == tuple(R.quant_tables(q)), q
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(C.case("smooth_16x16"), "RGB")
    for q in range(1, 101):
        out = io.BytesIO()
        im.save(out, "JPEG", quality=q)
        tables = Image.open(io.BytesIO(out.getvalue())).quantization
        luma, chroma = stages.jpeg_quant_tables(q)
        assert luma.tolist() == list(tables[0]) and chroma.tolist() == list(tables[1]), q  # (Pillow hands them out in natural order)


def test_every_file_decodes_and_stays_under_the_bound():
    for name, rgb, _ in C.cases():
        h, w = rgb.shape[:2]
        files, keys = [], []
        for sampling in R.SAMPLINGS:
            for q in QUALITIES:
                for r in RESTARTS:
                    f = ref(name, q, sampling, r)[0]
                    assert len(f) <= stages.jpeg_bound(w, h, q, sampling, r), (name, q, sampling, r)
                    files.append(f)
                    keys.append((name, q, sampling, r))
        _, status, _ = stages.jpeg_decode_host(files, w, h)
        assert status == [0] * len(files), [k for k, s in zip(keys, status) if s]


def test_decoded_planes_are_close_to_the_source():
    """the files hold the picture: at quality 100 and 4:4:4 every decoded sample is within 2 of the rule's plane"""
    rgb = C.case("mixed_33x49")
    f = ref("mixed_33x49", 100, "444", 1)[0]
    planes, status, layout = stages.jpeg_decode_host([f], 33, 49)
    assert status == [0]
    from tests.jpeg_cases import unpack
    got = unpack(planes, layout, 0, [(33, 49)] * 3)
    for g, want in zip(got, R.ycc(rgb)):
        assert np.abs(g.astype(np.int64) - want).max() <= 2


def test_strides_wider_than_the_picture():
    for (w, h), names in C.by_size().items():
        padded = C.stack32(names, row_pad=5, frame_pad=11)
        assert padded.strides[1] == (w + 5) * 4
        got = stages.jpeg_encode_host(padded, 90, "420", 1)
        assert got == [ref(n, 90, "420", 1)[0] for n in names], (w, h)


def _call_host(frames, stride, frame_px, nf, w, h, opt, out, cap, offs):
    L = lib()
    rc = L.tm_jpeg_encode_host(frames, stride, frame_px, nf, w, h, opt, out, cap, offs)
    return rc, L.tm_last_error().decode()


def test_refusals_name_their_reason():
    px = np.zeros((2, 4, 4), np.uint32)
    p = ctypes.c_void_p(px.ctypes.data)
    out = np.zeros(4096, np.uint8)
    o = ctypes.c_void_p(out.ctypes.data)
    offs = (ctypes.c_int64 * 3)()
    good = jpeg_options(90, "420", 1)
    ok = ctypes.byref(good)

    def refused(fragment, *args):
        rc, msg = _call_host(*args)
        assert rc == INVAL and fragment in msg and "tm_jpeg_encode_host" in msg, (fragment, rc, msg)

    refused("null options", p, 4, 16, 2, 4, 4, None, o, 4096, offs)
    for q in (0, 101, -5):
        refused("quality %d" % q, p, 4, 16, 2, 4, 4, ctypes.byref(JpegOptions(q, 0, 1)), o, 4096, offs)
    for s in (-1, 4):
        refused("unknown sampling %d" % s, p, 4, 16, 2, 4, 4, ctypes.byref(JpegOptions(90, s, 1)), o, 4096, offs)
    refused("restart_rows -1", p, 4, 16, 2, 4, 4, ctypes.byref(JpegOptions(90, 0, -1)), o, 4096, offs)
    for w, h in ((0, 4), (4, 0), (32769, 4), (4, 32769)):
        refused("a picture of %d x %d" % (w, h), p, w, w * h, 1, w, h, ok, o, 4096, offs)
    refused("restart interval", p, 32768, 32768 * 4, 0, 32768, 4, ctypes.byref(JpegOptions(90, 2, 16)), o, 4096, offs)
    refused("-1 frames", p, 4, 16, -1, 4, 4, ok, o, 4096, offs)
    refused("null frames", None, 4, 16, 1, 4, 4, ok, o, 4096, offs)
    refused("a row stride of 3", p, 3, 16, 1, 4, 4, ok, o, 4096, offs)
    refused("a frame stride of 15", p, 4, 15, 2, 4, 4, ok, o, 4096, offs)
    refused("null argument", p, 4, 16, 2, 4, 4, ok, o, 4096, None)
    refused("null argument", p, 4, 16, 2, 4, 4, ok, None, 4096, offs)
    refused("null argument", p, 4, 16, 2, 4, 4, ok, o, -1, offs)
    assert not out.any()
    # a single row has no row stride to check, a single frame no frame stride
    assert _call_host(p, 0, 0, 1, 4, 1, ok, o, 4096, offs)[0] == 0
    L = lib()
    bound = ctypes.c_int64()
    assert L.tm_jpeg_bound_host(4, 4, ok, None) == INVAL and "null argument" in L.tm_last_error().decode()
    assert L.tm_jpeg_bound_host(0, 4, ok, ctypes.byref(bound)) == INVAL and "a picture of 0 x 4" in L.tm_last_error().decode()
    assert L.tm_jpeg_bound_host(4, 4, ctypes.byref(JpegOptions(0, 0, 0)), ctypes.byref(bound)) == INVAL and "quality 0" in L.tm_last_error().decode()
    t = np.zeros(64, np.uint16)
    tp = ctypes.c_void_p(t.ctypes.data)
    assert L.tm_jpeg_quant_tables_host(0, tp, tp) == INVAL and "quality 0" in L.tm_last_error().decode()
    assert L.tm_jpeg_quant_tables_host(101, tp, tp) == INVAL and "quality 101" in L.tm_last_error().decode()
    assert L.tm_jpeg_quant_tables_host(50, None, tp) == INVAL and "null argument" in L.tm_last_error().decode()


def test_a_cap_too_small_says_what_is_needed_and_writes_nothing():
    names = C.by_size()[(17, 23)]
    frames = C.stack32(names)
    want = [ref(n, 90, "422", 2)[0] for n in names]
    need = sum(len(f) for f in want)
    for cap in (0, 1, need - 1):
        got = stages.jpeg_encode_host(frames, 90, "422", 2, cap=cap, guard=32, full=True)
        assert got["rc"] == INVAL and got["offsets"][len(names)] == need and (got["buffer"] == 0xA5).all(), cap
        assert "%d bytes needed, %d given" % (need, cap) in lib().tm_last_error().decode()
    got = stages.jpeg_encode_host(frames, 90, "422", 2, cap=need, guard=32, full=True)
    assert got["rc"] == 0 and got["files"] == want
    assert (got["buffer"][:32] == 0xA5).all() and (got["buffer"][32 + need:] == 0xA5).all()
