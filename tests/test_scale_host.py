"""The RGB32 scaling rule on the host (tm_scale_rgb32_host, tm_probe_scale_host; no GPU): bit for bit the numpy restatement's
(tests/scale_ref.py on tests/resample_ref.py) on every shape the device tests use, with both filters, with padded rows, and the probe's codes."""
import ctypes

import numpy as np
import pytest

from tests import scale_ref as ref

E_INVAL, E_UNSUPPORTED = -1, -6
PATTERN = 0x5A17C3E9


def _host(src, dst_w, dst_h, filter, src_pad=0, dst_pad=0):
    """tm_scale_rgb32_host of one frame [H][W] through buffers whose rows are src_pad / dst_pad pixels longer than the rows; the padding holds a
    pattern before and must hold it after"""
    from tiler_amd import lib
    h, w = src.shape
    sbuf = np.full((h, w + src_pad), PATTERN, np.uint32)
    sbuf[:, :w] = src
    dbuf = np.full((dst_h, dst_w + dst_pad), PATTERN, np.uint32)
    L = lib()
    rc = L.tm_scale_rgb32_host(sbuf.ctypes.data, w + src_pad, w, h, dbuf.ctypes.data, dst_w + dst_pad, dst_w, dst_h, ref.FILTERS[filter])
    assert rc == 0, L.tm_last_error()
    assert (dbuf[:, dst_w:] == PATTERN).all() and (sbuf[:, w:] == PATTERN).all() and np.array_equal(sbuf[:, :w], src)
    return dbuf[:, :dst_w]


@pytest.mark.parametrize("filter", ["lanczos", "nearest"])
@pytest.mark.parametrize("src,dst", ref.SHAPES)
def test_host_twin_is_the_restatement_bit_for_bit(src, dst, filter):
    (sw, sh), (dw, dh) = src, dst
    for name, frame in (("noise", ref.random_frames(sw * 1000 + dw, 1, sh, sw)[0]), ("edges", ref.edge_frames(2, sh, sw)[1])):
        want = ref.scale(frame, dw, dh, filter)
        assert not (want >> 24).any()
        got = _host(frame, dw, dh, filter)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, len(bad), [(int(y), int(x), hex(int(got[y, x])), hex(int(want[y, x]))) for y, x in bad[:6]])
        assert np.array_equal(_host(frame, dw, dh, filter, src_pad=3, dst_pad=5), want), (name, "padded rows")
        if src == dst:  # the identity: one tap of 16384 is left
            assert np.array_equal(got, frame & 0xFFFFFF)
        if name == "edges" and filter == "lanczos" and src != dst:  # the clamp bites at both ends
            chans = np.stack([(want >> s) & 255 for s in (16, 8, 0)])
            assert (chans == 0).any() and (chans == 255).any()


def test_probe_and_refusals():
    from tiler_amd import lib
    L = lib()
    assert L.tm_probe_scale_host(264, 136, 32, 136, ref.LANCZOS3) == E_UNSUPPORTED and b"more than 8" in L.tm_last_error()
    assert L.tm_probe_scale_host(264, 136, 264, 16, ref.LANCZOS3) == E_UNSUPPORTED
    assert L.tm_probe_scale_host(264, 136, 32, 16, ref.NEAREST) == 0
    assert L.tm_probe_scale_host(264, 136, 33, 17, ref.LANCZOS3) == 0
    for bad in ((0, 136, 33, 17), (264, 0, 33, 17), (264, 136, 0, 17), (264, 136, 33, -1)):
        assert L.tm_probe_scale_host(*bad, ref.LANCZOS3) == E_INVAL
    assert L.tm_probe_scale_host(264, 136, 33, 17, 2) == E_INVAL and L.tm_probe_scale_host(264, 136, 33, 17, -1) == E_INVAL
    for big in ((32769, 136, 32768, 136), (264, 32769, 264, 32768), (264, 136, 32769, 136), (264, 136, 264, 32769)):
        assert L.tm_probe_scale_host(*big, ref.NEAREST) == E_UNSUPPORTED
        assert L.tm_probe_scale_host(*big, ref.LANCZOS3) == E_UNSUPPORTED
    assert L.tm_probe_scale_host(32768, 32768, 32768, 32768, ref.LANCZOS3) == 0
    # the host twin refuses what the probe refuses, and bad pointers, strides and overlap, with nothing written
    src = np.zeros((24, 40), np.uint32)
    dst = np.full((60, 100), PATTERN, np.uint32)
    call = lambda *a: L.tm_scale_rgb32_host(*a)  # noqa: E731
    assert call(src.ctypes.data, 40, 40, 24, dst.ctypes.data, 100, 100, 60, 7) == E_INVAL
    assert call(src.ctypes.data, 40, 40, 24, dst.ctypes.data, 100, 4, 60, ref.LANCZOS3) == E_UNSUPPORTED
    assert call(None, 40, 40, 24, dst.ctypes.data, 100, 100, 60, ref.LANCZOS3) == E_INVAL
    assert call(src.ctypes.data, 40, 40, 24, None, 100, 100, 60, ref.LANCZOS3) == E_INVAL
    assert call(src.ctypes.data, 39, 40, 24, dst.ctypes.data, 100, 100, 60, ref.LANCZOS3) == E_INVAL
    assert call(src.ctypes.data, 40, 40, 24, dst.ctypes.data, 99, 100, 60, ref.NEAREST) == E_INVAL
    assert call(dst.ctypes.data, 100, 40, 24, dst.ctypes.data + 400 * 23, 100, 100, 30, ref.NEAREST) == E_INVAL and b"overlap" in L.tm_last_error()
    assert (dst == PATTERN).all()
