"""The match finder on the device (stages.lz_matches) against its host twin (tm_lz_matches_host) pair for pair, and the coder fed by it
(stages.lz_compress) against tm_lz_compress_host byte for byte, on the cases of tests/lz_cases.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import lz_cases  # noqa: E402
from tests.lz_cases import CASES, NAMES, PARSED  # noqa: E402

SMALL = [n for n in NAMES if n.startswith("small_")]
OTHERS = [n for n in NAMES if not n.startswith("small_")]


def _device_lists(data, first=0, count=None):
    from tiler_amd import stages
    src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    counts, pairs = stages.lz_matches(src, first, count)
    return counts.cpu().numpy(), pairs


def _same_lists(name, window):
    counts, pairs = lz_cases.expected(name)
    got_counts, got_pairs = _device_lists(CASES[name])
    assert np.array_equal(got_counts, counts), (name, window, int(np.argmax(got_counts != counts)) if got_counts.size == counts.size else -1)
    assert got_pairs.size == pairs.size
    bad = np.nonzero(got_pairs != pairs)[0]
    assert bad.size == 0, (name, window, int(bad[0]), got_pairs[bad[0]], pairs[bad[0]])


@pytest.mark.parametrize("window", [None, 4096])
@pytest.mark.parametrize("name", OTHERS)
def test_device_lists_equal_the_host_finder(monkeypatch, name, window):
    """at the default window, and at 4096 positions: window edges inside matches and inside the chain longer than 96"""
    if window:
        monkeypatch.setenv("TM_LZ_WINDOW", str(window))
    _same_lists(name, window)


@pytest.mark.parametrize("window", [None, 7])
def test_device_lists_of_every_small_size(monkeypatch, window):
    """0 .. 40 bytes over four symbols (an empty stream and a one-byte stream among them): the tail rules at n - i < 2, 3, 4"""
    if window:
        monkeypatch.setenv("TM_LZ_WINDOW", str(window))
    for name in SMALL:
        _same_lists(name, window)


def test_device_lists_of_a_range():
    """first / count inside the stream: the lists of those positions as the whole stream's"""
    name = "records"
    counts, pairs = lz_cases.expected(name)
    off = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    for first, count in ((0, 1), (5000, 12345), (len(CASES[name]) - 3, 3), (len(CASES[name]), 0)):
        c, p = _device_lists(CASES[name], first, count)
        assert np.array_equal(c, counts[first:first + count]) and np.array_equal(p, pairs[off[first]:off[first + count]]), (first, count)


@pytest.mark.parametrize("window", [None, 4096])
@pytest.mark.parametrize("name", [n for n in PARSED if not n.startswith("small_")])
def test_device_compress_equals_host_compress(monkeypatch, name, window):
    from tiler_amd import stages
    if window:
        monkeypatch.setenv("TM_LZ_WINDOW", str(window))
    assert stages.lz_compress(CASES[name]) == lz_cases.expected_stream(name)


def test_device_compress_of_every_small_size(monkeypatch):
    from tiler_amd import stages
    for window in (None, 5):
        if window:
            monkeypatch.setenv("TM_LZ_WINDOW", str(window))
        for name in SMALL:  # (the empty stream and the one-byte stream are small_00 and small_01)
            assert stages.lz_compress(CASES[name]) == lz_cases.expected_stream(name), (name, window)


def test_refusals():
    import ctypes
    from tiler_amd import lib
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(64, dtype=torch.uint8, device="cuda")
    need = ctypes.c_size_t()
    L = lib()
    assert L.tm_stage_lz_matches(src.data_ptr(), 1 << 31, 0, 1, counts.data_ptr(), None, 0, ctypes.byref(need), None) == -6  # TM_E_UNSUPPORTED, nothing read
    assert L.tm_stage_lz_matches(src.data_ptr(), 64, 60, 5, counts.data_ptr(), None, 0, ctypes.byref(need), None) == -1
    assert L.tm_stage_lz_matches(src.data_ptr(), 64, 0, 64, counts.data_ptr(), None, 0, ctypes.byref(need), None) == -1 and need.value == 62  # zeros: a pair at 1 .. 62
