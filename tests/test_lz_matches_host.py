"""The LZMA coder's match finder as a function of its own (tm_lz_matches_host) and the parser on supplied lists
(tm_lz_compress_from_matches_host): host code, no GPU.  The properties are the rule's (include/tilemotion.h); the cases are tests/lz_cases.py."""
import numpy as np
import pytest

from tests import lz_cases
from tests.lz_cases import CASES, DICT, MAX_LEN, MAX_PAIRS, NAMES, PARSED


def _offsets(counts):
    off = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def _common_prefix(buf, a, b, limit):
    """equal bytes of buf[a:] and buf[b:], at most limit, for arrays of positions a > b"""
    n = np.zeros(a.size, np.int64)
    live = np.arange(a.size)
    for k in range(limit):
        live = live[n[live] == k]  # still equal so far
        live = live[a[live] + k < buf.size]
        if live.size == 0:
            break
        eq = buf[a[live] + k] == buf[b[live] + k]
        n[live[eq]] += 1
    return n


@pytest.mark.parametrize("name", NAMES)
def test_lists_obey_the_rule(name):
    data = CASES[name]
    buf = np.frombuffer(data, np.uint8)
    n = buf.size
    counts, pairs = lz_cases.expected(name)
    assert counts.size == n
    assert int(counts.max(initial=0)) <= MAX_PAIRS
    if n == 0 or pairs.size == 0:
        assert n < 2 or name.startswith("small_")
        return
    off = _offsets(counts)
    pos = np.repeat(np.arange(n, dtype=np.int64), counts)
    ln, dist = pairs["len"].astype(np.int64), pairs["dist"].astype(np.int64) + 1
    assert not pairs["zero"].any()
    cap = np.minimum(MAX_LEN, n - pos)
    assert (ln >= 2).all() and (ln <= cap).all() and (dist >= 1).all() and (dist <= pos).all() and (dist <= DICT).all()
    # lengths strictly increase inside a list
    inner = np.ones(pairs.size, bool)
    inner[off[:-1][counts > 0]] = False  # the first pair of every list
    assert (ln[1:][inner[1:]] > ln[:-1][inner[1:]]).all()
    # every pair is a real match that cannot be extended, or it sits at the cap
    real = _common_prefix(buf, pos, pos - dist, MAX_LEN)
    real = np.minimum(real, cap)
    assert np.array_equal(real, ln)
    # the first pair's distance is the nearest earlier occurrence of the two bytes (and there is no list where there is none within reach)
    key = buf[:-1].astype(np.int64) | (buf[1:].astype(np.int64) << 8)
    order = np.argsort(key, kind="stable")
    prev = np.full(n, -1, np.int64)
    same = key[order[1:]] == key[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    heads = off[:-1][counts > 0]
    hp = pos[heads]
    assert np.array_equal(hp - prev[hp], dist[heads])
    reach = (prev >= 0) & (np.arange(n) - prev <= DICT)
    reach[n - 1] = False
    assert np.array_equal(counts > 0, reach)


def test_the_cases_reach_the_corners():
    """what each built case is there for does happen in it"""
    assert int(lz_cases.expected("list90")[0].max()) > 90
    counts, pairs = lz_cases.expected("chain200")
    data = CASES["chain200"]
    q = data.rindex(b"\xa1\xb2\xc3\xd4QUERY")
    off = _offsets(counts)
    best = pairs[off[q]:off[q + 1]]
    assert 1 <= best.size and int(best["len"].max()) < 20  # the 20-byte match lies 201 chain steps back: beyond the 96 visited
    counts, pairs = lz_cases.expected(lz_cases.BIG)
    off = _offsets(counts)
    for at, again, length in ((0, DICT, 40), (200, DICT, 2), (220, DICT, 3)):  # exactly at the dictionary's reach: found
        got = pairs[off[at + again]:off[at + again + 1]]
        assert got.size and int(got["len"][-1]) == length and int(got["dist"][-1]) + 1 == DICT
    for at, again in ((100, DICT + 1), (210, DICT + 1), (230, DICT + 1)):  # one byte beyond: no list
        assert counts[at + again] == 0
    q = 400 + DICT - 50
    got = pairs[off[q]:off[q + 1]]
    assert got.size == 1 and int(got["dist"][0]) + 1 == DICT - 50 and int(got["len"][0]) == 8


@pytest.mark.parametrize("name", NAMES)
def test_windows_equal_the_whole(name):
    data = CASES[name]
    n = len(data)
    counts, pairs = lz_cases.expected(name)
    off = _offsets(counts)
    if name == lz_cases.BIG:  # (each window is a forward pass from 0: two late ones)
        windows = [(DICT - 100, 300), (n - 5000, 5000)]
    else:
        step = max(1, min(4096, n // 3 + 1))
        windows = [(f, min(step, n - f)) for f in range(0, n, step)][:6] + [(n, 0), (max(0, n - 3), min(3, n))]
    for first, count in windows:
        c, p = lz_cases.matches_host(data, first, count)
        assert np.array_equal(c, counts[first:first + count]), (first, count)
        assert np.array_equal(p, pairs[off[first]:off[first + count]]), (first, count)


@pytest.mark.parametrize("name", PARSED)
def test_parser_on_supplied_lists_writes_the_same_stream(name):
    counts, pairs = lz_cases.expected(name)
    assert lz_cases.compress_from_matches_host(CASES[name], counts, pairs) == lz_cases.expected_stream(name)


def test_refusals():
    import ctypes
    L = lz_cases.host_lib()
    src = np.frombuffer(CASES["words40"], np.uint8)
    counts = np.zeros(src.size, np.uint8)
    need = ctypes.c_size_t()
    assert L.tm_lz_matches_host(src.ctypes.data, src.size, src.size - 2, 3, counts.ctypes.data, None, 0, ctypes.byref(need)) == -1  # outside the bytes
    assert L.tm_lz_matches_host(src.ctypes.data, 1 << 31, 0, 1, counts.ctypes.data, None, 0, ctypes.byref(need)) == -6  # TM_E_UNSUPPORTED
    c, p = lz_cases.expected("words40")
    dst = np.zeros(16, np.uint8)
    out_n = ctypes.c_size_t()
    rc = L.tm_lz_compress_from_matches_host(src.ctypes.data, src.size, c.ctypes.data, p.ctypes.data, dst.ctypes.data, 16, ctypes.byref(out_n))
    assert rc == -1 and out_n.value == len(lz_cases.expected_stream("words40"))  # the capacity convention of tm_lz_compress_host
