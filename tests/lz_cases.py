"""Inputs shared by the match-finder tests (tests/test_lz_matches_host.py, tests/test_gpu_lz_matches.py): seeded, each the smallest at which
the finder's rule (include/tilemotion.h, tm_lz_matches_host) can still go wrong, and the host library's answers to them, computed once."""
import ctypes
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LZ_PAIR = np.dtype([("len", "<u2"), ("zero", "<u2"), ("dist", "<u4")])  # tm_lz_pair
DICT, DEPTH, MAX_LEN, MAX_PAIRS = 1 << 22, 96, 273, 98

BIG = "far_4m"  # the one case whose parse is skipped for time


def host_lib():
    from tiler_amd import lib
    L = lib()
    L.tm_lz_compress_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.tm_lz_decompress_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.tm_last_error.restype = ctypes.c_char_p
    return L


def compress_host(data):
    L = host_lib()
    src = np.frombuffer(data, np.uint8)
    cap = len(data) + len(data) // 4 + 64
    dst = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t()
    rc = L.tm_lz_compress_host(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, cap, ctypes.byref(n))
    assert rc == 0, L.tm_last_error()
    return dst[:n.value].tobytes()


def decompress_host(blob, cap):
    L = host_lib()
    L.tm_lz_decompress_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    src = np.frombuffer(blob, np.uint8)
    dst = np.zeros(max(cap, 1), np.uint8)
    n = ctypes.c_size_t()
    rc = L.tm_lz_decompress_host(src.ctypes.data, src.size, dst.ctypes.data, cap, ctypes.byref(n), None)
    assert rc == 0, L.tm_last_error()
    return dst[:n.value].tobytes()


def matches_host(data, first=0, count=None):
    """tm_lz_matches_host -> (counts uint8 [count], pairs LZ_PAIR [sum])"""
    L = host_lib()
    src = np.frombuffer(data, np.uint8)
    count = len(data) - first if count is None else count
    counts = np.zeros(max(count, 1), np.uint8)
    need = ctypes.c_size_t()
    rc = L.tm_lz_matches_host(src.ctypes.data if src.size else None, src.size, first, count, counts.ctypes.data, None, 0, ctypes.byref(need))
    pairs = np.zeros(need.value, LZ_PAIR)
    if need.value:
        assert rc == -1  # TM_E_INVAL: the room asked for
        rc = L.tm_lz_matches_host(src.ctypes.data, src.size, first, count, counts.ctypes.data, pairs.ctypes.data, pairs.size, ctypes.byref(need))
    assert rc == 0, L.tm_last_error()
    assert need.value == pairs.size == int(counts[:count].sum())
    return counts[:count], pairs


def compress_from_matches_host(data, counts, pairs):
    L = host_lib()
    src = np.frombuffer(data, np.uint8)
    counts = np.ascontiguousarray(counts, np.uint8)
    pairs = np.ascontiguousarray(pairs)
    cap = len(data) + len(data) // 4 + 64
    dst = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t()
    rc = L.tm_lz_compress_from_matches_host(src.ctypes.data if src.size else None, src.size, counts.ctypes.data if counts.size else None,
                                            pairs.ctypes.data if pairs.size else None, dst.ctypes.data, cap, ctypes.byref(n))
    assert rc == 0, L.tm_last_error()
    return dst[:n.value].tobytes()


def _cases():
    rng = np.random.default_rng(11)
    c = {}
    # every small size over four symbols: the tail rules at n - i < 2, 3, 4
    for n in range(0, 41):
        c["small_%02d" % n] = bytes(rng.integers(0, 4, n, dtype=np.uint8))
    # the structures of the parser's fuzz (tests/test_gtm.py), restated
    rec = rng.integers(0, 256, 24, dtype=np.uint8)
    recs = np.tile(rec, (4000, 1))
    recs[:, 5] = rng.integers(0, 4, 4000)
    recs[::17, 11] = rng.integers(0, 256, recs[::17].shape[0])
    c["records"] = recs.tobytes()  # one changing field
    a, b = rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), rng.integers(0, 256, 900, dtype=np.uint8).tobytes()
    c["repeats"] = (a + b) * 3 + a * 2 + b + a[:300] + b[:129] + a[:128] + b[:127] + a[:274] + b[:273] + a[:272]  # past 128 and past 273
    c["runs"] = b"".join(bytes([i & 255]) * int(rng.integers(1, 9000)) for i in range(40))
    c["words40"] = rng.integers(0, 40, 30000).astype("<u2").tobytes()
    for n in (4095, 4096, 4097, 8191, 8193):
        c["ab_%d" % n] = (b"ab" * n)[:n] + bytes(rng.integers(0, 256, 50, dtype=np.uint8))
    # real command bytes: the reference's own key frame
    blob = open(os.path.join(GOLDEN, "football_cif_kf1.lzma"), "rb").read()
    c["football"] = decompress_host(blob, 680024 + 16)
    assert len(c["football"]) == 680024
    # a chain longer than the 96 visited: one 4-byte prefix 200 times with different continuations, then a query that matches the OLDEST best
    pre = b"\xa1\xb2\xc3\xd4"
    body = b"".join(pre + bytes([200 + (k & 31), k & 255, (k * 7) & 255]) + bytes(rng.integers(0, 256, 9, dtype=np.uint8)) for k in range(200))
    c["chain200"] = pre + b"QUERYTAIL0123456" + body + pre + b"QUERYTAIL0123456" + bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    # a list with more than 90 pairs: the nearest candidate matches least, every chain step sets a record
    x = bytes(rng.integers(0, 256, 120, dtype=np.uint8))
    blocks = b"".join(x[:m] + bytes([0xF0 | (m & 7), 0xEE ^ (m & 0xff)]) for m in range(100, 3, -1))
    c["list90"] = blocks + x
    # candidates just inside and just beyond the dictionary: a pattern at the start, again after 4 MiB of noise
    # (the noise holds bytes below 200 only and the patterns bytes from 200 up, so a pattern's only earlier occurrences are the planted ones)
    far = bytearray(rng.integers(0, 200, (4 << 20) + 8192, dtype=np.uint8).tobytes())
    fresh = iter(range(200, 256))

    def plant(length, at, again):  # `length` bytes nobody else holds at `at`, and once more `again` bytes further on
        p = bytes(next(fresh) for _ in range(min(length, 4))) + bytes(rng.integers(200, 256, max(0, length - 4), dtype=np.uint8))
        far[at:at + length] = p
        far[at + again:at + again + length] = p
        return p

    plant(40, 0, DICT)        # a long match at exactly the dictionary's reach
    plant(40, 100, DICT + 1)  # ... and one byte beyond it
    plant(2, 200, DICT)       # the 2-byte candidate alone, inside and beyond
    plant(2, 210, DICT + 1)
    plant(3, 220, DICT)       # the 3-byte candidate
    plant(3, 230, DICT + 1)
    p = plant(8, 300, 100)    # a chain whose nearest candidate is inside and whose next one is beyond: the walk stops there
    far[400 + DICT - 50:400 + DICT - 50 + 8] = p
    c[BIG] = bytes(far)
    return c


CASES = _cases()
NAMES = sorted(CASES)
PARSED = [n for n in NAMES if n != BIG]  # the cases whose streams are compared too


@functools.lru_cache(maxsize=None)
def expected(name):
    """the host finder's lists of a whole case: (counts, pairs), read-only"""
    counts, pairs = matches_host(CASES[name])
    counts.setflags(write=False)
    pairs.setflags(write=False)
    return counts, pairs


@functools.lru_cache(maxsize=None)
def expected_stream(name):
    return compress_host(CASES[name])
