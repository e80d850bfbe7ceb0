"""Equal distances are settled by original index INSIDE the scan: a query's best is (d'' + 1) << 32 | original index, every row
that reaches or ties it arrives at the epilogue's 64-bit atomic minimum, and a tile's rows stand in ascending original index, so the lowest
of a lane's winning rows is its lowest index.  No pass behind the scan looks at ties any more; these cases put them wherever the scan has a
seam, and compare EVERY query's index and error with an exact scan on the device (fp64 matmul on integer-valued doubles, lowest index
among equals, as tests/test_gpu_knn_epilogue.py does).  Every case runs with the defaults, with TM_KNN_FIRST_CHUNK=0, with
TM_KNN_LIST_ORDER=0 and in the dense mode (TM_KNN_NOPRUNE=1).

Two kinds of data.  `cloud`: every row within +-1 of one base row on a few columns, as in test_gpu_knn_epilogue.py -- distances take a handful
of values, most queries' nearest rows tie; `narrow` makes the library double the database digits (TD = true, plan <0, 0>), `wide` (64 far
rows on each side) keeps them plain (plan <1, 1>); the plan is asserted.  `spread`: bases far from each other (six box columns of falling
width, forty more at +-600), so that the only rows near a query are the ones planted for it and where they lie on the curve is known:
  twice-*          every row present twice, at i and i + nt / 2.  Copies are neighbours on the curve (stable sort: the lower index first), so
                   the tie sits in one tile or, every thirtieth pair or so, straddles two with the lower index in the earlier one.
  mirror-low-first the two rows at b - 1000 e and b + 1000 e of query b, e the widest column: the halves of that column are the halves of the
  mirror-low-last  curve, the tie spans two tiles far apart; the lower original index is in the earlier tile / in the later one (asserted from
                   the index's row order).
  pairs            2 363 rows, each twice at unrelated indices (and 37 single ones): where the tile's index order puts the two copies is asserted from the row
                   order -- pairs in one half-wave (several bits of the epilogue's mask) and pairs at rows r and r + 4 (the same register of
                   the two half-waves).
  three            a third row at the same distance that keeps the query's curve key (its offset lies on box columns that are no curve
                   columns): it stands next to the query on the curve, among the seed kernel's eight tiles for the queries near their
                   group's home, while the mirrored two reach the query through the lists: the hand-over through gbest.  Which of the
                   three has the lowest index is random (asserted: each kind wins for a third of the queries).
  parities         per base four rows at SSD s - 1, s - 1, s and s + 1 (s = 3..8) of the base: equal chain values with different row-norm
                   parities; queries on the bases and one step off them (both query-norm parities).
  identical-*      900 copies of one row at random indices of a cloud.
  tiny-*           nt = 1, 31, 33 with a query equal to the last row: the padding copies of the last tile carry that row's index."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODES = {"defaults": {}, "no-first-chunk": {"TM_KNN_FIRST_CHUNK": "0"}, "run-order": {"TM_KNN_LIST_ORDER": "0"}, "dense": {"TM_KNN_NOPRUNE": "1"}}
KNOBS = ("TM_KNN_FIRST_CHUNK", "TM_KNN_LIST_ORDER", "TM_KNN_NOPRUNE")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases' arrays are read-only)


def _brute(q, db):
    """exact nearest row by (SSD, lowest index): every product and sum of the fp64 matmul is exact"""
    dq, dd = _dev(q).to(torch.float64), _dev(db).to(torch.float64)
    nd = (dd * dd).sum(1)
    idx, err, ties = [], [], []
    for a in range(0, q.shape[0], 2048):
        x = dq[a:a + 2048]
        d = (x * x).sum(1)[:, None] + nd[None, :] - 2.0 * (x @ dd.T)
        e = d.min(dim=1).values
        hit = d == e[:, None]
        idx.append(hit.to(torch.uint8).argmax(dim=1).cpu().numpy())  # first maximum = lowest index
        err.append(e.cpu().numpy())
        ties.append((hit.sum(1) > 1).cpu().numpy())
    return np.concatenate(idx).astype(np.int32), np.concatenate(err).astype(np.uint64).astype(np.uint32), np.concatenate(ties)


def _cloud(rng, base, perm, n, cols):
    rows = np.tile(base, (n, 1))
    rows[:, perm[:cols]] += rng.integers(-1, 2, size=(n, cols))
    return rows


def _widen(rng, base, perm, rows):
    """the last 64 rows become far ones that set the column ranges: 27 two-digit columns, 10 whose doubled values would need a second digit"""
    far = perm[10:47]
    n = rows.shape[0]
    sel = np.arange(n - 64, n)
    rows[np.ix_(sel, far[:27])] = base[far[:27]] + rng.integers(-400, 401, size=(64, 27))
    rows[np.ix_(sel, far[27:])] = base[far[27:]] + rng.integers(-100, 101, size=(64, 10))
    rows[n - 1, far[:27]] = base[far[:27]] + 400
    rows[n - 2, far[:27]] = base[far[:27]] - 400
    rows[n - 1, far[27:]] = base[far[27:]] + 100
    rows[n - 2, far[27:]] = base[far[27:]] - 100


def _cloud_case(seed, kind, wide):
    rng = np.random.default_rng(seed)
    base = rng.integers(-30, 31, size=192).astype(np.int32)
    perm = rng.permutation(192)
    if kind == "twice":
        x = _cloud(rng, base, perm, 2400, 6)
        db = np.concatenate([x, x])
        q = _cloud(rng, base, perm, 4097, 8)
        q[:200] = x[rng.permutation(2400)[:200]]
    elif kind == "identical":
        db = _cloud(rng, base, perm, 3000, 6)
        src = db[17].copy()
        src[perm[9]] += 1  # a row of its own: no cloud row equals it
        db[rng.permutation(3000 - 64)[:900]] = src
        q = _cloud(rng, base, perm, 1000, 8)
        q[0] = src
        q[1] = src
        q[1, perm[8]] += 1
    else:  # tiny: kind = the number of database rows
        db = _cloud(rng, base, perm, int(kind), 6)
        q = _cloud(rng, base, perm, 33, 8)
        q[0] = db[-1]
    if wide:
        _widen(rng, base, perm, db)
        _widen(rng, base, perm, q)
    return db.astype(np.int16), q.astype(np.int16), {"plan": (1, 1, 0) if wide else (0, 0, 0)}


# half ranges of the bases on the six box columns.  A mirrored pair widens the first to 1990, and its two halves never meet; `three` adds 600
# and 800 to the fourth and fifth, which stay narrower than the three curve columns and wider than the forty columns at +-600.
WIDTHS = (990, 1100, 1050, 400, 400, 700)


def _bases(rng, nb):
    b = np.zeros((nb, 192), np.int32)
    cols = rng.permutation(192)
    for d, w in enumerate(WIDTHS):
        b[:, cols[d]] = rng.integers(-w, w + 1, size=nb)
    b[:, cols[6:46]] = rng.integers(-600, 601, size=(nb, 40))
    return b, cols


def _spread_case(seed, kind):
    rng = np.random.default_rng(seed)
    info = {}
    if kind in ("mirror-low-first", "mirror-low-last", "three"):
        nb = 1600 if kind == "three" else 2400
        b, cols = _bases(rng, nb)
        lo, hi = b.copy(), b.copy()
        lo[:, cols[0]] -= 1000
        hi[:, cols[0]] += 1000
        parts = [lo, hi] if kind != "mirror-low-last" else [hi, lo]
        if kind == "three":
            near = b.copy()
            near[:, cols[3]] += 600  # 600^2 + 800^2 = 1000^2, on box columns that are no curve columns: the row keeps the query's curve key
            near[:, cols[4]] += 800
            parts.append(near)
        db = np.concatenate(parts)
        if kind == "three":  # which of a base's three rows has the lowest index is random
            sh = np.argsort(rng.random((3, nb)), axis=0)
            db = db.reshape(3, nb, 192)[sh, np.arange(nb)[None, :]].reshape(3 * nb, 192)
            info["kind0"] = sh[0]  # which of the three (0 / 1: the mirrored two, 2: the one beside the query) holds the base's lowest index
        q = b[:2000].copy()
        info["nb"] = nb
    elif kind == "pairs":
        b, cols = _bases(rng, 2400)
        npair = 2363  # (the last 37 bases stand alone: without them every pair would sit at an even place of the curve order and none straddle two tiles)
        at = rng.permutation(2400 + npair)
        db = np.empty((2400 + npair, 192), np.int32)
        db[at[:2400]] = b
        db[at[2400:]] = b[:npair]
        q = np.concatenate([b[:1200], b[1200:2400]])
        q[1200:, cols[60]] += 1
        info["pair_a"], info["pair_b"] = np.minimum(at[:npair], at[2400:]), np.maximum(at[:npair], at[2400:])
    else:  # parities
        nb = 1200
        b, cols = _bases(rng, nb)

        def offset(ssd):  # a vector of that squared length on columns the bases leave at 0: fours, then ones, on distinct columns
            v = np.zeros(192, np.int32)
            c = rng.permutation(cols[60:])
            k = 0
            while ssd >= 4 and rng.random() < 0.7:
                v[c[k]] = rng.choice((-2, 2)); ssd -= 4; k += 1
            while ssd > 0:
                v[c[k]] = rng.choice((-1, 1)); ssd -= 1; k += 1
            return v
        rows = []
        for i in range(nb):
            s = 3 + i % 6
            rows += [b[i] + offset(s - 1), b[i] + offset(s), b[i] + offset(s + 1), b[i] + offset(s - 1)]
        db = np.stack(rows)[rng.permutation(4 * nb)]
        q = np.concatenate([b, b])
        q[nb:, cols[60]] += 1
    return db.astype(np.int16), q.astype(np.int16), info


CASES = {
    "twice-narrow": lambda: _cloud_case(21, "twice", False),
    "twice-wide": lambda: _cloud_case(22, "twice", True),
    "mirror-low-first": lambda: _spread_case(23, "mirror-low-first"),
    "mirror-low-last": lambda: _spread_case(24, "mirror-low-last"),
    "pairs": lambda: _spread_case(25, "pairs"),
    "three": lambda: _spread_case(26, "three"),
    "parities": lambda: _spread_case(27, "parities"),
    "identical-narrow": lambda: _cloud_case(28, "identical", False),
    "identical-wide": lambda: _cloud_case(29, "identical", True),
    "tiny-1": lambda: _cloud_case(30, "1", False),
    "tiny-31": lambda: _cloud_case(31, "31", False),
    "tiny-33": lambda: _cloud_case(32, "33", False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case's rows and its exact answer, made once and shared by the four modes (read-only)"""
    db, q, info = CASES[name]()
    assert q.shape[0] <= 4097 and db.shape[0] <= 5000
    eidx, eerr, ties = _brute(q, db)
    for a in (db, q, eidx, eerr, ties):
        a.setflags(write=False)
    return db, q, info, eidx, eerr, ties


def _positions(order):
    """original row -> (tile, place in the tile) under the index's row order"""
    pos = np.empty(order.shape[0], np.int64)
    pos[order] = np.arange(order.shape[0])
    return pos >> 5, pos & 31


def _check_inputs(name, db, q, info, eidx, eerr, ties, order):
    """the data is what the docstring says: properties of the inputs, from the brute force and the index's row order alone"""
    nt = db.shape[0]
    tile, place = _positions(order)
    if name.startswith("twice"):
        real = slice(0, q.shape[0] - 64) if name.endswith("wide") else slice(None)
        assert (np.mean(ties[real]) > 0.99 if name.endswith("wide") else np.all(ties)) and np.all(eidx[real] < nt // 2)
        a, b = np.arange(nt // 2 - 64), np.arange(nt // 2 - 64) + nt // 2
        assert np.sum(tile[a] != tile[b]) >= 10 and np.all(tile[a] <= tile[b])
    if name.startswith("mirror"):
        nb = info["nb"]
        assert np.mean(ties) > 0.9 and np.mean(eerr == 1000000) > 0.9
        first, second = np.arange(nb), np.arange(nb) + nb
        assert np.all(tile[first] != tile[second])
        assert np.all(tile[first] < tile[second]) if name == "mirror-low-first" else np.all(tile[first] > tile[second])
    if name == "pairs":
        a, b = info["pair_a"], info["pair_b"]
        assert np.all(ties[:2363]) and np.all(eerr[:1200] == 0) and np.all(eerr[1200:] == 1)
        same = tile[a] == tile[b]
        half = (place >> 2) & 1
        assert np.sum(same & (half[a] == half[b])) >= 100, "pairs in one half-wave"
        assert np.sum(same & (place[b] == place[a] + 4)) >= 10, "pairs at rows r and r + 4"
        assert np.sum(~same) >= 10, "pairs that straddle two tiles"
    if name == "three":
        nb = info["nb"]
        assert np.mean(eerr == 1000000) > 0.9
        t3 = np.stack([tile[np.arange(nb) + k * nb] for k in range(3)])
        assert np.mean((t3[0] != t3[1]) & (t3[1] != t3[2]) & (t3[0] != t3[2])) > 0.9, "the three rows lie in three tiles"
        tied = eerr == 1000000
        assert np.all(eidx[tied] < nb), "the lowest of the three indices wins"
        assert all(np.sum(info["kind0"][eidx[tied]] == k) > 300 for k in range(3)), "each of the three rows is the winner for a third of the queries"
    if name == "parities":
        nb = db.shape[0] // 4
        assert np.all(ties[:nb]) and np.all(eerr[:nb] == 2 + np.arange(nb) % 6)
        norms = (db.astype(np.int64) ** 2).sum(1) & 1
        assert 0.3 < norms.mean() < 0.7
    if name.startswith("identical"):
        assert eerr[0] == 0 and eerr[1] == 1 and ties[0] and ties[1] and eidx[0] == eidx[1]
        assert np.sum((db == db[eidx[0]]).all(1)) == 900
    if name.startswith("tiny"):
        assert eerr[0] == 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_ties_settled_in_scan(case, mode, monkeypatch):
    from tiler_amd import stages
    db, q, info, eidx, eerr, ties = _case(case)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    order = ix.row_order()
    ix.close()
    plan = stages.knn_last_plan()
    print("%s / %s: plan <HT %d, HQ %d>, %d queries x %d rows, tied %.3f, largest SSD %d" % (case, mode, plan[0], plan[1], q.shape[0], db.shape[0], np.mean(ties), int(eerr.max())))
    if "plan" in info and db.shape[0] > 64:
        assert plan[:3] == info["plan"], "the data was built for %r, the library planned %r" % (info["plan"], plan)
    _check_inputs(case, db, q, info, eidx, eerr, ties, order)
    got_err, got_idx = err.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    assert np.array_equal(got_err, eerr), "%d of %d errors differ" % (int((got_err != eerr).sum()), q.shape[0])
    assert np.array_equal(got_idx, eidx), "%d of %d indices differ" % (int((got_idx != eidx).sum()), q.shape[0])


def test_tile_rows_ascend_in_index():
    """the ordering step on its own, on a permutation that stands for a curve order (5 000 rows: a last tile of 8), and on a searched index:
    each tile's indices ascend, and each tile holds the rows it held before"""
    from tiler_amd import stages
    rng = np.random.default_rng(40)
    for n in (1, 31, 32, 33, 5000):
        curve = rng.permutation(n).astype(np.uint32)
        got = stages.knn_tile_order(_dev(curve.view(np.int32))).cpu().numpy().view(np.uint32)
        for t in range(0, n, 32):
            assert np.array_equal(got[t:t + 32], np.sort(curve[t:t + 32])), "tile %d of %d rows" % (t // 32, n)
    big = np.array([0xFFFFFFFE, 5, 0x80000000, 7], np.uint32)  # compared as unsigned
    assert np.array_equal(stages.knn_tile_order(_dev(big.view(np.int32))).cpu().numpy().view(np.uint32), np.sort(big))
    db, q = _case("pairs")[:2]
    ix = stages.KnnIndex(_dev(db))
    ix.search(_dev(q[:64]))
    order = ix.row_order()
    ix.close()
    assert np.array_equal(np.sort(order), np.arange(db.shape[0]))
    for t in range(0, db.shape[0], 32):
        assert np.all(np.diff(order[t:t + 32].astype(np.int64)) > 0)
