"""Both sides of a KNN search are sorted along a Hilbert curve (the default) or a Morton curve (TM_KNN_CURVE).  The search is exact
under any row order, so every case runs under each curve and compares EVERY query's index and error with the exact fp64 scan of
tests/test_gpu_knn_first_chunk.py (the lowest original index among equal minima), and the two curves' outputs with each other.

  * sizes           nq in {1, 33, 4 097} x nt in {1, 33, 5 000}, prefixes of one clustered cloud; on 5 000 rows the two curves must put the
                    database into different orders (the knob is alive).
  * every key ties  3 000 rows that all hold 0 in the three curve columns -- which the queries alone make the widest, +-6 000 -- and +-50 in
                    every other column (signs at random, both present in every column: the plan's centres are 0 and every row's radial
                    coordinate is the same 50 sqrt(186)).  Every database key is equal; the stable sort leaves the rows in their original
                    order, which row_order() must show.  Ten rows are copies of earlier ones.  The queries' noise is +-50 or +-30 per query,
                    so their radial coordinates take two values.
  * one radial      the three curve columns spread on both sides, every other column +-50 on both: one radial value in all (rhi == rlo in
                    choose_curve), the radial bits of every key are equal.
  * two clusters    two centres 12 000 apart on eight columns, 1 500 rows and 1 000 queries about each: neither count is a multiple of 32,
                    so one tile and one sub-tile straddle the gap.
  * two segments    i.i.d. noise in +-100, 40 960 rows, 1 800 queries (nothing is pruned by boxes: lists of two segments), with
                    TM_KNN_ARENA_ENTRIES=64: the search is repeated with the counted size.
  * k nearest       stages.knn_topk(k = 64), 2 000 queries on 3 000 rows, against the brute-force collection (TM_TOPK_BRUTE=1): first thresholds
                    from the curve window (TM_TOPK_ESTIMATE=0) and from a sample of the database (=1), under each curve and with the knob not
                    set, where the sample's index keeps the Morton order beside a Hilbert index.

Column ranges (the scan is exact where the squared ranges sum to less than 2^31): clusters 8 x 12 080^2 + 184 x 80^2 = 1.17e9; ties and one
radial 3 x 12 000^2 + 189 x 100^2 = 4.3e8.  Whether the Hilbert order lists fewer blocks is a measurement, not asserted here."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_knn_first_chunk import _chunk_decides, _dev, _exact_nearest  # noqa: E402

pytestmark = pytest.mark.gpu

CURVES = ("morton", "hilbert")


def _search(monkeypatch, curve, db, q, order=False):
    from tiler_amd import stages
    monkeypatch.setenv("TM_KNN_CURVE", curve)
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    torch.cuda.synchronize()
    rows = ix.row_order() if order else None
    ix.close()
    return idx.cpu().numpy(), err.cpu().numpy().view(np.uint32), rows


def _both(monkeypatch, tag, db, q, exact, order=False):
    """the search under each curve against the exact scan, and the two against each other -> {curve: (idx, err, row order)}"""
    eidx, eerr = exact
    res = {}
    for curve in CURVES:
        res[curve] = idx, err, _ = _search(monkeypatch, curve, db, q, order)
        print("%s/%s: %d of %d errors and %d of %d indices differ from the exact scan" %
              (tag, curve, int((err != eerr).sum()), eerr.size, int((idx != eidx).sum()), eidx.size))
        assert np.array_equal(err, eerr)
        assert np.array_equal(idx, eidx)
    assert np.array_equal(res["morton"][0], res["hilbert"][0]) and np.array_equal(res["morton"][1], res["hilbert"][1])
    return res


# ---------------------------------------------------------------------------------------------------------------- sizes
@pytest.fixture(scope="module")
def sized():
    """one cloud; every (nq, nt) is a prefix of it, its exact answers computed on first use and kept"""
    db, q = _chunk_decides(5000, 4097, seed=3611)
    cache = {}

    def case(nq, nt):
        if (nq, nt) not in cache:
            cache[(nq, nt)] = _exact_nearest(q[:nq], db[:nt])
        return db[:nt], q[:nq], cache[(nq, nt)]
    return case


@pytest.mark.parametrize("nt", [1, 33, 5000])
@pytest.mark.parametrize("nq", [1, 33, 4097])
def test_sizes(sized, monkeypatch, nq, nt):
    db, q, exact = sized(nq, nt)
    res = _both(monkeypatch, "sizes nq=%d nt=%d" % (nq, nt), db, q, exact, order=True)
    for curve in CURVES:
        assert np.array_equal(np.sort(res[curve][2]), np.arange(nt, dtype=np.uint32))
    if nt == 5000:
        assert not np.array_equal(res["morton"][2], res["hilbert"][2]), "TM_KNN_CURVE did not change the database's order"


# ---------------------------------------------------------------------------------------------------------------- ties, one radial value
def _signs(rng, n, a):
    """+-a in every column, both signs present in every column (rows 0 and 1 are each other's negatives)"""
    s = (rng.integers(0, 2, size=(n, 192)) * 2 - 1) * a
    s[1] = -s[0]
    return s


def _flat_cloud(seed, nt, nq, db_spread):
    rng = np.random.default_rng(seed)
    curve_cols = rng.permutation(192)[:3]
    db = _signs(rng, nt, 50)
    q = _signs(rng, nq, 50)
    if not db_spread:
        q[2::2] = q[2::2] // 50 * 30  # a second radial value among the queries (rows 0 and 1 keep the columns' ranges at +-50)
    q[:, curve_cols] = rng.integers(-6000, 6001, size=(nq, 3))
    q[0, curve_cols], q[1, curve_cols] = -6000, 6000
    if db_spread:
        db[:, curve_cols] = rng.integers(-6000, 6001, size=(nt, 3))
    else:
        db[:, curve_cols] = 0
        db[nt - 10:] = db[5:15]  # copies: the lowest index wins
    return db.astype(np.int16), q.astype(np.int16), curve_cols


@pytest.fixture(scope="module")
def every_key_ties():
    db, q, cols = _flat_cloud(3612, 3000, 1500, db_spread=False)
    return db, q, cols, _exact_nearest(q, db)


def test_every_database_key_ties(every_key_ties, monkeypatch):
    db, q, cols, exact = every_key_ties
    assert np.all(db[:, cols] == 0) and np.all(np.abs(np.delete(db, cols, axis=1)) == 50)  # the data is what the docstring says
    assert set(np.unique(np.abs(np.delete(q, cols, axis=1)).max(axis=1))) == {30, 50}
    res = _both(monkeypatch, "every key ties", db, q, exact, order=True)
    for curve in CURVES:
        assert np.array_equal(res[curve][2], np.arange(db.shape[0], dtype=np.uint32)), "equal keys did not keep the rows' original order"


@pytest.fixture(scope="module")
def one_radial():
    db, q, cols = _flat_cloud(3613, 3000, 1500, db_spread=True)
    return db, q, cols, _exact_nearest(q, db)


def test_one_radial_value(one_radial, monkeypatch):
    db, q, cols, exact = one_radial
    for side in (db, q):
        assert np.all(np.abs(np.delete(side, cols, axis=1)) == 50)
    _both(monkeypatch, "one radial value", db, q, exact)


# ---------------------------------------------------------------------------------------------------------------- two far clusters
@pytest.fixture(scope="module")
def two_clusters():
    rng = np.random.default_rng(3614)
    c = np.zeros((2, 192), np.int32)
    c[0, rng.permutation(192)[:8]] = 6000
    c[1] = -c[0]
    db = np.repeat(c, 1500, axis=0) + rng.integers(-40, 41, size=(3000, 192))
    q = np.repeat(c, 1000, axis=0) + rng.integers(-40, 41, size=(2000, 192))
    db, q = db[rng.permutation(3000)].astype(np.int16), q[rng.permutation(2000)].astype(np.int16)
    return db, q, _exact_nearest(q, db)


def test_runs_that_straddle_a_gap(two_clusters, monkeypatch):
    db, q, exact = two_clusters
    _both(monkeypatch, "two clusters", db, q, exact)


# ---------------------------------------------------------------------------------------------------------------- two segments, a tiny arena
@pytest.fixture(scope="module")
def segments():
    rng = np.random.default_rng(3615)
    db = rng.integers(-100, 101, size=(40960, 192)).astype(np.int16)
    q = rng.integers(-100, 101, size=(1800, 192)).astype(np.int16)
    return db, q, _exact_nearest(q, db)


def test_lists_of_two_segments_in_a_tiny_arena(segments, monkeypatch):
    from tiler_amd import stages
    db, q, exact = segments
    monkeypatch.setenv("TM_KNN_ARENA_ENTRIES", "64")
    before = stages.knn_last_plan()[3]
    _both(monkeypatch, "two segments", db, q, exact)
    assert stages.knn_last_plan()[3] >= before + 2, "the searches were not repeated: the arena did not overflow"


# ---------------------------------------------------------------------------------------------------------------- k nearest
@pytest.fixture(scope="module")
def collection():
    from tiler_amd import stages
    db, q = _chunk_decides(3000, 2000, seed=3616)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TM_TOPK_BRUTE", "1")
        bidx, berr = stages.knn_topk(_dev(q), _dev(db), 64)
        torch.cuda.synchronize()
    return db, q, bidx.cpu().numpy(), berr.cpu().numpy()


@pytest.mark.parametrize("estimate", ["window", "sample"])
def test_k_nearest_under_both_curves(collection, monkeypatch, estimate):
    """first thresholds from the curve window, and from a sample of the database (TM_TOPK_ESTIMATE=1), whose index keeps the Morton order where
    TM_KNN_CURVE is not set: that leg runs as well"""
    from tiler_amd import stages
    db, q, bidx, berr = collection
    monkeypatch.delenv("TM_TOPK_BRUTE", raising=False)
    monkeypatch.setenv("TM_TOPK_ESTIMATE", "1" if estimate == "sample" else "0")
    out = {}
    for curve in CURVES + ("not set",):
        if curve == "not set":
            monkeypatch.delenv("TM_KNN_CURVE")
        else:
            monkeypatch.setenv("TM_KNN_CURVE", curve)
        idx, err = stages.knn_topk(_dev(q), _dev(db), 64)
        torch.cuda.synchronize()
        out[curve] = idx.cpu().numpy(), err.cpu().numpy()
        assert stages.knn_last_plan()[2] == 1  # the pruned collection ran, not the brute force
        assert np.array_equal(out[curve][1], berr)
        assert np.array_equal(out[curve][0], bidx)
    assert np.array_equal(out["morton"][0], out["hilbert"][0]) and np.array_equal(out["morton"][1], out["hilbert"][1])
