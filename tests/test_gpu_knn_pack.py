"""k_knn_pack writes a tile's rows into LDS once, in packed column order, and makes its digits without a branch per value; every
byte it writes is what it wrote before.  The packs are not to be read from outside, so the searches that consume them are checked: EVERY
query's index and error against the exact fp64 scan of tests/test_gpu_knn_first_chunk.py, on shapes that reach the kernel's corners:

  * nq in {1, 31, 32, 33, 4 097} x nt in {1, 33, 5 000}: the packs' last tiles, rows replicated past n, a single tile; and 131 105 queries
    (4 098 tiles for a launch of 4 096 workgroups: two of them walk a second tile, with the vectors fetched ahead) on 33 rows;
  * 3 000 rows of which 400 are distinct (the lowest index among copies), and 3 000 rows all distinct;
  * plans <0, 0> (no high-digit chunk: every piece must fit one digit), <1, 0> and <0, 1> (high digits on one side only), <5, 4> with
    doubled database digits (the multiplier 2 on the database side, -1 on the queries') and <5, 4> with plain ones;
  * a column on which the database lies 40 000 from the queries' centre, and one on which the queries lie 40 000 from the database's:
    "exceeds the exact two-digit int8 split" on either side.

Column ranges (the scan is exact where the squared ranges sum to less than 2^31): <5, 4>: 160 x 1 200^2 + 32 x 200^2 = 2.3e8; the refused
columns: 40 400^2 + 191 x 20^2 = 1.63e9."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_knn_first_chunk import _chunk_decides, _dev, _exact_nearest  # noqa: E402

pytestmark = pytest.mark.gpu


def _search(db, q):
    from tiler_amd import stages
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    torch.cuda.synchronize()
    plan = stages.knn_last_plan()[:3]
    ix.close()
    return idx.cpu().numpy(), err.cpu().numpy().view(np.uint32), plan


def _check(tag, res, exact):
    idx, err, plan = res
    eidx, eerr = exact
    print("%s: plan %r; %d of %d errors and %d of %d indices differ from the exact scan" %
          (tag, plan, int((err != eerr).sum()), eerr.size, int((idx != eidx).sum()), eidx.size))
    assert np.array_equal(err, eerr)
    assert np.array_equal(idx, eidx)


SIZES = [(nq, nt) for nt in (1, 33, 5000) for nq in (1, 31, 32, 33, 4097)] + [(4096 * 32 + 33, 33)]


@pytest.fixture(scope="module")
def sized():
    """one cloud; every (nq, nt) is a prefix of it, its exact answers computed on first use and kept"""
    db, q = _chunk_decides(5000, 4096 * 32 + 33, seed=2401)
    cache = {}

    def case(nq, nt):
        if (nq, nt) not in cache:
            cache[(nq, nt)] = _exact_nearest(q[:nq], db[:nt])
        return db[:nt], q[:nq], cache[(nq, nt)]
    return case


@pytest.mark.parametrize("nq,nt", SIZES)
def test_sizes(sized, nq, nt):
    db, q, exact = sized(nq, nt)
    _check("sizes nq=%d nt=%d" % (nq, nt), _search(db, q), exact)


@pytest.fixture(scope="module", params=["400-of-3000-distinct", "all-distinct"])
def duplicated(request):
    rng = np.random.default_rng(2402)
    rows, q = _chunk_decides(3000, 1500, seed=2403)
    if request.param == "400-of-3000-distinct":
        db = rows[:400][rng.integers(0, 400, 3000)]
        db[rng.permutation(3000)[:400]] = rows[:400]  # every distinct row is there
        q[:500] = db[rng.integers(0, 3000, 500)]       # a third of the queries are copies of rows: error 0, the lowest index of the copies
        distinct = 400
    else:
        db, distinct = rows, 3000
    assert np.unique(db, axis=0).shape[0] == distinct
    return request.param, db, q, _exact_nearest(q, db)


def test_duplicated_rows(duplicated):
    name, db, q, exact = duplicated
    _check(name, _search(db, q), exact)


def _wide_cloud(seed, nt, nq, t_wide, q_wide, t_narrow, q_narrow=60):
    """columns (in a random order) 0..q_wide-1 wide on both sides, ..t_wide-1 wide on the database side only (t_wide >= q_wide), the rest narrow"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(192)

    def side(n, wide, narrow):
        r = rng.integers(-narrow, narrow + 1, size=(n, 192))
        r[:, perm[:wide]] = rng.integers(-600, 601, size=(n, wide))
        r[0], r[1] = -narrow, narrow  # the ranges are exactly symmetric: the centres are 0
        r[0, perm[:wide]], r[1, perm[:wide]] = -600, 600
        return r.astype(np.int16)
    return side(nt, t_wide, t_narrow), side(nq, q_wide, q_narrow)


PLANS = {
    "<0,0>": (lambda: _wide_cloud(2410, 2500, 1100, 0, 0, 60), (0, 0, 0)),
    "<1,0>": (lambda: _wide_cloud(2411, 2500, 1100, 20, 0, 60), (1, 0, 0)),
    "<0,1>": (lambda: tuple(reversed(_wide_cloud(2412, 1100, 2500, 20, 0, 60))), (0, 1, 0)),
    "<5,4>-doubled": (lambda: _wide_cloud(2413, 2500, 1100, 160, 128, 60), (5, 4, 0)),
    "<5,4>-plain": (lambda: _wide_cloud(2414, 2500, 1100, 160, 128, 100), (5, 4, 0)),
}


@pytest.fixture(scope="module", params=list(PLANS))
def planned(request):
    make, plan = PLANS[request.param]
    db, q = make()
    return request.param, db, q, plan, _exact_nearest(q, db)


def test_plans(planned):
    name, db, q, plan, exact = planned
    res = _search(db, q)
    _check("plan " + name, res, exact)
    assert res[2] == plan, "the data was built for plan %r, the library planned %r" % (plan, res[2])


@pytest.mark.parametrize("side", ["database", "queries"])
def test_range_beyond_two_digits_is_refused(side):
    """One column on which both sides need two digits whatever the centre, so the queries' midpoint is taken and the database lies 40 000
    from it; and one on which the database needs one digit about its own midpoint, which is therefore taken, and the queries lie 40 000 from
    it.  (The ranges stay inside the exact domain: that check comes first and says something else.)  Both are refused by the plan, on the
    host: plan_covers admits +-32 000 where the kernel's own flag would fire beyond +-32 639, and every batch passes it before a pack is
    launched, so the flag is a second line that no caller of the library can reach."""
    from tiler_amd._lib import TileMotionError
    rng = np.random.default_rng(2420)
    db = rng.integers(-10, 11, size=(300, 192)).astype(np.int16)
    q = rng.integers(-10, 11, size=(200, 192)).astype(np.int16)
    q[:, 7] = rng.integers(-20200, -19799, size=200)
    q[0, 7], q[1, 7] = -20200, -19800
    if side == "database":
        db[:, 7] = rng.integers(19800, 20201, size=300)
    else:
        db[:, 7] = rng.integers(19990, 20011, size=300)
    with pytest.raises(TileMotionError) as ei:
        _search(db, q)
    assert "exceeds the exact two-digit" in str(ei.value)
