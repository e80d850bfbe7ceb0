"""k_knn_consume judges a listed block on its first chunk -- the 32 columns the plan packs first, its widest -- before the block's chain runs,
and ends the block there when no query of it can gain or tie (k3_chunk_look).  Every case runs with the look (the default) and
with TM_KNN_FIRST_CHUNK=0 (every chain runs), and compares EVERY query's index and error with an exact scan on the device: an fp64 matmul
on integer-valued doubles (every product and sum below 2^53: exact), the lowest original index among equal minima.

  * chunk decides   64 centres uniform in +-6 000 on eight columns, noise +-40 everywhere; 4 096 rows, 2 048 queries.  The eight columns are
                    in the first chunk and tell the clusters apart: blocks are stopped (none with the knob off).
  * rest decides    the same centres, a second per-cluster offset (+-200) on 24 more columns, and NO noise on those 32: the first chunk is
                    identical within a cluster, the rows differ (+-60) in the 160 narrow columns only.  Every block of a query's own cluster
                    has SSD 0 over the chunk and must run on; the results stay exact.
  * ties            2 048 points p_k (corners of a cube of side 10 000 on eleven columns) as queries; per point the rows A = p_k + d e_in
                    (e_in the widest column: inside the chunk) and B = p_k + d e_out (a column only the database side widens, to 1 500:
                    packed 33rd, outside the chunk), both at SSD d^2, d = 1 500, in a random row order in which A has the lower index for
                    the even k and B for the odd.  4 096 filler rows lie far away (+-2 000 on 21 columns of their own, which complete the
                    chunk).  Every eighth point also has a row at SSD d^2 - 1 (1 499 on e_out, 54, 9 and 1 on narrow columns), every other
                    eighth one at d^2 + 1 (1 500 the other way on e_in, 1 on a narrow column): the exact scan's answer is expected, and it is
                    checked to be the lower index of A and B at d^2 wherever no row lies below.
  * parities        tests/test_gpu_knn_epilogue.py's clouds within SSD 8 of a base row: ties, mixed parities, runs of copies, queries that
                    are their own row with odd norms on both sides (where the look lies one below the truth, at -1), in both digit shapes
                    (narrow: doubled database digits; wide: plain).
  * masks           plans without high digits on the query side (<1, 0>: queries within +-100 of the origin, a clustered database) and on
                    the database side (<0, 1>: the roles swapped); and the clustered cloud with a 65th centre at the origin, whose tiles and
                    sub-tiles have all-zero high digits in the first chunk: on the database side, on the query side, and on both at once.
  * segments        i.i.d. noise in +-100, 40 960 rows, 1 800 queries: nothing is pruned by boxes, lists of two segments and a ragged last
                    group; the outputs with the knob on and off are identical (and exact).
  * collection, dense   stages.knn_topk(k = 64) and the TM_KNN_NOPRUNE=1 launch on the clustered cloud: the look is not part of either.

Column ranges: the scan is exact where the squared column ranges sum to less than 2^31.  Clusters: 8 x 12 080^2 + 24 x 400^2 + 160 x 120^2
= 1.17e9.  Ties: 13 000^2 + 10 x 10 000^2 + 21 x 4 000^2 + 1 540^2 + 159 x 100^2 = 1.51e9."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_knn_epilogue import _brute, make_cloud  # noqa: E402  (the parities' clouds and their brute force)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _exact_distances(q, db):
    dq, dd = _dev(q).to(torch.float64), _dev(db).to(torch.float64)
    nd = (dd * dd).sum(1)
    for a in range(0, q.shape[0], 2048):
        x = dq[a:a + 2048]
        yield a, (x * x).sum(1)[:, None] + nd[None, :] - 2.0 * (x @ dd.T)


def _exact_nearest(q, db):
    idx, err = [], []
    for _, d in _exact_distances(q, db):
        e = d.min(dim=1).values
        idx.append((d == e[:, None]).to(torch.uint8).argmax(dim=1).cpu().numpy())  # first maximum = lowest index
        err.append(e.cpu().numpy())
    return np.concatenate(idx).astype(np.int32), np.concatenate(err).astype(np.uint64).astype(np.uint32)


def _exact_topk(q, db, k):
    nt = db.shape[0]
    assert nt <= 1 << 15
    col = torch.arange(nt, dtype=torch.float64, device="cuda")
    idx, err = [], []
    for _, d in _exact_distances(q, db):
        key = torch.topk(d * 32768.0 + col[None, :], k, dim=1, largest=False, sorted=True).values.to(torch.int64)
        idx.append((key & 32767).cpu().numpy())
        err.append((key >> 15).cpu().numpy())
    return np.concatenate(idx).astype(np.int32), np.concatenate(err).astype(np.uint64).astype(np.uint32)


@pytest.fixture(params=["first-chunk", "every-chain"])
def knob(request, monkeypatch):
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    monkeypatch.delenv("TM_KNN_NOPRUNE", raising=False)
    if request.param == "every-chain":
        monkeypatch.setenv("TM_KNN_FIRST_CHUNK", "0")
    return request.param


def _search(db, q):
    """(idx, err as uint32, blocks looked at, blocks stopped, plan) of one KnnIndex search"""
    from tiler_amd import stages
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    torch.cuda.synchronize()
    looked, stopped = ix.last_chunk_counts()
    plan = stages.knn_last_plan()[:3]
    ix.close()
    return idx.cpu().numpy(), err.cpu().numpy().view(np.uint32), looked, stopped, plan


def _check(tag, knob, res, exact):
    idx, err, looked, stopped, plan = res
    eidx, eerr = exact
    print("%s/%s: plan %r, %d of %d listed blocks stopped at the first chunk; %d of %d errors and %d of %d indices differ from the exact scan" %
          (tag, knob, plan, stopped, looked, int((err != eerr).sum()), eerr.size, int((idx != eidx).sum()), eidx.size))
    assert np.array_equal(err, eerr)
    assert np.array_equal(idx, eidx)
    assert 0 <= stopped <= looked
    if knob == "every-chain":
        assert stopped == 0 and looked == 0


# ---------------------------------------------------------------------------------------------------------------- the clustered clouds
def _centres(rng, n=64, origin=False):
    cols = rng.permutation(192)
    c = np.zeros((n + (1 if origin else 0), 192), np.int32)
    c[:n, cols[:8]] = rng.integers(-6000, 6001, size=(n, 8))
    if origin:  # the column ranges made symmetric, so that the plan's centres lie within the noise of 0 and the rows about the origin need no high digit
        c[0, cols[:8]], c[1, cols[:8]] = 6000, -6000
    return c, cols


def _chunk_decides(nt, nq, origin=False, seed=2301):
    rng = np.random.default_rng(seed)
    c, _ = _centres(rng, origin=origin)
    db = c[rng.integers(0, c.shape[0], nt)] + rng.integers(-40, 41, size=(nt, 192))
    q = c[rng.integers(0, c.shape[0], nq)] + rng.integers(-40, 41, size=(nq, 192))
    return db.astype(np.int16), q.astype(np.int16)


@pytest.fixture(scope="module")
def chunk_decides():
    db, q = _chunk_decides(4096, 2048)
    return db, q, _exact_nearest(q, db)


@pytest.fixture(scope="module")
def rest_decides():
    rng = np.random.default_rng(2302)
    c, cols = _centres(rng)
    c[:, cols[8:32]] = rng.integers(-200, 201, size=(64, 24))
    narrow = cols[32:]

    def rows(n):
        r = c[rng.integers(0, 64, n)].copy()
        r[:, narrow] += rng.integers(-60, 61, size=(n, 160))
        return r.astype(np.int16)
    db, q = rows(4096), rows(2048)
    return db, q, _exact_nearest(q, db)


def test_chunk_decides(chunk_decides, knob):
    db, q, exact = chunk_decides
    res = _search(db, q)
    _check("chunk decides", knob, res, exact)
    assert res[4] == (1, 1, 0)
    if knob == "first-chunk":
        assert res[3] > 0, "no block was stopped at its first chunk"


def test_rest_decides(rest_decides, knob):
    db, q, exact = rest_decides
    assert np.all(exact[1] > 0) and np.all(exact[1] <= 160 * 120 * 120)  # every query's nearest row is one of its own cluster, and not itself
    res = _search(db, q)
    _check("rest decides", knob, res, exact)
    if knob == "first-chunk":
        # Other clusters' blocks differ on the chunk by millions and stop; a listed block of a query's own cluster has SSD 0 over the chunk for
        # that query and cannot.  Which blocks are listed at all is the boxes' and the seeds' affair (a cluster is two or three tiles, a
        # sub-tile of 32 consecutive queries draws from two clusters or more, the seeds are eight tiles), so the counters are bounded, not
        # pinned: some block stops, some block runs on.  A block of the own cluster that stopped would show above: it holds the nearest row.
        assert 0 < res[3] < res[2], "%d of %d listed blocks stopped" % (res[3], res[2])


# ---------------------------------------------------------------------------------------------------------------- ties across the boundary
DELTA = 1500


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(2303)
    perm = rng.permutation(192)
    code, mid, e_out, n1, n2, n3 = perm[:11], perm[11:32], perm[32], perm[33], perm[34], perm[35]
    e_in = code[0]
    n = 2048
    p = np.zeros((n, 192), np.int32)
    p[:, code] = (((np.arange(n)[:, None] >> np.arange(11)[None, :]) & 1) * 2 - 1) * 5000
    a_rows, b_rows = p.copy(), p.copy()
    a_rows[:, e_in] += DELTA
    b_rows[:, e_out] += DELTA
    below = p[3::8].copy()  # SSD d^2 - 1 = 1499^2 + 54^2 + 9^2 + 1^2
    below[:, e_out] += 1499
    below[:, n1] += 54
    below[:, n2] += 9
    below[:, n3] += 1
    above = p[5::8].copy()  # SSD d^2 + 1
    above[:, e_in] -= DELTA
    above[:, n1] += 1
    filler = np.zeros((4096, 192), np.int32)
    filler[:, code] = (rng.integers(0, 2, size=(4096, 11)) * 2 - 1) * 5000
    filler[:, mid] = (rng.integers(0, 2, size=(4096, 21)) * 2 - 1) * 2000
    filler += rng.integers(-40, 41, size=filler.shape)
    rows = np.concatenate([a_rows, b_rows, below, above, filler])
    place = rng.permutation(rows.shape[0])  # place[r] = the index row r ends at
    ia, ib = place[:n].copy(), place[n:2 * n].copy()
    swap = np.where(np.arange(n) % 2 == 0, ia > ib, ib > ia)  # A first for the even points, B first for the odd
    place[:n] = np.where(swap, ib, ia)
    place[n:2 * n] = np.where(swap, ia, ib)
    db = np.empty_like(rows)
    db[place] = rows
    lower = np.minimum(place[:n], place[n:2 * n]).astype(np.int32)
    has_below = np.zeros(n, bool)
    has_below[3::8] = True
    db, p = db.astype(np.int16), p.astype(np.int16)
    return db, p, lower, has_below, place[2 * n:2 * n + below.shape[0]].astype(np.int32), _exact_nearest(p, db)


def test_ties_across_the_boundary(ties, knob):
    db, q, lower, has_below, below_at, exact = ties
    # the data is what the docstring says
    assert np.array_equal(exact[0][~has_below], lower[~has_below]) and np.all(exact[1][~has_below] == DELTA * DELTA)
    assert np.array_equal(exact[0][has_below], below_at) and np.all(exact[1][has_below] == DELTA * DELTA - 1)
    res = _search(db, q)
    _check("ties", knob, res, exact)


# ---------------------------------------------------------------------------------------------------------------- parities, self-matches
_PARITY_CASES = {"narrow": (21, 3000, 1500, 6, False), "wide": (22, 3000, 1500, 6, True)}


@pytest.fixture(scope="module", params=list(_PARITY_CASES))
def parities(request):
    seed, nt, nq, db_cols, wide = _PARITY_CASES[request.param]
    db, q, n_runq, n_self = make_cloud(seed, nt, nq, db_cols, wide)
    eidx, eerr, tied, _ = _brute(q, db)
    assert np.all(eerr[n_runq:n_runq + n_self] == 0) and np.mean(tied) > 0.4
    return request.param, db, q, (eidx, eerr)


def test_parities_and_self_matches(parities, knob):
    shape, db, q, exact = parities
    res = _search(db, q)
    _check("parities-" + shape, knob, res, exact)
    assert res[4] == ((1, 1, 0) if shape == "wide" else (0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------- masks
@pytest.fixture(scope="module", params=["no-query-high-digits", "no-database-high-digits", "zero-tiles"])
def masks(request):
    rng = np.random.default_rng(2304)
    if request.param == "zero-tiles":
        db, q = _chunk_decides(4096, 2048, origin=True, seed=2305)
        # 256 more rows and 128 more queries about the origin.  Rows are packed in curve order and the next centre is thousands away, so the
        # rows about the origin are consecutive there: with 63 or more of them at least one 32-row tile, and one 32-query sub-tile, holds
        # nothing else -- every value within +-60 of its centre, all high digits zero (the counts are asserted in test_masks).
        db = np.concatenate([db, rng.integers(-40, 41, size=(256, 192)).astype(np.int16)])
        q = np.concatenate([q, rng.integers(-40, 41, size=(128, 192)).astype(np.int16)])
        plan = (1, 1, 0)
    else:
        c = np.zeros((33, 192), np.int32)  # 32 centres away from the origin and one on it
        c[:32, rng.permutation(192)[:8]] = rng.integers(-3000, 3001, size=(32, 8))
        wide = c[rng.integers(0, 33, 4096)] + rng.integers(-40, 41, size=(4096, 192))
        near = rng.integers(-100, 101, size=(2048, 192))
        db, q, plan = (wide, near, (1, 0, 0)) if request.param == "no-query-high-digits" else (near, wide, (0, 1, 0))
        db, q = db.astype(np.int16), q.astype(np.int16)
    return request.param, db, q, plan, _exact_nearest(q, db)


def test_masks(masks, knob):
    name, db, q, plan, exact = masks
    if name == "zero-tiles":
        for side in (db, q):
            wide = np.flatnonzero(np.abs(side.astype(np.int32)).max(0) > 1000)  # the eight centre columns
            assert wide.size == 8 and side[:, wide].min() < -5900 and side[:, wide].max() > 5900  # ranges symmetric within the noise: centres within +-60 of 0
            assert int((np.abs(side.astype(np.int32)).max(1) <= 40).sum()) >= 63  # rows about the origin: a whole tile / sub-tile of them
    res = _search(db, q)
    _check("masks-" + name, knob, res, exact)
    assert res[4] == plan, "the data was built for plan %r, the library planned %r" % (plan, res[4])


# ---------------------------------------------------------------------------------------------------------------- segments
@pytest.fixture(scope="module")
def segments():
    rng = np.random.default_rng(2306)
    db = rng.integers(-100, 101, size=(40960, 192)).astype(np.int16)
    q = rng.integers(-100, 101, size=(1800, 192)).astype(np.int16)
    return db, q, _exact_nearest(q, db)


def test_segments(segments, knob):
    db, q, exact = segments
    _check("segments", knob, _search(db, q), exact)


def test_segments_identical_either_way(segments, monkeypatch):
    db, q, _ = segments
    monkeypatch.delenv("TM_KNN_NOPRUNE", raising=False)
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    on = _search(db, q)
    monkeypatch.setenv("TM_KNN_FIRST_CHUNK", "0")
    off = _search(db, q)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert off[2] == 0 and off[3] == 0 and on[2] > 0


# ---------------------------------------------------------------------------------------------------------------- collection, dense
@pytest.fixture(scope="module")
def chunk_decides_topk(chunk_decides):
    db, q, _ = chunk_decides
    return db, q[:1024], _exact_topk(q[:1024], db, 64)


def test_collection_mode(chunk_decides_topk, knob):
    from tiler_amd import stages
    db, q, (eidx, eerr) = chunk_decides_topk
    idx, err = stages.knn_topk(_dev(q), _dev(db), 64)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), eidx)
    assert np.array_equal(err.cpu().numpy().view(np.uint32), eerr)


def test_dense_launch(chunk_decides, knob, monkeypatch):
    db, q, exact = chunk_decides
    monkeypatch.setenv("TM_KNN_NOPRUNE", "1")
    res = _search(db, q)
    print("dense/%s: %d blocks looked at, %d stopped" % (knob, res[2], res[3]))
    assert np.array_equal(res[1], exact[1]) and np.array_equal(res[0], exact[0])
    assert res[2] == 0 and res[3] == 0  # the look belongs to the lists' consumer
