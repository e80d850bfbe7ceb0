"""The scan's tile lists leave k_knn_lists sorted, segment by segment, by each entry's smallest lower bound, and k_knn_consume ends a
segment at the first entry no sub-tile can want.  Every case runs with the new order (the default) and with
TM_KNN_LIST_ORDER=0 (run order, no stop), and compares EVERY query's index and error with an exact scan on the device: an fp64 matmul on
integer-valued doubles (every product and sum below 2^53: exact), the lowest original index among equal minima.

  * segments     40 960 rows and 1 800 queries of i.i.d. noise in [-100, 100]: all boxes overlap, nothing is pruned, every group lists
                 the 1 280 tiles (minus its seeds) -- two segments, each sorted on its own; 1 800 queries = 56 full sub-tiles and one of
                 8 queries and 24 rows of padding, in a ragged last group.
  * clusters     64 centres on eight columns, 16 384 rows and 8 192 queries = a centre + noise in [-40, 40] on all columns.  A group's
                 sub-tiles outside the seeds' cluster list most of the database against a loose bound; sorted, their own clusters' tiles
                 come first, the bounds fall to the noise's size and the rest of the segment is refused at once: fewer entries are popped
                 than listed (equal with TM_KNN_LIST_ORDER=0).
  * ties         2 048 well separated points p_k as queries; the database holds p_k + d e and p_k - d e (e the widest column, the curve's
                 first: the two lie far apart on it), both at SSD d^2, and 16 384 filler rows far from every p_k, in a row order in which
                 the `+` row has the lower index for the even k and the `-` row for the odd: the lower index and d^2 are expected.
  * collection   stages.knn_topk(k = 64) on the clustered cloud against the exact 64 nearest in (SSD, index) order.

Column ranges.  The library's scan is exact where the squared column ranges (database and queries together) sum to less than 2^31
(tm_knn.hip: knn_index_search refuses anything else), so the clouds are as wide as that allows and no wider: the centres are uniform in
[-8 000, 8 000] on their eight columns (8 x 16 080^2 = 2.07e9; +-12 000 would be 4.6e9 and is refused), and the 2 048 points are the
corners of a cube of side 10 000 on eleven columns with d = 1 500 (10 x 10 000^2 + 13 000^2 + the filler's 4 x 12 000^2 = 1.75e9; a
spacing of 20 000 allows no more than a few dozen points).  Points 10 000 apart with d = 1 500 keep the property the case is about: every
row of another point is farther from p_k than its own two (a differing column other than e gives >= 10 000; on e, >= 10 000 - 1 500)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _exact_distances(q, db):
    """yields (first query, exact SSD matrix fp64 [<= 2048][nt]) 2 048 queries at a time"""
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
    """the k nearest rows in (SSD, index) order: smallest k of SSD * 2^15 + index (below 2^46: exact in fp64)"""
    nt = db.shape[0]
    assert nt <= 1 << 15
    col = torch.arange(nt, dtype=torch.float64, device="cuda")
    idx, err = [], []
    for _, d in _exact_distances(q, db):
        key = torch.topk(d * 32768.0 + col[None, :], k, dim=1, largest=False, sorted=True).values.to(torch.int64)
        idx.append((key & 32767).cpu().numpy())
        err.append((key >> 15).cpu().numpy())
    return np.concatenate(idx).astype(np.int32), np.concatenate(err).astype(np.uint64).astype(np.uint32)


@pytest.fixture(params=["sorted", "run-order"])
def order(request, monkeypatch):
    monkeypatch.delenv("TM_KNN_LIST_ORDER", raising=False)
    if request.param == "run-order":
        monkeypatch.setenv("TM_KNN_LIST_ORDER", "0")
    return request.param


@pytest.fixture(scope="module")
def segments():
    rng = np.random.default_rng(2101)
    db = rng.integers(-100, 101, size=(40960, 192)).astype(np.int16)
    q = rng.integers(-100, 101, size=(1800, 192)).astype(np.int16)
    return db, q, _exact_nearest(q, db)


def _cluster_cloud():
    rng = np.random.default_rng(2102)
    cols = rng.permutation(192)[:8]
    centres = np.zeros((64, 192), np.int32)
    centres[:, cols] = rng.integers(-8000, 8001, size=(64, 8))
    db = centres[rng.integers(0, 64, 16384)] + rng.integers(-40, 41, size=(16384, 192))
    q = centres[rng.integers(0, 64, 8192)] + rng.integers(-40, 41, size=(8192, 192))
    return db.astype(np.int16), q.astype(np.int16)


@pytest.fixture(scope="module")
def clusters():
    db, q = _cluster_cloud()
    return db, q, _exact_nearest(q, db)


@pytest.fixture(scope="module")
def clusters_topk():
    db, q = _cluster_cloud()
    return db, q, _exact_topk(q, db, 64)


DELTA = 1500


@pytest.fixture(scope="module")
def ties():
    rng = np.random.default_rng(2103)
    perm = rng.permutation(192)
    code, fill = perm[:11], perm[11:15]
    e = code[0]  # the widest column: 10 000 + 2 DELTA against the filler's 12 000 and the other code columns' 10 000
    n = 2048
    p = np.zeros((n, 192), np.int32)
    p[:, code] = (((np.arange(n)[:, None] >> np.arange(11)[None, :]) & 1) * 2 - 1) * 5000
    plus, minus = p.copy(), p.copy()
    plus[:, e] += DELTA
    minus[:, e] -= DELTA
    filler = np.zeros((16384, 192), np.int32)
    filler[:, code] = (rng.integers(0, 2, size=(16384, 11)) * 2 - 1) * 5000
    filler[:, fill] = (rng.integers(0, 2, size=(16384, 4)) * 2 - 1) * 6000
    filler += rng.integers(-40, 41, size=filler.shape)
    rows = np.concatenate([plus, minus, filler])
    # row order: a random one, then the two rows of a point swapped where needed: `+` first for the even points, `-` first for the odd
    place = rng.permutation(rows.shape[0])  # place[r] = the index row r ends at
    ip, im = place[:n].copy(), place[n:2 * n].copy()
    swap = np.where(np.arange(n) % 2 == 0, ip > im, im > ip)
    place[:n] = np.where(swap, im, ip)
    place[n:2 * n] = np.where(swap, ip, im)
    db = np.empty_like(rows)
    db[place] = rows
    lower = np.minimum(place[:n], place[n:2 * n]).astype(np.int32)
    assert np.array_equal(lower[0::2], place[:n][0::2]) and np.array_equal(lower[1::2], place[n:2 * n][1::2])
    return db.astype(np.int16), p.astype(np.int16), lower, _exact_nearest(p.astype(np.int16), db.astype(np.int16))


def _compare(tag, idx, err, exact):
    eidx, eerr = exact
    got_err, got_idx = err.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    print("%s: %d of %d errors and %d of %d indices differ from the exact scan" %
          (tag, int((got_err != eerr).sum()), eerr.size, int((got_idx != eidx).sum()), eidx.size))
    assert np.array_equal(got_err, eerr)
    assert np.array_equal(got_idx, eidx)


def _search(db, q):
    from tiler_amd import stages
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    torch.cuda.synchronize()
    listed, popped = ix.last_list_counts()
    ix.close()
    return idx, err, listed, popped


def test_lists_of_several_segments(segments, order):
    from tiler_amd import stages
    db, q, exact = segments
    idx, err = stages.knn(_dev(q), _dev(db))
    torch.cuda.synchronize()
    _compare("segments/%s (stages.knn)" % order, idx, err, exact)
    idx, err, listed, popped = _search(db, q)
    groups = -(-57 // 13)  # at most: a group holds 13 to 16 sub-tiles
    print("segments/%s: %d entries listed, %d popped" % (order, listed, popped))
    _compare("segments/%s (KnnIndex)" % order, idx, err, exact)
    assert listed > 1024 * 4, "every full group should list the whole database: more than one segment each"
    assert listed <= groups * 1280
    if order == "run-order":
        assert popped == listed


def test_lists_that_stop_early(clusters, order):
    db, q, exact = clusters
    idx, err, listed, popped = _search(db, q)
    print("clusters/%s: %d entries listed, %d popped" % (order, listed, popped))
    _compare("clusters/%s" % order, idx, err, exact)
    if order == "sorted":
        assert popped < listed, "no segment was ended early"
    else:
        assert popped == listed


def test_ties_across_the_stop(ties, order):
    db, q, lower, exact = ties
    assert np.array_equal(exact[0], lower) and np.all(exact[1] == DELTA * DELTA)  # the data is what the docstring says
    idx, err, listed, popped = _search(db, q)
    print("ties/%s: %d entries listed, %d popped" % (order, listed, popped))
    _compare("ties/%s" % order, idx, err, exact)
    assert np.array_equal(idx.cpu().numpy(), lower) and np.all(err.cpu().numpy().view(np.uint32) == DELTA * DELTA)


def test_collection_mode(clusters_topk, order):
    from tiler_amd import stages
    db, q, (eidx, eerr) = clusters_topk
    idx, err = stages.knn_topk(_dev(q), _dev(db), 64)
    torch.cuda.synchronize()
    got_idx, got_err = idx.cpu().numpy(), err.cpu().numpy().view(np.uint32)
    print("collection/%s: %d of %d errors and %d of %d indices differ from the exact 64 nearest" %
          (order, int((got_err != eerr).sum()), eerr.size, int((got_idx != eidx).sum()), eidx.size))
    assert np.array_equal(got_idx, eidx)
    assert np.array_equal(got_err, eerr)
