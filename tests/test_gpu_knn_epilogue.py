"""The scan's block epilogue takes the minimum's value and row from a mask of the registers that hold the smallest chain value:
data on which nearly every block goes down that path, with ties and mixed parities, against an exact brute force.

A block's epilogue ends at its first look unless one of its 32 queries finds a row no worse than its best so far.  Here every database row
and every query lies within SSD 8 of one base row (up to eight columns moved by +-1), so distances take a handful of small values: whatever
a query's best is, most tiles hold a row that reaches or ties it.  What the path has to get right is all over such data:
  * equal chain values with different parities (rows at SSD s and s + 1 of a query share Y when s - |q-c|^2 is even), in both row orders;
  * distinct rows at equal SSD (one column moved by +1 and by -1), and exact duplicates, far apart in index: the lowest index must win;
  * runs of 2, 3, 5, 33 and 70 copies of one row: copies are neighbours on the curve, so a run of 70 puts tied rows into one half-wave's
    sixteen rows, into both halves of a tile, and into different tiles, wherever the sort places it;
  * queries that are their own database row, in pairs R and R + e_0 whose norms about any centre differ in parity: one of each pair has
    odd norms on both sides, the case d'' + 1 = 0 in which the first look lies one below the truth.
Two column shapes: `narrow` (every column within +-1 of the base: the database digits are doubled, k_knn_consume<.., TD = true>, plan <0, 0>)
and `wide` (64 far rows on each side with 27 columns of +-400 and 10 of +-100: doubling would make 37 two-digit columns, a second high chunk,
so the plain digits are kept, TD = false, plan <1, 1> -- with doubled digits the library would report HT = 2).  tm_knn_last_plan is
asserted in each case.  `segments`: 40 000 database rows and 2 600 queries, six query groups whose lists hold every tile of the cloud
(1 250 > 1 024 entries: two segments each, a full refresh every 64 entries); the scan's pair counter is asserted to say so."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

RUNS = (2, 3, 5, 33, 70)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _brute(q, db):
    """exact nearest row by (SSD, lowest index): fp64 matmul on integer-valued doubles (every product and sum is exact), 2048 queries at a time"""
    dq, dd = _dev(q).to(torch.float64), _dev(db).to(torch.float64)
    nd = (dd * dd).sum(1)
    idx, err, ties, next_up = [], [], [], []
    for a in range(0, q.shape[0], 2048):
        x = dq[a:a + 2048]
        d = (x * x).sum(1)[:, None] + nd[None, :] - 2.0 * (x @ dd.T)
        e = d.min(dim=1).values
        hit = d == e[:, None]
        idx.append(hit.to(torch.uint8).argmax(dim=1).cpu().numpy())  # first maximum = lowest index
        err.append(e.cpu().numpy())
        ties.append((hit.sum(1) > 1).cpu().numpy())
        next_up.append((d == e[:, None] + 1.0).any(1).cpu().numpy())
    return (np.concatenate(idx).astype(np.int32), np.concatenate(err).astype(np.uint64).astype(np.uint32), np.concatenate(ties), np.concatenate(next_up))


def make_cloud(seed, nt, nq, db_cols, wide):
    """(db, q, queries on the runs, queries that are their own row): int16 rows.  The cloud moves `db_cols` columns of the base row by -1 / 0 / +1 on the database side and two more on
    the query side (so most queries are nobody's copy and their nearest rows tie); then the planted rows of the module's docstring."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-30, 31, size=192).astype(np.int32)
    perm = rng.permutation(192)
    cols_t, cols_q = perm[:db_cols], perm[:db_cols + 2]
    db = np.tile(base, (nt, 1))
    q = np.tile(base, (nq, 1))
    db[:, cols_t] += rng.integers(-1, 2, size=(nt, db_cols))
    q[:, cols_q] += rng.integers(-1, 2, size=(nq, db_cols + 2))
    # runs of copies of one row, scattered over the index range; a query on the row and one a step off it
    at = rng.permutation(nt - 64)[:sum(RUNS) + 64]  # (the last 64 rows of each side are the far ones of `wide`)
    k = 0
    for j, n in enumerate(RUNS):
        src = db[at[k]].copy()
        db[at[k:k + n]] = src
        k += n
        q[2 * j] = src
        q[2 * j + 1] = src
        q[2 * j + 1, perm[db_cols + 1]] += 1
    # queries that are their own database row, in pairs of opposite norm parity
    n_self = 64
    for j in range(n_self // 2):
        r = db[at[k]].copy()
        k += 1
        r2 = r.copy()
        r2[perm[0]] += -1 if r[perm[0]] >= base[perm[0]] else 1  # one step on one column, still within +-1 of the base: the norm's parity flips
        db[at[k]] = r2
        k += 1
        q[2 * len(RUNS) + 2 * j] = r
        q[2 * len(RUNS) + 2 * j + 1] = r2
    if wide:  # far rows that set the column ranges: 27 two-digit columns, 10 whose doubled values would need a second digit
        far = perm[db_cols + 2:db_cols + 2 + 37]
        for rows in (db, q):
            n = rows.shape[0]
            sel = np.arange(n - 64, n)
            rows[np.ix_(sel, far[:27])] = base[far[:27]] + rng.integers(-400, 401, size=(64, 27))
            rows[np.ix_(sel, far[27:])] = base[far[27:]] + rng.integers(-100, 101, size=(64, 10))
            rows[n - 1, far[:27]] = base[far[:27]] + 400
            rows[n - 2, far[:27]] = base[far[:27]] - 400
            rows[n - 1, far[27:]] = base[far[27:]] + 100
            rows[n - 2, far[27:]] = base[far[27:]] - 100
    return db.astype(np.int16), q.astype(np.int16), 2 * len(RUNS), n_self


CASES = {
    # name: (seed, database rows, queries, columns the database side moves, wide)
    "cloud-narrow": (11, 3000, 1500, 6, False),
    "cloud-wide": (12, 3000, 1500, 6, True),
    "segments-narrow": (13, 40000, 2600, 8, False),
    "segments-wide": (14, 40000, 2600, 8, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_knn_exact_path_against_brute_force(case):
    from tiler_amd import stages
    seed, nt, nq, db_cols, wide = CASES[case]
    db, q, n_runq, n_self = make_cloud(seed, nt, nq, db_cols, wide)
    eidx, eerr, ties, next_up = _brute(q, db)
    # the data is what the docstring says (properties of the inputs, from the brute force alone)
    cloud = slice(0, nq - 64) if wide else slice(0, nq)
    assert np.mean(ties[cloud]) > 0.5, "most queries' nearest rows should tie"
    assert np.mean(next_up[cloud]) > 0.5, "most queries should have rows at SSD min and min + 1 (equal chain value, different parity for one parity of the query's norm)"
    selfq = slice(n_runq, n_runq + n_self)
    assert np.all(eerr[selfq] == 0) and np.all(eerr[0:n_runq:2] == 0)
    idx, err = stages.knn(_dev(q), _dev(db))
    plan = stages.knn_last_plan()
    print("%s: plan <HT %d, HQ %d>, %d queries x %d rows, tied %.3f, min+1 present %.3f, largest SSD %d" %
          (case, plan[0], plan[1], nq, nt, np.mean(ties), np.mean(next_up), int(eerr.max())))
    assert plan[:3] == ((1, 1, 0) if wide else (0, 0, 0)), "the data was built for %s digits, the library planned %r" % ("plain" if wide else "doubled", plan)
    got_err, got_idx = err.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    assert np.array_equal(got_err, eerr), "%d of %d errors differ" % (int((got_err != eerr).sum()), nq)
    assert np.array_equal(got_idx, eidx), "%d of %d indices differ" % (int((got_idx != eidx).sum()), nq)
    if case.startswith("segments"):
        # every tile of the cloud is on every group's list (more than 1 024 entries: a second segment), and every block is evaluated
        ix = stages.KnnIndex(_dev(db))
        idx2, err2 = ix.search(_dev(q))
        _, _, pairs = ix.last_stats()
        ix.close()
        print("%s: %d exact pairs = %.0f rows per query" % (case, pairs, pairs / nq))
        assert np.array_equal(err2.cpu().numpy().view(np.uint32), eerr) and np.array_equal(idx2.cpu().numpy(), eidx)
        assert pairs >= (nq - 64) * 1024 * 32
