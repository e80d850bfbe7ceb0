"""k_knn_consume's two tasks: a wave either looks -- pops a list entry, loads the tile's first chunk, judges every sub-tile that wants
the tile on it -- or runs the chains of a tile some look let through, which it takes from the survivor queue in LDS (k3_ring_push / k3_ring_pop)
and loads whole.  A tile none of whose blocks gets past its look is never loaded beyond its first chunk.

Every case runs the default build's search and the same search with TM_KNN_FIRST_CHUNK=0 (every popped tile loaded whole, every chain run),
compares EVERY query's index and error of both with the exact fp64 scan on the device (tests/test_gpu_knn_first_chunk.py: _exact_nearest, the
lowest original index among equal minima) and the two with each other, and checks the queue's books: every tile with a survivor became exactly
one queue entry or one chain task run in place, and as many tiles were loaded whole as that (nothing lost, nothing run twice).

  * few survivors        the `chunk decides` cloud: clusters the first chunk tells apart.  Some tiles are never loaded whole; fewer entries are
                         pushed than tiles popped.
  * everything survives  the `rest decides` shape (rows of a cluster equal on the 32 widest columns), 5 000 rows against 768 queries: every block of
                         a query's own cluster gets past its look.  Some entry is turned away by the queue and its chains run in the looking
                         wave.  (A wave pops before it looks again, so fewer entries than waves are ever outstanding and the ring of 128 does
                         not fill: what turns an entry away here is a push that lost the tail to another wave's, which is tried once -- 2 of
                         144 entries when a push was tried four times, about one in nine now.)
  * ties                 the `ties` cloud: two rows at the same distance, one differing inside the chunk and one outside; the lowest original
                         index wins whichever wave and whichever task reaches it first.
  * two segments         the `segments` cloud, lists longer than K3_LCAP: the drain between the two barriers at a segment's end, with a segment
                         behind it; the blocks looked at are those stopped plus those completed.
  * edges                1 and 33 rows against 1 and 33 queries: one tile, a partly filled tile and sub-tile, padding rows.
  * masks                plans <1, 0> and <0, 1>, and tiles without high digits in the first chunk.
  * other modes          knn_topk(k = 64) and the dense launch (TM_KNN_NOPRUNE=1) give what the exact scan gives.

The clouds and their exact answers are the first-chunk test's own (fixtures imported: one exact scan per cloud and module)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_knn_first_chunk import (  # noqa: E402,F401  (fixtures are used by name)
    _centres, _dev, _exact_nearest, _exact_topk, chunk_decides, masks, segments, ties)

pytestmark = pytest.mark.gpu


def _search(db, q):
    from tiler_amd import stages
    ix = stages.KnnIndex(_dev(db))
    idx, err = ix.search(_dev(q))
    torch.cuda.synchronize()
    looked, stopped = ix.last_chunk_counts()
    tiles, no_surv, pushed, ring_full, whole, completed = ix.last_survivor_counts()
    plan = stages.knn_last_plan()[:3]
    ix.close()
    return dict(idx=idx.cpu().numpy(), err=err.cpu().numpy().view(np.uint32), looked=looked, stopped=stopped, tiles=tiles, no_surv=no_surv, pushed=pushed,
                ring_full=ring_full, whole=whole, completed=completed, plan=plan)


def _both(tag, db, q, exact, monkeypatch):
    """the search with the look (two tasks, the queue) and without (every chain): both exact, both alike, the queue's books in order"""
    monkeypatch.delenv("TM_KNN_NOPRUNE", raising=False)
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    on = _search(db, q)
    monkeypatch.setenv("TM_KNN_FIRST_CHUNK", "0")
    off = _search(db, q)
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    eidx, eerr = exact
    for name, r in (("two tasks", on), ("every chain", off)):
        print("%s/%s: plan %r, %d tiles popped, %d without a survivor, %d pushed, %d run in place, %d loaded whole; %d of %d blocks stopped, %d completed; "
              "%d errors and %d indices of %d differ from the exact scan" %
              (tag, name, r["plan"], r["tiles"], r["no_surv"], r["pushed"], r["ring_full"], r["whole"], r["stopped"], r["looked"], r["completed"],
               int((r["err"] != eerr).sum()), int((r["idx"] != eidx).sum()), eidx.size))
        assert np.array_equal(r["err"], eerr)
        assert np.array_equal(r["idx"], eidx)
    assert np.array_equal(on["idx"], off["idx"]) and np.array_equal(on["err"], off["err"])
    # with the look: a popped tile has no survivor, or is one queue entry, or one chain task run in place; that many tiles were loaded whole
    assert on["tiles"] == on["no_surv"] + on["pushed"] + on["ring_full"]
    assert on["whole"] == on["pushed"] + on["ring_full"]
    assert on["looked"] == on["stopped"] + on["completed"]
    # without: no look, no queue; every popped tile loaded whole
    assert off["looked"] == 0 and off["stopped"] == 0
    assert off["no_surv"] == 0 and off["pushed"] == 0 and off["ring_full"] == 0 and off["whole"] == off["tiles"]
    return on, off


def test_few_survivors(chunk_decides, monkeypatch):
    db, q, exact = chunk_decides
    on, _ = _both("few survivors", db, q, exact, monkeypatch)
    assert on["no_surv"] > 0, "every popped tile was loaded whole"
    assert on["whole"] < on["tiles"]
    assert on["pushed"] < on["tiles"], "as many entries pushed as tiles popped"


@pytest.fixture(scope="module")
def all_survive():
    """the `rest decides` shape: a cluster's rows are equal on the 32 widest columns and differ (+-60) on the 160 narrow ones only"""
    rng = np.random.default_rng(4101)
    c, cols = _centres(rng)
    c[:, cols[8:32]] = rng.integers(-200, 201, size=(64, 24))
    narrow = cols[32:]

    def rows(n):
        r = c[rng.integers(0, 64, n)].copy()
        r[:, narrow] += rng.integers(-60, 61, size=(n, 160))
        return r.astype(np.int16)
    db, q = rows(5000), rows(768)
    return db, q, _exact_nearest(q, db)


def test_everything_survives(all_survive, monkeypatch):
    db, q, exact = all_survive
    on, _ = _both("everything survives", db, q, exact, monkeypatch)
    assert on["pushed"] + on["ring_full"] > 0
    assert on["ring_full"] > 0, "the queue turned no entry away: no chain task ran in the looking wave (%d entries pushed)" % on["pushed"]


def test_ties(ties, monkeypatch):
    db, q, lower, has_below, below_at, exact = ties
    assert np.array_equal(exact[0][~has_below], lower[~has_below]) and np.array_equal(exact[0][has_below], below_at)  # the data is what its docstring says
    _both("ties", db, q, exact, monkeypatch)


def test_two_segments(segments, monkeypatch):
    db, q, exact = segments
    on, _ = _both("two segments", db, q, exact, monkeypatch)
    assert on["looked"] > 0 and on["looked"] == on["stopped"] + on["completed"]  # KnnIndex.last_chunk_counts(): every block looked at is accounted for


@pytest.mark.parametrize("nt", [1, 33])
@pytest.mark.parametrize("nq", [1, 33])
def test_edges(nt, nq, monkeypatch):
    rng = np.random.default_rng(4102 + 100 * nt + nq)
    c, _ = _centres(rng, n=4)
    db = (c[rng.integers(0, 4, nt)] + rng.integers(-40, 41, size=(nt, 192))).astype(np.int16)
    q = (c[rng.integers(0, 4, nq)] + rng.integers(-40, 41, size=(nq, 192))).astype(np.int16)
    _both("edges-%dx%d" % (nt, nq), db, q, _exact_nearest(q, db), monkeypatch)


def test_masks(masks, monkeypatch):
    name, db, q, plan, exact = masks
    on, _ = _both("masks-" + name, db, q, exact, monkeypatch)
    assert on["plan"] == plan, "the data was built for plan %r, the library planned %r" % (plan, on["plan"])


def test_collection_mode(chunk_decides, monkeypatch):
    from tiler_amd import stages
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    db, q, _ = chunk_decides
    q = q[:1024]
    eidx, eerr = _exact_topk(q, db, 64)
    idx, err = stages.knn_topk(_dev(q), _dev(db), 64)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), eidx)
    assert np.array_equal(err.cpu().numpy().view(np.uint32), eerr)


def test_dense_launch(chunk_decides, monkeypatch):
    db, q, exact = chunk_decides
    monkeypatch.delenv("TM_KNN_FIRST_CHUNK", raising=False)
    monkeypatch.setenv("TM_KNN_NOPRUNE", "1")
    r = _search(db, q)
    print("dense: %d tiles popped, %d loaded whole, %d blocks completed" % (r["tiles"], r["whole"], r["completed"]))
    assert np.array_equal(r["err"], exact[1]) and np.array_equal(r["idx"], exact[0])
    assert r["looked"] == 0 and r["stopped"] == 0 and r["pushed"] == 0 and r["ring_full"] == 0  # the look and its queue belong to the lists' consumer
    assert r["whole"] == r["tiles"]
