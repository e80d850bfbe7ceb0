"""The first look of the tile -> palette k-means (D = 192; tm_kmeans.h states the rule): the plain iterations decide every point in single
precision and leave the double-precision chain to the points the look cannot decide.  Every case runs three ways -- default,
TM_KM_FIRST_LOOK=0 (the chain for every point) and TM_KM_LAUNCHES=1 (the skipping iterations as three launches) -- and the three must agree
in assignments, centroids bit for bit, live centroid count and iteration count; where the oracle's seeding applies they must agree with
Oracle.kmeans too.  The counters of stages.kmeans_last_first_look say whether the chain ran."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LEGS = ({}, {"TM_KM_FIRST_LOOK": "0"}, {"TM_KM_LAUNCHES": "1"})
_CLOUD = {}


def _cloud(oracle):
    """the oracle's cluster features of four frames of the bench generator at 320 x 176: 3 520 rows, computed once"""
    if "rows" not in _CLOUD:
        from tiler_amd import synth
        frames = synth.video(4, 320, 176)
        tiles = frames.reshape(4, 22, 8, 40, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 64)
        _CLOUD["rows"] = oracle.features_cluster(tiles)
        _CLOUD["oracle"] = {}
    return _CLOUD["rows"]


def _rows(oracle, n):
    """the cloud cut (every so-manieth row) or tiled to n rows, and weights 1 .. 7"""
    cloud = _cloud(oracle)
    idx = (np.arange(n, dtype=np.int64) * cloud.shape[0]) // n if n <= cloud.shape[0] else np.arange(n) % cloud.shape[0]
    return np.ascontiguousarray(cloud[idx]), (np.arange(n) % 7 + 1).astype(np.uint32)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _three_legs(monkeypatch, pts, w, k, max_iter, seeds=None):
    """-> [(kk, assign, centroid bits, iters, (looked, exact))] of the three legs, after asserting that they agree"""
    from tiler_amd import stages
    d_pts, d_w = _dev(pts), (_dev(w) if w is not None else None)
    out = []
    for env in LEGS:
        for name in ("TM_KM_FIRST_LOOK", "TM_KM_LAUNCHES"):
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        if seeds is None:
            kk, assign, cent, iters = stages.kmeans(d_pts, d_w, k, max_iter)
        else:
            kk, assign, cent, iters = stages.kmeans_seeded(d_pts, d_w, k, seeds, max_iter)
        out.append((kk, assign.cpu().numpy(), cent.cpu().numpy().view(np.uint64), iters, stages.kmeans_last_first_look()))
    for name in ("TM_KM_FIRST_LOOK", "TM_KM_LAUNCHES"):
        monkeypatch.delenv(name, raising=False)
    for leg, o in zip(LEGS[1:], out[1:]):
        print("leg %s: kk %d / %d, iterations %d / %d, %d assignments differ, counters %s / %s" % (
            leg, o[0], out[0][0], o[3], out[0][3], int((o[1] != out[0][1]).sum()), o[4], out[0][4]))
        assert (o[0], o[3]) == (out[0][0], out[0][3])
        assert np.array_equal(o[1], out[0][1])
        assert np.array_equal(o[2], out[0][2]), "centroids must match bit for bit"
    assert out[1][4] == (0, 0)  # TM_KM_FIRST_LOOK=0: no look at all
    assert out[0][4][0] >= pts.shape[0] and out[0][4][1] <= out[0][4][0]
    return out


def _against_oracle(oracle, out, pts, w, k, max_iter):
    kk, assign, cent, iters = oracle.kmeans(pts, w, k, max_iter)
    g = out[0]
    print("oracle: kk %d / %d, iterations %d / %d, %d assignments differ" % (kk, g[0], iters, g[3], int((g[1] != assign).sum())))
    assert (g[0], g[3]) == (kk, iters)
    assert np.array_equal(g[1], assign)
    assert np.array_equal(g[2][:kk], cent[:kk].view(np.uint64)), "centroids must match the oracle's bit for bit"


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("n", [1, 15, 64, 65, 767, 768, 769, 1025, 2049, 3073])
def test_shapes(oracle, monkeypatch, n, k):
    """one point, less than a wave, a wave and one more, one short of a 256 x 3 slice, the slice, one past it, a second, third and fourth
    resident workgroup; one iteration, the first resident iteration, and a clustering that runs on"""
    pts, w = _rows(oracle, n)
    for max_iter in (1, 6, 40):
        out = _three_legs(monkeypatch, pts, w, k, max_iter)
        _against_oracle(oracle, out, pts, w, k, max_iter)


@pytest.mark.parametrize("k", [17, 32])
def test_more_centroids_than_a_pass(oracle, monkeypatch, k):
    """17 and 32 centroids: the passes over the centroids sixteen at a time (the resident launch does not apply)"""
    pts, w = _rows(oracle, 769)
    for max_iter in (1, 6, 40):
        out = _three_legs(monkeypatch, pts, w, k, max_iter)
        _against_oracle(oracle, out, pts, w, k, max_iter)


# ---- exact ties -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 3])
def test_exact_ties(monkeypatch, max_iter):
    """two seeds that differ in one coordinate by 2a; points on the bisecting plane and one unit either side of it (and anywhere in the
    other coordinates, which add the same to both distances): the point on the plane goes to the lower index, and only the chain can say so"""
    rng = np.random.default_rng(7)
    a, m = 37, 300
    base = rng.integers(-2000, 2001, 192).astype(np.int32)
    s0, s1 = base.copy(), base.copy()
    s1[5] += 2 * a
    other = rng.integers(-500, 501, (m, 192)).astype(np.int32)
    other[:, 5] = 0
    trip = np.repeat(base[None] + other, 3, axis=0)
    trip[0::3, 5] += a - 1
    trip[1::3, 5] += a
    trip[2::3, 5] += a + 1
    pts = np.concatenate([s0[None], s1[None], trip]).astype(np.int32)
    out = _three_legs(monkeypatch, pts, None, 2, max_iter, seeds=[0, 1])
    assert out[0][4][1] > 0  # the chain ran
    if max_iter == 1:
        assert np.array_equal(out[0][1], np.concatenate([[0, 1], np.tile([0, 0, 1], m)]))


# ---- near ties across the margin ---------------------------------------------------------------------------------------------------------
_DELTA = {1: (1,), 2: (1, 1), 10 ** 3: (30, 10), 10 ** 5: (316, 12), 10 ** 7: (3162, 41, 5, 5, 5)}  # delta as a sum of squares


@pytest.mark.parametrize("near", [0, 1])
@pytest.mark.parametrize("delta", sorted(_DELTA))
def test_near_ties(oracle, monkeypatch, delta, near):
    """integer points and seeds with squared distances X = 4 x 15 811^2 = 999 950 884 and X + delta to the two seeds (relative gaps 1e-9 ..
    1e-2), the nearer seed once the lower and once the higher index; one iteration, so the answer is known in integers"""
    rng = np.random.default_rng(delta + near)
    m = 40
    p = rng.integers(-3000, 3001, (m, 192)).astype(np.int64)
    A = np.zeros(192, np.int64)
    A[10:14] = 15811
    B = A.copy()
    B[20:20 + len(_DELTA[delta])] = _DELTA[delta]
    assert int((A * A).sum()) == 999950884 and int((B * B).sum()) == 999950884 + delta
    # every point i sits at p_i; the seeds are point 0 displaced: s_near = p_0 + A, s_far = p_0 + B.  The other points are p_0 too (plus a
    # shift along coordinates neither A nor B uses, which adds the same to both distances)
    shift = np.zeros((m, 192), np.int64)
    shift[:, 100:] = rng.integers(-50, 51, (m, 92))
    shift[0] = 0
    q = p[0][None] + shift
    s_near, s_far = p[0] + A, p[0] + B
    seeds = [s_near, s_far] if near == 0 else [s_far, s_near]
    pts = np.concatenate([np.stack(seeds), q]).astype(np.int32)
    d0 = ((pts.astype(np.int64) - pts[0].astype(np.int64)) ** 2).sum(1)
    d1 = ((pts.astype(np.int64) - pts[1].astype(np.int64)) ** 2).sum(1)
    want = np.where(d1 < d0, 1, 0)
    assert np.all(np.abs(d0[2:] - d1[2:]) == delta)
    out = _three_legs(monkeypatch, pts, None, 2, 1, seeds=[0, 1])
    assert np.array_equal(out[0][1], want)
    if delta <= 10 ** 3:
        assert out[0][4][1] > 0  # inside the look's margin: the chain ran


# ---- conversions that round ---------------------------------------------------------------------------------------------------------------
def test_inexact_conversions(oracle, monkeypatch):
    """coordinates at +-(2^24 - 1), +-2^24, +-(2^24 + 1) and around 2^26 among ordinary rows: a row with a coordinate no Single holds is in
    doubt by definition"""
    pts, w = _rows(oracle, 600)
    pts = pts.copy()
    big = [(1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 26) - 1, (1 << 26) + 1, (1 << 26) + 3]
    for i, v in enumerate(big + [-x for x in big]):
        pts[17 * i + 3, (5 * i) % 192] = v
        pts[17 * i + 4, (5 * i) % 192] = v + (1 if v > 0 else -1)  # a neighbour one unit on, so that clusters of such rows form
    for max_iter in (1, 6, 12):
        out = _three_legs(monkeypatch, pts, w, 6, max_iter)
        _against_oracle(oracle, out, pts, w, 6, max_iter)
        assert out[0][4][1] > 0


# ---- centroids that no Single holds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [2, 3, 10])
def test_centroids_no_single_holds(monkeypatch, max_iter):
    """weights that make the centroids quotients like 1/3 and 2/7 of large sums; a cluster that owns nothing (a second seed on the same row:
    ties go to the lower index, it keeps its centroid), a seed of weight zero, and a centroid that is exactly zero (rows +v and -v around
    the origin with equal weights)"""
    rng = np.random.default_rng(11)
    x = rng.integers(15000, 22000, 192).astype(np.int64)
    y = -x + rng.integers(-300, 301, 192)
    rows, wts = [], []
    for j in range(60):  # around x: weights 2 and 1 a unit apart -> thirds; around y: weights 5 and 2 -> sevenths
        e = np.zeros(192, np.int64)
        e[j % 192] = 1
        jit = rng.integers(-3, 4, 192)
        rows += [x + jit, x + jit + e, y + jit, y + jit + 2 * e]
        wts += [2, 1, 5, 2]
    v = rng.integers(-40, 41, (30, 192))
    rows += list(v) + list(-v)  # around the origin, symmetric
    wts += [3] * 60
    origin, dup = len(rows), len(rows) + 1
    rows += [np.zeros(192, np.int64), x.copy() + 7]
    wts += [4, 0]
    far = len(rows)
    rows += [x // 2]
    wts += [0]  # a seed of weight zero far from everything else
    pts = np.stack(rows).astype(np.int32)
    w = np.array(wts, np.uint32)
    seeds = [0, 2, origin, dup, dup, far]  # seeds 3 and 4 on one row: 4 owns nothing
    out = _three_legs(monkeypatch, pts, w, 6, max_iter, seeds=seeds)
    cent = out[0][2].view(np.float64)
    assert not np.any(out[0][1] == 4)
    assert np.all(cent[2] == 0.0)
    assert np.any(cent[0] != cent[0].astype(np.float32).astype(np.float64))


# ---- the look must decide ---------------------------------------------------------------------------------------------------------------
def test_the_look_decides(oracle, monkeypatch):
    """the 3 520-row cloud, 16 centroids, 40 iterations: the rule applied on the CPU leaves no point of it undecided, so at most 1 % of the
    scorings looked at may go to the chain -- a cap on the kernel, not on the data"""
    pts, w = _rows(oracle, 3520)
    out = _three_legs(monkeypatch, pts, w, 16, 40)
    looked, exact = out[0][4]
    print("looked at %d, to the chain %d" % (looked, exact))
    assert looked >= 3520 and exact * 100 <= looked
