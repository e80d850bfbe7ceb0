"""The by-index dedup Reconstruct groups its database rows with (stages.dedup_by_index, 384-byte rows) against numpy: the distinct rows in
ascending order of their first occurrence, every row mapped to its first occurrence's position, the group sizes and the count.  Under the
table front end the order is the table's own (no ranking sort); the hash sort and the plain sort rank by row number.  All three must agree."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FRONTS = {"table": None, "hash-sort": "TM_DEDUP_SORT", "plain": "TM_DEDUP_PLAIN"}
SIZES = (1, 33, 3000)


def _rows(n):
    """int16 [n][192] (384 bytes a row): at most 400 distinct rows scattered over the index range, some differing in their last dword only"""
    rng = np.random.default_rng(9100 + n)
    nd = min(400, max(1, (n * 2) // 3))
    base = rng.integers(-3000, 3000, size=(nd, 192)).astype(np.int16)
    base[nd // 2:, :190] = base[: nd - nd // 2, :190]  # pairs of rows that share everything but their last dword
    base[nd // 2:, 190:] += 1
    src = np.concatenate([np.arange(nd), rng.integers(0, nd, size=n - nd)]) if n >= nd else np.arange(n)
    return np.ascontiguousarray(base[rng.permutation(src)])


def _expected(rows):
    _, first, inverse, counts = np.unique(rows, axis=0, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")  # groups in ascending order of their first row
    pos = np.empty_like(by_first)
    pos[by_first] = np.arange(by_first.size)
    return first[by_first].astype(np.int32), pos[inverse.ravel()].astype(np.int32), counts[by_first].astype(np.int32)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for n in SIZES:
        rows = _rows(n)
        out[n] = (rows, _expected(rows))
    return out


@pytest.mark.parametrize("front", list(FRONTS))
@pytest.mark.parametrize("n", SIZES)
def test_dedup_by_index(cases, monkeypatch, n, front):
    from tiler_amd import stages
    for name in ("TM_DEDUP_DEGRADE_HASH", "TM_DEDUP_PLAIN", "TM_DEDUP_SORT"):
        monkeypatch.delenv(name, raising=False)
    if FRONTS[front]:
        monkeypatch.setenv(FRONTS[front], "1")
    rows, (order, remap, use) = cases[n]
    nu, g_remap, g_order, g_use = stages.dedup_by_index(torch.from_numpy(rows).cuda())
    g_remap, g_order, g_use = g_remap.cpu().numpy(), g_order.cpu().numpy(), g_use.cpu().numpy()
    print("n %d, %s: %d distinct rows (numpy %d)" % (n, front, nu, order.size))
    assert nu == order.size
    assert np.array_equal(g_order, order)
    assert np.array_equal(g_remap, remap)
    assert np.array_equal(g_use, use)
    assert np.array_equal(rows[g_order[g_remap]], rows)  # every row equals the first occurrence it is mapped to
