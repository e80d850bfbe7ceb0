"""curve_key (tm_knn_kernel.h) through its seam, tm_stage_curve_keys / stages.curve_keys: the key both sides of a KNN search are sorted by
(DESIGN 36).  The reference is a restatement of Skilling's algorithm here (J. Skilling, "Programming the Hilbert curve", AIP Conf. Proc.
707, 2004: axes to transposed index, then the interleave), and of the Morton interleave.

  * kind 1, every cell of a 4 x 4-bit grid (65 536): the keys are a permutation of 0 .. 65 535, and in key order consecutive cells differ by
    exactly one step on exactly one axis -- the property the Hilbert order is chosen for;
  * kind 0, bits 8, 7, 7, 8, 10 000 random cells: the coordinates' bits interleaved from the top, a dimension with more bits first;
  * kind 1, bits 3, 2, 2, 3 (1 024 cells): an axis with fewer bits is shifted up to the grid's three, so the keys are distinct and equal
    the 3-bit-grid keys of the shifted coordinates;
  * kind 1, bits 8, 7, 7, 8 and 8, 8, 8, 8, 10 000 random cells: the restatement, and the key uses all 32 bits without loss."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _hilbert(cells, nb):
    """Skilling: cells [n][4], every coordinate below 2^nb -> the Hilbert index (4 nb bits)"""
    x = [cells[:, d].astype(np.uint64) for d in range(4)]
    top = 1 << (nb - 1)
    bit = top
    while bit > 1:  # inverse undo
        low = np.uint64(bit - 1)
        for d in range(4):
            has = (x[d] & np.uint64(bit)) != 0
            if d == 0:
                x[0] = np.where(has, x[0] ^ low, x[0])
            else:
                t = (x[0] ^ x[d]) & low
                x[0], x[d] = np.where(has, x[0] ^ low, x[0] ^ t), np.where(has, x[d], x[d] ^ t)
        bit >>= 1
    for d in range(1, 4):  # Gray encode
        x[d] = x[d] ^ x[d - 1]
    t = np.zeros_like(x[0])
    bit = top
    while bit > 1:
        t = np.where((x[3] & np.uint64(bit)) != 0, t ^ np.uint64(bit - 1), t)
        bit >>= 1
    x = [v ^ t for v in x]
    key = np.zeros_like(x[0])
    for b in range(nb - 1, -1, -1):
        for d in range(4):
            key = (key << np.uint64(1)) | ((x[d] >> np.uint64(b)) & np.uint64(1))
    return key


def _hilbert_padded(cells, bits):
    nb = max(bits)
    return _hilbert(np.stack([cells[:, d].astype(np.uint64) << np.uint64(nb - bits[d]) for d in range(4)], axis=1), nb)


def _morton(cells, bits):
    key = np.zeros(cells.shape[0], np.uint64)
    for b in range(15, -1, -1):
        for d in range(4):
            if bits[d] > b:
                key = (key << np.uint64(1)) | ((cells[:, d].astype(np.uint64) >> np.uint64(b)) & np.uint64(1))
    return key


def _keys(cells, bits, kind):
    from tiler_amd import stages
    dev = torch.from_numpy(np.ascontiguousarray(cells.astype(np.uint32)).view(np.int32)).cuda()
    out = stages.curve_keys(dev, bits, kind)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).astype(np.uint64)


def _grid(bits):
    axes = np.meshgrid(*[np.arange(1 << b) for b in bits], indexing="ij")
    return np.stack([a.ravel() for a in axes], axis=1)


def _random_cells(seed, n, bits):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 1 << b, size=n) for b in bits], axis=1)


def test_hilbert_visits_every_cell_by_unit_steps():
    cells = _grid((4, 4, 4, 4))
    keys = _keys(cells, (4, 4, 4, 4), 1)
    assert np.array_equal(np.sort(keys), np.arange(65536, dtype=np.uint64))
    walk = cells[np.argsort(keys)].astype(np.int64)
    step = np.abs(np.diff(walk, axis=0))
    assert np.all(step.sum(axis=1) == 1) and np.all((step != 0).sum(axis=1) == 1)
    assert np.array_equal(keys, _hilbert(cells, 4))


def test_morton_is_the_interleave():
    bits = (8, 7, 7, 8)
    cells = _random_cells(3601, 10000, bits)
    cells[0], cells[1] = 0, [(1 << b) - 1 for b in bits]
    keys = _keys(cells, bits, 0)
    assert np.array_equal(keys, _morton(cells, bits))
    assert keys[0] == 0 and keys[1] == (1 << 30) - 1


def test_hilbert_shifts_an_axis_with_fewer_bits():
    bits = (3, 2, 2, 3)
    cells = _grid(bits)
    assert cells.shape[0] == 1024
    keys = _keys(cells, bits, 1)
    assert np.unique(keys).size == 1024 and keys.max() < 4096
    shifted = cells * np.array([1, 2, 2, 1])
    assert np.array_equal(keys, _keys(shifted, (3, 3, 3, 3), 1))
    assert np.array_equal(keys, _hilbert(shifted, 3))


@pytest.mark.parametrize("bits", [(8, 7, 7, 8), (8, 8, 8, 8)])
def test_hilbert_at_the_search_bit_counts(bits):
    cells = _random_cells(3602, 10000, bits)
    cells[0], cells[1] = 0, [(1 << b) - 1 for b in bits]
    keys = _keys(cells, bits, 1)
    assert np.array_equal(keys, _hilbert_padded(cells, bits))
    assert keys.max() >= 1 << 31  # the top bit of the 32 is in use: nothing was cut off
    assert np.unique(keys).size == np.unique(cells, axis=0).shape[0]


def test_bit_counts_that_do_not_fit_are_refused():
    from tiler_amd._lib import TileMotionError
    cells = np.zeros((4, 4), np.uint32)
    with pytest.raises(TileMotionError):
        _keys(cells, (9, 8, 8, 7), 1)  # a 9-bit grid needs 36 bits
    with pytest.raises(TileMotionError):
        _keys(cells, (9, 8, 8, 8), 0)  # 33 bits
    with pytest.raises(TileMotionError):
        _keys(cells, (8, 7, 7, 8), 2)
