"""PreparePalettes' colour keys in 32 bits (PaletteCount <= 256) and in 64, the refusal of palette numbers a 32-bit key cannot carry, the
u64 pair list Dither reads, the ranking of the palettes by tile count on the device (up to 1 024 palettes) and on the host, and the number
of times PreparePalettes makes the host wait.  Palettes are compared with the oracle per palette, exactly."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


# ---- both widths of the key ---------------------------------------------------------------------------------------------------------------
NPAL = 256


@pytest.fixture(scope="module")
def ends_case(oracle):
    """600 tiles over 256 palettes: palettes 0 and 255 and about a hundred between them hold tiles, the others none; every pixel carries a
    top byte (it must not reach the key); the second half of a tile repeats its first (weights above 1) -> (tiles, pal_idx, the oracle's palettes)"""
    rng = np.random.default_rng(8800)
    used = np.concatenate([[0, NPAL - 1], rng.choice(np.arange(1, NPAL - 1), size=100, replace=False)])
    pal_idx = np.concatenate([used, rng.choice(used, size=600 - used.size)]).astype(np.int32)
    pal_idx = rng.permutation(pal_idx)
    tiles = rng.integers(0, 1 << 24, size=(600, 64)).astype(np.uint32)
    tiles[:, 32:] = tiles[:, :32]
    tiles |= rng.integers(1, 256, size=(600, 64)).astype(np.uint32) << 24
    want = np.stack([oracle.quantize_palette(tiles[pal_idx == p].ravel(), 16) for p in range(NPAL)])
    assert (want[0] != -65281).any() and (want[NPAL - 1] != -65281).any() and (np.bincount(pal_idx, minlength=NPAL) == 0).sum() > 100
    return tiles, pal_idx, want


def test_both_ends_of_the_palette_field(ends_case):
    """PaletteCount = 256: the largest count with 32-bit keys; palette 255 fills the key's top byte"""
    from tiler_amd import stages
    tiles, pal_idx, want = ends_case
    got = stages.quantize_palettes(_dev(tiles), _dev(pal_idx), NPAL, 16).cpu().numpy()
    print("palettes that differ: %s" % np.nonzero((got != want).any(1))[0].tolist())
    assert np.array_equal(got, want)


def test_narrow_and_wide_keys_agree(ends_case):
    """the same tiles with PaletteCount = 257, the first count with 64-bit keys: the oracle's palettes again (the 257th holds nothing), and
    the first 256 equal the 32-bit call's"""
    from tiler_amd import stages
    tiles, pal_idx, want = ends_case
    narrow = stages.quantize_palettes(_dev(tiles), _dev(pal_idx), NPAL, 16).cpu().numpy()
    wide = stages.quantize_palettes(_dev(tiles), _dev(pal_idx), NPAL + 1, 16).cpu().numpy()
    assert wide.shape == (NPAL + 1, 16)
    assert np.array_equal(wide[:NPAL], want) and (wide[NPAL] == -65281).all()
    assert np.array_equal(wide[:NPAL], narrow)


@pytest.mark.parametrize("bad,npal", [(259, 5), (256, 256), (-1, 5)])
def test_refuses_a_palette_number_out_of_range(bad, npal):
    """259 would pass for palette 3 in a 32-bit key and 256 for palette 0; -1 is no palette either"""
    from tiler_amd import stages
    from tiler_amd._lib import TileMotionError
    rng = np.random.default_rng(8900)
    tiles = rng.integers(0, 1 << 24, size=(40, 64)).astype(np.uint32)
    pal_idx = (np.arange(40) % npal).astype(np.int32)
    pal_idx[17] = bad
    with pytest.raises(TileMotionError) as e:
        stages.quantize_palettes(_dev(tiles), _dev(pal_idx), npal, 16)
    assert e.value.code == -1  # TM_E_INVAL


# ---- the pair list Dither reads -------------------------------------------------------------------------------------------------------------
def _small_clip():
    """4 frames of 256 x 128, every pixel one of 500 colours: 2 048 different frame tiles -- Dither's distinct-pair path wants 1 024 global
    tiles for 4 palettes -- and at most 2 000 (palette, colour) pairs, far below half the pixels, so the path is kept"""
    rng = np.random.default_rng(8950)
    colours = rng.choice(1 << 24, size=500, replace=False).astype(np.uint32)
    return rng.choice(colours, size=(4, 128, 256)) | np.uint32(0xFF000000)


def _encoder(frames, **settings):
    from tiler_amd.encoder import TilingEncoder
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in settings.items():
        setattr(enc, k, v)
    nf, h, w = frames.shape
    enc.SetVideo(w, h, 24.0, nf)
    for f in range(nf):
        enc.PushFrame(f, frames[f])
    return enc


def test_dither_reads_the_same_pair_list(monkeypatch):
    """Run through Dither with PreparePalettes' unique keys handed over (32-bit keys, written out as the u64 list Dither reads) and with
    Dither marking the pairs from the pixels itself (TM_DITHER_OWN_KEYS): the same palette-index pixels, the same number of pairs"""
    from tiler_amd.encoder import TEncoderStep
    frames = _small_clip()
    outs = []
    for own in (False, True):
        monkeypatch.delenv("TM_DITHER_OWN_KEYS", raising=False)
        if own:
            monkeypatch.setenv("TM_DITHER_OWN_KEYS", "1")
        enc = _encoder(frames, PaletteCount=4, MotionPredictRadius=0)
        for st in (TEncoderStep.esLoad, TEncoderStep.esPredictMotion, TEncoderStep.esReduce, TEncoderStep.esPreparePalettes, TEncoderStep.esDither):
            enc.Run(st)
        outs.append((enc.Tiles()[1], enc.DitherPairs(), enc.counts()["tiles"]))
        enc.close()
    print("global tiles %d, pairs %d / %d" % (outs[0][2], outs[0][1], outs[1][1]))
    assert 0 < outs[0][1] <= outs[0][2] * 64  # the distinct-pair path was taken
    assert outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][0], outs[1][0])


# ---- the ranking of the palettes ------------------------------------------------------------------------------------------------------------
def _rank_case(npal):
    """-> (feat, use, max_iter).  16 palettes: 15 distinct rows only, far apart, each many times -- two of them equally often -- so every
    palette holds one of them, two palettes tie and the sixteenth stays empty.  1 025 palettes (the first count ranked on the host): 1 100
    distinct rows in 2 600, so most tile counts are 1, 2, 3 or 4 and tie many times over"""
    rng = np.random.default_rng(9000 + npal)
    if npal == 16:
        sizes = [300, 200, 200, 170, 150, 120, 100, 90, 80, 70, 60, 50, 40, 30, 20]
        base = rng.integers(-3000, 3000, size=(len(sizes), 192)).astype(np.int32)
        which = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        return base[which], rng.integers(1, 50, size=which.size).astype(np.uint32), 300
    base = rng.integers(-3000, 3000, size=(1100, 192)).astype(np.int32)
    which = rng.permutation(np.concatenate([np.arange(1100), rng.integers(0, 1100, size=1500)]))
    return base[which], rng.integers(1, 50, size=which.size).astype(np.uint32), 2


@pytest.mark.parametrize("npal", [16, 1025])
def test_rank_palettes(oracle, npal):
    from tiler_amd import stages
    feat, use, max_iter = _rank_case(npal)
    want = oracle.palettize(feat, use, npal, max_iter)
    got = stages.palettize(_dev(feat), _dev(use), npal, max_iter).cpu().numpy()
    counts = np.bincount(want, minlength=npal)
    print("tiles per palette (oracle, first 20): %s; %d palettes share a count with another" % (counts[:20].tolist(), int((np.bincount(counts)[counts] > 1).sum())))
    assert (np.diff(counts) <= 0).all()  # ranked: descending
    assert (np.bincount(counts)[counts[counts > 0]] > 1).any()  # a tie among the palettes that hold tiles
    if npal == 16:
        assert counts[15] == 0 and counts[14] > 0  # one empty palette, ranked last
    assert np.array_equal(got, want)


# ---- round trips ------------------------------------------------------------------------------------------------------------------------------
def test_prepare_palettes_waits_for_the_device_four_times():
    """the resident leg's read-back (with the segment and the first look's counters), the one read of the colour runs (count, bounds,
    flag), the resident pixel k-means' read-back (the centroids stay on the host), and the upload of the optimised palettes"""
    from tiler_amd import stages
    from tiler_amd.encoder import TEncoderStep
    enc = _encoder(_small_clip(), PaletteCount=4, MotionPredictRadius=0)
    enc.Run()  # warm-up: tables, page-locked areas, the pool
    before = stages.host_waits()
    enc.Run(TEncoderStep.esPreparePalettes)
    waits = stages.host_waits() - before
    resident = stages.kmeans_last_resident()
    enc.close()
    print("Run(esPreparePalettes): %d host waits, resident %s" % (waits, resident))
    if not resident:
        pytest.skip("a resident k-means gave up at its barrier: the fallback has reads of its own")
    assert waits <= 4
