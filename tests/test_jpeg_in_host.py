"""The JPEG reader's rule on the host (tm_jpeg.h through tm_jpeg_decode_host), no GPU: against Pillow (libjpeg) on the
files an encoder writes, against the plain restatement tests/jpeg_ref.py on the hand-written cases, every refusal of the container walk,
and seeded damages."""
import io

import numpy as np
import pytest

from tests import jpeg_cases as C
from tests import jpeg_ref, resample_ref, yuv_ref
from tiler_amd import stages
from tiler_amd._lib import TileMotionError

SHAPES = [(8, 8), (16, 16), (17, 23), (33, 49), (72, 64)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def _picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 7 + yy * 3) % 256, (xx * yy + 40) % 256, (255 - xx * 5 + yy) % 256], -1)
    return (a + rng.integers(-24, 25, a.shape)).clip(0, 255).astype(np.uint8)


def pillow_files(w, h):
    """[(what, file)]: sampling x quality x (plain, optimised tables, an interval of one block, of one MCU row)"""
    from PIL import Image
    out = []
    for layout in ("444", "422", "420", "grey"):
        im = Image.fromarray(_picture(w, h, w * 100 + h)).convert("L" if layout == "grey" else "RGB")
        for q in (5, 85, 100):
            for opt in ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}):
                buf = io.BytesIO()
                kw = dict(opt) if layout == "grey" else dict(opt, subsampling=SUBSAMPLING[layout])
                im.save(buf, "JPEG", quality=q, **kw)
                out.append(((layout, q, tuple(opt)), buf.getvalue()))
    return out


def _sizes(f):
    i = stages.jpeg_probe(f)
    return jpeg_ref.plane_sizes(dict(w=i["width"], h=i["height"], ncomp=i["components"], hs=i["h_samp"], vs=i["v_samp"]))


def twin(files):
    """the host twin on a batch -> [(status, planes)]"""
    planes, status, layout = stages.jpeg_decode_host(files)
    sizes = [_sizes(f) for f in files]
    assert np.all(C.outside(planes, layout, sizes) == 0xA5), "a byte outside a file's planes was written"
    return [(status[i], C.unpack(planes, layout, i, sizes[i])) for i in range(len(files))]


@pytest.mark.parametrize("shape", SHAPES)
def test_pillow_files_bit_for_bit(shape):
    pytest.importorskip("PIL")
    from PIL import Image
    w, h = shape
    cases = pillow_files(w, h)
    got = twin([f for _, f in cases])
    worst, total, count = 0, 0.0, 0
    for (what, f), (status, planes) in zip(cases, got):
        layout = what[0]
        assert status == 0, what
        im = Image.open(io.BytesIO(f))
        im.draft("L" if layout == "grey" else "YCbCr", im.size)
        ycc = np.asarray(im)
        assert ycc.shape[:2] == (h, w) and im.mode == ("L" if layout == "grey" else "YCbCr"), what
        assert np.array_equal(planes[0], ycc if layout == "grey" else ycc[..., 0]), ("Y", what)
        rstatus, rplanes, info = jpeg_ref.decode(f)
        assert rstatus == 0 and len(rplanes) == len(planes)
        for c in range(len(planes)):
            assert np.array_equal(planes[c], rplanes[c]), ("the restatement", c, what)
        rgb = np.asarray(Image.open(io.BytesIO(f)).convert("RGB")).astype(np.int64)
        if layout in ("444", "grey"):
            if layout == "444":
                assert np.array_equal(planes[1], ycc[..., 1]) and np.array_equal(planes[2], ycc[..., 2]), ("chroma", what)
            y, u, v = (planes + [np.full_like(planes[0], 128)] * 2)[:3]
            mine = yuv_ref.to_rgb32(y.astype(np.int64), u.astype(np.int64), v.astype(np.int64), yuv_ref.BT601_FULL)
            assert np.array_equal(mine, (rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]).astype(np.uint32)), ("RGB", what)
        else:  # reported, not asserted: libjpeg upsamples with a triangle filter, this build with the Lanczos rule of its YUV input
            geom = (2, 2, 0.5, 0.5) if layout == "420" else (2, 1, 0.5, 0.0)  # JFIF: chroma between the luma samples
            up = [np.asarray(resample_ref.resample(p, w, h, w, h, *geom)).astype(np.int64) for p in planes[1:]]
            mine = yuv_ref.to_rgb32(planes[0].astype(np.int64), up[0], up[1], yuv_ref.BT601_FULL)
            ch = np.stack([(mine >> 16) & 255, (mine >> 8) & 255, mine & 255], -1).astype(np.int64)
            d = np.abs(ch - rgb)
            worst, total, count = max(worst, int(d.max())), total + float(d.sum()), count + d.size
    print("subsampled files at %dx%d: RGB differs from Pillow's by at most %d, %.3f on average" % (w, h, worst, total / max(count, 1)))


def test_hand_written_cases_equal_the_restatement():
    cases = C.good()
    got = twin([f for _, f, _ in cases])
    for (name, f, _), (status, planes) in zip(cases, got):
        rstatus, rplanes, _ = jpeg_ref.decode(f)
        assert status == 0 and rstatus == 0, name
        assert len(planes) == len(rplanes)
        for c in range(len(planes)):
            assert np.array_equal(planes[c], rplanes[c]), (name, c)


def test_probe_reports_the_geometry():
    by_name = {name: f for name, f, _ in C.good()}
    i = stages.jpeg_probe(by_name["444_72x64_ri1"])
    assert (i["width"], i["height"], i["components"], i["h_samp"], i["v_samp"], i["restart_interval"], i["segments"], i["sof"], i["chroma"], i["status"]) == (72, 64, 3, 1, 1, 1, 72, 0, 0, 0)
    i = stages.jpeg_probe(by_name["420_33x49_row"])
    assert (i["h_samp"], i["v_samp"], i["restart_interval"], i["segments"], i["chroma"]) == (2, 2, 3, 4, 2)
    i = stages.jpeg_probe(by_name["sof1_dqt16"])
    assert i["sof"] == 1 and i["segments"] == 1 and i["restart_interval"] == 0
    assert stages.jpeg_probe(by_name["422_17x23"])["chroma"] == 1 and stages.jpeg_probe(by_name["grey_2x2_factors"])["chroma"] == 4
    assert stages.jpeg_probe(dict((n, f) for n, f, _ in C.statuses())["rst_missing"])["status"] == jpeg_ref.BAD_RESTART


def test_a_file_without_dht_equals_its_parent():
    f = dict((n, f) for n, f, _ in C.good())["no_dht"]
    parent = C.no_dht_parent()
    assert b"\xff\xc4" not in f and b"\xff\xc4" in parent
    (s0, p0), (s1, p1) = twin([f, parent])
    assert s0 == 0 and s1 == 0 and all(np.array_equal(a, b) for a, b in zip(p0, p1))


def test_pillows_tables_are_annex_k():
    """what a writer that does not optimise puts into DHT is Annex K.3: with the segments cut out the file decodes to the same planes"""
    pytest.importorskip("PIL")
    f = [f for what, f in pillow_files(17, 23) if what == ("420", 85, ())][0]
    cut = bytearray(f)
    while True:
        at = cut.find(b"\xff\xc4")
        if at < 0 or at > cut.find(b"\xff\xda"):
            break
        del cut[at:at + 2 + int.from_bytes(cut[at + 2:at + 4], "big")]
    assert len(cut) < len(f) - 400
    (s0, p0), (s1, p1) = twin([f, bytes(cut)])
    assert s0 == 0 and s1 == 0 and all(np.array_equal(a, b) for a, b in zip(p0, p1))


@pytest.mark.parametrize("case", C.refused(), ids=[c[0] for c in C.refused()])
def test_the_walk_refuses(case):
    name, f, code, fragment = case
    for call in (lambda: stages.jpeg_probe(f), lambda: stages.jpeg_decode_host([f], 64, 64), lambda: stages.jpeg_decode_host([C.good()[0][1], f], 64, 64)):
        with pytest.raises(TileMotionError) as ei:
            call()
        assert ei.value.code == code and fragment in str(ei.value), str(ei.value)
    assert "file 1" in str(ei.value)
    with pytest.raises(jpeg_ref.Refused) as ri:
        jpeg_ref.walk(f)
    assert ri.value.code == code


@pytest.mark.parametrize("case", C.statuses(), ids=[c[0] for c in C.statuses()])
def test_what_only_decoding_finds_is_a_status(case):
    name, f, want = case
    good = C.good()[1][1]
    got = twin([good, f, good])
    assert [s for s, _ in got] == [0, want, 0]
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1], got[2][1]))
    assert jpeg_ref.decode(f)[0] == want


def test_batch_refusals():
    f = C.good()[0][1]
    with pytest.raises(TileMotionError) as ei:
        stages.jpeg_decode_host([f], 7, 8)  # the file is larger than the planes
    assert ei.value.code == -1
    planes, status, _ = stages.jpeg_decode_host([])
    assert status == []


def test_seeded_damages_reach_the_restatement_s_verdict():
    files = C.damaged(5000)
    verdicts = {}
    batch, want = [], []
    for f in files:
        try:
            rstatus, rplanes, _ = jpeg_ref.decode(f)
        except jpeg_ref.Refused as e:
            with pytest.raises(TileMotionError) as ei:
                stages.jpeg_probe(f)
            assert ei.value.code == e.code, (str(ei.value), str(e))
            verdicts[e.code] = verdicts.get(e.code, 0) + 1
            continue
        batch.append(f)
        want.append((rstatus, rplanes))
        verdicts[rstatus] = verdicts.get(rstatus, 0) + 1
    for k in range(0, len(batch), 500):
        got = twin(batch[k:k + 500])
        for (status, planes), (rstatus, rplanes), f in zip(got, want[k:k + 500], batch[k:k + 500]):
            assert status == rstatus, f.hex()
            if status == 0:
                assert all(np.array_equal(a, b) for a, b in zip(planes, rplanes)), f.hex()
    print("verdicts of 5000 damaged files:", dict(sorted(verdicts.items())))
    assert verdicts.get(0, 0) > 200 and verdicts.get(jpeg_ref.TRUNCATED, 0) > 200 and verdicts.get(jpeg_ref.IO, 0) > 100
