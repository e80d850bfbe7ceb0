"""JPEG input on the device (tm_jpeg_in.hip): k_jpeg_decode through its stage seam against the host twin, and Load of
JPEG sequences and of lent JPEG files under TM_JPEG_DECODE=device against the host path.  The files are written by the tests' own writer
(tests/jpeg_cases.py): no imaging library takes part."""
import os

import numpy as np
import pytest

from tests import jpeg_cases as C
from tests import jpeg_ref, resample_ref, yuv_ref
from tiler_amd import synth
from tiler_amd._lib import TileMotionError
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S

pytestmark = pytest.mark.gpu

E_INVAL, E_UNSUPPORTED = -1, -6
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=150)
CHROMA = {"444": 0, "420": 2, "grey": 4}  # TM_CHROMA_*


@pytest.fixture(scope="module")
def stages():
    import torch
    from tiler_amd import stages
    assert torch.cuda.is_available()
    return stages


def _sizes(stages, f):
    i = stages.jpeg_probe(f)
    return jpeg_ref.plane_sizes(dict(w=i["width"], h=i["height"], ncomp=i["components"], hs=i["h_samp"], vs=i["v_samp"]))


def _both(stages, files):
    """the batch through the kernel and through the host twin: every byte of the planes and of the guards around them, and the statuses"""
    dev, dstatus, dl = stages.jpeg_decode(files)
    host, hstatus, hl = stages.jpeg_decode_host(files)
    assert dl == hl
    sizes = [_sizes(stages, f) for f in files]
    assert np.all(C.outside(host, hl, sizes) == 0xA5)
    dev = [p.cpu().numpy() for p in dev]
    return dev, dstatus, host, hstatus, hl, sizes


def test_every_good_case_in_one_launch(stages):
    cases = C.good()
    files = [f for _, f, _ in cases]
    dev, dstatus, host, hstatus, layout, sizes = _both(stages, files)
    assert dstatus == hstatus == [0] * len(files)
    for c in range(3):
        assert np.array_equal(dev[c], host[c]), "plane %d or its guards" % c
    # and the twin's planes are the restatement's (the host test holds every case to it; here the two largest)
    for name in ("444_72x64_ri1", "420_33x49_row"):
        i = [n for n, _, _ in cases].index(name)
        for a, b in zip(C.unpack(dev, layout, i, sizes[i]), jpeg_ref.decode(files[i])[1]):
            assert np.array_equal(a, b), name


def test_damaged_files_beside_good_neighbours(stages):
    good = [f for n, f, _ in C.good() if n in ("420_17x23", "444_72x64_ri1", "grey_33x49_ri1")]
    bad = []
    for f in C.damaged(3000, seed=11):
        try:
            stages.jpeg_probe(f)  # (what the walk refuses fails the call: the host test covers it)
        except TileMotionError:
            continue
        bad.append(f)
        if len(bad) == 500:
            break
    assert len(bad) == 500
    bad += [f for _, f, _ in C.statuses()]
    files = []
    for k, f in enumerate(bad):
        files += [f, good[k % len(good)]]
    dev, dstatus, host, hstatus, layout, sizes = _both(stages, files)
    assert dstatus == hstatus
    assert all(s == 0 for s in dstatus[1::2]) and sum(s != 0 for s in dstatus[0::2]) > 150
    for c in range(3):
        assert np.array_equal(dev[c], host[c]), "plane %d or its guards" % c  # (a refused segment stops where the twin's stops)
    want = []
    for g in good:
        planes, _, lay = stages.jpeg_decode_host([g])
        want.append(C.unpack(planes, lay, 0, _sizes(stages, g)))
    for k in range(len(bad)):
        for a, b in zip(C.unpack(dev, layout, 2 * k + 1, sizes[2 * k + 1]), want[k % len(good)]):
            assert np.array_equal(a, b)


def test_batch_refusals(stages):
    good = C.good()[0][1]
    with pytest.raises(TileMotionError) as ei:
        stages.jpeg_decode([good, C.refused()[0][1]], 64, 64)
    assert ei.value.code == E_UNSUPPORTED and "file 1" in str(ei.value)
    with pytest.raises(TileMotionError) as ei:
        stages.jpeg_decode([good], 7, 8)
    assert ei.value.code == E_INVAL
    assert stages.jpeg_decode([])[1] == []


# ---- Load
def _encoder(**kw):
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in {**BASE, **kw}.items():
        setattr(enc, k, v)
    return enc


def _clip_rgb(nf, w, h):
    fr = synth.video(nf, w, h, cut=max(nf // 2, 1)) & 0xffffff
    return np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8)


def _files(nf, w, h, layout, **kw):
    return [C.encode_rgb(fr, layout, **kw) for fr in _clip_rgb(nf, w, h)]


def _twin_planes(stages, files):
    """[Y, U, V] as arrays [F][ph][pw] of the host twin's planes"""
    planes, status, layout = stages.jpeg_decode_host(files)
    assert status == [0] * len(files)
    sizes = _sizes(stages, files[0])
    per_file = [C.unpack(planes, layout, i, sizes) for i in range(len(files))]
    return [np.stack([p[c] for p in per_file]) for c in range(len(sizes))]


def _expected_rgb32(stages, files, layout):
    import torch
    planes = _twin_planes(stages, files)
    h, w = planes[0].shape[1:]
    if layout in CHROMA:  # the stage seam of the kernel Load converts with
        t = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes] + [None, None]
        return stages.yuv_to_rgb32(t[0], t[1], t[2], CHROMA[layout], w, h, yuv_ref.BT601_FULL).cpu().numpy().view(np.uint32)
    # 4:2:2 sited between the luma pairs is no public layout: the rule's restatement
    up = [resample_ref.resample(p, w, h, w, h, 2, 1, 0.5, 0.0).astype(np.int64) for p in planes[1:]]
    return yuv_ref.to_rgb32(resample_ref.resample(planes[0], w, h, w, h).astype(np.int64), up[0], up[1], yuv_ref.BT601_FULL)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("layout", ["420", "444", "422", "grey"])
def test_lent_files_give_the_planes_converted(stages, monkeypatch, layout, where):
    monkeypatch.setenv("TM_JPEG_DECODE", where)
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "4")  # 6 frames in two chunks, the last one short
    nf, w, h = 6, 33, 49
    files = _files(nf, w, h, layout, ri=0 if layout == "444" else 3)
    enc = _encoder(MotionPredictRadius=0, Scaling=0.5)  # (Scaling stays ignored)
    assert enc.SetFramesJPEG(files, 30.0) == dict(width=w, height=h, fps=30.0, frames=nf)
    enc.Run(S.esLoad)
    got = enc.RenderFrames(input=True, device=False)
    assert got.shape == (nf, 56, 40)  # (rendered in whole tiles)
    assert np.array_equal(got[:, :h, :w], _expected_rgb32(stages, files, layout))
    st = enc.InputStats()
    assert st["where"] == where and st["kind"] == 12 and st["frames"] == nf and st["file_bytes"] == sum(len(f) for f in files)
    if layout == "444":  # no chroma rule takes part: the restatement's planes through the pixel rule, lent as RGB
        rgb = np.stack([jpeg_ref.to_rgb_444(jpeg_ref.decode(f)[1]) for f in files])
        ref = _encoder(MotionPredictRadius=0)
        ref.SetFramesRGB(rgb, "rgb24", fps=30.0)
        ref.Run(S.esLoad)
        assert np.array_equal(got, ref.RenderFrames(input=True, device=False))
        ref.close()
    enc.Run(S.esLoad)  # the clip it has
    enc.SetFramesJPEG(files[:2], 30.0)  # lending again after Load
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), got[:2])
    for bad in ([], [b""], [files[0][:40]], [b"x" * 100]):
        with pytest.raises(TileMotionError):
            enc.SetFramesJPEG(bad, 30.0)
    enc.close()


def test_a_sequence_on_the_device_equals_the_host_path(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    nf, w, h = 6, 64, 48
    files = _files(nf, w, h, "420", ri=4)
    for f, data in enumerate(files):
        open("seq_%04d.jpg" % f, "wb").write(data)
    for f in (3, nf - 2):
        open("seq_%04d.kf" % f, "wb").close()
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "4")
    want = _expected_rgb32(stages, files, "420")
    got = {}
    for where in ("host", "device"):
        monkeypatch.setenv("TM_JPEG_DECODE", where)
        enc = _encoder(InputFileName="seq_%.4d.jpg", OutputFileName="out.gtm", MotionPredictRadius=0, Scaling=0.5)
        assert enc.OpenInput() == dict(width=w, height=h, fps=24.0, frames=nf)
        enc.Run(S.esLoad)
        st = enc.InputStats()
        assert st["where"] == where and st["kind"] == 8 and st["frames"] == nf and st["file_bytes"] == sum(len(f) for f in files)
        assert np.array_equal(enc.RenderFrames(input=True, device=False), want)
        assert enc.KeyFrames().tolist() == [0, 3, nf - 2]
        enc.Run()
        enc.Save()
        got[where] = open("out.gtm", "rb").read()
        os.remove("out.gtm")
        enc.close()
    assert got["device"] == got["host"] and len(got["host"]) > 1000


def test_set_jpeg_decode_and_the_environment(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("TM_JPEG_DECODE", raising=False)
    for f, data in enumerate(_files(2, 32, 24, "420")):
        open("seq_%04d.jpg" % f, "wb").write(data)
    enc = _encoder(InputFileName="seq_%.4d.jpg")
    assert enc.JpegDecode() == "auto"
    with pytest.raises(TileMotionError):
        enc.SetJpegDecode(7)
    for setting, env, want in (("auto", None, "host"), ("host", None, "host"), ("device", None, "device"), ("device", "host", "host"), ("host", "device", "device")):  # (auto: no restart markers)
        enc.SetJpegDecode(setting)
        assert enc.JpegDecode() == setting
        if env:
            monkeypatch.setenv("TM_JPEG_DECODE", env)
        enc.OpenInput()
        enc.Run(S.esLoad)
        assert enc.InputStats()["where"] == want, (setting, env)
    enc.close()
    monkeypatch.delenv("TM_JPEG_DECODE")
    for ri, want in ((2, "host"), (1, "device")):  # auto goes by the first file's segments: two of two MCUs, four of one
        for f, data in enumerate(_files(2, 32, 24, "420", ri=ri)):
            open("rst%d_%04d.jpg" % (ri, f), "wb").write(data)
        enc = _encoder(InputFileName="rst%d_%%.4d.jpg" % ri)
        enc.OpenInput()
        enc.Run(S.esLoad)
        assert enc.InputStats()["where"] == want, ri
        enc.close()


def test_refusals_name_the_file_like_the_host_path(stages, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    files = _files(5, 64, 48, "420", ri=4)
    other = _files(1, 64, 40, "420")[0]
    sampled = _files(1, 64, 48, "444")[0]
    damaged = bytearray(files[2])
    damaged[damaged.find(b"\xff\xda") + 40] ^= 0x55
    assert stages.jpeg_decode_host([bytes(damaged)])[1][0] != 0
    progressive = bytearray(files[0])
    progressive[progressive.find(b"\xff\xc0") + 1] = 0xc2
    for stem, third in (("size", other), ("samp", sampled), ("dmg", bytes(damaged))):
        for f, data in enumerate(files):
            open("%s_%04d.jpg" % (stem, f), "wb").write(third if f == 2 else data)
    open("prog_0000.jpg", "wb").write(bytes(progressive))
    enc = _encoder(InputFileName="prog_%.4d.jpg")
    with pytest.raises(TileMotionError) as ei:
        enc.OpenInput()
    assert ei.value.code == E_UNSUPPORTED and "SOF2" in str(ei.value) and "prog_0000.jpg" in str(ei.value)
    enc.close()
    seen = {}
    for where in ("host", "device"):
        monkeypatch.setenv("TM_JPEG_DECODE", where)
        for stem in ("size", "samp", "dmg"):
            enc = _encoder(InputFileName=stem + "_%.4d.jpg")
            enc.OpenInput()
            with pytest.raises(TileMotionError) as ei:
                enc.Run(S.esLoad)
            seen[where, stem] = ei.value.code
            assert stem + "_0002.jpg" in str(ei.value), str(ei.value)
            # the encoder is usable afterwards
            for f, data in enumerate(files):
                open("%s_%04d.jpg" % (stem, f), "wb").write(data)
            enc.OpenInput()
            enc.Run(S.esLoad)
            assert enc.RenderFrames(input=True, device=False).shape == (5, 48, 64)
            open("%s_0002.jpg" % stem, "wb").write({"size": other, "samp": sampled, "dmg": bytes(damaged)}[stem])
            enc.close()
    assert all(code == E_INVAL for code in seen.values()) and len(seen) == 6
    # a PNG pattern behaves as before: the first file decides
    open("p_0000.jpg", "wb").write(b"\x89PNG\r\n\x1a\n" + bytes(40))
    enc = _encoder(InputFileName="p_%.4d.jpg")
    with pytest.raises(TileMotionError) as ei:
        enc.OpenInput()
    assert "PNG" in str(ei.value) or "IHDR" in str(ei.value) or "chunk" in str(ei.value) or "CRC" in str(ei.value)
    enc.close()
