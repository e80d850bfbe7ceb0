"""PNG input on the device (tm_png_in.hip): k_inflate and k_png_unfilter through their stage seams against zlib and
against the host reader, and Load of PNG sequences and of lent PNG files under TM_PNG_DECODE=device against the host path."""
import ctypes
import io
import os
import zlib

import numpy as np
import pytest

from tests import png_cases
from tests import png_in_cases as C
from tiler_amd import lib, synth
from tiler_amd._lib import TileMotionError
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S

pytestmark = pytest.mark.gpu

E_INVAL = -1
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=150)


@pytest.fixture(scope="module")
def stages():
    import torch
    from tiler_amd import stages
    assert torch.cuda.is_available()
    return stages


def _guarded(stages, spans, caps, order, shift=0):
    """the streams `order` names in one launch: destinations 48 + (i % 5) bytes apart (never a multiple of 16 twice running), sources at
    offsets that are no multiples of 4; everything outside a destination must come back 0xA5 -> [(code, in_pos, out_n, bytes)] in order"""
    dst_offs, src_offs, at, sat = [], [], 3 + shift, 1
    for i in order:
        dst_offs.append(at)
        at += caps[i] + 48 + (i % 5)
        for s in spans[i]:
            if sat % 4 == 0:
                sat += 1
            src_offs.append(sat)
            sat += len(s)
    dst, status = stages.inflate([list(spans[i]) for i in order], [caps[i] for i in order], dst_offs, src_offs, guard=64)
    dst = dst.cpu().numpy()
    used = np.zeros(dst.size, bool)
    out = []
    for k, i in enumerate(order):
        code, in_pos, out_n = status[k]
        assert out_n <= caps[i]
        used[dst_offs[k]:dst_offs[k] + (out_n if code == 0 else caps[i])] = True  # (a refused stream may have written inside its own destination)
        out.append((code, in_pos, out_n, dst[dst_offs[k]:dst_offs[k] + out_n].tobytes()))
    assert np.all(dst[~used] == 0xA5), "a byte outside the decoded data was written"
    return out


def test_every_stream_in_one_launch_shuffled_and_alone(stages):
    cases = C.streams()
    spans = [s for _, s, _, _ in cases]
    caps = [len(d) for _, _, d, _ in cases]
    orders = [list(range(len(cases))), list(np.random.default_rng(5).permutation(len(cases)))]
    for shift, order in enumerate(orders):
        got = _guarded(stages, spans, caps, order, shift * 7)
        for k, i in enumerate(order):
            name, sp, data, zlib_ok = cases[i]
            z = b"".join(sp)
            if zlib_ok:
                assert zlib.decompress(z) == data
            assert got[k] == (0, len(z), len(data), data), (name, got[k][:3])
    for i in (0, 8, len(cases) - 2):  # alone: the empty stream, the 1 MiB stream, a span list with empty spans
        name, sp, data, _ = cases[i]
        assert _guarded(stages, spans, caps, [i]) == [(0, len(b"".join(sp)), len(data), data)], name


def _twin_codes(streams, caps):
    from tiler_amd._lib import InflateStatus, inflate_batch
    blob, spans, descs, dst_bytes, nspans = inflate_batch(streams, caps)
    dst = np.zeros(dst_bytes + 16, np.uint8)
    st = (InflateStatus * len(streams))()
    assert lib().tm_inflate_streams_host(blob.ctypes.data_as(ctypes.c_void_p), blob.size, spans, nspans, descs, len(streams), dst.ctypes.data_as(ctypes.c_void_p), dst_bytes, st) == 0
    return [(s.code, s.in_pos) for s in st]


def test_damaged_streams_beside_good_ones(stages):
    """refusals, which the kernel bounds by construction (the random fuzz is the host program's: tools/asan_png_in.sh)"""
    bad = C.damaged_streams()
    good = [c for c in C.streams() if len(c[2]) <= 70000][:len(bad)]
    spans, caps = [], []
    for k in range(len(bad)):
        spans += [(bad[k][1],), good[k % len(good)][1]]
        caps += [bad[k][2], len(good[k % len(good)][2])]
    got = _guarded(stages, spans, caps, list(range(len(spans))))
    twin = _twin_codes([b"".join(s) for s in spans], caps)
    for k in range(len(bad)):
        code, in_pos, out_n, _ = got[2 * k]
        assert code != 0 and out_n == 0 and (code, in_pos) == twin[2 * k], (bad[k][0], code, in_pos, twin[2 * k])
        name, sp, data, _ = good[k % len(good)]
        assert got[2 * k + 1] == (0, len(b"".join(sp)), len(data), data), name


@pytest.fixture(scope="module")
def expected_pixels(tmp_path_factory):
    """tm_read_png_host of every picture, once"""
    d = tmp_path_factory.mktemp("png_in")
    out = {}
    for name, w, h, png in C.pictures():
        p = d / "p.png"
        p.write_bytes(png)
        out[name] = png_cases.read_png_host(p, w, h)
    return out


def test_every_picture_against_the_host_reader(stages, expected_pixels):
    by_shape = {}
    for case in C.pictures():
        by_shape.setdefault((case[1], case[2]), []).append(case)
    for (w, h), cases in by_shape.items():
        pad = 0 if (w + h) % 2 else 37  # a padded frame stride for half of the shapes
        out, status = stages.png_decode([c[3] for c in cases], w, h, w * h + pad)
        out = out.cpu().numpy().view(np.uint32)
        assert status == [0] * len(cases), (w, h, status)
        for k, (name, _, _, _) in enumerate(cases):
            assert np.array_equal(out[k, :w * h].reshape(h, w), expected_pixels[name]), name
        assert np.all(out[:, w * h:] == 0xFFFFFFFF)


def test_batches_of_1_2_and_70_files(stages, expected_pixels):
    cases = [c for c in C.pictures() if (c[1], c[2]) == (5, 3)] + [c for c in C.pictures() if (c[1], c[2]) == (37, 21)]
    for shape in ((5, 3), (37, 21)):
        same = [c for c in cases if (c[1], c[2]) == shape]
        for n in (1, 2, 70):
            batch = [same[(3 * k) % len(same)] for k in range(n)]  # files of mixed sizes, colour types and filters in one batch
            out, status = stages.png_decode([c[3] for c in batch], *shape)
            out = out.cpu().numpy().view(np.uint32)
            assert status == [0] * n
            for k, c in enumerate(batch):
                assert np.array_equal(out[k].reshape(shape[1], shape[0]), expected_pixels[c[0]]), (n, c[0])


def test_damaged_pictures_beside_good_ones(stages, expected_pixels):
    bad = C.damaged_pictures()
    w, h = bad[0][1], bad[0][2]
    rows, _ = C._content(w, h, 2, 16)
    good = C.make_png(rows, w, h, 2, [4] * h)
    files = []
    for c in bad:
        files += [c[3], good]
    out, status = stages.png_decode(files, w, h)
    from tests.test_png_in_host import decode_host
    rc, want, want_status = decode_host(files, w, h)
    assert rc == 0 and status == want_status and [s != 0 for s in status] == [True, False] * len(bad), (status, want_status)
    out = out.cpu().numpy().view(np.uint32)
    for k in range(len(bad)):
        assert np.array_equal(out[2 * k + 1], want[2 * k + 1])
    with pytest.raises(TileMotionError) as ei:
        stages.png_decode([good, good[:len(good) // 2]], w, h)
    assert ei.value.code == E_INVAL and "file 1" in str(ei.value)


# ---- Load
def _encoder(**kw):
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    for k, v in {**BASE, **kw}.items():
        setattr(enc, k, v)
    return enc


def _clip(nf, w, h):
    return synth.video(nf, w, h, cut=max(nf // 2, 1)) & 0xffffff


def _write_sequence(frames, stem, writer):
    """the clip as <stem>_NNNN.png: by Pillow at its defaults, or by this library's level-1 export -> the files' bytes"""
    from PIL import Image
    files = []
    if writer == "pillow":
        for f, fr in enumerate(frames):
            rgb = np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(rgb, "RGB").save(buf, "PNG")
            files.append(buf.getvalue())
    else:
        files = png_cases.encode_host(np.ascontiguousarray(frames, np.uint32), 1, "adaptive")
    for f, data in enumerate(files):
        with open("%s_%04d.png" % (stem, f), "wb") as fh:
            fh.write(data)
    return files


@pytest.mark.parametrize("writer", ["pillow", "own"])
@pytest.mark.parametrize("shape", [(6, 64, 48), (40, 264, 136)])
def test_load_on_the_device_equals_the_host_path(tmp_path, monkeypatch, shape, writer):
    monkeypatch.chdir(tmp_path)
    nf, w, h = shape
    frames = _clip(nf, w, h)
    files = _write_sequence(frames, "seq", writer)
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "32")  # the 40-frame clip crosses a chunk
    for f in (3, nf - 2):
        open("seq_%04d.kf" % f, "wb").close()
    got = {}
    for where in ("host", "device"):
        monkeypatch.setenv("TM_PNG_DECODE", where)
        enc = _encoder(InputFileName="seq_%.4d.png", OutputFileName="out.gtm", MotionPredictRadius=0)  # (the stream holds the settings' text: one name)
        assert enc.OpenInput() == dict(width=w, height=h, fps=24.0, frames=nf)
        enc.Run(S.esLoad)
        st = enc.InputStats()
        assert st["where"] == where and st["frames"] == nf and st["file_bytes"] == sum(len(f) for f in files)
        if where == "device":
            assert st["bytes_uploaded"] <= st["file_bytes"] + 1024 * nf, st  # only the files and their descriptors cross
        else:
            assert st["bytes_uploaded"] == nf * w * h * 4
        src = enc.RenderFrames(input=True, device=False)
        assert np.array_equal(src, frames)
        assert enc.KeyFrames().tolist() == [0, 3, nf - 2]
        enc.Run(S.esLoad)  # a second Load reads the clip it has
        assert np.array_equal(enc.RenderFrames(input=True, device=False), frames)
        enc.Run()
        enc.Save()
        got[where] = open("out.gtm", "rb").read()
        os.remove("out.gtm")
        enc.close()
    assert got["device"] == got["host"] and len(got["host"]) > 1000


def test_start_frame_and_frame_count(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _clip(14, 64, 48)
    _write_sequence(frames, "seq", "own")
    open("seq_0004.kf", "wb").close()
    monkeypatch.setenv("TM_PNG_DECODE", "device")
    monkeypatch.setenv("TM_INPUT_CHUNK_FRAMES", "4")  # 9 frames in three chunks, the last one short
    enc = _encoder(InputFileName="seq_%.4d.png", StartFrame=2, FrameCount=9, MotionPredictRadius=0)
    enc.Run(S.esLoad)
    assert enc.KeyFrames().tolist() == [0, 2] and enc.InputStats()["frames"] == 9
    assert np.array_equal(enc.RenderFrames(input=True, device=False), frames[2:11])
    enc.close()


def test_set_png_decode_and_the_environment(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("TM_PNG_DECODE", raising=False)
    frames = _clip(3, 64, 48)
    _write_sequence(frames, "seq", "pillow")
    enc = _encoder(InputFileName="seq_%.4d.png")
    assert enc.PngDecode() == "auto"
    with pytest.raises(TileMotionError):
        enc.SetPngDecode(7)
    for setting, env, want in (("auto", None, "device"), ("host", None, "host"), ("device", None, "device"), ("device", "host", "host"), ("host", "device", "device")):
        enc.SetPngDecode(setting)
        assert enc.PngDecode() == setting
        if env:
            monkeypatch.setenv("TM_PNG_DECODE", env)
        enc.OpenInput()
        enc.Run(S.esLoad)
        assert enc.InputStats()["where"] == want, (setting, env)
        assert np.array_equal(enc.RenderFrames(input=True, device=False), frames)
    enc.close()


def test_refusals_name_the_file_like_the_host_path(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    frames = _clip(5, 64, 48)
    files = _write_sequence(frames, "size", "pillow")
    _write_sequence(_clip(1, 64, 40), "other", "pillow")
    os.replace("other_0000.png", "size_0002.png")  # another size in the middle
    _write_sequence(frames, "dmg", "pillow")
    at = files[3].index(b"IDAT") + 4
    n = int.from_bytes(files[3][at - 8:at - 4], "big")
    z = bytearray(files[3][at:at + n])
    z[len(z) // 2] ^= 0x55  # the stream is damaged, the chunk's CRC is mended
    open("dmg_0003.png", "wb").write(files[3][:at - 8] + C.chunk(b"IDAT", bytes(z)) + files[3][at + n + 4:])
    seen = {}
    for where in ("host", "device"):
        monkeypatch.setenv("TM_PNG_DECODE", where)
        for stem, name in (("size", "size_0002.png"), ("dmg", "dmg_0003.png")):
            enc = _encoder(InputFileName=stem + "_%.4d.png")
            enc.OpenInput()
            with pytest.raises(TileMotionError) as ei:
                enc.Run(S.esLoad)
            seen[where, stem] = ei.value.code
            if where == "device" or stem == "size":
                assert name in str(ei.value), str(ei.value)  # (the host path's inflate does not know its file's name)
            # the encoder is usable afterwards
            enc.SetVideo(64, 48, 24.0, 5)
            for f in range(5):
                enc.PushFrame(f, frames[f])
            enc.Run(S.esLoad)
            assert np.array_equal(enc.RenderFrames(input=True, device=False), frames)
            enc.close()
    assert seen["device", "size"] == seen["host", "size"] == E_INVAL and seen["device", "dmg"] == seen["host", "dmg"] == E_INVAL


# ---- lent files
def _tables(enc):
    nf = enc.counts()["frames"]
    hdr, pal, rgb = enc.Tiles()
    return dict(tilemaps=np.stack([enc.TileMap(f) for f in range(nf)]), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(), keyframes=enc.KeyFrames())


@pytest.mark.parametrize("where", ["host", "device"])
def test_lent_files_give_what_the_decoded_pixels_give(tmp_path, monkeypatch, where):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_PNG_DECODE", where)
    nf, w, h = 40, 264, 136
    frames = _clip(nf, w, h)
    files = _write_sequence(frames, "seq", "own")
    ref = _encoder(MotionPredictRadius=0)
    rgb = np.stack([(frames >> 16) & 255, (frames >> 8) & 255, frames & 255], -1).astype(np.uint8)
    ref.SetFramesRGB(rgb, "rgb24", fps=30.0)
    ref.Run()
    want = _tables(ref)
    ref.close()
    enc = _encoder(MotionPredictRadius=0, Scaling=0.5)  # (Scaling stays ignored for PNGs)
    assert enc.SetFramesPNG(files, 30.0) == dict(width=w, height=h, fps=30.0, frames=nf)
    enc.Run()
    got = _tables(enc)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    st = enc.InputStats()
    assert st["where"] == where and st["kind"] == 6 and st["frames"] == nf
    enc.Run(S.esLoad)  # the clip it has
    enc.SetFramesPNG(files[:7], 30.0)  # lending again after Load
    enc.Run(S.esLoad)
    assert np.array_equal(enc.RenderFrames(input=True, device=False), frames[:7])
    # refusals: at the call, and a file of another size at Load
    for bad in ([], [b""], [files[0][:40]], [b"x" * 100]):
        with pytest.raises(TileMotionError):
            enc.SetFramesPNG(bad, 30.0)
    with pytest.raises(TileMotionError):
        enc.SetFramesPNG(files[:2], 0.0)
    small = _write_sequence(_clip(1, 64, 40), "small", "pillow")
    enc.SetFramesPNG([files[0], small[0], files[1]], 30.0)
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esLoad)
    assert ei.value.code == E_INVAL and "frame 1" in str(ei.value)
    enc.close()


def test_device_group_of_two_shards(tmp_path, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("two devices are needed")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TM_PNG_DECODE", "device")
    frames = _clip(12, 64, 48)
    _write_sequence(frames, "seq", "own")
    one = _encoder(InputFileName="seq_%.4d.png", MotionPredictRadius=0)
    one.Run()
    want = _tables(one)
    one.close()
    grp = TilingEncoder()
    grp.SetDevices([0, 1])
    grp.LoadDefaultSettings()
    for k, val in {**BASE, "InputFileName": "seq_%.4d.png", "MotionPredictRadius": 0}.items():
        setattr(grp, k, val)
    grp.Run()
    got = _tables(grp)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    grp.close()
