"""One process, several devices (tm_set_devices / tm_set_device_mask): the encoder becomes a group of shards, each on its own host thread,
and Run(step) shards and merges inside the library through its in-process communicator.  Shards may share a device, so a one-GPU box
rehearses the whole path: every result must be the single encoder's, bit for bit."""
import ctypes
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from tiler_amd._lib import TileMotionError
from tiler_amd.encoder import TilingEncoder, TEncoderStep as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "tiler_amd", "lib")
NF, W, H = 12, 64, 48
BASE = dict(PaletteCount=3, ShotTransMinSecondsPerKF=0.1, GlobalTilingTileCount=150)


def _clip(seed=None):
    from tiler_amd import synth
    return synth.video(NF, W, H, cut=3) if seed is None else synth.video(NF, W, H, seed=seed, cut=4)


def _encoder(devices=None, frames=None, host=False, **kw):
    enc = TilingEncoder()
    if devices is not None:
        enc.SetDevices(devices)
    enc.LoadDefaultSettings()
    for k, v in {**BASE, **kw}.items():
        setattr(enc, k, v)
    enc.SetVideo(W, H, 24.0, NF)
    if frames is not None:
        if host:
            enc.SetFramesHost(frames)
        else:
            for f in range(NF):
                enc.PushFrame(f, frames[f])
    return enc


def _state(enc):
    hdr, pal, rgb = enc.Tiles()
    return dict(tilemaps=np.stack([enc.TileMap(f) for f in range(NF)]), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(),
                keyframes=enc.KeyFrames(), correl=enc.FrameCorrelations().view(np.uint32))


def _assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), k


_REF = {}


def _reference(tmp_path_factory, frames_seed=None, **kw):
    """the single encoder's state and the .gtm it writes as "clip.gtm" (a relative name: the file embeds its settings, the name included)"""
    key = (frames_seed, tuple(sorted(kw.items())), os.environ.get("TM_PP_SHARDED"))
    if key not in _REF:
        here = os.getcwd()
        os.chdir(str(tmp_path_factory.mktemp("ref")))
        try:
            enc = _encoder(frames=_clip(frames_seed), OutputFileName="clip.gtm", **kw)
            enc.Run()
            _REF[key] = (_state(enc), open("clip.gtm", "rb").read())
            enc.close()
        finally:
            os.chdir(here)
    return _REF[key]


@pytest.mark.parametrize("pp_sharded", [False, True])
@pytest.mark.parametrize("epu", [False, True])
@pytest.mark.parametrize("radius", [0, 8])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0], [0] * 5])
def test_group_equals_the_single_encoder(monkeypatch, tmp_path, tmp_path_factory, devices, radius, epu, pp_sharded):
    """the clip and settings of test_sharded_ranks_merge_to_the_single_run; tile maps, tiles, palettes, key frames, correlations and the
    .gtm that Run(esAll) writes are the single encoder's"""
    if pp_sharded:
        monkeypatch.setenv("TM_PP_SHARDED", "1")
    else:
        monkeypatch.delenv("TM_PP_SHARDED", raising=False)
    want, want_gtm = _reference(tmp_path_factory, MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=epu)
    monkeypatch.chdir(tmp_path)
    enc = _encoder(devices, _clip(), MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=epu, OutputFileName="clip.gtm")
    enc.Run()
    _assert_same(_state(enc), want)
    assert open("clip.gtm", "rb").read() == want_gtm
    assert enc.CollectiveStats()["bytes"] > 0  # the merges went through the group's communicator
    enc.close()


def test_group_equals_the_single_encoder_at_another_dithering_mode(monkeypatch, tmp_path, tmp_path_factory):
    """test_group_equals_the_single_encoder with DitheringMode = 3 on three shards, the clustering sharded (every shard makes the clustering
    features of its own share of the tiles): the setting reaches every shard, and it matters on this clip"""
    monkeypatch.setenv("TM_PP_SHARDED", "1")
    kw = dict(MotionPredictRadius=8, FrameTilingExtendedPaletteUsage=True)
    default, _ = _reference(tmp_path_factory, **kw)
    want, want_gtm = _reference(tmp_path_factory, DitheringMode=3, **kw)
    a, b = want["hdr"]["PalIdx_Initial"], default["hdr"]["PalIdx_Initial"]
    assert a.shape != b.shape or (a != b).any(), "DitheringMode=3 changes no tile's palette here"
    monkeypatch.chdir(tmp_path)
    enc = _encoder([0, 0, 0], _clip(), DitheringMode=3, OutputFileName="clip.gtm", **kw)
    assert enc.DitheringMode == 3
    enc.Run()
    _assert_same(_state(enc), want)
    assert open("clip.gtm", "rb").read() == want_gtm
    assert enc.CollectiveStats()["bytes"] > 0
    enc.close()


def test_group_from_host_clips_and_prefetch(tmp_path_factory):
    """the host-clip Load (every shard loads the whole clip) and a second clip queued by PrefetchFramesHost"""
    a, b = _clip(), _clip(seed=7)
    want_a, _ = _reference(tmp_path_factory, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    want_b, _ = _reference(tmp_path_factory, frames_seed=7, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    enc = _encoder([0, 0], a, host=True, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    enc.PrefetchFramesHost(b)
    enc.Run()
    _assert_same(_state(enc), want_a)
    enc.SetFramesHost(b)
    enc.Run()
    _assert_same(_state(enc), want_b)
    enc.close()


@pytest.mark.parametrize("radius", [0, 8])
def test_group_step_by_step(tmp_path_factory, radius):
    """every step run on its own gives what TM_STEP_ALL gives; a step out of order fails and leaves the group usable"""
    want, _ = _reference(tmp_path_factory, MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=True)
    enc = _encoder([0, 0, 0], _clip(), MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=True)
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esReduce)
    assert ei.value.code == -1
    for step in (S.esLoad, S.esPredictMotion, S.esReduce, S.esPreparePalettes, S.esDither, S.esReconstruct, S.esReindex):
        enc.Run(step)
    _assert_same(_state(enc), want)
    enc.close()


@pytest.mark.parametrize("radius", [0, 8])
def test_group_quality_and_render(radius):
    """FrameQuality over the clip and over a range across a shard border, and both renders, are the single encoder's"""
    frames = _clip()
    kw = dict(MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=False)
    ref = _encoder(frames=frames, **kw)
    ref.Run()
    enc = _encoder([0, 0], frames, **kw)
    enc.Run()
    for first, count in ((0, NF), (3, 6), (5, 2)):  # shard 0 loaded frames 0-5, shard 1 frames 6-11
        a, b = ref.FrameQuality(first, count), enc.FrameQuality(first, count)
        for k in ("sse", "psnr", "ssim_y"):
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (first, count, k)
        assert a["clip_psnr"] == b["clip_psnr"] and a["clip_ssim_y"] == b["clip_ssim_y"]
    for inp in (False, True):
        assert np.array_equal(ref.RenderFrames(input=inp, device=False), enc.RenderFrames(input=inp, device=False))
        assert np.array_equal(ref.RenderFrames(input=inp, device=True).cpu().numpy(), enc.RenderFrames(input=inp, device=True).cpu().numpy())
        assert np.array_equal(ref.RenderFrames(4, 5, input=inp, device=False), enc.RenderFrames(4, 5, input=inp, device=False))
    ref.close()
    enc.close()


_PROG = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)


def _progress_events(enc):
    events = []
    cb = _PROG(lambda user, step, pos, mx, hg: events.append((threading.get_ident(), step, pos, mx)))
    enc._L.tm_set_progress_cb(ctypes.c_void_p(enc._h), ctypes.cast(cb, ctypes.c_void_p), None)
    enc.Run()
    enc._L.tm_set_progress_cb(ctypes.c_void_p(enc._h), None, None)
    return events, cb


@pytest.mark.parametrize("radius", [0, 8])
def test_group_progress_on_the_calling_thread(radius):
    frames = _clip()
    kw = dict(MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=True)
    ref = _encoder(frames=frames, **kw)
    want, _cb0 = _progress_events(ref)
    enc = _encoder([0, 0, 0], frames, **kw)
    got, _cb1 = _progress_events(enc)
    me = threading.get_ident()
    assert got and all(t == me for t, *_ in got)
    assert [e[1:] for e in got] == [e[1:] for e in want]
    ref.close()
    enc.close()


def test_group_refusals():
    L = TilingEncoder()._L
    n = L.tm_device_count()

    def code(fn, *a):
        try:
            fn(*a)
        except TileMotionError as e:
            return e.code
        return 0

    enc = TilingEncoder()
    assert code(enc.SetDeviceMask, 0) == -1
    assert code(enc.SetDeviceMask, 1 << n) == -1
    assert code(enc.SetDevices, [n]) == -1
    assert code(enc.SetDevices, [-1]) == -1
    assert code(enc.SetDevices, []) == -1
    assert code(enc.SetDevices, [0] * 33) == -1
    enc.SetVideo(W, H, 24.0, NF)
    assert code(enc.SetDevices, [0, 0]) == -1
    enc.close()
    # an encoder with a host communicator, or with the library's own
    cbt = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    dummy = cbt(lambda *a: -1)
    enc = TilingEncoder()
    assert L.tm_set_collective(ctypes.c_void_p(enc._h), 0, 2, ctypes.cast(dummy, ctypes.c_void_p), None) == 0
    assert code(enc.SetDevices, [0, 0]) == -1
    enc.close()
    enc = TilingEncoder()
    enc.CommInit(TilingEncoder.CommUniqueId(), 0, 1)
    assert code(enc.SetDevices, [0, 0]) == -1
    enc.CommDestroy()
    enc.close()
    # a group refuses the calls that would shard it from outside
    enc = TilingEncoder()
    enc.SetDevices([0, 0])
    assert L.tm_set_collective(ctypes.c_void_p(enc._h), 0, 2, ctypes.cast(dummy, ctypes.c_void_p), None) == -1
    assert code(enc.CommInit, TilingEncoder.CommUniqueId(), 0, 1) == -1
    assert code(enc.SetQueryShard, 0, 6) == -1
    assert code(enc.SetDitherShard, 0, 2) == -1
    assert code(enc.SetDevices, [0, 0]) == -1
    enc.close()
    # a list of one device is tm_set_device: no group
    enc = TilingEncoder()
    enc.SetDevices([0])
    enc.SetQueryShard(0, -1)
    enc.close()


def test_group_failing_shard_ends_the_step_at_once(monkeypatch, tmp_path_factory):
    """TM_GROUP_FAIL_SHARD=1: shard 1 fails before it queues any work; the others leave their collectives at once instead of waiting
    out TM_COMM_TIMEOUT_S, the message names shard 1, and the group can be destroyed and a fresh one runs cleanly"""
    monkeypatch.delenv("TM_PP_SHARDED", raising=False)
    enc = _encoder([0, 0, 0], _clip(), MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    enc.Run(S.esLoad)
    monkeypatch.setenv("TM_GROUP_FAIL_SHARD", "1")
    t0 = time.monotonic()
    with pytest.raises(TileMotionError) as ei:
        enc.Run(S.esReduce)
    assert time.monotonic() - t0 < 10.0
    assert ei.value.code == -1 and "shard 1" in str(ei.value) and "forced" in str(ei.value)
    enc.close()
    monkeypatch.delenv("TM_GROUP_FAIL_SHARD")
    want, _ = _reference(tmp_path_factory, MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    enc = _encoder([0, 0, 0], _clip(), MotionPredictRadius=0, FrameTilingExtendedPaletteUsage=False)
    enc.Run()
    _assert_same(_state(enc), want)
    enc.close()


def test_group_over_several_devices(tmp_path_factory):
    L = TilingEncoder()._L
    if L.tm_device_count() < 2:
        pytest.skip("one device visible")
    for radius in (0, 8):
        want, _ = _reference(tmp_path_factory, MotionPredictRadius=radius, FrameTilingExtendedPaletteUsage=True)
        enc = TilingEncoder()
        enc.SetDeviceMask(0b11)
        enc.LoadDefaultSettings()
        for k, v in {**BASE, "MotionPredictRadius": radius, "FrameTilingExtendedPaletteUsage": True}.items():
            setattr(enc, k, v)
        enc.SetVideo(W, H, 24.0, NF)
        for f, fr in enumerate(_clip()):
            enc.PushFrame(f, fr)
        enc.Run()
        _assert_same(_state(enc), want)
        enc.close()


@pytest.fixture(scope="module")
def c_host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("group") / "device_group")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-std=c11", "-D_DEFAULT_SOURCE", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "device_group.c"),
                           "-o", out, "-L", LIBDIR, "-ltilemotion", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("mode", ["pair", "all"])
def test_c_host_drives_a_group(c_host, tmp_path, mode):
    """a plain C host in a fresh process: the single run and the group run (two shards on device 0, or one per visible device) dump
    the same bytes"""
    dumps = []
    for what in ("single", mode):
        out = str(tmp_path / (what + ".bin"))
        p = subprocess.run([c_host, what, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout
        dumps.append(open(out, "rb").read())
    assert len(dumps[0]) > 1000 and dumps[0] == dumps[1]
