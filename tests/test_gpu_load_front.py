"""Load and PredictMotion's sliding-window features against the oracle past one chunk, batch, strip and grid: the Pearson sums
(k_pearson_frames) through their seam, k_load_tiles, k_window_dcts in both layouts, the motion search from a frame buffer in every form, and
Run(esLoad) itself.  Bit for bit everywhere: no comparison here carries a tolerance.  The inputs, and what each reaches, are in
tests/load_cases.py; tests/test_load_cases_host.py asserts on the oracle alone that they can discriminate."""
import numpy as np
import pytest

from tests import load_cases as lc
from tests import oracle_pipeline

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _dev(a):
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)  # (the cases are read-only: torch wants a writable array)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_cache = {}


def _once(key, make):
    """an oracle result, computed once for all the forms that are compared with it"""
    if key not in _cache:
        v = make()
        for a in v if isinstance(v, tuple) else (v,):
            a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- the Pearson seam --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", lc.PEARSON_SIZES)
def test_pearson(oracle, per):
    """k_pearson_frames and its host tail on [nframes][per] Singles: every kind of frame pair, one, two and seven frames"""
    from tiler_amd import stages
    for nframes in lc.PEARSON_FRAMES:
        for kind in lc.PEARSON_KINDS:
            lab = lc.pearson_case(kind, per, nframes)
            exp = np.zeros(nframes, np.float32)
            for f in range(1, nframes):
                exp[f] = oracle.pearson(lab[f - 1], lab[f])
            got = stages.pearson(_dev(lab))
            print(kind, per, nframes, got, exp)
            assert got.dtype == np.float32 and got.shape == (nframes,)
            assert np.array_equal(_bits(got), _bits(exp)), (kind, per, nframes, got, exp)
            if kind.startswith("const"):
                assert np.all(got[1:] == 1.0)


# ---- the Load seam -----------------------------------------------------------------------------------------------------------------------
def _oracle_load(oracle, frames, tm_w, tm_h):
    tiles, flags, lab = [], [], []
    for f in range(frames.shape[0]):
        t = oracle.load_from_image(frames[f], tm_w, tm_h)
        lab.append(oracle.inter_frame_data(t))
        c, fl = oracle.canonicalise(t)
        tiles.append(c)
        flags.append(fl)
    return np.concatenate(tiles), np.concatenate(flags), np.concatenate(lab)


@pytest.mark.parametrize("content", lc.LOAD_CONTENTS)
@pytest.mark.parametrize("shape", lc.LOAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_load(oracle, shape, content):
    """k_load_tiles: tiles, mirror flags and Lab means"""
    from tiler_amd import stages
    frames = lc.load_case(content, shape)
    tm_w, tm_h = shape[3], shape[4]
    tiles, flags, lab = stages.load(_dev(frames), tm_w, tm_h)
    torch.cuda.synchronize()
    exp_tiles, exp_flags, exp_lab = _oracle_load(oracle, frames, tm_w, tm_h)
    assert np.array_equal(_host_u32(tiles), exp_tiles)
    assert np.array_equal(flags.cpu().numpy(), exp_flags)
    assert np.array_equal(_bits(lab.cpu().numpy()), _bits(exp_lab)), "Lab tile means must match bit for bit"


# ---- window features ---------------------------------------------------------------------------------------------------------------------
WINDOW_FORMS = (None, "TM_FEATURES_PLAIN", "TM_WINDOW_DCTS_BY_TILE")


@pytest.mark.parametrize("form", WINDOW_FORMS, ids=lambda f: f or "default")
@pytest.mark.parametrize("content,buf", lc.WINDOW_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_window_dcts(oracle, monkeypatch, content, buf, form):
    """k_window_dcts<false> by strips, with every rounding left to the exact sum, and a window at a time"""
    from tiler_amd import stages
    fb = lc.frame_buffer(content, buf)
    exp = _once(("win", content, buf), lambda: oracle.window_dcts(fb))
    if form:
        monkeypatch.setenv(form, "1")
    got = stages.window_dcts(_dev(fb))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), exp)


# ---- motion search from a frame buffer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", lc.MOTION_FORMS, ids=lambda f: f or "default")
@pytest.mark.parametrize("content,grid,radius", lc.MOTION_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else "r%d" % v)
def test_motion_search_fb(oracle, monkeypatch, content, grid, radius, form):
    """what PredictMotion runs per frame -- k_window_dcts<true> and the matrix search --, its two-pass form, its fallback and the VALU search
    against the oracle's window features and search"""
    from tiler_amd import stages
    tm_w, tm_h = grid
    fb = lc.motion_frame_buffer(content, grid)
    cur = _once(("cur", content, grid), lambda: oracle.features_rgb(lc.screen_to_tiles(lc.motion_second_frame(content, grid)), None, 1, False))
    win = _once(("win", content, (tm_w * 8, tm_h * 8)), lambda: oracle.window_dcts(fb))
    e_err, e_px, e_py = _once(("search", content, grid, radius), lambda: oracle.motion_search(cur, tm_w, tm_h, win, radius))
    if form:
        monkeypatch.setenv(form, "1")
    err, px, py = stages.motion_search_fb(_dev(cur), tm_w, tm_h, _dev(fb), radius)
    torch.cuda.synchronize()
    assert np.array_equal(_host_u32(err), e_err)
    assert np.array_equal(px.cpu().numpy(), e_px) and np.array_equal(py.cpu().numpy(), e_py)
    if content == "flat":  # every candidate is equal: the penalty leaves the tile where it is
        assert not e_px.any() and not e_py.any()


# ---- the step itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_s", lc.STEP_MIN_SECONDS, ids=lambda v: "min-%s" % v)
@pytest.mark.parametrize("name", sorted(lc.STEP_CLIPS))
def test_run_load_only(oracle, name, min_s):
    """Run(esLoad) alone: the correlations' bits and the key frames, on clips of two and five chunks a frame"""
    from tiler_amd.encoder import TilingEncoder, TEncoderStep
    frames = lc.step_clip(name)
    nf, h, w = frames.shape
    exp = _once(("step", name, min_s), lambda: tuple(
        oracle_pipeline.run(oracle, frames, fps=lc.STEP_FPS, stop_after="load", **({} if min_s is None else dict(min_s=min_s)))[k] for k in ("correl", "keyframes")))
    enc = TilingEncoder()
    try:
        enc.LoadDefaultSettings()
        if min_s is not None:
            enc.ShotTransMinSecondsPerKF = min_s
        enc.SetVideo(w, h, lc.STEP_FPS, nf)
        for f in range(nf):
            enc.PushFrame(f, frames[f])
        enc.Run(TEncoderStep.esLoad)
        assert np.array_equal(_bits(enc.FrameCorrelations()), _bits(exp[0]))
        assert enc.KeyFrames().tolist() == exp[1].tolist()
        assert exp[1].tolist() == (lc.STEP_CLIPS[name][5] if min_s is not None else [0])
    finally:
        enc.close()
