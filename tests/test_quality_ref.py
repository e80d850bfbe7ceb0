"""CPU checks of tests/quality_ref.py, the numpy statement of the frame quality the GPU tests compare tm_get_frame_quality with."""
import numpy as np

from tests import quality_ref


def test_hand_worked_window():
    # a = 10 everywhere, b = 10 on the left half and 20 on the right: Sa = 640, Sb = 960, Q = 64*100 + 32*100 + 32*400, P = 32*100 + 32*200
    a = np.full((8, 8), 10)
    b = np.full((8, 8), 10)
    b[:, 4:] = 20
    sa, sb, q, p = 640, 960, 64 * 100 + 32 * 100 + 32 * 400, 32 * 100 + 32 * 200
    mu_a, mu_b, var_a, var_b, cov = 10.0, 15.0, 0.0, 25.0, 0.0
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    textbook = (2 * mu_a * mu_b + c1) * (2 * cov + c2) / ((mu_a ** 2 + mu_b ** 2 + c1) * (var_a + var_b + c2))
    assert abs(quality_ref.window_ssim(sa, sb, q, p) - textbook) < 1e-12
    assert abs(quality_ref.ssim(a, b) - textbook) < 1e-12  # one window in an 8x8 frame


def test_window_count_and_symmetry():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (16, 24))
    b = np.clip(a + rng.integers(-30, 31, a.shape), 0, 255)
    s = quality_ref.ssim(a, b)
    assert s == quality_ref.ssim(b, a)
    assert 0 < s < 1
    # (24/4 - 1) x (16/4 - 1) = 15 windows: the mean of their terms
    terms = []
    for wy in range(3):
        for wx in range(5):
            wa, wb = a[wy * 4:wy * 4 + 8, wx * 4:wx * 4 + 8].astype(np.int64), b[wy * 4:wy * 4 + 8, wx * 4:wx * 4 + 8].astype(np.int64)
            terms.append(quality_ref.window_ssim(wa.sum(), wb.sum(), (wa * wa + wb * wb).sum(), (wa * wb).sum()))
    assert abs(s - np.mean(terms)) < 1e-15


def test_identical_inputs_give_one():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (32, 40))
    assert quality_ref.ssim(a, a) == 1.0
    img = rng.integers(0, 1 << 24, (8, 16)).astype(np.uint32)
    assert quality_ref.sse_rgb(img, img).tolist() == [0, 0, 0]
    assert quality_ref.psnr([0, 0, 0], 16, 8) == float("inf")


def test_sse_and_psnr():
    a = np.array([[0x00102030]], np.uint32)
    b = np.array([[0x00112233]], np.uint32)
    assert quality_ref.sse_rgb(a, b).tolist() == [1, 4, 9]
    assert abs(quality_ref.psnr([1, 4, 9], 1, 1) - 10 * np.log10(3 * 255.0 ** 2 / 14)) < 1e-12


def test_luma_matches_rgb_to_yuv_rounding():
    # pure channels and a grey: y = 0.299 R + 0.587 G + 0.114 B, rounded half to even after narrowing to single
    img = np.array([[0x00FF0000, 0x0000FF00, 0x000000FF, 0x00808080, 0x00FFFFFF, 0]], np.uint32)
    assert quality_ref.luma(img).tolist() == [[76, 150, 29, 128, 255, 0]]
