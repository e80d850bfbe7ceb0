"""numpy float64 restatement of the frame quality tm_get_frame_quality reports: RGB SSE and PSNR, and SSIM of
the luma plane on 8x8 windows placed on a 4-pixel grid, from each window's exact integer sums."""
import numpy as np

C1 = 64 ** 2 * (0.01 * 255) ** 2
C2 = 64 ** 2 * (0.03 * 255) ** 2


def sse_rgb(a, b):
    """a, b: uint32 [H][W] 0x00RRGGBB -> int64 [3] squared errors of R, G, B"""
    a = np.asarray(a, np.uint32).astype(np.int64)
    b = np.asarray(b, np.uint32).astype(np.int64)
    return np.array([(((a >> s) & 255) - ((b >> s) & 255)) ** 2 for s in (16, 8, 0)]).reshape(3, -1).sum(axis=1)


def psnr(sse, w, h, nframes=1):
    tot = int(np.sum(sse))
    return float("inf") if tot == 0 else 10.0 * np.log10(3.0 * w * h * nframes * 255.0 ** 2 / tot)


def window_ssim(sa, sb, q, p):
    """one window's term from its integer sums over 64 pixels: Sa, Sb, Q = sum(a^2 + b^2), P = sum(ab) (textbook SSIM, population
    variances, multiplied through by 64^2)"""
    sa, sb, q, p = (np.asarray(v, np.int64) for v in (sa, sb, q, p))
    num = (2.0 * (sa * sb) + C1) * (2.0 * (64 * p - sa * sb) + C2)
    den = ((sa * sa + sb * sb) + C1) * ((64 * q - sa * sa - sb * sb) + C2)
    return num / den


def ssim(ya, yb):
    """ya, yb: uint8 / int [H][W] luma planes (H, W multiples of 4) -> mean SSIM over the (W/4 - 1)(H/4 - 1) windows"""
    ya = np.asarray(ya, np.int64)
    yb = np.asarray(yb, np.int64)
    h, w = ya.shape
    assert h % 4 == 0 and w % 4 == 0 and h >= 8 and w >= 8

    def blocks(v):  # per 4x4 block sums
        return v.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))

    def windows(v):  # 2x2 blocks = one 8x8 window at every 4-pixel step
        return v[:-1, :-1] + v[1:, :-1] + v[:-1, 1:] + v[1:, 1:]

    sa, sb = windows(blocks(ya)), windows(blocks(yb))
    q, p = windows(blocks(ya * ya + yb * yb)), windows(blocks(ya * yb))
    return float(np.mean(window_ssim(sa, sb, q, p)))


def luma(img):
    """GenerateY4M's Y plane of uint32 [H][W] 0x00RRGGBB: RGBToYUV's y in double narrowed to single, rounded half to even, clamped"""
    img = np.asarray(img, np.uint32)
    r, g, b = ((img >> 16) & 255).astype(np.float64), ((img >> 8) & 255).astype(np.float64), (img & 255).astype(np.float64)
    y = (r * (299.0 / 1000) + g * (587.0 / 1000) + b * (114.0 / 1000)).astype(np.float32)
    return np.clip(np.rint(y.astype(np.float64)), 0, 255).astype(np.uint8)
