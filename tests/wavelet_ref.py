"""CPU restatement of the reference's Haar wavelet (WaveletGS / DeWaveletGS, tilingencoder.pas:2727-2917) and of the
wavelet branch of ComputeTilePsyVisFeatures (3150-3157, 3177-3179) in Python doubles.  The oracle has no wavelet
branch, so this is the checker of DitheringMode = pvsWavelets.  Test infrastructure only."""
import math

import numpy as np

W = 8  # cTileWidth: the row stride of every plane and temporary
FACTOR = 1.0 / math.sqrt(2.0)  # (1.0 / sqrt(2.0)) in double steps = 0.7071067811865475, one ulp below 1/sqrt(2) correctly rounded


def wavelet_gs(data, output, dx, dy, depth):
    """WaveletGS<Double>(Data, Output, dx, dy, depth) on flat lists of 64 floats (Data may be Output)"""
    temp_x = [0.0] * (W * W)
    temp_y = [0.0] * (W * W)
    factor = FACTOR
    for y in range(dy):  # Transform Rows
        offset = y * W
        for x in range(dx // 2):
            temp_x[x + offset] = (data[x * 2 + offset] + data[(x * 2 + 1) + offset]) * factor  # LOW-PASS
            temp_x[(x + dx // 2) + offset] = (data[x * 2 + offset] - data[(x * 2 + 1) + offset]) * factor  # HIGH-PASS
    for x in range(dx):  # Transform Columns
        for y in range(dy // 2):
            temp_y[x + y * W] = (temp_x[x + y * 2 * W] + temp_x[x + (y * 2 + 1) * W]) * factor  # LOW-PASS
            temp_y[x + (y + dy // 2) * W] = (temp_x[x + y * 2 * W] - temp_x[x + (y * 2 + 1) * W]) * factor  # HIGH-PASS
    for y in range(dy):
        output[y * W:y * W + dx] = temp_y[y * W:y * W + dx]  # Copy to Wavelet
    if depth > 0:
        wavelet_gs(output, output, dx // 2, dy // 2, depth - 1)


def dewavelet_gs(wl, pic, dx, dy, depth):
    """DeWaveletGS<Double>(wl, pic, dx, dy, depth): the reference's inverse, with its "fake" interpolation where a
    high-pass coefficient is zero (wl is changed in place by the recursion, as in the reference)"""
    temp_x = [0.0] * (W * W)
    temp_y = [0.0] * (W * W)
    if depth > 0:
        dewavelet_gs(wl, wl, dx // 2, dy // 2, depth - 1)
    factor = FACTOR

    yhalf = (dy // 2) - 1
    dyoff = (dy // 2) * W
    yhalfoff = yhalf * W
    yhalfoff2 = (yhalf + (dy // 2)) * W
    yhalfoff3 = yhalfoff * 2 + W
    if yhalf > 0:  # The first and last pixel has to be done "normal"
        for x in range(dx):
            temp_y[x] = (wl[x] + wl[x + dyoff]) * factor
            temp_y[x + W] = (wl[x] - wl[x + dyoff]) * factor
            temp_y[x + yhalfoff * 2] = (wl[x + yhalfoff] + wl[x + yhalfoff2]) * factor
            temp_y[x + yhalfoff3] = (wl[x + yhalfoff] - wl[x + yhalfoff2]) * factor
    else:
        for x in range(dx):
            temp_y[x] = (wl[x] + wl[x + dyoff]) * factor
            temp_y[x + W] = (wl[x] - wl[x + dyoff]) * factor

    dyoff = (dy // 2) * W
    yhalf = (dy // 2) - 2
    if yhalf >= 1:
        if dy >= 4:
            for x in range(dx):  # Inverse Transform Columns
                offsetm1, offset, offsetp1 = 0, W, W * 2
                for y in range(1, yhalf + 1):
                    if wl[x + offset + dyoff] != 0.0:
                        temp_y[x + offset * 2] = (wl[x + offset] + wl[x + offset + dyoff]) * factor
                        temp_y[x + offset * 2 + W] = (wl[x + offset] - wl[x + offset + dyoff]) * factor
                    else:
                        if wl[x + offsetm1 + dyoff] == 0.0 and wl[x + offsetp1] != wl[x + offset] and \
                                (y == yhalf or wl[x + offsetp1] != wl[x + offsetp1 + W]):
                            temp_y[x + offset * 2] = (wl[x + offset] * 0.8 + wl[x + offsetm1] * 0.2) * factor
                        else:
                            temp_y[x + offset * 2] = wl[x + offset] * factor
                        if wl[x + offsetp1 + dyoff] == 0.0 and wl[x + offsetm1] != wl[x + offset] and \
                                (y == 1 or wl[x + offsetm1] != wl[x + offsetm1 - W]):
                            temp_y[x + offset * 2 + W] = (wl[x + offset] * 0.8 + wl[x + offsetp1] * 0.2) * factor
                        else:
                            temp_y[x + offset * 2 + W] = wl[x + offset] * factor
                    offsetm1 += W
                    offset += W
                    offsetp1 += W
        else:  # DY < 4
            for x in range(dx):
                offset = W
                for y in range(1, yhalf + 1):
                    temp_y[x + offset * 2] = (wl[x + offset] + wl[x + offset + dyoff]) * factor
                    temp_y[x + offset * 2 + W] = (wl[x + offset] - wl[x + offset + dyoff]) * factor
                    offset += W

    offset = 0
    yhalf = (dx // 2) - 1
    yhalfoff = yhalf + dx // 2
    yhalfoff2 = yhalf * 2 + 1
    if yhalf > 0:
        for y in range(dy):
            temp_x[offset] = (temp_y[offset] + temp_y[yhalf + 1 + offset]) * factor
            temp_x[offset + 1] = (temp_y[offset] - temp_y[yhalf + 1 + offset]) * factor
            temp_x[yhalf * 2 + offset] = (temp_y[yhalf + offset] + temp_y[yhalfoff + offset]) * factor
            temp_x[yhalfoff2 + offset] = (temp_y[yhalf + offset] - temp_y[yhalfoff + offset]) * factor
            offset += W
    else:
        for y in range(dy):
            temp_x[offset] = (temp_y[offset] + temp_y[yhalf + 1 + offset]) * factor
            temp_x[offset + 1] = (temp_y[offset] - temp_y[yhalf + 1 + offset]) * factor
            offset += W

    dyoff = dx // 2
    yhalf = (dx // 2) - 2
    if yhalf >= 1:
        if dx >= 4:
            offset = 0
            for y in range(dy):  # Inverse Transform Rows
                for x in range(1, yhalf + 1):
                    if temp_y[x + dyoff + offset] != 0.0:
                        temp_x[x * 2 + offset] = (temp_y[x + offset] + temp_y[x + dyoff + offset]) * factor
                        temp_x[x * 2 + 1 + offset] = (temp_y[x + offset] - temp_y[x + dyoff + offset]) * factor
                    else:
                        if temp_y[x - 1 + dyoff + offset] == 0.0 and temp_y[x + 1 + offset] != temp_y[x + offset] and \
                                (x == yhalf or temp_y[x + 1 + offset] != temp_y[x + 2 + offset]):
                            temp_x[x * 2 + offset] = (temp_y[x + offset] * 0.8 + temp_y[x - 1 + offset] * 0.2) * factor
                        else:
                            temp_x[x * 2 + offset] = temp_y[x + offset] * factor
                        if temp_y[x + 1 + dyoff + offset] == 0.0 and temp_y[x - 1 + offset] != temp_y[x + offset] and \
                                (x == 1 or temp_y[x - 1 + offset] != temp_y[x - 2 + offset]):
                            temp_x[x * 2 + 1 + offset] = (temp_y[x + offset] * 0.8 + temp_y[x + 1 + offset] * 0.2) * factor
                        else:
                            temp_x[x * 2 + 1 + offset] = temp_y[x + offset] * factor
                offset += W
        else:  # DX < 4
            offset = 0
            for y in range(dy):
                for x in range(1, yhalf + 1):
                    temp_x[x * 2 + offset] = (temp_y[x + offset] + temp_y[x + dyoff + offset]) * factor
                    temp_x[x * 2 + 1 + offset] = (temp_y[x + offset] - temp_y[x + dyoff + offset]) * factor
                offset += W

    for y in range(dy):
        pic[y * W:y * W + dx] = temp_x[y * W:y * W + dx]  # Copy to Pic


def snake(oracle):
    """cDCTSnake (utils.pas:59-68) as the oracle holds it"""
    import ctypes
    return np.frombuffer((ctypes.c_uint8 * 64).in_dll(oracle.L, "tmo_dct_snake"), np.uint8).astype(np.int64)


def features_f64(cpn, snk):
    """ComputeTilePsyVisFeatures(Mode = pvsWavelets) of one tile's planes (float32 [192]) -> double [192], snake order"""
    out = [0.0] * 192
    for c in range(3):
        plane = [float(v) for v in cpn[c * 64:(c + 1) * 64]]
        local = [0.0] * 64
        wavelet_gs(plane, local, W, W, 2)
        for i in range(64):
            out[int(snk[i]) + c * 64] = local[i]
    return out


def inv_features_f64(feat, snk):
    """ComputeInvTilePsyVisFeatures(Mode = pvsWavelets) up to the planes: double [192] -> double planes [192]"""
    planes = [0.0] * 192
    for c in range(3):
        local = [feat[int(snk[i]) + c * 64] for i in range(64)]
        pic = [0.0] * 64
        dewavelet_gs(local, pic, W, W, 2)
        planes[c * 64:(c + 1) * 64] = pic
    return planes


def _level(a, d):
    """one WaveletGS level of size d on the top-left d x d of a [n][8][8], every element the same IEEE double steps"""
    h = d // 2
    s = a[:, :d, :d]
    tx = np.concatenate([(s[:, :, 0::2] + s[:, :, 1::2]) * FACTOR, (s[:, :, 0::2] - s[:, :, 1::2]) * FACTOR], axis=2)
    ty = np.concatenate([(tx[:, 0::2, :] + tx[:, 1::2, :]) * FACTOR, (tx[:, 0::2, :] - tx[:, 1::2, :]) * FACTOR], axis=1)
    assert ty.shape[1] == 2 * h
    a = a.copy()
    a[:, :d, :d] = ty
    return a


def features_cluster_wavelet(planes, snk):
    """the cluster features of many tiles: Lab planes float32 [n][3][64] -> WaveletGS(8, 8, depth 2) per plane, snake
    scatter, Round (half to even) -> int32 [n][192].  Vectorised form of features_f64, element for element the same steps."""
    n = planes.shape[0]
    a = planes.astype(np.float64).reshape(n * 3, 8, 8)
    for d in (8, 4, 2):
        a = _level(a, d)
    loc = a.reshape(n, 3, 64)
    out = np.empty((n, 3, 64), np.float64)
    out[:, :, snk] = loc
    return np.rint(out).astype(np.int32).reshape(n, 192)


def lab_planes(oracle, tiles):
    """ConvertToCpnPixels with UseLAB (no mirroring) of tiles uint32 [n][64] (0x00BBGGRR) -> float32 [n][3][64]"""
    t = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
    rgb = ((t & 0xFF) << 16) | (t & 0xFF00) | ((t >> 16) & 0xFF)  # rgb_to_lab_array takes 0x00RRGGBB
    lab = oracle.rgb_to_lab_array(rgb, det=True)
    return np.ascontiguousarray(lab.reshape(-1, 64, 3).transpose(0, 2, 1))
