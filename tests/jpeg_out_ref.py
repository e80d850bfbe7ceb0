"""A plain Python / numpy integer restatement of the JPEG writer's rule (tiler_amd/csrc/tm_jpeg_out.h): libjpeg's
baseline encoder from the pixels to the file -- quantisers, colour, edges and chroma, the "islow" forward DCT, quantisation, the Annex K.3
Huffman code, the container.  It shares no code with the library; the tests hold the host twin to it, and it to Pillow
(tests/test_jpeg_out_host.py).  The container pieces and the names of the layouts come from tests/jpeg_cases.py; the header is written
here, since write_jpeg orders its DHT segments differently.

  encode(rgb, quality, sampling, restart_rows) -> (file, reached)   rgb: uint8 [h][w][3]; sampling: "420" | "422" | "444" | "grey"
  reached: what the picture's code holds -- ff00, zrl, no_eob, dc_cat, ac_cat, dummy_right, dummy_below, segments"""
import struct

import numpy as np

try:
    from tests.jpeg_cases import LAYOUTS, code_of, dht_body, dqt_body, seg
    from tests.jpeg_ref import STD_TABLES, ZIGZAG
except ImportError:  # run as a script
    from jpeg_cases import LAYOUTS, code_of, dht_body, dqt_body, seg
    from jpeg_ref import STD_TABLES, ZIGZAG

SAMPLINGS = ("420", "422", "444", "grey")

# T.81 Annex K.1, natural order
K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K1_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quant_tables(quality):
    """(luma, chroma), 64 values each in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(255, max(1, (b * scale + 50) // 100)) for b in base] for base in (K1_LUMA, K1_CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    """uint8 [h][w][3] -> Y, Cb, Cr as int64 [h][w]"""
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_planes(rgb, sampling):
    """the planes the transform reads, each a whole number of REAL blocks: [(plane int64, block rows, block columns)]"""
    h, w = rgb.shape[:2]
    y, cb, cr = ycc(rgb)
    hs, vs = (1, 1) if sampling == "grey" else LAYOUTS[sampling][0][1:3]
    out = []
    for c, p in enumerate((y,) if sampling == "grey" else (y, cb, cr)):
        fh, fv = (hs, vs) if c else (1, 1)  # how far this component is shrunk
        cw, ch = -(-w // fh), -(-h // fv)
        cols, rows = -(-cw // 8), -(-ch // 8)
        p = _edge(p, ch * fv, cols * 8 * fh)  # whole row groups below, whole blocks of output to the right
        if fh == 2 and fv == 2:
            bias = np.tile([1, 2], cols * 4)[None, :]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fh == 2:
            bias = np.tile([0, 1], cols * 4)[None, :]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append((_edge(p, rows * 8, cols * 8), rows, cols))  # (the shrunk plane's own last row, repeated)
    return out


_C = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069, f2_053=16819,
          f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct8(d, first):
    """d: int64 [8][...], one transform along axis 0"""
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _C["f0_541"]
    o[2] = _descale(z1 + t13 * _C["f0_765"], n)
    o[6] = _descale(z1 - t12 * _C["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C["f1_175"]
    t4, t5, t6, t7 = t4 * _C["f0_298"], t5 * _C["f2_053"], t6 * _C["f3_072"], t7 * _C["f1_501"]
    z1, z2, z3, z4 = -z1 * _C["f0_899"], -z2 * _C["f2_562"], -z3 * _C["f1_961"] + z5, -z4 * _C["f0_390"] + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o)


def quantised_blocks(plane, rows, cols, q):
    """int64 [rows][cols][64] in natural order"""
    b = plane.reshape(rows, 8, cols, 8).transpose(1, 3, 0, 2) - 128  # [y][x][row][col]
    b = _fdct8(b.transpose(1, 0, 2, 3), True)                        # along x: [u][y]...
    b = _fdct8(b.transpose(1, 0, 2, 3), False)                       # along y: [v][u]...
    co = b.transpose(2, 3, 0, 1).reshape(rows, cols, 64)
    qv = 8 * np.array(q, np.int64)
    t = (np.abs(co) + (qv >> 1)) // qv
    return np.where(co < 0, -t, t)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = self.acc << length | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = self.acc >> self.n & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _cat(v):
    return abs(int(v)).bit_length()


def _put_block(b, zz, pred, dc, ac, reached):
    diff = int(zz[0]) - pred
    s = _cat(diff)
    reached["dc_cat"] = max(reached["dc_cat"], s)
    b.put(*dc[s])
    if s:
        b.put(diff if diff >= 0 else diff + (1 << s) - 1, s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if not v:
            run += 1
            continue
        while run > 15:
            b.put(*ac[0xf0])
            reached["zrl"] += 1
            run -= 16
        s = _cat(v)
        reached["ac_cat"] = max(reached["ac_cat"], s)
        b.put(*ac[run << 4 | s])
        b.put(v if v >= 0 else v + (1 << s) - 1, s)
        run = 0
    if run:
        b.put(*ac[0x00])
    else:
        reached["no_eob"] += 1
    return int(zz[0])


def header(w, h, sampling, quality, restart_rows, mcus_per_row):
    comps = LAYOUTS[sampling]
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8")
    out += seg(0xe0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xdb, dqt_body(0, [ql[ZIGZAG[k]] for k in range(64)]))
    if len(comps) == 3:
        out += seg(0xdb, dqt_body(1, [qc[ZIGZAG[k]] for k in range(64)]))
    out += seg(0xc0, struct.pack(">BHHB", 8, h, w, len(comps)) + b"".join(bytes([c[0], c[1] << 4 | c[2], c[3]]) for c in comps))
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1))[:2 if len(comps) == 1 else 4]:
        out += seg(0xc4, dht_body(tc, th, *STD_TABLES[(tc, th)]))
    if restart_rows:
        out += seg(0xdd, struct.pack(">H", restart_rows * mcus_per_row))
    out += seg(0xda, bytes([len(comps)]) + b"".join(bytes([c[0], c[4] << 4 | c[5]]) for c in comps) + b"\x00\x3f\x00")
    return bytes(out)


def y_plane(rgb):
    """the rule's Y of a picture, uint8 [h][w]: what Pillow is given as an "L" image for grey"""
    return ycc(rgb)[0].astype(np.uint8)


def encode(rgb, quality=90, sampling="420", restart_rows=1):
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    comps = LAYOUTS[sampling]
    single = len(comps) == 1
    hmax, vmax = (1, 1) if single else comps[0][1:3]
    mcx, mcy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    quant = quant_tables(quality)
    blocks = []
    for c, (plane, rows, cols) in enumerate(component_planes(rgb, sampling)):
        co = quantised_blocks(plane, rows, cols, quant[comps[c][3]])
        blocks.append((co[:, :, ZIGZAG], rows, cols))
    codes = {k: code_of(*v) for k, v in STD_TABLES.items()}
    reached = dict(ff00=0, zrl=0, no_eob=0, dc_cat=0, ac_cat=0, dummy_right=0, dummy_below=0, segments=0)
    out = bytearray(header(w, h, sampling, quality, restart_rows, mcx))
    total = mcx * mcy
    per = restart_rows * mcx if restart_rows else total
    nseg = -(-total // per)
    reached["segments"] = nseg
    zero = [0] * 64
    for i in range(nseg):
        b = _Bits()
        pred = [0] * len(comps)
        for m in range(i * per, min((i + 1) * per, total)):
            mx, my = m % mcx, m // mcx
            for c, comp in enumerate(comps):
                ch, cv = (1, 1) if single else comp[1:3]
                zz_all, rows, cols = blocks[c]
                before = None  # the DC of the block before this one in the MCU
                for v in range(cv):
                    for hh in range(ch):
                        bx, by = mx * ch + hh, my * cv + v
                        if by < rows and bx < cols:
                            zz = zz_all[by, bx]
                        else:
                            reached["dummy_right" if by < rows else "dummy_below"] += 1
                            zz = [before] + zero[1:]
                        pred[c] = _put_block(b, zz, pred[c], codes[(0, comp[4])], codes[(1, comp[5])], reached)
                        before = pred[c]
        data = b.finish()
        reached["ff00"] += data.count(b"\xff\x00")
        out += data
        if i + 1 < nseg:
            out += bytes([0xff, 0xd0 + (i & 7)])
    out += b"\xff\xd9"
    return bytes(out), reached
