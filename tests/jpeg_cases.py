"""The cases of the JPEG reader's tests, with what each one reaches, and the tests' own small baseline WRITER: Huffman
coding of given coefficient blocks with given tables, so that the GPU tests depend on no imaging library and the files hold what an
encoder never writes.  `python tests/jpeg_cases.py FILE` writes them for tests/c/jpeg_decode.c (tools/asan_jpeg_in.sh).

  good()      [(name, file, reaches)]: files that decode (status 0)
  refused()   [(name, file, code, fragment of the message)]: what the container walk refuses (TM_E_IO -5, TM_E_UNSUPPORTED -6)
  statuses()  [(name, file, TM_JPG_* status)]: what only decoding, or the segment list, finds
  damaged(n)  n seeded damages (cuts and single-byte changes) of the small good files"""
import functools
import struct
import sys

import numpy as np

try:
    from tests import jpeg_ref
except ImportError:  # run as a script
    import jpeg_ref
STD_TABLES = jpeg_ref.STD_TABLES
ZIGZAG = jpeg_ref.ZIGZAG

IO, UNSUPPORTED = -5, -6


# ---- the writer
def code_of(counts, symbols):
    """{symbol: (code, length)} of a canonical table"""
    out, code, at = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[symbols[at]] = (code, l)
            code += 1
            at += 1
        code <<= 1
    return out


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, code, length):
        self.v = self.v << length | (code & ((1 << length) - 1))
        self.n += length

    def bytes(self, pad=1):
        """padded to a byte with 1-bits (or 0-bits), FF stuffed"""
        k = -self.n % 8
        v = self.v << k | (((1 << k) - 1) if pad else 0)
        raw = v.to_bytes((self.n + k) // 8, "big") if self.n else b""
        return raw.replace(b"\xff", b"\xff\x00")


def _cat(v):
    return int(abs(int(v))).bit_length()


def _mag(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def put_block(b, zz, pred, dc, ac):
    """zz: 64 coefficients in zig-zag order, or a list of raw items ("dc" | "ac", symbol, extra bits value) -> the new prediction"""
    if not len(zz) or isinstance(zz[0], tuple):
        for kind, sym, extra in zz:
            b.put(*(dc if kind == "dc" else ac)[sym])
            nbits = sym if kind == "dc" else sym & 15
            if nbits and extra is not None:
                b.put(extra, nbits)
        return pred
    diff = int(zz[0]) - pred
    s = _cat(diff)
    b.put(*dc[s])
    if s:
        b.put(_mag(diff, s), s)
    run = 0
    last = max([k for k in range(1, 64) if zz[k]] + [0])
    for k in range(1, last + 1):
        if not zz[k]:
            run += 1
            continue
        while run > 15:
            b.put(*ac[0xf0])
            run -= 16
        s = _cat(zz[k])
        b.put(*ac[run << 4 | s])
        b.put(_mag(int(zz[k]), s), s)
        run = 0
    if last < 63:
        b.put(*ac[0x00])
    return int(zz[0])


def seg(marker, body):
    return bytes([0xff, marker]) + struct.pack(">H", len(body) + 2) + body


def dqt_body(tq, qzz, wide=False):
    return bytes([(16 if wide else 0) | tq]) + (b"".join(struct.pack(">H", v) for v in qzz) if wide else bytes(qzz))


def dht_body(tc, th, counts, symbols):
    return bytes([tc << 4 | th]) + bytes(counts) + bytes(symbols)


def flat_quant(v=1):
    return [v] * 64


def ramp_quant(lo=2, step=1):
    return [min(255, lo + step * k) for k in range(64)]


def write_jpeg(w, h, comps, blocks, quant, huff=None, ri=0, sof=0xc0, wide_dqt=(), dht="split", dqt="split", fill_rst=0, fill_eoi=0, before=(),
               after_eoi=b"", rst=None, pad=1, soi=True, precision=8, sof_size=None, eoi=True, between=b""):
    """comps: [(id, h, v, tq, td, ta)]; blocks[c]: [rows][columns] of 64 zig-zag coefficients (or raw item lists), whole MCUs; quant: {tq: 64
    values in zig-zag order}; huff: {(class, id): (counts, symbols)} (default: Annex K.3 as tables 0 and 1); dht / dqt: "split" (a segment
    per table), "joined" (one segment), "none"; fill_rst / fill_eoi: FF bytes added before every RSTn / before EOI; before: segments put
    in front of the tables; rst(i): the number of the marker behind segment i (None: left out; default i & 7); between: bytes put between
    the scan's last segment and EOI"""
    huff = dict(STD_TABLES) if huff is None else huff
    out = bytearray(b"\xff\xd8" if soi else b"")
    for s in before:
        out += s
    if dqt == "joined":
        out += seg(0xdb, b"".join(dqt_body(t, q, t in wide_dqt) for t, q in sorted(quant.items())))
    elif dqt == "split":
        for t, q in sorted(quant.items()):
            out += seg(0xdb, dqt_body(t, q, t in wide_dqt))
    sw, sh = sof_size if sof_size else (w, h)
    out += seg(sof, struct.pack(">BHHB", precision, sh, sw, len(comps)) + b"".join(bytes([c[0], c[1] << 4 | c[2], c[3]]) for c in comps))
    if dht == "joined":
        out += seg(0xc4, b"".join(dht_body(tc, th, *huff[(tc, th)]) for tc, th in sorted(huff)))
    elif dht == "split":
        for tc, th in sorted(huff):
            out += seg(0xc4, dht_body(tc, th, *huff[(tc, th)]))
    if ri:
        out += seg(0xdd, struct.pack(">H", ri))
    out += seg(0xda, bytes([len(comps)]) + b"".join(bytes([c[0], c[4] << 4 | c[5]]) for c in comps) + b"\x00\x3f\x00")
    codes = {k: code_of(*v) for k, v in huff.items()}
    single = len(comps) == 1
    hmax, vmax = (1, 1) if single else (max(c[1] for c in comps), max(c[2] for c in comps))
    mcx, mcy = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    total = mcx * mcy
    per = ri if ri else total
    nseg = (total + per - 1) // per
    for i in range(nseg):
        b = Bits()
        pred = [0] * len(comps)
        for m in range(i * per, min((i + 1) * per, total)):
            mx, my = m % mcx, m // mcx
            for c, comp in enumerate(comps):
                ch, cv = (1, 1) if single else (comp[1], comp[2])
                for v in range(cv):
                    for hh in range(ch):
                        pred[c] = put_block(b, blocks[c][my * cv + v][mx * ch + hh], pred[c], codes[(0, comp[4])], codes[(1, comp[5])])
        out += b.bytes(pad)
        if i + 1 < nseg:
            number = (i & 7) if rst is None else rst(i)
            if number is not None:
                out += b"\xff" * fill_rst + bytes([0xff, 0xd0 + number])
    out += between
    if eoi:
        out += b"\xff" * fill_eoi + b"\xff\xd9"
    return bytes(out + after_eoi)


# ---- content
LAYOUTS = {"grey": [(1, 1, 1, 0, 0, 0)], "444": [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)],
           "422": [(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], "420": [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]}


def grid(w, h, comps):
    """[(rows, columns)] of the blocks of every component, whole MCUs"""
    single = len(comps) == 1
    hmax, vmax = (1, 1) if single else (max(c[1] for c in comps), max(c[2] for c in comps))
    mcx, mcy = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    return [(mcy * (1 if single else c[2]), mcx * (1 if single else c[1])) for c in comps]


def content(seed, w, h, comps, kind="mixed", amp=60):
    """seeded coefficient blocks: "mixed" (a DC walk and sparse AC), "dc" (DC only), "zrl" (one coefficient far out: runs above 15),
    "full" (every coefficient set: no EOB), "small" (|AC| <= 7, runs of 0 and 1: the symbols of LONG_AC)"""
    rng = np.random.default_rng(seed)
    out = []
    for rows, cols in grid(w, h, comps):
        plane = []
        for _ in range(rows):
            row = []
            for _ in range(cols):
                zz = [0] * 64
                zz[0] = int(rng.integers(-amp, amp + 1))
                if kind == "mixed":
                    for k in range(1, 64):
                        if rng.random() < 0.25 / (1 + k / 8):
                            zz[k] = int(rng.integers(-amp, amp + 1)) // (1 + k // 6)
                elif kind == "zrl":
                    zz[int(rng.integers(20, 63))] = int(rng.integers(1, 4))
                    if rng.random() < 0.5:
                        zz[int(rng.integers(40, 64))] = -int(rng.integers(1, 4))
                elif kind == "full":
                    for k in range(1, 64):
                        zz[k] = int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1)
                elif kind == "small":
                    zz[0] = int(rng.integers(-7, 8))
                    k = 1
                    while k < 20:
                        zz[k] = int(rng.integers(1, 8)) * (1 if rng.random() < 0.5 else -1)
                        k += 1 + int(rng.integers(0, 2))
                row.append(zz)
            plane.append(row)
        out.append(plane)
    return out


QUANT2 = {0: ramp_quant(2, 1), 1: ramp_quant(3, 2)}

# codes of lengths 1..15 and one of 16 (the all-ones code of every length stays free)
LONG_DC = ([1] * 11 + [0, 0, 0, 0, 1], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
LONG_AC = ([1] * 7 + [0] * 8 + [1], [0x01, 0x00, 0x02, 0x11, 0x03, 0x12, 0xf0, 0x13])
LONG_TABLES = {(0, 0): LONG_DC, (0, 1): LONG_DC, (1, 0): LONG_AC, (1, 1): LONG_AC}
# tables that hold the symbols a decoder must refuse: DC category 12, AC category 11
WILD_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], list(range(13)))
WILD_AC = ([0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0x00, 0x01, 0x0b, 0xf1])


def simple(layout, w, h, seed, kind="mixed", quant=None, **kw):
    comps = LAYOUTS[layout]
    quant = quant if quant is not None else ({0: QUANT2[0]} if layout == "grey" else QUANT2)
    return write_jpeg(w, h, comps, content(seed, w, h, comps, kind), quant, **kw)


def _mcu_row(layout, w):
    return (w + (7 if layout in ("grey", "444") else 15)) // (8 if layout in ("grey", "444") else 16)


def _stuffed_last():
    """a grey 16x8 file with an interval of one block whose first segment ends on a stuffed FF"""
    for seed in range(4000):
        f = simple("grey", 16, 8, 7000 + seed, ri=1)
        at = f.find(b"\xff\x00\xff\xd0")
        if at > 0:
            return f
    raise AssertionError("no seed gives a segment that ends on FF 00")


@functools.lru_cache(maxsize=None)
def good():
    out = []

    def add(name, f, reaches):
        out.append((name, f, reaches))
    add("grey_8x8", simple("grey", 8, 8, 1), "one block")
    add("420_16x16", simple("420", 16, 16, 2), "one MCU of six blocks")
    add("444_8x8_dc", simple("444", 8, 8, 3, "dc"), "DC-only blocks")
    for i, layout in enumerate(("grey", "444", "422", "420")):
        add("%s_17x23" % layout, simple(layout, 17, 23, 10 + i), "partial MCUs on both axes, odd chroma sizes")
        add("%s_33x49" % layout, simple(layout, 33, 49, 20 + i), "partial MCUs, more than one block per row")
    add("444_72x64_ri1", simple("444", 72, 64, 30, ri=1), "72 segments: more than a wave of lanes, RSTn wraps past 7")
    for i, layout in enumerate(("422", "420", "grey")):
        add("%s_33x49_ri1" % layout, simple(layout, 33, 49, 40 + i, ri=1), "an interval of one MCU")
        add("%s_33x49_row" % layout, simple(layout, 33, 49, 50 + i, ri=_mcu_row(layout, 33)), "an interval of one MCU row")
    add("420_33x49_ri5", simple("420", 33, 49, 60, ri=5), "an interval that is no divisor of the MCU count: a short last segment")
    add("sof1_dqt16", simple("444", 17, 23, 61, sof=0xc1, wide_dqt=(0, 1), quant={0: ramp_quant(200, 9), 1: ramp_quant(300, 5)}, dqt="joined"),
        "SOF1 with 16-bit quantisers above 255 in one DQT")
    add("long_codes", simple("420", 17, 23, 62, "small", huff=LONG_TABLES), "codes 16 bits long: the walk behind the look-up")
    add("fill_bytes", simple("422", 33, 49, 63, ri=2, fill_rst=2, fill_eoi=3), "FF FF before RSTn and before EOI")
    add("stuffed_last", _stuffed_last(), "a stuffed FF 00 as a segment's last byte")
    add("zrl", simple("444", 17, 23, 64, "zrl"), "ZRL runs")
    add("no_eob", simple("420", 17, 23, 65, "full"), "blocks whose 63rd coefficient is set: no EOB")
    add("dc_only_420", simple("420", 33, 49, 66, "dc", ri=3), "DC-only blocks in segments")
    add("app1_60k", simple("444", 17, 23, 67, before=(seg(0xe1, b"Exif\0\0" + bytes(range(256)) * 234), seg(0xfe, b"a comment"), seg(0xe0, b"JFIF\0\1\1\0\0\1\0\1\0\0"))),
        "a 60 KB APP1, COM and APP0: skipped")
    add("dht_dqt_joined", simple("420", 17, 23, 68, dht="joined", dqt="joined"), "all tables in one DHT and one DQT")
    add("no_dht", simple("420", 17, 23, 69, dht="none"), "no DHT at all: the tables of Annex K.3")
    add("after_eoi", simple("444", 8, 8, 70, after_eoi=b"\xff\xda trailing bytes \xff\xd8"), "data after EOI: ignored")
    add("grey_2x2_factors", write_jpeg(17, 23, [(7, 2, 2, 0, 0, 0)], content(71, 17, 23, LAYOUTS["grey"]), {0: QUANT2[0]}),
        "one component with sampling factors 2x2: treated as 1x1")
    add("adobe_ycc", simple("444", 8, 8, 72, before=(seg(0xee, b"Adobe\0\x64\0\0\0\0\1"),)), "APP14 with transform 1: YCbCr")
    add("pad_zero", simple("420", 16, 16, 73, pad=0), "a segment padded with 0-bits")
    add("no_eoi", simple("444", 8, 8, 74, eoi=False), "no EOI: the data runs to the end of the file")
    return out


def no_dht_parent():
    return simple("420", 17, 23, 69)


def _raw_grey(items, huff=None, **kw):
    return write_jpeg(8, 8, LAYOUTS["grey"], [[[items]]], {0: flat_quant(1)}, huff=huff, **kw)


@functools.lru_cache(maxsize=None)
def refused():
    out = []
    base = simple("444", 8, 8, 100)
    comps3 = LAYOUTS["444"]

    def add(name, f, code, fragment):
        out.append((name, f, code, fragment))
    add("sof2", simple("444", 8, 8, 100, sof=0xc2), UNSUPPORTED, "SOF2")
    for k in (3, 5, 6, 7, 9, 10, 11, 13, 14, 15):
        add("sof%d" % k, simple("444", 8, 8, 100, sof=0xc0 + k), UNSUPPORTED, "SOF%d" % k)
    add("precision12", simple("444", 8, 8, 100, sof=0xc1, precision=12), UNSUPPORTED, "precision 12")
    add("two_components", write_jpeg(8, 8, comps3[:2], content(100, 8, 8, comps3[:2]), QUANT2), UNSUPPORTED, "2 components")
    add("four_components", write_jpeg(8, 8, comps3 + [(4, 1, 1, 1, 1, 1)], content(100, 8, 8, comps3 + [(4, 1, 1, 1, 1, 1)]), QUANT2), UNSUPPORTED, "4 components")
    for name, luma in (("440", (1, 2)), ("411", (4, 1)), ("luma_1x4", (1, 4))):
        c = [(1, luma[0], luma[1], 0, 0, 0)] + comps3[1:]
        add(name, write_jpeg(32, 32, c, content(100, 32, 32, c), QUANT2), UNSUPPORTED, "sampling")
    c = [(1, 2, 2, 0, 0, 0), (2, 2, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
    add("chroma_2x1", write_jpeg(16, 16, c, content(100, 16, 16, c), QUANT2), UNSUPPORTED, "sampling")
    one = simple("grey", 8, 8, 100)
    sos = one.find(b"\xff\xda")
    add("second_scan", one[:-2] + one[sos:], UNSUPPORTED, "more than one scan")
    f = bytearray(write_jpeg(8, 8, comps3, content(100, 8, 8, comps3), QUANT2))
    at = f.find(b"\xff\xda")
    add("scan_of_one_component", bytes(f[:at]) + seg(0xda, bytes([1, 1, 0x00, 0, 63, 0])) + bytes(f[at + 14:]), UNSUPPORTED, "more than one scan")
    add("adobe_rgb", simple("444", 8, 8, 100, before=(seg(0xee, b"Adobe\0\x64\0\0\0\0\0"),)), UNSUPPORTED, "APP14")
    add("dnl", simple("444", 8, 8, 100, between=seg(0xdc, b"\0\x08")), UNSUPPORTED, "DNL")
    add("height_0", simple("444", 8, 8, 100, sof_size=(8, 0)), UNSUPPORTED, "height 0")
    add("no_soi", base[2:], IO, "SOI")
    add("not_jpeg", b"\x89PNG\r\n\x1a\n" + bytes(40), IO, "SOI")
    add("segment_past_file", base[:30], IO, "runs past the file")
    add("cut_before_sos", base[:base.find(b"\xff\xda")], IO, "no SOS")
    f = bytearray(base)
    at = f.find(b"\xff\xda")
    f[at + 6] = 0x22  # the first component's tables: DC 2, AC 2
    add("missing_table", bytes(f), IO, "which no DHT defines")
    add("missing_quantiser", write_jpeg(8, 8, [(1, 1, 1, 3, 0, 0)], content(100, 8, 8, LAYOUTS["grey"]), {0: QUANT2[0]}), IO, "which no DQT defines")
    f = bytearray(base)
    f[at + 5] = 9  # the scan's first component id
    add("missing_component", bytes(f), IO, "which the frame does not have")
    add("dht_oversubscribed", simple("444", 8, 8, 100, before=(seg(0xc4, dht_body(0, 1, [3] + [0] * 15, [0, 1, 2])),)), IO, "over-subscribe")
    add("dht_328_symbols", simple("444", 8, 8, 100, before=(seg(0xc4, dht_body(1, 1, [0] * 14 + [128, 200], [k & 255 for k in range(328)])),)), IO, "256 at most")
    add("width_0", simple("444", 8, 8, 100, sof_size=(0, 8)), IO, "width 0")
    add("eoi_first", b"\xff\xd8\xff\xd9", IO, "EOI before any scan")
    return out


@functools.lru_cache(maxsize=None)
def statuses():
    out = []
    T, C, R, M, RST = jpeg_ref.TRUNCATED, jpeg_ref.BAD_CODE, jpeg_ref.BAD_RUN, jpeg_ref.BAD_MAGNITUDE, jpeg_ref.BAD_RESTART

    def add(name, f, status):
        out.append((name, f, status))
    base = simple("420", 33, 49, 200)
    add("cut_scan", base[:-40] + b"\xff\xd9", T)
    add("cut_file", base[:-40], T)
    add("empty_scan", _raw_grey([]), T)
    add("no_code", _raw_grey([], between=b"\xff\x00\xff\x00\xff\x00"), C)
    add("run_past_63", _raw_grey([("dc", 0, None)] + [("ac", 0xf1, 1)] * 4), R)
    add("zrl_past_63", _raw_grey([("dc", 0, None)] + [("ac", 0xf0, None)] * 4), R)
    wild = {(0, 0): WILD_DC, (1, 0): WILD_AC}
    add("dc_category_12", _raw_grey([("dc", 12, 0xfff), ("ac", 0x00, None)], huff=wild), M)
    add("ac_category_11", _raw_grey([("dc", 0, None), ("ac", 0x0b, 0x7ff), ("ac", 0x00, None)], huff=wild), M)
    add("rst_missing", simple("444", 33, 16, 201, ri=2, rst=lambda i: None if i == 3 else i & 7), RST)
    add("rst_out_of_sequence", simple("444", 33, 16, 201, ri=2, rst=lambda i: (i + 1) & 7 if i == 2 else i & 7), RST)
    add("rst_without_dri", simple("444", 8, 8, 202, between=b"\xff\xd0\x00"), RST)
    add("last_segment_cut", simple("grey", 24, 8, 203, ri=1)[:-5] + b"\xff\xd9", T)
    return out


def small_good():
    return [f for name, f, _ in good() if len(f) < 1500]


def damaged(n, seed=5):
    """n seeded damages of the small good files: cuts and single-byte changes"""
    rng = np.random.default_rng(seed)
    base = small_good()
    out = []
    for i in range(n):
        f = bytearray(base[i % len(base)])
        if rng.random() < 0.3:
            f = f[:int(rng.integers(0, len(f)))]
        else:
            # most changes fall into the scan, some into the headers
            lo = 0 if rng.random() < 0.3 else max(0, f.find(b"\xff\xda"))
            f[int(rng.integers(lo, len(f)))] = int(rng.integers(0, 256))
        out.append(bytes(f))
    return out


def _fdct_matrix():
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    m[0] *= 1 / np.sqrt(2)
    return m


def encode_rgb(rgb, layout="420", quant=None, **kw):
    """a picture uint8 [h][w][3] as a baseline file by this writer: JFIF's YCbCr, chroma averaged, a floating-point forward DCT, quantised"""
    h, w = rgb.shape[:2]
    comps = LAYOUTS[layout]
    quant = quant if quant is not None else ({0: QUANT2[0]} if layout == "grey" else QUANT2)
    r, g, b = [rgb[..., i].astype(np.float64) for i in range(3)]
    planes = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b][:len(comps)]
    m = _fdct_matrix()
    blocks = []
    for c, (rows, cols) in enumerate(grid(w, h, comps)):
        p = planes[c]
        sx, sy = (comps[0][1], comps[0][2]) if c else (1, 1)
        p = np.pad(p, ((0, rows * 8 * sy - h), (0, cols * 8 * sx - w)), mode="edge")
        p = p.reshape(rows * 8, sy, cols * 8, sx).mean((1, 3)) - 128
        q = np.array(quant[comps[c][3]], np.float64)
        plane = []
        for by in range(rows):
            row = []
            for bx in range(cols):
                co = m @ p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] @ m.T
                zz = [int(np.rint(co.flat[ZIGZAG[k]] / q[k])) for k in range(64)]
                row.append(zz)
            plane.append(row)
        blocks.append(plane)
    return write_jpeg(w, h, comps, blocks, quant, **kw)


def unpack(planes, layout, i, sizes):
    """file i's planes, of `sizes` [(w, h)], out of what stages.jpeg_decode / jpeg_decode_host return (flat arrays and their layout)"""
    out = []
    for c, (pw, ph) in enumerate(sizes):
        at = layout["first"] + i * layout["frame"]
        out.append(np.asarray(planes[c][at:at + layout["row"] * ph]).reshape(ph, layout["row"])[:, :pw])
    return out


def outside(planes, layout, sizes_per_file):
    """every byte of the three flat arrays that lies in no file's plane: the guards, the row padding, the unused slots"""
    out = []
    for c in range(3):
        used = np.zeros(len(planes[c]), bool)
        for i, sizes in enumerate(sizes_per_file):
            if c < len(sizes):
                pw, ph = sizes[c]
                at = layout["first"] + i * layout["frame"]
                used[at:at + layout["row"] * ph].reshape(ph, layout["row"])[:, :pw] = True
        out.append(np.asarray(planes[c])[~used])
    return np.concatenate(out)


def dump(path):
    with open(path, "wb") as fh:
        items = [(0, 0, f) for _, f, _ in good()] + [(1, code, f) for _, f, code, _ in refused()] + [(2, st, f) for _, f, st in statuses()]
        fh.write(struct.pack("<I", len(items)))
        for kind, code, f in items:
            fh.write(struct.pack("<IiI", kind, code, len(f)) + f)


if __name__ == "__main__":
    dump(sys.argv[1])
