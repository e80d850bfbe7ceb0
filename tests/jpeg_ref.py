"""A plain Python / numpy restatement of the JPEG reader's rule (tiler_amd/csrc/tm_jpeg.h): the container walk, the
sequential Huffman decode per restart segment, the "islow" integer inverse DCT.  It shares no code with the library; the tests hold the
host twin to it, and it to Pillow (tests/test_jpeg_in_host.py)."""
import numpy as np

IO, UNSUPPORTED = -5, -6  # TM_E_IO, TM_E_UNSUPPORTED
OK, TRUNCATED, BAD_CODE, BAD_RUN, BAD_MAGNITUDE, BAD_RESTART = 0, 48, 49, 50, 51, 52  # TM_JPG_*

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# T.81 Annex K.3: (counts of lengths 1..16, symbols in code order)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
STD_TABLES = {(0, 0): STD_DC_LUMA, (0, 1): STD_DC_CHROMA, (1, 0): STD_AC_LUMA, (1, 1): STD_AC_CHROMA}


class Refused(Exception):
    """the container walk's refusal: code IO or UNSUPPORTED"""

    def __init__(self, code, what):
        Exception.__init__(self, what)
        self.code = code


def _need(cond, code, what):
    if not cond:
        raise Refused(code, what)


def _be16(d, at):
    return d[at] << 8 | d[at + 1]


def walk(data):
    """The container walk -> a dict: w, h, ncomp, hs, vs, sof, ri, q {table: 64 quantisers in natural order}, codes {(class, id): (counts,
    symbols)}, tq / td / ta per component, segs [(offset, length)], nsegs, status0 (OK or BAD_RESTART).  Raises Refused."""
    d = bytes(data)
    n = len(d)
    _need(n >= 2 and d[0] == 0xff and d[1] == 0xd8, IO, "no SOI")
    o = dict(w=0, h=0, ncomp=0, hs=1, vs=1, sof=-1, ri=0, q={}, codes={}, tq=[0] * 4, td=[0] * 4, ta=[0] * 4)
    comp_id = [0] * 4
    adobe = -1
    pos = 2
    while True:
        _need(pos < n, IO, "no SOS")
        _need(d[pos] == 0xff, IO, "no marker")
        while pos < n and d[pos] == 0xff:
            pos += 1
        _need(pos < n, IO, "no SOS")
        m = d[pos]
        pos += 1
        _need(m != 0xd9, IO, "EOI before a scan")
        _need(m != 0xd8 and m != 0 and not 0xd0 <= m <= 0xd7, IO, "marker outside a scan")
        if m == 0x01:
            continue
        _need(pos + 2 <= n, IO, "segment past the file")
        ln = _be16(d, pos)
        _need(2 <= ln <= n - pos, IO, "segment past the file")
        s = d[pos + 2:pos + ln]
        dn = ln - 2
        pos += ln
        if m in (0xc0, 0xc1):
            _need(o["sof"] < 0, UNSUPPORTED, "second frame header")
            _need(dn >= 6, IO, "short SOF")
            _need(s[0] == 8, UNSUPPORTED, "precision")
            o["h"], o["w"] = _be16(s, 1), _be16(s, 3)
            _need(o["h"] != 0, UNSUPPORTED, "height 0")
            _need(o["w"] != 0, IO, "width 0")
            nc = s[5]
            _need(nc not in (2, 4), UNSUPPORTED, "components")
            _need(nc in (1, 3) and dn == 6 + 3 * nc, IO, "components")
            hv = []
            for c in range(nc):
                comp_id[c] = s[6 + 3 * c]
                hv.append((s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15))
                _need(1 <= hv[c][0] <= 4 and 1 <= hv[c][1] <= 4, IO, "sampling factors")
                _need(s[8 + 3 * c] <= 3, IO, "quantiser index")
                o["tq"][c] = s[8 + 3 * c]
            if nc == 3:
                _need(hv[1] == (1, 1) and hv[2] == (1, 1) and hv[0] in ((1, 1), (2, 1), (2, 2)), UNSUPPORTED, "sampling")
                o["hs"], o["vs"] = hv[0]
            o["ncomp"], o["sof"] = nc, m - 0xc0
        elif 0xc0 <= m <= 0xcf and m != 0xc4:
            raise Refused(UNSUPPORTED, "SOF%d" % (m - 0xc0))
        elif m == 0xdb:
            at = 0
            while at < dn:
                pq, tq = s[at] >> 4, s[at] & 15
                _need(pq <= 1 and tq <= 3, IO, "DQT")
                need = 1 + 64 * (pq + 1)
                _need(need <= dn - at, IO, "DQT past its segment")
                q = [0] * 64
                for k in range(64):
                    q[ZIGZAG[k]] = _be16(s, at + 1 + 2 * k) if pq else s[at + 1 + k]
                o["q"][tq] = q
                at += need
        elif m == 0xc4:
            at = 0
            while at < dn:
                tc, th = s[at] >> 4, s[at] & 15
                _need(tc <= 1 and th <= 3, IO, "DHT")
                _need(17 <= dn - at, IO, "DHT past its segment")
                counts = list(s[at + 1:at + 17])
                left = 1
                for l in range(16):
                    left = (left << 1) - counts[l]
                    _need(left >= 0, IO, "DHT over-subscribed")
                total = sum(counts)
                _need(total <= 256, IO, "DHT symbols")
                _need(total <= dn - at - 17, IO, "DHT past its segment")
                o["codes"][(tc, th)] = (counts, list(s[at + 17:at + 17 + total]))
                at += 17 + total
        elif m == 0xdd:
            _need(dn == 2, IO, "DRI")
            o["ri"] = _be16(s, 0)
        elif m == 0xdc:
            raise Refused(UNSUPPORTED, "DNL")
        elif m in (0xde, 0xdf):
            raise Refused(UNSUPPORTED, "hierarchical")
        elif m == 0xee:
            if dn >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
        elif m == 0xda:
            _need(o["sof"] >= 0, IO, "SOS before SOF")
            _need(dn >= 1, IO, "short SOS")
            ns = s[0]
            _need(1 <= ns <= 4 and dn == 4 + 2 * ns, IO, "SOS")
            for j in range(ns):
                _need(s[1 + 2 * j] in comp_id[:o["ncomp"]], IO, "SOS names a missing component")
            _need(ns == o["ncomp"], UNSUPPORTED, "more than one scan")
            for j in range(ns):
                _need(comp_id[j] == s[1 + 2 * j], UNSUPPORTED, "component order")
                o["td"][j], o["ta"][j] = s[2 + 2 * j] >> 4, s[2 + 2 * j] & 15
                _need(o["td"][j] <= 3 and o["ta"][j] <= 3, IO, "SOS tables")
            tail = s[1 + 2 * ns:]
            _need(tail[0] == 0 and tail[1] == 63 and tail[2] == 0, UNSUPPORTED, "Ss Se Ah Al")
            _need(not (o["ncomp"] == 3 and adobe == 0), UNSUPPORTED, "Adobe RGB")
            if not o["codes"]:
                o["codes"] = dict(STD_TABLES)
            for j in range(ns):
                _need(o["tq"][j] in o["q"], IO, "missing quantiser")
                _need((0, o["td"][j]) in o["codes"], IO, "missing DC table")
                _need((1, o["ta"][j]) in o["codes"], IO, "missing AC table")
            break
    # the scan, cut at every RSTn
    mcx, mcy = mcus(o)
    total = mcx * mcy
    segs, start, p, end_marker, in_order = [], pos, pos, 0, True
    while p < n:
        if d[p] != 0xff:
            p += 1
            continue
        if p + 1 < n and d[p + 1] == 0:
            p += 2
            continue
        q = p
        while q < n and d[q] == 0xff:
            q += 1
        if q >= n:
            p = n
            break
        m = d[q]
        if m == 0:
            p = q + 1
            continue
        segs.append((start, p - start))
        if 0xd0 <= m <= 0xd7:
            if m - 0xd0 != (len(segs) - 1) & 7:
                in_order = False
            start = p = q + 1
            continue
        end_marker = m
        p = q + 1
        start = None
        break
    if start is not None:
        segs.append((start, n - start))
    m = end_marker
    while m and m != 0xd9:
        _need(m != 0xda, UNSUPPORTED, "second SOS")
        _need(m != 0xdc, UNSUPPORTED, "DNL")
        _need(p + 2 <= n, IO, "segment past the file")
        ln = _be16(d, p)
        _need(2 <= ln <= n - p, IO, "segment past the file")
        p += ln
        while p < n and d[p] == 0xff:
            p += 1
        if p >= n:
            break
        m = d[p]
        p += 1
    ri = o["ri"] if o["ri"] else total
    o["nsegs"] = len(segs)
    o["status0"] = OK if in_order and len(segs) == (total + ri - 1) // ri else BAD_RESTART
    o["segs"] = segs
    return o


def mcus(o):
    bw, bh = (8, 8) if o["ncomp"] == 1 else (8 * o["hs"], 8 * o["vs"])
    return (o["w"] + bw - 1) // bw, (o["h"] + bh - 1) // bh


def plane_sizes(o):
    if o["ncomp"] == 1:
        return [(o["w"], o["h"])]
    c = ((o["w"] + o["hs"] - 1) // o["hs"], (o["h"] + o["vs"] - 1) // o["vs"])
    return [(o["w"], o["h"]), c, c]


class _Bits:
    def __init__(self, seg):
        out = bytearray()
        i, n = 0, len(seg)
        while i < n:
            b = seg[i]
            if b == 0xff:
                if i + 1 >= n or seg[i + 1] != 0:
                    break
                i += 2
            else:
                i += 1
            out.append(b)
        self.v = int.from_bytes(bytes(out), "big") if out else 0
        self.nb = 8 * len(out)
        self.pos = 0

    def peek(self, at, k):
        return (self.v >> (self.nb - at - k)) & ((1 << k) - 1)

    def take(self, k):
        if self.pos + k > self.nb:
            return None
        v = self.peek(self.pos, k)
        self.pos += k
        return v

    def symbol(self, table):
        for l in range(1, 17):
            if self.pos + l > self.nb:
                return -TRUNCATED
            s = table.get((l, self.peek(self.pos, l)))
            if s is not None:
                self.pos += l
                return s
        return -BAD_CODE


def _code_map(counts, symbols):
    out, code, at = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[(l, code)] = symbols[at]
            code += 1
            at += 1
        code <<= 1
    return out


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _block(bits, dc, ac, pred):
    """-> (status, 64 coefficients in natural order as Python ints, new prediction)"""
    co = [0] * 64
    t = bits.symbol(dc)
    if t < 0:
        return -t, co, pred
    if t > 11:
        return BAD_MAGNITUDE, co, pred
    if t:
        v = bits.take(t)
        if v is None:
            return TRUNCATED, co, pred
        pred = (pred + _extend(v, t)) & 0xffffffff
    co[0] = ((pred + 0x8000) & 0xffff) - 0x8000
    k = 1
    while k < 64:
        rs = bits.symbol(ac)
        if rs < 0:
            return -rs, co, pred
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            if k + 15 > 63:
                return BAD_RUN, co, pred
            k += 16
            continue
        if s > 10:
            return BAD_MAGNITUDE, co, pred
        k += r
        if k > 63:
            return BAD_RUN, co, pred
        v = bits.take(s)
        if v is None:
            return TRUNCATED, co, pred
        co[ZIGZAG[k]] = _extend(v, s)
        k += 1
    return OK, co, pred


_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069, f2_053=16819,
          f2_562=20995, f3_072=25172)


def _idct8(x, shift):
    """x: uint32 [8][n], one transform per column of the array -> int32 [8][n]; wrapping 32-bit arithmetic"""
    u = np.uint32
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * u(_F["f0_541"])
    tmp2 = z1 - z3 * u(_F["f1_847"])
    tmp3 = z1 + z2 * u(_F["f0_765"])
    tmp0 = (x[0] + x[4]) << u(13)
    tmp1 = (x[0] - x[4]) << u(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * u(_F["f1_175"])
    tmp0 = tmp0 * u(_F["f0_298"])
    tmp1 = tmp1 * u(_F["f2_053"])
    tmp2 = tmp2 * u(_F["f3_072"])
    tmp3 = tmp3 * u(_F["f1_501"])
    z1 = u(0) - z1 * u(_F["f0_899"])
    z2 = u(0) - z2 * u(_F["f2_562"])
    z3 = u(0) - z3 * u(_F["f1_961"]) + z5
    z4 = u(0) - z4 * u(_F["f0_390"]) + z5
    tmp0 = tmp0 + z1 + z3
    tmp1 = tmp1 + z2 + z4
    tmp2 = tmp2 + z2 + z3
    tmp3 = tmp3 + z1 + z4
    rows = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(r + u(1 << (shift - 1))).astype(np.uint32).view(np.int32) >> np.int32(shift) for r in rows])


def idct_block(co, q):
    """64 coefficients and 64 quantisers in natural order -> uint8 [8][8]"""
    with np.errstate(over="ignore"):
        x = (np.array(co, np.int64).astype(np.int32).view(np.uint32) * np.array(q, np.uint32)).reshape(8, 8)
        ws = _idct8(x, 11)                           # columns: ws[r][c]
        out = _idct8(ws.view(np.uint32).T.copy(), 18)  # rows: out[c][r]
    return np.clip(out.T.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def decode(data, fill=0xA5):
    """-> (status, planes, info): planes = uint8 arrays of the file's own plane sizes (what no block covered stays `fill`).  Raises Refused."""
    d = bytes(data)
    o = walk(d)
    sizes = plane_sizes(o)
    planes = [np.full((ph, pw), fill, np.uint8) for pw, ph in sizes]
    if o["status0"] != OK:
        return o["status0"], planes, o
    maps = {k: _code_map(*v) for k, v in o["codes"].items()}
    mcx, mcy = mcus(o)
    total = mcx * mcy
    ri = o["ri"] if o["ri"] else total
    status = OK
    for i, (off, ln) in enumerate(o["segs"]):
        bits = _Bits(d[off:off + ln])
        pred = [0, 0, 0]
        rc = OK
        for m in range(i * ri, min((i + 1) * ri, total)):
            mx, my = m % mcx, m // mcx
            for c in range(o["ncomp"]):
                ch, cv = (o["hs"], o["vs"]) if c == 0 and o["ncomp"] == 3 else (1, 1)
                for v in range(cv):
                    for h in range(ch):
                        rc, co, pred[c] = _block(bits, maps[(0, o["td"][c])], maps[(1, o["ta"][c])], pred[c])
                        if rc != OK:
                            break
                        px = idct_block(co, o["q"][o["tq"][c]])
                        x, y = 8 * (mx * ch + h), 8 * (my * cv + v)
                        pw, ph = sizes[c]
                        if x < pw and y < ph:
                            planes[c][y:y + 8, x:x + 8] = px[:min(8, ph - y), :min(8, pw - x)]
                    if rc != OK:
                        break
                if rc != OK:
                    break
            if rc != OK:
                break
        if rc != OK and status == OK:
            status = rc
    return status, planes, o


def to_rgb_444(planes):
    """4:4:4 (or grey) planes through the BT601_FULL rule (tm_yuv_in.hip, libjpeg's 16-bit constants) -> uint8 [h][w][3]"""
    y = planes[0].astype(np.int64)
    d = (planes[1].astype(np.int64) - 128) if len(planes) == 3 else np.zeros_like(y)
    e = (planes[2].astype(np.int64) - 128) if len(planes) == 3 else np.zeros_like(y)
    r = (65536 * y + 91881 * e + 32768) >> 16
    g = (65536 * y - 22554 * d - 46802 * e + 32768) >> 16
    b = (65536 * y + 116130 * d + 32768) >> 16
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
