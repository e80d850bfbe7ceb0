"""A plain-Python restatement of the WebP writer's rule (tiler_amd/csrc/tm_webp_out.h) and a VP8L / container reader of
its own; it shares no code with the library.

  encode(frames, fps, **options) -> (file, canvas uint32 [F][h][w], info): info is a dict per frame of rect, colours (0: subtract green),
      per, symbols, segments, tokens, matches, longest, seg_bits, kinds (per alphabet "simple0" / "simple1" / "simple2" / "normal"),
      deepest (per alphabet the unlimited Huffman depth), reaches_back (matches whose source starts before their segment), ends_at_border
      (matches cut by their segment's end that is not the image's), payload_bytes
  decode(file) -> (frames [uint32 [h][w]], parsed): the canvas after every frame; parsed: width, height, loop, frames [dict of x, y, w, h,
      duration, flags]
Refusals raise Refused(code)."""
import math
import struct

import numpy as np

INVAL, UNSUPPORTED = -1, -6
PALETTE = {"auto": 0, "off": 1}
MIN_MATCH, MAX_LEN, MAX_DIST, FAR3, DEPTH = 3, 4096, (1 << 20) - 120, 512, 8
ALPHABETS = (280, 256, 256, 256, 40)  # green + lengths, red, blue, alpha, distance
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
M32 = 0xFFFFFFFF


class Refused(Exception):
    def __init__(self, code, what):
        super().__init__(what)
        self.code = code


def options(diff=True, palette="auto", lz77=True, segment_pixels=4096, loop=0, duration_ms=0):
    return dict(diff=diff, palette=palette, lz77=lz77, segment_pixels=segment_pixels, loop=loop, duration_ms=duration_ms)


def duration_of(fps, o):
    if o["diff"] not in (0, 1, False, True) or o["lz77"] not in (0, 1, False, True) or o["palette"] not in PALETTE or o["segment_pixels"] < 0:
        raise Refused(INVAL, "options")
    if not 0 <= o["loop"] <= 65535 or not 0 <= o["duration_ms"] < 1 << 24:
        raise Refused(INVAL, "options")
    if o["duration_ms"]:
        return o["duration_ms"]
    if not fps > 0:
        raise Refused(INVAL, "rate")
    v = math.floor(1000.0 / fps + 0.5)
    if v >= 1 << 24:
        raise Refused(INVAL, "rate")
    return max(1, int(v))


# ---- bits
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0 and v == 0
        self.acc |= v << self.n
        self.n += n

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def code_lengths(freq, max_bits):
    """-> (lengths, the depth an unlimited Huffman code would reach).  Used symbols ordered by (count, symbol); two queues, of two equal
    weights the leaf first; leaves deeper than the limit are set to it and the oversubscription is paid back one unit at a time by moving a
    leaf of the deepest level above the limit's that has one down; the longest codes go to the rarest symbols.  Fewer than two used symbols
    are padded to two."""
    n = len(freq)
    lens = [0] * n
    used = [s for s in range(n) if freq[s]]
    if not used:
        lens[0] = lens[1] = 1
        return lens, 0
    if len(used) == 1:
        lens[used[0]] = 1
        lens[1 if used[0] == 0 else 0] = 1
        return lens, 0
    used.sort(key=lambda s: (freq[s], s))
    nu = len(used)
    weight = [freq[s] for s in used] + [0] * (nu - 1)
    parent = [0] * (2 * nu - 1)
    leaf, inner = 0, nu
    for made in range(nu, 2 * nu - 1):
        for _ in range(2):
            if leaf < nu and (inner >= made or weight[leaf] <= weight[inner]):
                node, leaf = leaf, leaf + 1
            else:
                node, inner = inner, inner + 1
            weight[made] += weight[node]
            parent[node] = made
    depth = [0] * (2 * nu - 1)
    count = [0] * (max_bits + 1)
    deepest = 0
    for node in range(2 * nu - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
        if node < nu:
            count[min(depth[node], max_bits)] += 1
            deepest = max(deepest, depth[node])
    total = sum(count[b] << (max_bits - b) for b in range(1, max_bits + 1))
    while total > 1 << max_bits:
        count[max_bits] -= 1
        for b in range(max_bits - 1, 0, -1):
            if count[b]:
                count[b] -= 1
                count[b + 1] += 2
                break
        total -= 1
    k = 0
    for b in range(max_bits, 0, -1):
        for _ in range(count[b]):
            lens[used[k]] = b
            k += 1
    return lens, deepest


def canonical(lens):
    """-> {symbol: (code with its bits reversed, length)}"""
    out, code = {}, 0
    for b in range(1, 16):
        for s, l in enumerate(lens):
            if l == b:
                out[s] = (int(format(code, "0%db" % b)[::-1], 2), b)
                code += 1
        code <<= 1
    return out


def write_code(bits, freq):
    """-> ({symbol: (code, length)}, kind, deepest)"""
    used = [s for s in range(len(freq)) if freq[s]]
    if len(used) <= 2 and all(s < 256 for s in used):
        syms = used or [0]
        bits.put(1, 1)
        bits.put(len(syms) - 1, 1)
        wide = syms[0] > 1
        bits.put(int(wide), 1)
        bits.put(syms[0], 8 if wide else 1)
        if len(syms) == 2:
            bits.put(syms[1], 8)
            return {syms[0]: (0, 1), syms[1]: (1, 1)}, "simple2", 1
        return {syms[0]: (0, 0)}, "simple%d" % len(used), 0
    lens, deepest = code_lengths(freq, 15)
    items, s = [], 0
    while s < len(lens):
        if lens[s]:
            items.append((lens[s], 0, 0))
            s += 1
            continue
        run = 1
        while s + run < len(lens) and not lens[s + run]:
            run += 1
        s += run
        while run >= 11:
            take = min(run, 138)
            items.append((18, 7, take - 11))
            run -= take
        if run >= 3:
            items.append((17, 3, run - 3))
            run = 0
        items += [(0, 0, 0)] * run
    cf = [0] * 19
    for sym, _, _ in items:
        cf[sym] += 1
    cl, _ = code_lengths(cf, 7)
    ce = canonical(cl)
    count = 19
    while count > 4 and not cl[CL_ORDER[count - 1]]:
        count -= 1
    bits.put(0, 1)
    bits.put(count - 4, 4)
    for k in range(count):
        bits.put(cl[CL_ORDER[k]], 3)
    bits.put(0, 1)
    for sym, eb, ev in items:
        bits.put(*ce[sym])
        bits.put(ev, eb)
    return canonical(lens), "normal", deepest


def prefix_of(v):
    """a length or distance code v >= 1 -> (symbol, extra bits, their value)"""
    if v <= 4:
        return v - 1, 0, 0
    v -= 1
    h = v.bit_length() - 1
    return 2 * h + (v >> (h - 1) & 1), h - 1, v & ((1 << (h - 1)) - 1)


def key_of(a, b, c):
    v = a * 0x9E3779B1 & M32
    v = ((v ^ v >> 15) + b * 0x85EBCA77) & M32
    v = ((v ^ v >> 13) + c * 0xC2B2AE3D) & M32
    v = ((v ^ v >> 16) * 0x27D4EB2F) & M32
    return v >> 5


def links_of(s):
    """prev[i]: the nearest earlier position whose three symbols (missing ones 0) have i's key, or -1"""
    n = len(s)
    key = [key_of(s[i], s[i + 1] if i + 1 < n else 0, s[i + 2] if i + 2 < n else 0) for i in range(n)]
    order = sorted(range(n), key=lambda i: (key[i], i))
    prev = [-1] * n
    for r in range(1, n):
        if key[order[r]] == key[order[r - 1]]:
            prev[order[r]] = order[r - 1]
    return prev


def best_match(s, prev, i, end):
    cap = min(MAX_LEN, end - i)
    if cap < MIN_MATCH:
        return 0, 0
    best, bd, j, d = 0, 0, prev[i], 0
    while d < DEPTH and j >= 0 and i - j <= MAX_DIST:
        if not (best and s[j + best] != s[i + best]):
            l = 0
            while l < cap and s[j + l] == s[i + l]:
                l += 1
            if l > best:
                best, bd = l, i - j
                if l == cap:
                    break
        d += 1
        j = prev[j]
    if best < MIN_MATCH or (best == MIN_MATCH and bd > FAR3):
        return 0, 0
    return best, bd


def parse(s, seg, lz77):
    """-> [tokens of every segment]; a token: (symbol,) or (length, distance)"""
    n = len(s)
    prev = links_of(s) if lz77 else None
    seg = seg or n
    out = []
    for begin in range(0, n, seg):
        end, i, toks = min(n, begin + seg), begin, []
        while i < end:
            l, d = best_match(s, prev, i, end) if lz77 else (0, 0)
            if l:
                toks.append((l, d, i))
                i += l
            else:
                toks.append((s[i],))
                i += 1
        out.append((begin, end, toks))
    return out


def slots_of(tok):
    """-> [(alphabet, symbol)]"""
    if len(tok) == 1:
        v = tok[0]
        return [(0, v >> 8 & 255), (1, v >> 16 & 255), (2, v & 255), (3, v >> 24)]
    return [(0, 256 + prefix_of(tok[0])[0]), (4, prefix_of(tok[1] + 120)[0])]


def put_token(bits, codes, tok):
    if len(tok) == 1:
        for a, sym in slots_of(tok):
            bits.put(*codes[a][sym])
        return
    ls, le, lv = prefix_of(tok[0])
    ds, de, dv = prefix_of(tok[1] + 120)
    bits.put(*codes[0][256 + ls])
    bits.put(lv, le)
    bits.put(*codes[4][ds])
    bits.put(dv, de)


def write_group(bits, toks):
    hist = [[0] * n for n in ALPHABETS]
    for t in toks:
        for a, sym in slots_of(t):
            hist[a][sym] += 1
    codes, kinds, deep = [], [], []
    for a in range(5):
        c, kind, d = write_code(bits, hist[a])
        codes.append(c)
        kinds.append(kind)
        deep.append(d)
    return codes, kinds, deep


def bundle_of(colours):
    return 8 if colours <= 2 else 4 if colours <= 4 else 2 if colours <= 16 else 1


def rect_of(cur, old):
    ys, xs = np.nonzero(cur != old)
    if len(ys) == 0:
        return (0, 0, 1, 1)
    x0, y0 = int(xs.min()) & ~1, int(ys.min()) & ~1
    return (x0, y0, int(xs.max()) - x0 + 1, int(ys.max()) - y0 + 1)


def image(px, o):
    """one rectangle's pixels [h][w] of 0x00RRGGBB -> (VP8L payload, info)"""
    h, w = px.shape
    table = sorted(set(int(v) for v in px.reshape(-1)))
    colours = len(table) if o["palette"] == "auto" and len(table) <= 256 else 0
    bits = Bits()
    bits.put(0x2F, 8)
    bits.put(w - 1, 14)
    bits.put(h - 1, 14)
    bits.put(0, 4)
    if colours:
        per = bundle_of(colours)
        rank = {c: k for k, c in enumerate(table)}
        pw = (w + per - 1) // per
        s = []
        for y in range(h):
            for p in range(pw):
                g = 0
                for k in range(per):
                    if p * per + k < w:
                        g |= rank[int(px[y, p * per + k])] << (k * (8 // per))
                s.append(0xFF000000 | g << 8)
        bits.put(1, 1)
        bits.put(3, 2)
        bits.put(colours - 1, 8)
        before, diffs = 0, []
        for c in table:
            c |= 0xFF000000
            diffs.append(sum((((c >> b) - (before >> b)) & 255) << b for b in (0, 8, 16, 24)))
            before = c
        bits.put(0, 1)
        codes, _, _ = write_group(bits, [(d,) for d in diffs])
        for d in diffs:
            put_token(bits, codes, (d,))
    else:
        per = 1
        s = []
        for v in px.reshape(-1):
            v = int(v)
            g = v >> 8 & 255
            s.append(0xFF000000 | ((v >> 16) - g & 255) << 16 | g << 8 | (v - g & 255))
        bits.put(1, 1)
        bits.put(2, 2)
    bits.put(0, 3)  # no further transform, no colour cache, no meta codes
    segs = parse(s, o["segment_pixels"], o["lz77"])
    toks = [t for _, _, ts in segs for t in ts]
    codes, kinds, deep = write_group(bits, toks)
    seg_bits = []
    for _, _, ts in segs:
        at = bits.n
        for t in ts:
            put_token(bits, codes, t)
        seg_bits.append(bits.n - at)
    matches = [(b, e, t) for b, e, ts in segs for t in ts if len(t) == 3]
    info = dict(colours=colours, per=per, symbols=len(s), segments=len(segs), tokens=len(toks), matches=len(matches), longest=max([t[0] for _, _, t in matches] or [0]),
                seg_bits=seg_bits, kinds=kinds, deepest=deep, reaches_back=sum(1 for b, _, t in matches if t[2] - t[1] < b),
                ends_at_border=sum(1 for _, e, t in matches if t[2] + t[0] == e and e < len(s) and s[e] == s[e - t[1]]), distances=sorted(set(t[1] for _, _, t in matches)))
    out = bits.bytes()
    info["payload_bytes"] = len(out)
    return out, info


def encode(frames, fps, **opt):
    o = options(**opt)
    duration = duration_of(fps, o)
    nf, h, w = frames.shape
    if nf < 1 or w < 1 or h < 1:
        raise Refused(INVAL, "shape")
    if w > 16384 or h > 16384:
        raise Refused(UNSUPPORTED, "side")
    frames = frames.astype(np.uint32) & 0xFFFFFF
    body = b"WEBP" + b"VP8X" + struct.pack("<II", 10, 2) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    body += b"ANIM" + struct.pack("<IIH", 6, 0, o["loop"])
    canvas, info = [], []
    for f in range(nf):
        x, y, rw, rh = rect_of(frames[f], frames[f - 1]) if f and o["diff"] else (0, 0, w, h)
        payload, i = image(frames[f, y:y + rh, x:x + rw], o)
        i["rect"] = (x, y, rw, rh)
        info.append(i)
        chunk = b"VP8L" + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) & 1)
        head = b"".join(v.to_bytes(3, "little") for v in (x // 2, y // 2, rw - 1, rh - 1, duration)) + b"\x02"
        body += b"ANMF" + struct.pack("<I", len(head) + len(chunk)) + head + chunk
        shown = canvas[-1].copy() if f else np.zeros((h, w), np.uint32)
        shown[y:y + rh, x:x + rw] = frames[f, y:y + rh, x:x + rw]
        canvas.append(shown)
    return b"RIFF" + struct.pack("<I", len(body)) + body, np.stack(canvas), info


# ---- the reader
class Reader:
    def __init__(self, data):
        self.v, self.at, self.n = int.from_bytes(data, "little"), 0, 8 * len(data)

    def get(self, n):
        assert self.at + n <= self.n, "the bits end early"
        v = self.v >> self.at & ((1 << n) - 1)
        self.at += n
        return v


def read_code(r, nsym):
    """-> {(length, code read bit by bit, first bit highest): symbol}; a code of one symbol: {(0, 0): symbol}"""
    if r.get(1):
        n = r.get(1) + 1
        syms = [r.get(8 if r.get(1) else 1)]
        if n == 2:
            syms.append(r.get(8))
            return {(1, 0): min(syms), (1, 1): max(syms)} if syms[0] != syms[1] else {(0, 0): syms[0]}
        return {(0, 0): syms[0]}
    count = r.get(4) + 4
    cl = [0] * 19
    for k in range(count):
        cl[CL_ORDER[k]] = r.get(3)
    clc = table_of(cl)
    most = nsym
    if r.get(1):
        nb = 2 + 2 * r.get(3)
        most = 2 + r.get(nb)
    lens, before = [], 8
    while len(lens) < nsym and most > 0:
        most -= 1
        sym = read_symbol(r, clc)
        if sym < 16:
            lens.append(sym)
            before = sym or before
        elif sym == 16:
            lens += [before] * (3 + r.get(2))
        elif sym == 17:
            lens += [0] * (3 + r.get(3))
        else:
            lens += [0] * (11 + r.get(7))
    assert len(lens) <= nsym, "the lengths run past the alphabet"
    lens += [0] * (nsym - len(lens))
    return table_of(lens)


def table_of(lens):
    used = [s for s, l in enumerate(lens) if l]
    if len(used) == 1:
        return {(0, 0): used[0]}
    out, code = {}, 0
    for b in range(1, 16):
        for s, l in enumerate(lens):
            if l == b:
                out[(b, code)] = s
                code += 1
        code <<= 1
    assert sum(1 << (15 - l) for l in lens if l) == 1 << 15, "the code is not complete"
    return out


def read_symbol(r, table):
    if (0, 0) in table:
        return table[(0, 0)]
    code = 0
    for n in range(1, 16):
        code = code << 1 | r.get(1)
        if (n, code) in table:
            return table[(n, code)]
    raise AssertionError("no such code")


def read_value(r, sym):
    if sym < 4:
        return sym + 1
    eb = (sym - 2) >> 1
    return ((2 + (sym & 1)) << eb) + r.get(eb) + 1


def read_pixels(r, n, main):
    assert r.get(1) == 0, "a colour cache"
    if main:
        assert r.get(1) == 0, "meta codes"
    codes = [read_code(r, k) for k in ALPHABETS]
    out = []
    while len(out) < n:
        g = read_symbol(r, codes[0])
        if g < 256:
            red, blue, alpha = (read_symbol(r, codes[k]) for k in (1, 2, 3))
            out.append(alpha << 24 | red << 16 | g << 8 | blue)
            continue
        length = read_value(r, g - 256)
        dist = read_value(r, read_symbol(r, codes[4]))
        assert dist > 120, "a short distance code"
        dist -= 120
        assert dist <= len(out) and len(out) + length <= n, "a match outside the image"
        for _ in range(length):
            out.append(out[-dist])
    return out


def read_vp8l(data):
    """-> uint32 [h][w] of 0xAARRGGBB"""
    r = Reader(data)
    assert r.get(8) == 0x2F
    w, h = r.get(14) + 1, r.get(14) + 1
    assert r.get(4) == 0
    table, green, seen, pw = None, False, set(), w
    while r.get(1):
        t = r.get(2)
        assert t not in seen and t in (2, 3)
        seen.add(t)
        if t == 2:
            green = True
        else:
            n = r.get(8) + 1
            d = read_pixels(r, n, False)
            table, before = [], 0
            for v in d:
                before = sum((((v >> b) + (before >> b)) & 255) << b for b in (0, 8, 16, 24))
                table.append(before)
            pw = (w + bundle_of(n) - 1) // bundle_of(n)
    px = read_pixels(r, pw * h, True)
    assert (r.at + 7) // 8 == len(data), "bytes behind the image"
    out = np.zeros((h, w), np.uint32)
    for y in range(h):
        for x in range(w):
            if table is not None:
                per = bundle_of(len(table))
                k = px[y * pw + x // per] >> 8 & 255
                k = k >> (x % per * (8 // per)) & ((1 << (8 // per)) - 1)
                out[y, x] = table[k] if k < len(table) else 0
            else:
                v = px[y * w + x]
                g = v >> 8 & 255 if green else 0
                out[y, x] = v & 0xFF00FF00 | ((v >> 16) + g & 255) << 16 | (v + g & 255)
    return out


def chunks_of(data):
    at = 0
    while at < len(data):
        tag, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + n <= len(data), "a chunk runs past its parent"
        yield tag, data[at + 8:at + 8 + n]
        at += 8 + n + (n & 1)
    assert at == len(data) or at == len(data) + 1


def decode(file):
    assert file[:4] == b"RIFF" and file[8:12] == b"WEBP" and struct.unpack("<I", file[4:8])[0] == len(file) - 8
    parsed, frames, canvas = dict(frames=[]), [], None
    for tag, body in chunks_of(file[12:]):
        if tag == b"VP8X":
            assert len(body) == 10 and body[0] == 2
            parsed["width"], parsed["height"] = int.from_bytes(body[4:7], "little") + 1, int.from_bytes(body[7:10], "little") + 1
            canvas = np.zeros((parsed["height"], parsed["width"]), np.uint32)
        elif tag == b"ANIM":
            assert len(body) == 6 and body[:4] == b"\0\0\0\0"
            parsed["loop"] = struct.unpack("<H", body[4:])[0]
        else:
            assert tag == b"ANMF"
            x, y, w, h, duration = (int.from_bytes(body[k:k + 3], "little") for k in (0, 3, 6, 9, 12))
            x, y, w, h = 2 * x, 2 * y, w + 1, h + 1
            parsed["frames"].append(dict(x=x, y=y, w=w, h=h, duration=duration, flags=body[15]))
            (tag2, data), = list(chunks_of(body[16:]))
            assert tag2 == b"VP8L"
            px = read_vp8l(data)
            assert px.shape == (h, w) and y + h <= canvas.shape[0] and x + w <= canvas.shape[1]
            assert (px >> 24 == 0xFF).all()
            canvas = canvas.copy()
            canvas[y:y + h, x:x + w] = px & 0xFFFFFF
            frames.append(canvas)
    return frames, parsed
