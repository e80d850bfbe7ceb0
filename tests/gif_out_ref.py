"""A plain-Python restatement of the GIF writer's rule (include/tilemotion.h) that shares no code with the library:
the changed rectangle, the exact table, the median cut over 15-bit cells, the segments and the container.  The codes of a segment are
tests/gif_ref.py's lzw_codes, their widths the ones its pack_codes gives (pack below is the same rule writing bytes as it goes: pack_codes
keeps one growing integer, which a 192 x 192 picture makes slow; test_gif_out_host.py holds the two equal)."""
import struct

import numpy as np

from tests import gif_ref

INVAL, UNSUPPORTED = -1, -6
AUTO, EXACT, QUANTISE = 0, 1, 2
COLOURS = {"auto": AUTO, "exact": EXACT, "quantise": QUANTISE}
DEFAULTS = dict(colours="auto", max_colours=256, diff=True, segment_pixels=4096, loop=0, delay_cs=0)


class Refused(Exception):
    def __init__(self, code, kind):
        super().__init__("%d: %s" % (code, kind))
        self.code, self.kind = code, kind


def options(**kw):
    opt = dict(DEFAULTS)
    for k in kw:
        if k not in opt:
            raise TypeError(k)
    opt.update(kw)
    if opt["colours"] not in COLOURS:
        raise Refused(INVAL, "colours")
    if not 2 <= opt["max_colours"] <= 256:
        raise Refused(INVAL, "max_colours")
    if opt["diff"] not in (0, 1, False, True):
        raise Refused(INVAL, "diff")
    if opt["segment_pixels"] != 0 and opt["segment_pixels"] < 256:
        raise Refused(INVAL, "segment_pixels")
    if not -1 <= opt["loop"] <= 65535:
        raise Refused(INVAL, "loop")
    if opt["delay_cs"] != 0 and not 2 <= opt["delay_cs"] <= 65535:
        raise Refused(INVAL, "delay_cs")
    return opt


def delay_of(fps, delay_cs=0):
    if delay_cs:
        return delay_cs
    if not fps > 0:
        raise Refused(INVAL, "rate")
    d = int(np.floor(100.0 / fps + 0.5))
    if d > 65535:
        raise Refused(INVAL, "delay")
    return max(2, d)


def rectangle(cur, prev):
    """(x, y, w, h) of the pixels of cur that differ from prev; none: the 1 x 1 at (0, 0)"""
    ys, xs = np.nonzero((cur & 0xFFFFFF) != (prev & 0xFFFFFF))
    if len(ys) == 0:
        return 0, 0, 1, 1
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def exact_table(px):
    table, idx = np.unique(px, return_inverse=True)
    return [int(c) for c in table], idx.reshape(px.shape).astype(np.uint8) if len(table) <= 256 else None


def median_cut(px, max_colours):
    """-> (table, indices, what it met: dict(cells, boxes, ties))"""
    px = px.astype(np.int64)
    ch = [(px >> 16) & 255, (px >> 8) & 255, px & 255]
    cell = ((ch[0] >> 3) << 10 | (ch[1] >> 3) << 5 | ch[2] >> 3).reshape(-1)
    cnt = np.bincount(cell, minlength=32768).astype(np.int64).reshape(32, 32, 32)
    sums = [np.bincount(cell, weights=c.reshape(-1).astype(np.float64), minlength=32768).astype(np.int64).reshape(32, 32, 32) for c in ch]
    met = dict(cells=int((cnt > 0).sum()), ties=set())

    def tight(lo, hi):
        sl = tuple(slice(lo[a], hi[a] + 1) for a in range(3))
        nz = np.nonzero(cnt[sl])
        lo2 = [lo[a] + int(nz[a].min()) for a in range(3)]
        hi2 = [lo[a] + int(nz[a].max()) for a in range(3)]
        sl = tuple(slice(lo2[a], hi2[a] + 1) for a in range(3))
        return dict(lo=lo2, hi=hi2, n=int(cnt[sl].sum()), cells=len(nz[0]), sl=sl)

    boxes = [tight([0, 0, 0], [31, 31, 31])]
    while len(boxes) < max_colours:
        cands = [i for i, b in enumerate(boxes) if b["cells"] >= 2]
        if not cands:
            break
        most = max(boxes[i]["n"] for i in cands)
        first = [i for i in cands if boxes[i]["n"] == most]
        if len(first) > 1:
            met["ties"].add("box")
        b = boxes[first[0]]
        ext = [b["hi"][a] - b["lo"][a] for a in range(3)]
        longest = [a for a in (1, 0, 2) if ext[a] == max(ext)]
        if len(longest) > 1:
            met["ties"].add("axis")
        axis = longest[0]
        per = cnt[b["sl"]].sum(axis=tuple(a for a in range(3) if a != axis))
        k = int(np.nonzero(np.cumsum(per) >= (b["n"] + 1) // 2)[0][0])
        if k == len(per) - 1:
            k -= 1
            met["ties"].add("cut moved")
        lo_hi, up_lo = list(b["hi"]), list(b["lo"])
        lo_hi[axis] = b["lo"][axis] + k
        up_lo[axis] = b["lo"][axis] + k + 1
        boxes[first[0]] = tight(b["lo"], lo_hi)
        boxes.append(tight(up_lo, b["hi"]))
    box_of = np.zeros((32, 32, 32), np.uint8)
    table = []
    for i, b in enumerate(boxes):
        box_of[b["sl"]] = i
        c = [(2 * int(s[b["sl"]].sum()) + b["n"]) // (2 * b["n"]) for s in sums]
        table.append(c[0] << 16 | c[1] << 8 | c[2])
    met["boxes"] = len(boxes)
    return table, box_of.reshape(-1)[cell].reshape(px.shape).astype(np.uint8), met


def palettise(px, colours="auto", max_colours=256, frame=0):
    """px: uint32 [h][w] -> (table, exact, indices, met)"""
    px = px & 0xFFFFFF
    table, idx = exact_table(px)
    if colours != "quantise" and len(table) <= max_colours:
        return table, True, idx, dict(colours=len(table))
    if colours == "exact":
        raise Refused(UNSUPPORTED, "frame %d holds %d colours" % (frame, len(table)))
    table, idx, met = median_cut(px, max_colours)
    met["colours"] = len(np.unique(px))
    return table, False, idx, met


def min_code_of(ncol):
    bits = 1
    while (1 << bits) < ncol:
        bits += 1
    return max(2, bits)


def segment_codes(indices, mn, segment_pixels):
    """[codes of every segment]"""
    indices = np.asarray(indices).reshape(-1)
    n = len(indices)
    step = segment_pixels if segment_pixels else n
    parts = [indices[at:at + step] for at in range(0, n, step)]
    return [gif_ref.lzw_codes(p, mn, clear="full", initial_clear=True, eoi=i + 1 == len(parts)) for i, p in enumerate(parts)]


def pack(codes, mn):
    """gif_ref.pack_codes, bytes written as they fill -> (bytes, bits, [the width every code was written at])"""
    cl, nxt, width, fresh = 1 << mn, (1 << mn) + 2, mn + 1, True
    out, acc, n, bits, widths = bytearray(), 0, 0, 0, []
    for c in codes:
        acc |= c << n
        n += width
        bits += width
        widths.append(width)
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
        if c == cl:
            nxt, width, fresh = cl + 2, mn + 1, True
        elif c == cl + 1:
            pass
        elif fresh:
            fresh = False
        elif nxt < 4096:
            nxt += 1
            if nxt == 1 << width and width < 12:
                width += 1
    if n:
        out.append(acc & 255)
    return bytes(out), bits, widths


def payload(indices, mn, segment_pixels):
    """-> (the image data before sub-blocks, met: dict(segments, seg_bits, codes, clears, longest, double_clear, widen_last))"""
    segs = segment_codes(indices, mn, segment_pixels)
    allc = [c for s in segs for c in s]
    data, bits, widths = pack(allc, mn)
    cl = 1 << mn
    # the bits that belong to segment k: its codes without the clear that opens it (but for k = 0), and the clear that opens k + 1
    seg_bits, at = [], 0
    for k, s in enumerate(segs):
        first = at if k == 0 else at + 1
        last = at + len(s) + (1 if k + 1 < len(segs) else 0)
        seg_bits.append(sum(widths[first:last]))
        at += len(s)
    met = dict(segments=len(segs), seg_bits=seg_bits, codes=len(allc), clears=sum(1 for c in allc if c == cl), bits=bits)
    # a table that fills on a segment's last index: clear, one literal, the segment's end
    met["fills_on_last"] = any(len(s) >= 3 and s[-3 if k + 1 == len(segs) else -2] == cl for k, s in enumerate(segs))
    # a segment whose last code widens the width: the clear (or eoi) behind it is written wider than that code
    ends, at = [], 0
    for k, s in enumerate(segs):
        at += len(s)
        last_code = at - (2 if k + 1 == len(segs) else 1)
        ends.append(last_code + 1 < len(widths) and widths[last_code + 1] > widths[last_code])
    met["widen_last"] = any(ends)
    # and the reader's view of it: the indices again, and the longest string it met
    flat = np.asarray(indices, np.uint8).reshape(-1)
    back, status, seen = gif_ref.lzw_decode(gif_ref.sub_blocks(data), mn, len(flat))
    assert status[0] == 0 and back == flat.tobytes()
    met["longest"] = seen["longest"]
    return data, met


def encode(frames, fps, **kw):
    """frames: uint32 [F][h][w] -> (file, canvas uint32 [F][h][w], info: a dict per frame of rect, exact, colours, min_code, payload_bytes
    and what palettise and payload met)"""
    opt = options(**kw)
    frames = np.asarray(frames)
    nf, h, w = frames.shape
    if nf < 1 or w < 1 or h < 1:
        raise Refused(INVAL, "shape")
    if w > 65535 or h > 65535:
        raise Refused(UNSUPPORTED, "side")
    delay = delay_of(fps, opt["delay_cs"])
    out = bytearray(b"GIF89a" + struct.pack("<HHBBB", w, h, 0x70, 0, 0))
    if opt["loop"] >= 0:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", opt["loop"]) + b"\0"
    canvas = np.zeros((nf, h, w), np.uint32)
    info = []
    for f in range(nf):
        x, y, rw, rh = rectangle(frames[f], frames[f - 1]) if opt["diff"] and f > 0 else (0, 0, w, h)
        table, exact, idx, met = palettise(frames[f, y:y + rh, x:x + rw], opt["colours"], opt["max_colours"], f)
        mn = min_code_of(len(table))
        data, lz = payload(idx, mn, opt["segment_pixels"])
        tb, bits = gif_ref.table_bytes(table)
        out += b"\x21\xf9\x04" + struct.pack("<BHB", 1 << 2, delay, 0) + b"\0"
        out += b"\x2c" + struct.pack("<HHHHB", x, y, rw, rh, 0x80 | bits) + tb + bytes([mn]) + gif_ref.sub_blocks(data)
        if f > 0:
            canvas[f] = canvas[f - 1]
        canvas[f, y:y + rh, x:x + rw] = np.asarray(table, np.uint32)[idx]
        met.update(lz)
        met.update(rect=(x, y, rw, rh), exact=exact, table=len(table), min_code=mn, payload_bytes=len(data))
        info.append(met)
    out += b"\x3b"
    return bytes(out), canvas, info
