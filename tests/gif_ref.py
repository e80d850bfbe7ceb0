"""A plain-Python restatement of the GIF reader's rule (include/tilemotion.h) that shares no code with the library:
the container walk, the LZW decoder (in the textbook form, a table of strings), the compositor and the rate -- and the tests' own GIF
WRITER, with the switches the edge cases and the damage need (minimum code size, when clears are written, no initial clear, no eoi,
sub-block sizes, interlace, local tables, any graphic control, other extensions, no trailer)."""
import struct

import numpy as np

IO, UNSUPPORTED = -5, -6
TRUNCATED, BAD_CODE, BAD_DESC = 64, 65, 66


class Refused(Exception):
    def __init__(self, code, kind):
        super().__init__("%d: %s" % (code, kind))
        self.code, self.kind = code, kind


# ---- the container walk
def _skip_blocks(d, pos, what):
    while True:
        if pos >= len(d):
            raise Refused(IO, "past the end: " + what)
        n = d[pos]
        pos += 1
        if n == 0:
            return pos
        if n > len(d) - pos:
            raise Refused(IO, "past the end: sub-block of " + what)
        pos += n


def parse(d):
    """-> dict(width, height, version, loop, global_table (list of 0xRRGGBB), bg_index, bg, images=[dict], fps, uniform_delay)"""
    d = bytes(d)
    if len(d) < 6 or d[:6] not in (b"GIF87a", b"GIF89a"):
        raise Refused(UNSUPPORTED, "signature")
    if len(d) >= 1 << 32:
        raise Refused(UNSUPPORTED, "4 GiB")
    if len(d) < 13:
        raise Refused(IO, "past the end: screen")
    w, h, packed, bgi = struct.unpack_from("<HHBB", d, 6)
    if w == 0 or h == 0:
        raise Refused(IO, "empty screen")
    pos = 13
    gct = []
    if packed & 0x80:
        n = 2 << (packed & 7)
        if pos + 3 * n > len(d):
            raise Refused(IO, "past the end: global table")
        gct = [d[pos + 3 * i] << 16 | d[pos + 3 * i + 1] << 8 | d[pos + 3 * i + 2] for i in range(n)]
        pos += 3 * n
    out = dict(width=w, height=h, version=87 if d[4:5] == b"7" else 89, loop=-1, global_table=gct, bg_index=bgi, bg=gct[bgi] if bgi < len(gct) else 0, images=[])
    gce = dict(delay=0, disposal=0, transparent=-1)
    while True:
        if pos >= len(d):
            if not out["images"]:
                raise Refused(IO, "no image")
            break
        b = d[pos]
        if b == 0x3B:
            break
        if b == 0x21:
            if pos + 2 > len(d):
                raise Refused(IO, "past the end: extension")
            label = d[pos + 1]
            pos += 2
            if label == 0xF9 and pos < len(d) and d[pos] >= 4 and d[pos] <= len(d) - pos - 1:
                f, delay, tr = struct.unpack_from("<BHB", d, pos + 1)
                gce = dict(delay=delay, disposal=(f >> 2) & 7, transparent=tr if f & 1 else -1)
            if label == 0xFF and pos + 16 <= len(d) and d[pos] == 11 and d[pos + 1:pos + 12] in (b"NETSCAPE2.0", b"ANIMEXTS1.0") and d[pos + 12] >= 3 and d[pos + 13] == 1:
                out["loop"] = d[pos + 14] | d[pos + 15] << 8
            pos = _skip_blocks(d, pos, "extension")
            continue
        if b != 0x2C:
            raise Refused(IO, "introducer")
        if pos + 10 > len(d):
            raise Refused(IO, "past the end: image descriptor")
        l, t, iw, ih, p = struct.unpack_from("<HHHHB", d, pos + 1)
        pos += 10
        if iw == 0 or ih == 0:
            raise Refused(IO, "empty rectangle")
        table, local = gct, 0
        if p & 0x80:
            n = 2 << (p & 7)
            if pos + 3 * n > len(d):
                raise Refused(IO, "past the end: local table")
            table = [d[pos + 3 * i] << 16 | d[pos + 3 * i + 1] << 8 | d[pos + 3 * i + 2] for i in range(n)]
            local = 1
            pos += 3 * n
        elif not gct:
            raise Refused(IO, "no table")
        if pos >= len(d):
            raise Refused(IO, "past the end: code size")
        mn = d[pos]
        pos += 1
        if mn < 2 or mn > 8:
            raise Refused(IO, "code size")
        start = pos
        pos = _skip_blocks(d, pos, "image data")
        out["images"].append(dict(left=l, top=t, width=iw, height=ih, interlaced=1 if p & 0x40 else 0, table=table, local_table=local, min_code_size=mn, data_off=start,
                                  data_bytes=pos - start, **gce))
        gce = dict(delay=0, disposal=0, transparent=-1)
    if not out["images"]:
        raise Refused(IO, "no image")
    ds = [10 if im["delay"] < 2 else im["delay"] for im in out["images"]]
    out["fps"] = 100.0 * len(ds) / sum(ds)
    out["uniform_delay"] = 1 if len(set(ds)) == 1 else 0
    return out


def payload(span):
    """the data a sub-block chain holds; the end of the span ends it like a terminator"""
    out, pos = bytearray(), 0
    while pos < len(span):
        n = span[pos]
        pos += 1
        if n == 0:
            break
        out += span[pos:pos + n]
        pos += n
    return bytes(out)


# ---- LZW, the textbook form: a table of strings
def lzw_decode(span, mn, npix):
    """-> (indices (bytes, out_n of them), (code, in_pos, out_n), what it met: dict(longest, farthest, full, kwkwk, kwkwk_periods, clears))"""
    data = payload(span)
    total = len(data) * 8
    clear, eoi = 1 << mn, (1 << mn) + 1
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    born = [0] * len(table)  # where in the output an entry's string was first written (for `farthest` only)
    width, prev, prev_at, bit, rc = mn + 1, None, 0, 0, 0
    out = bytearray()
    met = dict(longest=0, farthest=0, full=False, kwkwk=0, kwkwk_periods=set(), clears=0)
    while len(out) < npix:
        if bit + width > total:
            rc = TRUNCATED
            break
        code = (int.from_bytes(data[bit >> 3:(bit >> 3) + 3], "little") >> (bit & 7)) & ((1 << width) - 1)
        bit += width
        if code == clear:
            del table[clear + 2:]
            del born[clear + 2:]
            width, prev = mn + 1, None
            met["clears"] += 1
            continue
        if code == eoi:
            rc = TRUNCATED
            break
        if prev is None:
            if code >= clear:
                rc = BAD_CODE
                break
            prev, prev_at = table[code], len(out)
            out.append(code)
            continue
        if code < len(table):
            s = table[code]
            if code >= clear:
                met["farthest"] = max(met["farthest"], len(out) - born[code])
        elif code == len(table) and len(table) < 4096:
            s = prev + prev[:1]
            met["kwkwk"] += 1
            met["kwkwk_periods"].add(len(prev))
        else:
            rc = BAD_CODE
            break
        met["longest"] = max(met["longest"], len(s))
        at = len(out)
        out += s[:npix - at]
        if len(table) < 4096:
            table.append(prev + s[:1])
            born.append(prev_at)
            if len(table) == 1 << width and width < 12:
                width += 1
        else:
            met["full"] = True
        prev, prev_at = s, at
    return bytes(out), (rc, (bit + 7) // 8, len(out)), met


# ---- frames
def stored_rows(h, interlaced):
    """the picture row of every stored row"""
    if not interlaced:
        return list(range(h))
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def decode(d, first=0, count=None, background=None):
    """-> (frames uint32 [count][h][w] of 0x00RRGGBB, status per image 0 .. first + count - 1, info); frames from the first image with a
    status on are None"""
    info = parse(d)
    ims = info["images"]
    count = len(ims) - first if count is None else count
    W, H = info["width"], info["height"]
    bg = info["bg"] if background is None else background & 0xFFFFFF
    canvas = np.full((H, W), bg, np.uint32)
    saved = canvas.copy()
    frames, status, failed = [], [], False
    for i in range(first + count):
        im = ims[i]
        idx, st, _ = lzw_decode(d[im["data_off"]:im["data_off"] + im["data_bytes"]], im["min_code_size"], im["width"] * im["height"])
        status.append(st[0])
        failed = failed or st[0] != 0
        if failed:
            if i >= first:
                frames.append(None)
            continue
        if i > 0:
            p = ims[i - 1]
            x0, y0, x1, y1 = min(p["left"], W), min(p["top"], H), min(p["left"] + p["width"], W), min(p["top"] + p["height"], H)
            if p["disposal"] == 2:
                canvas[y0:y1, x0:x1] = bg
            elif p["disposal"] == 3:
                canvas[y0:y1, x0:x1] = saved[y0:y1, x0:x1]
        saved = canvas.copy()
        stored = np.frombuffer(idx, np.uint8).reshape(im["height"], im["width"])
        pic = np.empty_like(stored)
        pic[stored_rows(im["height"], im["interlaced"])] = stored
        table = np.zeros(256, np.uint32)
        table[:len(im["table"])] = im["table"]
        x0, y0, x1, y1 = min(im["left"], W), min(im["top"], H), min(im["left"] + im["width"], W), min(im["top"] + im["height"], H)
        part = pic[:y1 - y0, :x1 - x0]
        canvas[y0:y1, x0:x1] = np.where(part == im["transparent"], canvas[y0:y1, x0:x1], table[part])
        if i >= first:
            frames.append(canvas.copy())
    return frames, status, info


# ---- the writer
def lzw_codes(indices, mn, clear="full", initial_clear=True, eoi=True):
    """the codes of a picture's indices.  clear: "full" (a clear when the table is full), "never" (the table fills and stays: deferred
    clear), or N (a clear behind every N codes)"""
    cl, table, nxt, codes = 1 << mn, {}, (1 << mn) + 2, []
    if initial_clear:
        codes.append(cl)
    s, since = (), 0
    for v in indices:
        v = int(v)
        t = s + (v,)
        if len(t) == 1 or t in table:
            s = t
            continue
        codes.append(s[0] if len(s) == 1 else table[s])
        since += 1
        if nxt < 4096:
            table[t] = nxt
            nxt += 1
        s = (v,)
        if (clear == "full" and nxt == 4096) or (isinstance(clear, int) and since >= clear):
            codes.append(cl)
            table, nxt, since = {}, cl + 2, 0
    if s:
        codes.append(s[0] if len(s) == 1 else table[s])
    if eoi:
        codes.append(cl + 1)
    return codes


def pack_codes(codes, mn):
    """LSB first, at the widths a decoder is at when it reads them"""
    cl, nxt, width, fresh = 1 << mn, (1 << mn) + 2, mn + 1, True
    acc, n = 0, 0
    for c in codes:
        acc |= c << n
        n += width
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
    return acc.to_bytes((n + 7) // 8, "little")


def sub_blocks(data, size=255):
    out = bytearray()
    for i in range(0, len(data), size):
        part = data[i:i + size]
        out += bytes([len(part)]) + part
    return bytes(out) + b"\0"


def table_bytes(colours):
    n = 2
    while n < len(colours):
        n *= 2
    colours = list(colours) + [0] * (n - len(colours))
    return b"".join(bytes([c >> 16 & 255, c >> 8 & 255, c & 255]) for c in colours), n.bit_length() - 2


def gce_bytes(disposal=0, transparent=-1, delay=0, user_input=0):
    return b"\x21\xf9\x04" + struct.pack("<BHB", disposal << 2 | user_input << 1 | (1 if transparent >= 0 else 0), delay, max(transparent, 0)) + b"\0"


def image_bytes(indices, left=0, top=0, table=None, interlace=False, min_code=None, clear="full", initial_clear=True, eoi=True, sub=255, codes=None, after=b"",
                min_code_byte=None):
    """one image block.  indices: uint8 [h][w]; table: a local colour table; codes: written in place of the picture's own; after: payload
    bytes behind the last code; min_code_byte: what the file says the minimum code size is"""
    indices = np.asarray(indices, np.uint8)
    h, w = indices.shape
    if min_code is None:
        min_code = max(2, int(indices.max()).bit_length())
    stored = indices[stored_rows(h, interlace)]
    if codes is None:
        codes = lzw_codes(stored.reshape(-1), min_code, clear, initial_clear, eoi)
    packed, tb = 0x40 if interlace else 0, b""
    if table is not None:
        tb, bits = table_bytes(table)
        packed |= 0x80 | bits
    return b"\x2c" + struct.pack("<HHHHB", left, top, w, h, packed) + tb + bytes([min_code if min_code_byte is None else min_code_byte]) + sub_blocks(
        pack_codes(codes, min_code) + after, sub)


def write_gif(width, height, blocks, table=None, bg_index=0, version=b"89a", loop=None, trailer=True, after=b""):
    """blocks: what image_bytes, gce_bytes and the extensions below return, in file order"""
    packed, tb = 0, b""
    if table is not None:
        tb, bits = table_bytes(table)
        packed = 0x80 | bits | bits << 4
    out = b"GIF" + version + struct.pack("<HHBBB", width, height, packed, bg_index, 0) + tb
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\0"
    return out + b"".join(blocks) + (b"\x3b" if trailer else b"") + after


def comment(text=b"a comment"):
    return b"\x21\xfe" + sub_blocks(text, 7)


def plain_text(text=b"plain text"):
    return b"\x21\x01" + bytes([12]) + bytes(12) + sub_blocks(text, 254)
