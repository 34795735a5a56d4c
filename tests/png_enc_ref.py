"""The definition of pt_canvas_encode_png's bytes (include/pt.h), in numpy and Python's zlib (1.2.11 here).

The image is the canvas top-down: rows[0] is scanline 0. Filters are the PNG specification's over bpp = 3 or 4
bytes; the adaptive choice takes, per row, the type whose filtered row has the least sum of |byte as int8|, the
lowest type on a tie. The filtered stream (each row's filter byte, then its bytes) is cut into chunks of 16,320 bytes;
chunk i is what compressobj(6, DEFLATED, 15, 8, Z_RLE) writes when it is fed that chunk in one compress() call
followed by flush(Z_FULL_FLUSH), or flush(Z_FINISH) after the last. A full flush resets the window, so every chunk
stands alone; the one stream object carries the zlib header into the first chunk and the Adler-32 of the whole
filtered stream behind the last. One IDAT per chunk."""
import struct
import zlib

import numpy as np

CHUNK = 255 * 64
RGB, RGBA = 0, 1
NONE, SUB, UP, AVERAGE, PAETH, ADAPTIVE = range(6)
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def filter_row(kind, cur, above, bpp):
    """cur, above: uint8 arrays of one row's bytes -> the filtered bytes"""
    x = cur.astype(np.int32)
    b = above.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if len(x) > bpp else np.zeros(len(x), np.int32)
    if len(x) > bpp:
        c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]])
    else:
        c = np.zeros(len(x), np.int32)
    if kind == NONE:
        pred = 0
    elif kind == SUB:
        pred = a
    elif kind == UP:
        pred = b
    elif kind == AVERAGE:
        pred = (a + b) >> 1
    else:
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return ((x - pred) & 255).astype(np.uint8)


def filtered_stream(rows, filt):
    """rows: (H, W, bpp) uint8 top-down -> (the filtered stream, the filter type of every row)"""
    h, w, bpp = rows.shape
    flat = rows.reshape(h, w * bpp)
    out = bytearray()
    types = []
    above = np.zeros(w * bpp, np.uint8)
    for y in range(h):
        if filt == ADAPTIVE:
            cands = [filter_row(k, flat[y], above, bpp) for k in range(5)]
            costs = [int(np.abs(c.view(np.int8).astype(np.int32)).sum()) for c in cands]
            k = costs.index(min(costs))
            f = cands[k]
        else:
            k = filt
            f = filter_row(k, flat[y], above, bpp)
        types.append(k)
        out.append(k)
        out += f.tobytes()
        above = flat[y]
    return bytes(out), types


def deflate_chunks(stream):
    """the IDAT payloads, one per chunk of the filtered stream"""
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    n = (len(stream) + CHUNK - 1) // CHUNK
    out = []
    for i in range(n):
        data = z.compress(stream[i * CHUNK:(i + 1) * CHUNK])
        data += z.flush(zlib.Z_FINISH if i == n - 1 else zlib.Z_FULL_FLUSH)
        out.append(data)
    return out


def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def head(w, h, colour):
    return SIGNATURE + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if colour == RGBA else 2, 0, 0, 0))


TAIL = png_chunk(b"IEND", b"")


def encode_stats(rows_rgba, colour=RGB, filt=ADAPTIVE):
    """rows_rgba: (H, W, 4) uint8 top-down -> (the file, {"types", "stream", "payloads"})"""
    rows = np.ascontiguousarray(rows_rgba if colour == RGBA else rows_rgba[..., :3])
    h, w = rows.shape[:2]
    stream, types = filtered_stream(rows, filt)
    payloads = deflate_chunks(stream)
    data = head(w, h, colour) + b"".join(png_chunk(b"IDAT", p) for p in payloads) + TAIL
    return data, {"types": types, "stream": stream, "payloads": payloads}


def encode(rows_rgba, colour=RGB, filt=ADAPTIVE):
    return encode_stats(rows_rgba, colour, filt)[0]


# ---- a deflate block walker: what a case reaches ----
class _Bits:
    def __init__(self, data):
        self.d, self.at = data, 0

    def get(self, n):
        v = 0
        for i in range(n):
            v |= (self.d[self.at >> 3] >> (self.at & 7) & 1) << i
            self.at += 1
        return v

    def align(self):
        self.at = (self.at + 7) & ~7


def _decoder(lengths):
    """canonical codes (RFC 1951 3.2.2) -> {(length, code): symbol}"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.get(1)
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no such code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def walk_blocks(raw):
    """raw deflate data (no zlib header) -> [{"type", "final", "symbols", "matches", "maxlen": (l, d, bl), "out", "clcounts"}]
    (clcounts: how often the header used each code-length symbol);
    distances other than 1 raise: this encoder writes none"""
    bits = _Bits(raw)
    blocks = []
    while True:
        final, btype = bits.get(1), bits.get(2)
        info = {"type": ("stored", "fixed", "dynamic")[btype], "final": final, "symbols": 0, "matches": 0,
                "maxlen": (0, 0, 0), "out": 0, "clcounts": [0] * 19}
        if btype == 0:
            bits.align()
            n = bits.get(16)
            assert bits.get(16) == n ^ 0xFFFF
            bits.at += 8 * n
            info["out"] = n
        else:
            if btype == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_BL_ORDER[i]] = bits.get(3)
                ct = _decoder(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, ct)
                    info["clcounts"][s] += 1
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                info["maxlen"] = (max(ll), max(dl), max(cl))
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = _symbol(bits, lt)
                if s == 256:
                    break
                info["symbols"] += 1
                if s < 256:
                    info["out"] += 1
                else:
                    length = _LBASE[s - 257] + bits.get(_LEXTRA[s - 257])
                    if _symbol(bits, dt) != 0:
                        raise ValueError("a distance other than 1")
                    info["matches"] += 1
                    info["out"] += length
        blocks.append(info)
        if final:
            return blocks
