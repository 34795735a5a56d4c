"""The definition of pt_targets_encode_exr's bytes (include/pt.h), in numpy and Python's zlib (1.2.11 here).

A channel is (name, texels, component, scale, type): texels is an (H, W, 4) float32 array with rows bottom-up, as
pt_read_pixels returns a render target; type is HALF or FLOAT. The file is a single-part scanline OpenEXR file,
version 2, with short names: the magic and version, the header's attributes, the offset table, the chunks. Channels
are stored sorted by name as unsigned bytes. Scanline y is the targets' row H - 1 - y. A chunk holds 1 scanline (NONE,
ZIPS) or 16 (ZIP), the last one fewer. ZIP data is the block's bytes with the even ones before the odd ones, each
byte but the first replaced by its difference to the one before it plus 128, deflated as a zlib stream of its own the
way png_enc_ref deflates the filtered stream (Z_RLE, level 6, a full flush behind every 16,320 bytes); where that
stream is not shorter than the block, the chunk holds the block's bytes as they are.

decode() is written apart from the layout above: it parses whatever attributes it finds, follows the offset table
and inflates with zlib.decompress."""
import struct
import zlib

import numpy as np

import png_enc_ref as P

HALF, FLOAT = 1, 2
NONE, ZIPS, ZIP = 0, 2, 3
LINES = {NONE: 1, ZIPS: 1, ZIP: 16}
CHANNELS_MAX = 16
MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])
PIECE = P.CHUNK


def half_bits(v):
    """float32 array -> binary16 bits, round to nearest even, every NaN 0x7E00"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16).view(np.uint16).copy()
    h[np.isnan(v)] = 0x7E00
    return h


def samples(texels, component, scale, kind):
    """one channel's stored samples: (H, W) uint16 or uint32, rows still bottom-up"""
    x = np.ascontiguousarray(texels[..., component], np.float32)
    scale = np.float32(scale)
    if scale == np.float32(1.0):
        v = x
    else:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            v = x * scale
    if kind == HALF:
        return half_bits(v)
    bits = v.view(np.uint32).copy()
    if scale != np.float32(1.0):
        bits[np.isnan(v)] = 0x7FC00000
    return bits


def _attr(name, kind, value):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def header(chans, w, h, compression):
    """chans: sorted [(name bytes, type)] -> the magic, the version and the header"""
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in chans) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (MAGIC + struct.pack("<I", 2)
            + _attr("channels", "chlist", chlist)
            + _attr("compression", "compression", bytes([compression]))
            + _attr("dataWindow", "box2i", box)
            + _attr("displayWindow", "box2i", box)
            + _attr("lineOrder", "lineOrder", b"\0")
            + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
            + b"\0")


def sort_channels(channels):
    return sorted(channels, key=lambda c: c[0].encode() if isinstance(c[0], str) else bytes(c[0]))


def raw_blocks(channels, compression):
    """the blocks' raw bytes, top scanline first"""
    chans = sort_channels(channels)
    h, w = chans[0][1].shape[:2]
    planes = [samples(t, comp, s, k)[::-1] for _, t, comp, s, k in chans]   # top-down
    lines = [b"".join(p[y].astype("<u2" if p.dtype == np.uint16 else "<u4").tobytes() for p in planes) for y in range(h)]
    step = LINES[compression]
    return [b"".join(lines[y:y + step]) for y in range(0, h, step)]


def predict(raw):
    """the byte reorder and the delta predictor"""
    r = np.frombuffer(raw, np.uint8)
    t = np.concatenate([r[0::2], r[1::2]]).astype(np.int32)
    p = t.copy()
    p[1:] = t[1:] - t[:-1] + 128
    return (p & 255).astype(np.uint8).tobytes()


def block_stream(raw):
    """the zlib stream of a block's predicted bytes, piece by piece"""
    return P.deflate_chunks(predict(raw))


def encode_stats(channels, compression=ZIP):
    chans = sort_channels(channels)
    h, w = chans[0][1].shape[:2]
    names = [c[0].encode() if isinstance(c[0], str) else bytes(c[0]) for c in chans]
    head = header([(n, c[4]) for n, c in zip(names, chans)], w, h, compression)
    blocks = raw_blocks(channels, compression)
    datas, fell_back, pieces = [], [], []
    for raw in blocks:
        if compression == NONE:
            datas.append(raw)
            continue
        parts = block_stream(raw)
        stream = b"".join(parts)
        pieces.append(parts)
        fell_back.append(len(stream) >= len(raw))
        datas.append(raw if len(stream) >= len(raw) else stream)
    at = len(head) + 8 * len(blocks)
    table, body = [], []
    for i, d in enumerate(datas):
        table.append(at)
        body.append(struct.pack("<ii", i * LINES[compression], len(d)) + d)
        at += 8 + len(d)
    data = head + struct.pack("<%dQ" % len(table), *table) + b"".join(body)
    return data, {"header": len(head), "blocks": blocks, "pieces": pieces, "fell_back": fell_back, "table": table}


def encode(channels, compression=ZIP):
    return encode_stats(channels, compression)[0]


def file_max(channels, compression):
    """what no file of these channels and this size exceeds: every block stored raw"""
    chans = sort_channels(channels)
    h, w = chans[0][1].shape[:2]
    head = 277 - 18 + sum(len(c[0]) + 17 for c in chans)
    line = w * sum(2 if c[4] == HALF else 4 for c in chans)
    nblocks = (h + LINES[compression] - 1) // LINES[compression]
    return head + 8 * nblocks + 8 * nblocks + h * line


# ---- an independent reader ----
def _cstr(data, at):
    end = data.index(b"\0", at)
    return data[at:end], end + 1


def decode(data):
    """file -> ({"name": (H, W) uint16 or uint32 sample bits, rows top-down}, attributes)"""
    assert data[:4] == MAGIC
    version, = struct.unpack_from("<I", data, 4)
    assert version & 0xFF == 2 and version >> 8 == 0, "single-part scanline, short names"
    at, attrs = 8, {}
    while data[at] != 0:
        name, at = _cstr(data, at)
        kind, at = _cstr(data, at)
        size, = struct.unpack_from("<i", data, at)
        attrs[name.decode()] = (kind.decode(), data[at + 4:at + 4 + size])
        at += 4 + size
    at += 1
    chans, v, p = [], attrs["channels"][1], 0
    while v[p] != 0:
        name, p = _cstr(v, p)
        kind, linear, xs, ys = struct.unpack_from("<iB3xii", v, p)
        assert kind in (HALF, FLOAT) and xs == 1 and ys == 1
        chans.append((name.decode(), kind))
        p += 16
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    compression = attrs["compression"][1][0]
    step = {0: 1, 2: 1, 3: 16}[compression]
    assert attrs["lineOrder"][1][0] == 0
    line = w * sum(2 if k == HALF else 4 for _, k in chans)
    nblocks = (h + step - 1) // step
    table = struct.unpack_from("<%dQ" % nblocks, data, at)
    out = {n: np.zeros((h, w), np.uint16 if k == HALF else np.uint32) for n, k in chans}
    end = at + 8 * nblocks
    for off in table:
        y, size = struct.unpack_from("<ii", data, off)
        rows = min(step, h - (y - y0))
        n = rows * line
        body = data[off + 8:off + 8 + size]
        assert len(body) == size
        if compression != 0 and size < n:
            p = np.frombuffer(zlib.decompress(body), np.uint8)
            assert len(p) == n
            t = (np.cumsum(p.astype(np.int64)) - 128 * np.arange(n)) & 255   # undo the deltas
            r = np.empty(n, np.uint8)
            r[0::2] = t[:(n + 1) // 2]
            r[1::2] = t[(n + 1) // 2:]
            body = r.tobytes()
        assert len(body) == n
        q = 0
        for k in range(rows):
            for name, kind in chans:
                width = 2 if kind == HALF else 4
                out[name][y - y0 + k] = np.frombuffer(body, "<u2" if kind == HALF else "<u4", w, q)
                q += w * width
        end = max(end, off + 8 + size)
    assert end == len(data)
    return out, attrs


def certificate(channels, compression):
    """what a case reaches: pieces per block, which blocks fell back to raw, the block types of their streams"""
    _, st = encode_stats(channels, compression)
    types = set()
    for parts in st["pieces"]:
        stream = b"".join(parts)
        for b in P.walk_blocks(stream[2:-4]):
            if not (b["type"] == "stored" and b["out"] == 0):   # (a full flush's empty block)
                types.add(b["type"])
    return {"blocks": len(st["blocks"]), "block_bytes": [len(b) for b in st["blocks"]],
            "pieces": [len(p) for p in st["pieces"]], "piece_tail": [len(b) % PIECE for b in st["blocks"]],
            "fell_back": st["fell_back"], "types": types, "header": st["header"]}
