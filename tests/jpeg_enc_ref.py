"""numpy restatement of pt_canvas_encode_jpeg (include/pt.h): a baseline sequential JFIF file, 8-bit, three
components, 4:4:4, the Annex K tables, one restart interval per row of 8x8 MCUs. Integer arithmetic throughout,
so the bytes are exact: they are what libjpeg-turbo writes for the same pixels, quality, subsampling=0 and
restart_marker_rows=1 (tests/test_jpeg_encode.py pins that against Pillow).

encode(rgb, quality) takes top-down uint8 [H, W, 3] and returns the file; encode_stats returns it with the
number of ZRL codes and stuffed 0x00 bytes it emitted, for tests that must know a case reached those paths."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

QBASE = (
    np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]),
    np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32),
)

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
)


def _huff(bits, vals):
    """symbol -> (code, length), the canonical codes of Annex C"""
    tab, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return tab


DC_TAB = tuple(_huff(DC_BITS[i], DC_VALS[i]) for i in range(2))
AC_TAB = tuple(_huff(AC_BITS[i], AC_VALS[i]) for i in range(2))


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * s + 50) // 100, 1, 255).astype(np.int64) for b in QBASE)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.168735892) * r - _fix(.331264108) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.418687589) * g - _fix(.081312411) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's one pass over the last axis of d [..., 8] (int64); `first`: the row pass"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct(blocks):
    """blocks [..., 8, 8] of sample - 128 (int64) -> coefficients, scaled by 8 as jfdctint leaves them"""
    rows = _fdct_1d(blocks, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table):
    """coef [..., 64] natural order, table [64] natural order"""
    t8 = table * 8
    a = np.abs(coef) + (t8 >> 1)
    a = np.where(a >= t8, a // t8, 0)
    return np.where(coef < 0, -a, a)


def blocks_zigzag(rgb, quality):
    """quantised coefficients [mcu_rows, mcus_per_row, 3, 64] in zigzag order"""
    h, w = rgb.shape[:2]
    hp, wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    planes = [np.pad(p, ((0, hp - h), (0, wp - w)), mode="edge") for p in ycc(rgb)]
    qt = quant_tables(quality)
    out = np.empty((hp // 8, wp // 8, 3, 64), np.int64)
    for c, p in enumerate(planes):
        b = (p - 128).reshape(hp // 8, 8, wp // 8, 8).swapaxes(1, 2)
        q = quantise(fdct(b).reshape(hp // 8, wp // 8, 64), qt[min(c, 1)])
        out[:, :, c] = q[..., ZIGZAG]
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _nbits_val(v):
    n = int(abs(v)).bit_length()
    return n, (v - 1 if v < 0 else v) & ((1 << n) - 1)


def _encode_row(blocks, stats):
    """blocks [mcus, 3, 64] -> the row's entropy-coded bytes before stuffing"""
    bw = _Bits()
    pred = [0, 0, 0]
    for mcu in blocks.tolist():
        for c, blk in enumerate(mcu):
            t = min(c, 1)
            n, bits = _nbits_val(blk[0] - pred[c])
            pred[c] = blk[0]
            bw.put(*DC_TAB[t][n])
            if n:
                bw.put(bits, n)
            run = 0
            ac = AC_TAB[t]
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bw.put(*ac[0xF0])
                    stats["zrl"] += 1
                    run -= 16
                n, bits = _nbits_val(v)
                bw.put(*ac[(run << 4) | n])
                bw.put(bits, n)
                run = 0
            if run:
                bw.put(*ac[0x00])
    bw.flush()
    return bytes(bw.out)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(width, height, quality):
    """SOI .. SOS: everything before the first entropy-coded byte"""
    qt = quant_tables(quality)
    mcus = (width + 7) // 8
    out = bytes([0xFF, 0xD8])
    out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(qt[i][ZIGZAG].astype(np.uint8).tolist()))
    out += _seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big")
                + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for i in range(2):
        out += _seg(0xC4, bytes([0x00 | i]) + bytes(DC_BITS[i]) + bytes(DC_VALS[i]))
        out += _seg(0xC4, bytes([0x10 | i]) + bytes(AC_BITS[i]) + bytes(AC_VALS[i]))
    out += _seg(0xDD, mcus.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode_stats(rgb, quality):
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and 1 <= quality <= 100
    h, w = rgb.shape[:2]
    blocks = blocks_zigzag(rgb, quality)
    stats = {"zrl": 0, "stuffed": 0}
    out = bytearray(header(w, h, quality))
    rows = blocks.shape[0]
    for r in range(rows):
        raw = _encode_row(blocks[r], stats)
        stats["stuffed"] += raw.count(0xFF)
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < rows else bytes([0xFF, 0xD9])
    return bytes(out), stats


def encode(rgb, quality):
    return encode_stats(rgb, quality)[0]
