"""numpy restatement of pt_canvas_encode_jpeg_sub (include/pt.h): the file of tests/jpeg_enc_ref.py with Y sampled
hs x vs against Cb and Cr, 2x1 for 4:2:2 (subsampling 1) and 2x2 for 4:2:0 (subsampling 2), as libjpeg-turbo writes
it for the same pixels, quality, subsampling and restart_marker_rows=1 (tests/test_jpeg_encode_sub.py pins that
against Pillow). The tables, the FDCT, the quantiser, the bit writer and the colour conversion are jpeg_enc_ref's.

What differs from 4:4:4, stage by stage:
  header      SOF0's Y sampling byte is hs << 4 | vs, DRI holds ceil(W / (8 hs)) MCUs.
  MCU         8 hs x 8 vs pixels; its blocks are the vs rows of hs Y blocks, then Cb, then Cr. One restart interval
              per MCU row; every component's DC prediction runs over its blocks in coded order from 0.
  chroma      converted per pixel, then downsampled as integers: sample (cx, cy) reads the columns min(2cx, W-1) and
              min(2cx+1, W-1) of the rows 2cy' and min(2cy'+1, H-1) (4:2:0; 4:2:2: row cy'), cy' = min(cy,
              ceil(H / vs) - 1), and is (sum + bias) >> 2 with bias 1 + (cx & 1), for 4:2:2 (sum + (cx & 1)) >> 1.
  dummy       a Y block outside the ceil(W / 8) x ceil(H / 8) real ones has 63 zero ACs and the quantised DC of the
              block before it in the MCU (which may be a dummy too).

encode_stats(rgb, quality, subsampling) takes top-down uint8 [H, W, 3] and returns the file and {"zrl", "stuffed",
"dummy"}: the ZRL codes, stuffed 0x00 bytes and dummy blocks it emitted."""
import numpy as np

import jpeg_enc_ref as R

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}     # Pillow's numbering -> Y's (hs, vs)


def _ceil(a, b):
    return -(-a // b)


def header(width, height, quality, subsampling):
    hs, vs = SAMPLING[subsampling]
    out = bytearray(R.header(width, height, quality))
    sof = out.index(b"\xff\xc0")
    assert out[sof + 10:sof + 13] == bytes([1, 0x11, 0])
    out[sof + 11] = hs << 4 | vs
    dri = out.index(b"\xff\xdd\x00\x04")
    out[dri + 4:dri + 6] = _ceil(width, 8 * hs).to_bytes(2, "big")
    return bytes(out)


def chroma_plane(p, hs, vs, cw, ch):
    """the full-resolution plane p [H, W] (int64) downsampled to [ch, cw] samples"""
    h, w = p.shape
    cx = np.arange(cw)
    cy = np.minimum(np.arange(ch), _ceil(h, vs) - 1)
    x0, x1 = np.minimum(hs * cx, w - 1), np.minimum(hs * cx + hs - 1, w - 1)
    if (hs, vs) == (2, 2):
        y0, y1 = 2 * cy, np.minimum(2 * cy + 1, h - 1)
        s = p[y0][:, x0] + p[y0][:, x1] + p[y1][:, x0] + p[y1][:, x1]
        return (s + (1 + (cx & 1))[None, :]) >> 2
    if (hs, vs) == (2, 1):
        return (p[cy][:, x0] + p[cy][:, x1] + (cx & 1)[None, :]) >> 1
    return p[cy][:, x0]


def _quantised(plane, table):
    """plane [8 a, 8 b] -> quantised coefficients [a, b, 64] in zigzag order"""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    blk = (plane - 128).reshape(a, 8, b, 8).swapaxes(1, 2)
    return R.quantise(R.fdct(blk).reshape(a, b, 64), table)[..., R.ZIGZAG]


def mcu_rows(rgb, quality, subsampling, stats):
    """per MCU row, the list of (component, coefficients [64]) in coded order"""
    hs, vs = SAMPLING[subsampling]
    h, w = rgb.shape[:2]
    mx, my = _ceil(w, 8 * hs), _ceil(h, 8 * vs)
    y, cb, cr = R.ycc(rgb)
    qt = R.quant_tables(quality)
    yq = _quantised(np.pad(y, ((0, my * 8 * vs - h), (0, mx * 8 * hs - w)), mode="edge"), qt[0])
    cq = [_quantised(chroma_plane(p, hs, vs, mx * 8, my * 8), qt[1]) for p in (cb, cr)]
    wb, hb = _ceil(w, 8), _ceil(h, 8)
    rows = []
    for r in range(my):
        row = []
        for m in range(mx):
            last = None
            for j in range(hs * vs):
                bx, by = m * hs + j % hs, r * vs + j // hs
                if bx < wb and by < hb:
                    blk = yq[by, bx].tolist()
                else:
                    blk = [last[0]] + [0] * 63
                    stats["dummy"] += 1
                row.append((0, blk))
                last = blk
            row.append((1, cq[0][r, m].tolist()))
            row.append((2, cq[1][r, m].tolist()))
        rows.append(row)
    return rows


def _encode_row(row, stats):
    bw = R._Bits()
    pred = [0, 0, 0]
    for c, blk in row:
        t = min(c, 1)
        n, bits = R._nbits_val(blk[0] - pred[c])
        pred[c] = blk[0]
        bw.put(*R.DC_TAB[t][n])
        if n:
            bw.put(bits, n)
        run = 0
        ac = R.AC_TAB[t]
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bw.put(*ac[0xF0])
                stats["zrl"] += 1
                run -= 16
            n, bits = R._nbits_val(v)
            bw.put(*ac[(run << 4) | n])
            bw.put(bits, n)
            run = 0
        if run:
            bw.put(*ac[0x00])
    bw.flush()
    return bytes(bw.out)


def encode_stats(rgb, quality, subsampling):
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and 1 <= quality <= 100
    assert subsampling in SAMPLING
    h, w = rgb.shape[:2]
    stats = {"zrl": 0, "stuffed": 0, "dummy": 0}
    rows = mcu_rows(rgb, quality, subsampling, stats)
    out = bytearray(header(w, h, quality, subsampling))
    for r, row in enumerate(rows):
        raw = _encode_row(row, stats)
        stats["stuffed"] += raw.count(0xFF)
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < len(rows) else bytes([0xFF, 0xD9])
    return bytes(out), stats


def encode(rgb, quality, subsampling):
    return encode_stats(rgb, quality, subsampling)[0]
