"""numpy restatement of pt_canvas_encode_jpeg_opt (include/pt.h) with optimize = 1: the file of
tests/jpeg_enc_sub_ref.py coded with Huffman tables made for its own coefficients, as libjpeg-turbo writes it for the
same pixels, quality and subsampling with optimize_coding and restart_marker_rows=1 (tests/test_jpeg_encode_opt.py
pins that against Pillow). The coefficients are jpeg_enc_sub_ref's, the bit writer and the header's other segments
jpeg_enc_ref's; only the entropy code changes, so a decoder reconstructs the same pixels.

What differs from the standard tables, stage by stage:
  statistics  four histograms of 257 counters, DC 0, AC 0, DC 1, AC 1 (Y tables 0; Cb and Cr share tables 1), of
              exactly the symbols the emitter writes (libjpeg's htest_one_block): the DC category of the difference
              against the predecessor (0 at the start of every MCU row), per non-zero AC run >> 4 ZRLs (0xF0) and one
              (run & 15) << 4 | size, an EOB (0x00) when the last coefficient is zero. Dummy Y blocks count.
  tables      jpeg_gen_optimal_table per histogram (gen_optimal_table below).
  codes       canonical (Annex C) from bits / huffval.
  header      the same segments in the same order; each DHT carries its own bits[16] and huffval, so the header's
              length varies with the pixels.

encode_stats(rgb, quality, subsampling) takes top-down uint8 [H, W, 3] and returns the file and {"zrl", "stuffed",
"dummy", "limited", "tables", "lane_bits"}: `limited` how many of the four tables had a raw code length past 16,
`tables` the four (bits, huffval) in the header's order, `lane_bits` the most bits one coefficient contributes (its
ZRLs, code and value), which the device's lanes must carry."""
import numpy as np

import jpeg_enc_ref as R
import jpeg_enc_sub_ref as S

MAX_CLEN = 32


def block_symbols(blk, pred):
    """the Huffman symbols of one block in coded order: (DC category, [AC symbols])"""
    n = int(abs(blk[0] - pred)).bit_length()
    syms, run = [], 0
    for v in blk[1:]:
        if v == 0:
            run += 1
            continue
        syms += [0xF0] * (run >> 4)
        syms.append((run & 15) << 4 | int(abs(v)).bit_length())
        run = 0
    if run:
        syms.append(0x00)
    return n, syms


def gather(rows):
    """the four histograms [257] (DC 0, AC 0, DC 1, AC 1) of the rows of jpeg_enc_sub_ref.mcu_rows"""
    hist = np.zeros((4, 257), np.int64)
    for row in rows:
        pred = [0, 0, 0]
        for c, blk in row:
            t = min(c, 1)
            n, syms = block_symbols(blk, pred[c])
            pred[c] = blk[0]
            hist[2 * t, n] += 1
            for s in syms:
                hist[2 * t + 1, s] += 1
    return hist


def code_sizes(freq):
    """the merge loop of jpeg_gen_optimal_table: every symbol's raw code length [257] (0: the symbol does not occur)"""
    freq = [int(f) for f in freq]
    assert len(freq) == 257
    freq[256] = 1                     # the reserved symbol: no real one gets the all-ones code
    size = [0] * 257
    others = [-1] * 257
    while True:
        # the least non-zero count, the largest index on a tie (libjpeg scans upwards with <=); then the same
        # among the rest
        c1 = c2 = -1
        v = 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        v = 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    return size


def limit_lengths(size):
    """bits[0..32] from the raw code lengths, limited to 16 in libjpeg's order, the reserved code removed; and
    whether the limiting loop ran"""
    bits = [0] * (MAX_CLEN + 1)
    for s in size:
        if s:
            assert s <= MAX_CLEN
            bits[s] += 1
    limited = any(bits[17:])
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    return bits, limited


def gen_optimal_table(freq):
    """(bits[16] for lengths 1..16, huffval, limited)"""
    size = code_sizes(freq)
    bits, limited = limit_lengths(size)
    assert not any(bits[17:]) and bits[0] == 0
    vals = [j for i in range(1, MAX_CLEN + 1) for j in range(256) if size[j] == i]
    assert len(vals) == sum(bits)
    return bits[1:17], vals, limited


def header(width, height, quality, subsampling, tables):
    """SOI .. SOS with the four DHT segments carrying `tables` = [(bits, huffval)] for DC 0, AC 0, DC 1, AC 1"""
    std = S.header(width, height, quality, subsampling)
    first = std.index(b"\xff\xc4")
    dri = std.index(b"\xff\xdd\x00\x04")
    out = std[:first]
    for (bits, vals), tc_th in zip(tables, (0x00, 0x10, 0x01, 0x11)):
        out += R._seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + std[dri:]


def _encode_row(row, tabs, stats):
    bw = R._Bits()
    pred = [0, 0, 0]
    for c, blk in row:
        t = min(c, 1)
        dc, ac = tabs[2 * t], tabs[2 * t + 1]
        d = blk[0] - pred[c]
        n, syms = block_symbols(blk, pred[c])
        pred[c] = blk[0]
        bw.put(*dc[n])
        if n:
            bw.put(R._nbits_val(d)[1], n)
        values = [v for v in blk[1:] if v]
        lane = 0
        for s in syms:
            bw.put(*ac[s])
            lane += ac[s][1]
            if s == 0xF0:
                stats["zrl"] += 1
            elif s:
                n, bits = R._nbits_val(values.pop(0))
                bw.put(bits, n)
                stats["lane_bits"] = max(stats["lane_bits"], lane + n)
                lane = 0
    bw.flush()
    return bytes(bw.out)


def encode_stats(rgb, quality, subsampling=0):
    rgb = np.ascontiguousarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and 1 <= quality <= 100
    assert subsampling in S.SAMPLING
    h, w = rgb.shape[:2]
    stats = {"zrl": 0, "stuffed": 0, "dummy": 0, "limited": 0, "lane_bits": 0}
    rows = S.mcu_rows(rgb, quality, subsampling, stats)
    tables = []
    for freq in gather(rows):
        bits, vals, limited = gen_optimal_table(freq)
        stats["limited"] += limited
        tables.append((bits, vals))
    stats["tables"] = tables
    tabs = [R._huff(bits, vals) for bits, vals in tables]
    out = bytearray(header(w, h, quality, subsampling, tables))
    for r, row in enumerate(rows):
        raw = _encode_row(row, tabs, stats)
        stats["stuffed"] += raw.count(0xFF)
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < len(rows) else bytes([0xFF, 0xD9])
    return bytes(out), stats


def encode(rgb, quality, subsampling=0):
    return encode_stats(rgb, quality, subsampling)[0]


# ---- frames the CPU and GPU tests share ----

def graded_noise(w, h, seed, power=1.0, lo=0.0, top=128.0, grey=False):
    """Gaussian noise whose amplitude rises block by block in raster order from `lo` to `top`: every zero run and
    size occurs, with counts from one to thousands, so the tables are deep (rare symbols get codes of 14 to 16 bits)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    bw, bh = -(-w // 8), -(-h // 8)
    t = ((xx // 8) + (yy // 8) * bw) / float(bw * bh)
    amp = lo + (top - lo) * t ** power
    px = 128 + rng.normal(0, 1, (h, w, 1 if grey else 3)) * amp[..., None]
    return np.rint(np.clip(np.broadcast_to(px, (h, w, 3)), 0, 255)).astype(np.uint8)


def lone_coefficient_63(size=256, seed=1):
    """grey graded noise (4 .. 128) with the first block holding only its DC and zigzag coefficient 63: that lane
    follows a run of 62 zeros, three ZRLs and the symbol 0xE0 | size, all of them rare. At 256 x 256, seed 1 and
    quality 95 the Y AC table's raw lengths pass 16 (the limiting loop runs), ZRL gets a 16-bit code and the lane's
    share is 70 bits (found by a search over size, quality, the noise's range and seed; quality 100 leaves rounding
    noise in the block's other coefficients, so no run of 62)."""
    rgb = graded_noise(size, size, seed, 1.0, 4.0, 128.0, grey=True)
    yy, xx = np.mgrid[0:8, 0:8]
    tile = 128 + 120 * np.cos((2 * xx + 1) * 7 * np.pi / 16) * np.cos((2 * yy + 1) * 7 * np.pi / 16)
    rgb[:8, :8] = np.rint(tile).astype(np.uint8)[..., None]
    return rgb
