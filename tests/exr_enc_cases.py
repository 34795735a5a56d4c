"""The images of the EXR encoder's tests: W x H, channels and content the smallest at which each stage of
pt_targets_encode_exr can go wrong. A case is (textures, specs, compression): textures a list of (H, W, 4) float32
arrays with rows bottom-up, specs a list of (name, texture index, component, scale, type) in the caller's order.
channels(case) is what exr_enc_ref takes. test_exr_enc_ref.py asserts from the reference's certificate that each case
still reaches what it is for."""
import numpy as np

import exr_enc_ref as R

HALF, FLOAT, NONE, ZIPS, ZIP = R.HALF, R.FLOAT, R.NONE, R.ZIPS, R.ZIP
SCAN_TILE = 256      # blocks of scanlines pt_exr_scan takes per trip of its loop: the only bounded loop of the kernels
                     # (every grid is exact: a lane per texel and per word, a block per piece)


def bits(values):
    return np.array(values, np.uint32).view(np.float32)


# NaNs of both signs and several payloads (quiet and signalling), denormals, zeros, infinities, and floats around
# the ends of the half range
SPECIAL = bits([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF,
                0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00000000, 0x80000000,
                0x7F800000, 0xFF800000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0xC77FF000, 0x7149F2CA,
                0x33000000, 0x33000001, 0xB3000001, 0x33800000, 0x38800000, 0x387FFFFF, 0x387FF000,
                0x3EAAAAAB, 0x3F800000, 0xBF800000, 0x40490FDB, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF])


def half_table():
    """for every positive half below inf: itself, the midpoint to the next half and that midpoint's two float
    neighbours; the ends of the range; all of it negated; NaNs. 512 x 512 floats."""
    h = np.arange(0x7C00, dtype=np.uint16)
    v = h.view(np.float16).astype(np.float32)
    nxt = np.append(v[1:], np.float32(65536.0))      # (past 65504 the next half would be 2^16)
    mid = ((v.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (v.astype(np.float64) + nxt.astype(np.float64)) / 2)
    lo, hi = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    extra = np.array([65519.996, 65520.0, 1e30, np.inf, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                      1e-45, 0.0], np.float32)
    pos = np.concatenate([v, mid, lo, hi, extra])
    nans = bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFFA00000])
    flat = np.concatenate([pos, -pos, nans])
    out = np.zeros(512 * 512, np.float32)
    out[:len(flat)] = flat
    return out.reshape(512, 512), len(flat)


def _tex(h, w, fill):
    t = np.zeros((h, w, 4), np.float32)
    t[...] = fill
    return t


def ramp(h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    t = np.zeros((h, w, 4), np.float32)
    t[..., 0] = x * np.float32(0.25) - np.float32(seed)
    t[..., 1] = y * np.float32(3.0) + x
    t[..., 2] = (x + y) * np.float32(-0.001)
    t[..., 3] = x * y
    return t


def noise(h, w, seed):
    """uniform random float bits"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)


def special(h, w, shift=0):
    n = h * w * 4
    return np.resize(np.roll(SPECIAL, shift), n).reshape(h, w, 4).copy()


RGB_HALF = [("R", 0, 0, 1.0, HALF), ("G", 0, 1, 1.0, HALF), ("B", 0, 2, 1.0, HALF)]


def cases():
    c = {}
    # sizes: H below, at and past the 16 scanlines of a ZIP block, a short last block
    c["zip-1x1"] = ([ramp(1, 1, 5)], [("R", 0, 0, 1.0, FLOAT)], ZIP)
    c["zip-2x1"] = ([ramp(1, 2, 5)], RGB_HALF, ZIP)
    for h in (1, 15, 16, 17, 33):
        c["zip-3x%d" % h] = ([ramp(h, 3)], RGB_HALF, ZIP)
    c["zips-3x17"] = ([ramp(17, 3)], RGB_HALF, ZIPS)
    c["none-3x17"] = ([ramp(17, 3)], RGB_HALF, NONE)
    c["none-1x1"] = ([ramp(1, 1, 5)], [("R", 0, 0, 1.0, HALF)], NONE)
    # pieces: a block of exactly one piece, a second piece of 32 and of 4 bytes, five pieces and a shorter last block
    c["piece-510"] = ([ramp(16, 510)], [("Y", 0, 1, 1.0, HALF)], ZIP)
    c["piece-511"] = ([ramp(16, 511)], [("Y", 0, 1, 1.0, HALF)], ZIP)
    c["piece-4080"] = ([ramp(2, 4080)], [("Y", 0, 1, 1.0, FLOAT)], ZIPS)
    c["piece-4081"] = ([ramp(2, 4081)], [("Y", 0, 1, 1.0, FLOAT)], ZIPS)
    c["pieces-5"] = ([ramp(20, 600)], [("u", 0, 0, 1.0, FLOAT), ("v", 0, 3, 1.0, FLOAT)], ZIP)
    # more blocks than one trip of the scan's loop, and more pieces than blocks
    c["scan-5x300"] = ([ramp(300, 5)], RGB_HALF, ZIPS)
    c["scan-2100x260"] = ([_tex(260, 2100, (0.5, 0.25, 1.0, 7.0))], [("a", 0, 0, 1.0, FLOAT), ("b", 0, 3, 1.0, FLOAT)], ZIPS)
    # content: constant planes (runs across pieces and across the even / odd halves), noise (every block raw), a mix
    c["const-zip"] = ([_tex(32, 600, (0.5, -2.0, 0.0, 3.0))], RGB_HALF + [("A", 0, 3, 1.0, FLOAT)], ZIP)
    c["noise-zips"] = ([noise(3, 200, 1)], [("R", 0, 0, 1.0, FLOAT)], ZIPS)
    c["noise-zip"] = ([noise(16, 200, 2)], [("R", 0, 0, 1.0, FLOAT)], ZIP)
    mixed = noise(8, 250, 3)
    mixed[0::2, :, 1] = np.float32(0.75)
    mixed[0::2, :, 2] = ramp(4, 250)[..., 0]
    # (the other rows: noise in the HALF channels too, as random finite halves)
    mixed[1::2, :, 1:3] = np.random.default_rng(4).integers(0, 0x7C00, (4, 250, 2)).astype(np.uint16).view(np.float16)
    c["mixed-zips"] = ([mixed], [("n", 0, 0, 1.0, FLOAT), ("c", 0, 1, 1.0, HALF), ("r", 0, 2, 1.0, HALF)], ZIPS)
    # channels: names out of order, uppercase before lowercase, two channels of one texture, four textures, 16 channels
    c["names"] = ([ramp(5, 7), ramp(5, 7, 3)],
                  [("id", 1, 3, 1.0, FLOAT), ("B", 0, 2, 1.0, HALF), ("normal.X", 1, 0, 1.0, HALF), ("G", 0, 1, 1.0, HALF),
                   ("R", 0, 0, 1.0, HALF), ("A", 0, 3, 1.0, HALF), ("Z", 1, 1, 1.0, FLOAT), ("a", 1, 2, 1.0, HALF)], ZIP)
    texs = [ramp(18, 9, k) for k in range(4)]
    names16 = ["n%02d.%s" % (15 - i, "xyzw"[i % 4]) for i in range(16)]
    c["chan-16"] = (texs, [(names16[i], i % 4, (i // 4 + i) % 4, 1.0, HALF if i % 3 else FLOAT) for i in range(16)], ZIP)
    c["chan-16-none"] = (texs, c["chan-16"][1], NONE)
    # scales: 1 keeps NaN payloads and denormals (FLOAT) or canonicalises and flushes them (HALF); others multiply
    sp = special(6, 35)
    for name, s in (("scale-1", 1.0), ("scale-half", 0.5), ("scale-neg", -2.0), ("scale-third", 1.0 / 3.0)):
        c[name] = ([sp, special(6, 35, 3)], [("f", 0, 0, s, FLOAT), ("h", 0, 1, s, HALF), ("g", 1, 2, s, FLOAT),
                                             ("k", 1, 3, s, HALF), ("one", 0, 3, 1.0, HALF)], ZIPS)
    table, _ = half_table()
    t = np.zeros((512, 512, 4), np.float32)
    t[..., 0] = table
    t[..., 1] = table[::-1]
    c["half-table"] = ([t], [("h", 0, 0, 1.0, HALF), ("f", 0, 1, 1.0, FLOAT)], ZIP)
    return c


def channels(case):
    texs, specs, _ = case
    return [(name, texs[k], comp, scale, kind) for name, k, comp, scale, kind in specs]
