"""The images the HDR encoder's tests share (tests/test_hdr_enc_ref.py on the CPU, tests/test_gpu_hdr_encode.py on
the device): RGBA32F textures, rows bottom-up, whose RGBE byte planes are chosen. With G = 255/256 the largest
component lies in [0.5, 1), so e = 0, the E plane is 128 throughout, the G plane 255 throughout (two all-equal planes
in every row), and R = r/256, B = b/256 give exactly the bytes r and b: two planes a row to shape freely."""
import numpy as np

import hdr_enc_ref as R

RUN_LENGTHS = (3, 4, 126, 127, 128, 129, 130, 131, 254, 255, 258, 381)
LITERAL_LENGTHS = (127, 128, 129, 256, 257)
SIZES = ((1, 1), (7, 3), (32768, 1), (8, 2), (9, 1), (63, 2), (64, 2), (65, 2), (127, 1), (128, 2), (129, 2), (131, 2),
         (258, 2), (300, 5), (32767, 1), (16, 600))
SPECIALS = (np.nan, -1.0, -0.0, np.inf, 1e-33, 1e-32, 0.5, 1.0, float(R.CAP), float(np.finfo(np.float32).max))


def tex_of_planes(r, b, seed=0):
    """rows of R and B byte planes, scanline 0 first -> the texture, rows bottom-up, alpha junk"""
    r, b = np.atleast_2d(np.asarray(r, np.uint8)), np.atleast_2d(np.asarray(b, np.uint8))
    tex = np.empty(r.shape + (4,), np.float32)
    tex[..., 0] = r.astype(np.float32) / 256
    tex[..., 1] = np.float32(255 / 256)
    tex[..., 2] = b.astype(np.float32) / 256
    tex[..., 3] = np.random.default_rng(seed).standard_normal(r.shape).astype(np.float32)
    return np.ascontiguousarray(tex[::-1])


def literal(n, phase=0):
    """n bytes below 240, no two neighbours equal"""
    return ((np.arange(n) + phase) * 7 % 239).astype(np.uint8)


def plane(width, *parts):
    """parts: an int n is a run of n bytes (values 255, 254, .. 240 in turn), an array is taken as it is; the plane
    is filled up to `width` with a literal, or cut there"""
    out, v = [], 255
    for p in parts:
        if isinstance(p, (int, np.integer)):
            out.append(np.full(int(p), v, np.uint8))
            v = v - 1 if v > 240 else 255
        else:
            out.append(np.asarray(p, np.uint8))
    got = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if len(got) < width:
        got = np.concatenate((got, literal(width - len(got), 3)))
    return got[:width]


def mixed_row(width, rng):
    """random segments: runs of the lengths that matter, literals, short stretches"""
    parts = []
    n = 0
    while n < width:
        if rng.random() < 0.5:
            L = int(rng.choice((1, 2, 3, 4, 5, 8, 126, 127, 128, 130, 131)))
            parts.append(L)
        else:
            L = int(rng.choice((1, 2, 3, 5, 40, 127, 128, 129)))
            parts.append(literal(L, int(rng.integers(0, 200))))
        n += L
    return plane(width, *parts)


def sized(width, height, seed=1):
    """the size cases: rows in turn mixed, noise (every plane of a coded width at its bound), all-equal, mixed"""
    rng = np.random.default_rng(seed + width * 131 + height)
    r, b = np.empty((height, width), np.uint8), np.empty((height, width), np.uint8)
    for y in range(height):
        kind = y % 4
        if kind in (0, 3):
            r[y], b[y] = mixed_row(width, rng), mixed_row(width, rng)
        elif kind == 1:
            r[y], b[y] = literal(width, y), literal(width, y + 11)[::-1]
        else:
            r[y], b[y] = 77, 78
    return tex_of_planes(r, b, seed)


def run_rows(width=800):
    """every run length at the plane's start, in its middle and at its end; B holds them the other way round"""
    rows = []
    for L in RUN_LENGTHS:
        rows.append(plane(width, L))
        rows.append(plane(width, literal(101), L))
        rows.append(plane(width, literal(width - L), L))
    r = np.stack(rows)
    return tex_of_planes(r, r[:, ::-1])


def stretch_rows(width=400):
    """between runs: stretches of 1, 2 and 3 equal bytes, of 2 and 3 unequal ones, the remainders 1..3 of runs of
    128..130 next to short runs, and the literal lengths"""
    a, b, c = 1, 2, 3
    rows = [plane(width, 10, [a], 10, [a, a], 10, [a, a, a], 10, [a, b], 10, [a, b, c], 10, [a, a, b], 10, [a, b, b], 10,
                  128, 10, 129, 10, 130, [b], 10, 129, [a, a], 10)]
    for n in LITERAL_LENGTHS:
        rows.append(plane(width, 9, literal(n), 9))
        rows.append(plane(width, literal(n), 9))
    rows.append(plane(width, literal(width - 2), [a, a]))   # a short run that is no stretch of its own
    rows.append(plane(width, 12, literal(width - 15), 3))   # the short token at the plane's end
    r = np.stack(rows)
    return tex_of_planes(r, np.roll(r, 1, axis=0))


def straddle_rows(width=330):
    """runs of 8 across every multiple of the byte step, by every split; and rows of runs of 2 and 1 whose stretches
    cross every multiple of 64 runs"""
    rows = []
    for split in range(1, 8):
        parts, at = [], 0
        for k in range(R.STEP, width - 8, R.STEP):
            parts += [literal(k - split - at, k), 8]
            at = k - split + 8
        rows.append(plane(width, *parts))
    rows.append(plane(width, *([2, 1] * 100)))
    rows.append(plane(width, 5, *([1, 2, 1] * 80)))
    r = np.stack(rows)
    return tex_of_planes(r, r[::-1])


def specials(scale=1.0):
    """the special values in every component position, beside ordinary ones and beside each other"""
    rows = []
    for other in (0.25, None):
        row = []
        for s in SPECIALS:
            for k in range(3):
                t = [other if other is not None else s] * 3 + [1.0]
                t[k] = s
                row.append(t)
        rows.append(row)
    return np.asarray(rows, np.float32)


def lognormal(width=37, height=9, seed=5):
    rng = np.random.default_rng(seed)
    t = np.exp2(rng.uniform(-60, 60, (height, width, 4))).astype(np.float32)
    t[rng.random((height, width)) < 0.1] = 0.0
    return t


def past_the_grid(width, height):
    """cheap images of more texels than one trip of the conversion's grid takes (R.TEXELS): blocks of equal bytes
    that shift from row to row, a band of literals, a short run, and a column whose value is the row's, so that a texel
    converted into the wrong row or column shows"""
    y, x = np.mgrid[0:height, 0:width]
    r = ((x // 97 + y // 5) % 200).astype(np.uint8)
    b = ((x // 275 + y) % 251).astype(np.uint8)
    if width > 40:
        r[:, 20:36] = ((x[:, 20:36] * 7 + y[:, 20:36]) % 239).astype(np.uint8)
        r[:, 50:52] = 250   # two equal bytes between runs: the short token
    b[:, width // 2] = (y[:, 0] // 256 + 3 * (y[:, 0] % 83)).astype(np.uint8)
    return tex_of_planes(r, b, 2)


GRID_SIZES = ((1100, 960), (7, 150000))   # coded and flat, the smallest round sizes past R.TEXELS = 1,048,576


def cases():
    """name -> (texture, scale)"""
    out = {}
    for w, h in GRID_SIZES:
        out["grid-%dx%d" % (w, h)] = (past_the_grid(w, h), 1.0)
    for w, h in SIZES:
        out["size-%dx%d" % (w, h)] = (sized(w, h), 1.0)
    out["runs"] = (run_rows(), 1.0)
    out["stretches"] = (stretch_rows(), 1.0)
    out["straddle"] = (straddle_rows(), 1.0)
    out["specials"] = (specials(), 1.0)
    for name, s in (("half", 0.5), ("third", 1.0 / 3.0), ("2^-20", 2.0 ** -20)):
        out["lognormal-" + name] = (lognormal(), s)
        out["specials-" + name] = (specials(), s)
    return out
