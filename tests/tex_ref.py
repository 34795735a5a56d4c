"""texture() at level 0 with LINEAR filtering and REPEAT wrapping, from the specification (test infrastructure,
host only, numpy).

OpenGL ES 3.0 section 3.8.10-11 (GLSL ES 3.00 section 8.14 `texture`), for a two-dimensional texture of w x h
texels sampled at normalised (s, t) with no offset and level of detail 0:

    u' = s * w                 v' = t * h                       the unnormalised coordinates
    i0 = wrap(floor(u' - 1/2))      i1 = wrap(floor(u' - 1/2) + 1)        alpha = frac(u' - 1/2)
    j0 = wrap(floor(v' - 1/2))      j1 = wrap(floor(v' - 1/2) + 1)        beta  = frac(v' - 1/2)
    tau = (1 - alpha)(1 - beta) tau[i0, j0] + alpha (1 - beta) tau[i1, j0]
        + (1 - alpha) beta tau[i0, j1] + alpha beta tau[i1, j1]
    wrap(i) = i mod size (REPEAT; the mathematical modulus, 0 <= wrap(i) < size)
    frac(x) = x - floor(x)

An RGBA8 texel's component c is the float c / 255 (section 2.1.6.1); an RGBA32F texel's is the float stored.
The specification leaves the arithmetic's precision open. This file fixes it - every step below is one
np.float32 operation, so the bits of `sample` are defined - and carries the project's two pins, which the
specification does not decide:

    PIN 1 (non-finite coordinates): where floor(u' - 1/2) is NaN or +-inf, wrap() of it is texel 0, and
        wrap() of it plus one is texel 1 mod size. (The fraction is then NaN, and so is every component.)
    PIN 2 (the blend): tau = mix(mix(tau00, tau10, alpha), mix(tau01, tau11, alpha), beta) with
        mix(x, y, a) = x * (1 - a) + y * a, four float32 operations, none of them fused.

`sample64` evaluates the specification's sum of four weighted texels in float64 from the same texels and the
same float32 fractions; BOUND_RGBA8 / BOUND_RGBA32F bound |sample - sample64| (derivation at the constants).
"""
import numpy as np

F32 = np.float32
HALF = F32(0.5)
ONE = F32(1.0)


def _wrap(f, size):
    """wrap(f) for integer-valued float32 f (PIN 1 for the non-finite ones), exactly, as int64."""
    f = np.asarray(f, np.float32)
    out = np.zeros(f.shape, np.int64)
    fin = np.isfinite(f)
    small = fin & (np.abs(f) < F32(2.0 ** 62))
    out[small] = np.mod(f[small].astype(np.int64), np.int64(size))        # floor modulus of exact integers
    big = fin & ~small
    if big.any():                                                         # beyond int64: Python's integers
        out[big] = [int(x) % size for x in f[big].astype(np.float64).tolist()]
    return out


def coords(s, size):
    """One axis: (i0, i1, alpha) of normalised float32 coordinates `s` on `size` texels."""
    s = np.asarray(s, np.float32)
    with np.errstate(all="ignore"):
        up = s * F32(size)                       # u' (float32)
        x = up - HALF                            # u' - 1/2 (float32)
        fl = np.floor(x)
        alpha = x - fl                           # frac
    i0 = _wrap(fl, size)
    i1 = np.mod(i0 + 1, size)                    # wrap(floor + 1) == (wrap(floor) + 1) mod size, in integers
    return i0, i1, alpha.astype(np.float32)


def _texels(tex):
    """The texel components as float32: c / 255 for RGBA8, as stored for RGBA32F."""
    tex = np.asarray(tex)
    assert tex.ndim == 3 and tex.shape[2] == 4 and tex.dtype in (np.uint8, np.float32)
    if tex.dtype == np.uint8:
        return tex.astype(np.float32) / F32(255.0)
    return tex


def _mix(x, y, a):
    """PIN 2: x * (1 - a) + y * a in four float32 operations."""
    return (x * (ONE - a) + y * a).astype(np.float32)


def taps(tex, s, t):
    """The texels the specification reads: (i0, j0, i1, j1) per coordinate."""
    h, w = np.asarray(tex).shape[:2]
    i0, i1, _ = coords(s, w)
    j0, j1, _ = coords(t, h)
    return i0, j0, i1, j1


def sample(tex, s, t):
    """texture(tex, (s, t)) for a (h, w, 4) uint8 or float32 map (row 0 is t = 0): (n, 4) float32."""
    tx = _texels(tex)
    h, w = tx.shape[:2]
    i0, i1, a = coords(s, w)
    j0, j1, b = coords(t, h)
    a, b = a[:, None], b[:, None]
    with np.errstate(all="ignore"):
        return _mix(_mix(tx[j0, i0], tx[j0, i1], a), _mix(tx[j1, i0], tx[j1, i1], a), b)


def sample64(tex, s, t):
    """The specification's weighted sum of the same four texels in float64: RGBA8 components are c / 255 in
    float64, RGBA32F components the stored floats, alpha and beta the float32 fractions taken as given."""
    tex = np.asarray(tex)
    tx = tex.astype(np.float64) / 255.0 if tex.dtype == np.uint8 else tex.astype(np.float64)
    h, w = tx.shape[:2]
    i0, i1, a = coords(s, w)
    j0, j1, b = coords(t, h)
    a, b = a.astype(np.float64)[:, None], b.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        return ((1 - a) * (1 - b) * tx[j0, i0] + a * (1 - b) * tx[j0, i1]
                + (1 - a) * b * tx[j1, i0] + a * b * tx[j1, i1])


# |sample - sample64| for texel components in [0, 1] and fractions in [0, 1].
#
# Let U = 2^-25: a float32 operation whose exact result lies in [0, 1] rounds by at most U (half a unit in the
# last place of [1/2, 1); smaller results round by less). One mix(x, y, a) of x, y in [0, 1] is
#     s = fl(1 - a) = 1 - a + e1      p = fl(x s) = x s + e2      q = fl(y a) = y a + e3      r = fl(p + q) = p + q + e4
# with every |e| <= U (p + q <= s + a <= 1 + U, which rounds to at most 1, so r stays in [0, 1]), hence
#     r - (x (1 - a) + y a) = x e1 + e2 + e3 + e4,      at most 4 U.        (1 - a is exact only for a >= 1/2.)
# Inputs that carry errors of at most d add (s dx + a dy), at most d (1 + U). With RGBA8 texels each component
# is fl(c / 255), off by at most D8 = U from c / 255; RGBA32F components are exact (D32 = 0). The two inner
# mixes are then off by at most E1 = 4 U + D (1 + U), the outer one by 4 U + E1 (1 + U). The float64 side's own
# rounding (a dozen operations at 2^-53 on values in [0, 1]) is covered by 16 * 2^-53.
U = 2.0 ** -25


def _bound(d):
    e1 = 4 * U + d * (1 + U)
    return 4 * U + e1 * (1 + U) + 16 * 2.0 ** -53


BOUND_RGBA8 = _bound(U)        # 9 U and second-order terms: about 2.68e-7
BOUND_RGBA32F = _bound(0.0)    # 8 U and second-order terms: about 2.38e-7, for components in [0, 1]
