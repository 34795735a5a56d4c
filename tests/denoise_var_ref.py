"""The reference for pt_denoise_variance (include/pt.h, INTEGRATION.md "Denoising"): the variance-guided a-trous
filter in numpy float32, in the style of tests/denoise_ref.py - one IEEE binary32 operation per product, sum and
quotient, taps in row-major order (dy outer, dx inner), exp through the oracle's pinned sequence
(ptoracle.math_probe(8, .)), a skipped tap left out with np.where, never multiplied by zero (test infrastructure).

Arrays are (h, w, 4) float32 as RenderTargetTexture.read() returns them; results are compared as uint32 views."""
import numpy as np

from denoise_ref import F32, K, _gexp, _shift, _sq3, same_bits  # noqa: F401  (same_bits: for the tests)

B = (F32(0.5), F32(0.25))


def lum(v):
    return (F32(0.2126) * v[..., 0] + F32(0.7152) * v[..., 1]) + F32(0.0722) * v[..., 2]


def _pos(v):
    """v where v > 0, else +0.0 (a NaN becomes 0)."""
    return np.where(v > 0, v, F32(0.0))


def prep(beauty, normal_id, albedo_weight, moments, demodulate):
    """(d, n, id, valid, den, w, var, branch) of every pixel; an invalid pixel has d = n = var = 0. `branch` is
    True where the spatial estimate was taken (moments.w < 4)."""
    beauty, normal_id, albedo_weight, moments = (np.asarray(t, F32) for t in (beauty, normal_id, albedo_weight, moments))
    ids = normal_id[..., 3].copy()
    with np.errstate(all="ignore"):
        w = albedo_weight[..., 3]
        mw = moments[..., 3]
        valid = (w > 0) & (mw > 0)
        iw = (F32(1.0) / w)[..., None]
        n = normal_id[..., :3] * iw
        a = albedo_weight[..., :3] * iw
        c = beauty[..., :3] * iw
        den = np.where(a < F32(1e-3), F32(1e-3), a)   # GLSL max(a, 1e-3): a NaN stays
        d = c / den if demodulate else c
        # temporal: this pixel's own moments
        mu1 = moments[..., 0] / mw
        mu2 = moments[..., 1] / mw
        vt = _pos(mu2 - mu1 * mu1)
        # spatial: the kept taps of the 7x7 window, the centre included
        mwv = np.where(valid, mw, F32(0.0))
        S1 = np.zeros_like(mw)
        S2 = np.zeros_like(mw)
        SW = np.zeros_like(mw)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                xq = _shift(moments[..., 0], dx, dy, F32(0.0))
                yq = _shift(moments[..., 1], dx, dy, F32(0.0))
                wq = _shift(mwv, dx, dy, F32(0.0))
                iq = _shift(ids, dx, dy, F32(0.0))
                ok = (wq > 0) & ~(iq != ids)
                S1 = np.where(ok, S1 + xq, S1)
                S2 = np.where(ok, S2 + yq, S2)
                SW = np.where(ok, SW + wq, SW)
        s1 = S1 / SW
        s2 = S2 / SW
        vs = _pos(s2 - s1 * s1)
        branch = mw < F32(4.0)
        var = np.where(branch, vs, vt) / mw
        if demodulate:
            l = lum(den)
            var = var / (l * l)
    v3 = valid[..., None]
    return (np.where(v3, d, F32(0.0)), np.where(v3, n, F32(0.0)), ids, valid, den, w,
            np.where(valid, var, F32(0.0)).astype(F32), branch)


def filter_pass(d, var, n, ids, valid, s, inv_n, sl2):
    """One 5x5 pass at tap spacing s: the new (d, var)."""
    h, w = d.shape[:2]
    with np.errstate(all="ignore"):
        gs = np.zeros((h, w), F32)
        gw = np.zeros((h, w), F32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq = _shift(var, dx, dy, F32(0.0))
                iq = _shift(ids, dx, dy, F32(0.0))
                ok = _shift(valid, dx, dy, False) & ~(iq != ids)
                k = B[abs(dx)] * B[abs(dy)]
                gs = np.where(ok, gs + k * vq, gs)
                gw = np.where(ok, gw + k, gw)
        gv = gs / gw
        inv_l = F32(1.0) / (sl2 * gv + F32(1e-8))
        lp = lum(d)
        sm = np.zeros((h, w, 3), F32)
        ws = np.zeros((h, w), F32)
        sv = np.zeros((h, w), F32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                dq = _shift(d, s * dx, s * dy, F32(0.0))
                vq = _shift(var, s * dx, s * dy, F32(0.0))
                nq = _shift(n, s * dx, s * dy, F32(0.0))
                iq = _shift(ids, s * dx, s * dy, F32(0.0))
                ok = _shift(valid, s * dx, s * dy, False) & ~(iq != ids)
                dl = lp - lum(dq)
                e = _sq3(n, nq) * inv_n + (dl * dl) * inv_l
                wt = (K[abs(dx)] * K[abs(dy)]) * _gexp(-e)
                sm = np.where(ok[..., None], sm + dq * wt[..., None], sm)
                ws = np.where(ok, ws + wt, ws)
                sv = np.where(ok, sv + (wt * wt) * vq, sv)
        out = sm / ws[..., None]
        vout = sv / (ws * ws)
    return np.where(valid[..., None], out, F32(0.0)).astype(F32), np.where(valid, vout, F32(0.0)).astype(F32)


def denoise(beauty, normal_id, albedo_weight, moments, iterations=3, sigma_normal=0.5, sigma_luminance=4.0,
            demodulate=True):
    """dst of pt_denoise_variance for the four input arrays."""
    assert 1 <= iterations <= 5
    sn, sl = F32(sigma_normal), F32(sigma_luminance)
    inv_n = F32(1.0) / (sn * sn)
    sl2 = sl * sl
    d, n, ids, valid, den, w, var, _ = prep(beauty, normal_id, albedo_weight, moments, demodulate)
    for i in range(iterations):
        d, var = filter_pass(d, var, n, ids, valid, 1 << i, inv_n, sl2)
    with np.errstate(all="ignore"):
        r = d * den if demodulate else d
        rgb = r * w[..., None]
    out = np.zeros(d.shape[:2] + (4,), F32)
    out[..., :3] = np.where(valid[..., None], rgb, F32(0.0))
    out[..., 3] = F32(1.0)
    return out
