"""The reference for pt_denoise (include/pt.h, INTEGRATION.md "Denoising"): the edge-avoiding a-trous filter in
numpy float32, one IEEE binary32 operation per product, sum and quotient, taps in row-major order (dy outer, dx
inner), exp through the oracle's pinned sequence (ptoracle.math_probe(8, .)). A skipped tap is left out with
np.where, never multiplied by zero: whatever it holds, NaN included, contributes nothing (test infrastructure).

Arrays are (h, w, 4) float32 as RenderTargetTexture.read() returns them; results are compared as uint32 views."""
import numpy as np

F32 = np.float32
K = (F32(0.375), F32(0.25), F32(0.0625))


def _gexp(x):
    import ptoracle as po
    return po.math_probe(8, np.ascontiguousarray(x, F32)).reshape(x.shape)


def _shift(a, ox, oy, fill):
    """out[y, x] = a[y + oy, x + ox] where that lies inside the image, `fill` elsewhere."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(h, h - oy)
    xs0, xs1 = max(0, -ox), min(w, w - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def _sq3(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def prep(beauty, normal_id, albedo_weight, demodulate):
    """(d, n, id, valid, den, w) of every pixel; an invalid pixel has d = n = 0."""
    beauty, normal_id, albedo_weight = (np.asarray(t, F32) for t in (beauty, normal_id, albedo_weight))
    with np.errstate(all="ignore"):
        w = albedo_weight[..., 3]
        valid = w > 0
        iw = (F32(1.0) / w)[..., None]
        n = normal_id[..., :3] * iw
        a = albedo_weight[..., :3] * iw
        c = beauty[..., :3] * iw
        den = np.where(a < F32(1e-3), F32(1e-3), a)   # GLSL max(a, 1e-3): a NaN stays
        d = c / den if demodulate else c
    v3 = valid[..., None]
    return np.where(v3, d, F32(0.0)), np.where(v3, n, F32(0.0)), normal_id[..., 3].copy(), valid, den, w


def filter_pass(d, n, ids, valid, s, inv_n, inv_c):
    """One 5x5 pass at tap spacing s: the new d."""
    h, w = d.shape[:2]
    sm = np.zeros((h, w, 3), F32)
    ws = np.zeros((h, w), F32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                dq = _shift(d, s * dx, s * dy, F32(0.0))
                nq = _shift(n, s * dx, s * dy, F32(0.0))
                iq = _shift(ids, s * dx, s * dy, F32(0.0))
                vq = _shift(valid, s * dx, s * dy, False)
                ok = vq & ~(iq != ids)
                e = _sq3(n, nq) * inv_n + _sq3(d, dq) * inv_c
                wt = (K[abs(dx)] * K[abs(dy)]) * _gexp(-e)
                sm = np.where(ok[..., None], sm + dq * wt[..., None], sm)
                ws = np.where(ok, ws + wt, ws)
        out = sm / ws[..., None]
    return np.where(valid[..., None], out, F32(0.0)).astype(F32)


def denoise(beauty, normal_id, albedo_weight, iterations=3, sigma_normal=0.5, sigma_colour=1.0, demodulate=True):
    """dst of pt_denoise for the three input arrays."""
    assert 1 <= iterations <= 5
    sn, sc = F32(sigma_normal), F32(sigma_colour)
    inv_n = F32(1.0) / (sn * sn)
    inv_c0 = F32(1.0) / (sc * sc)
    d, n, ids, valid, den, w = prep(beauty, normal_id, albedo_weight, demodulate)
    for i in range(iterations):
        d = filter_pass(d, n, ids, valid, 1 << i, inv_n, inv_c0 * F32(4 ** i))
    with np.errstate(all="ignore"):
        r = d * den if demodulate else d
        rgb = r * w[..., None]
    out = np.zeros(d.shape[:2] + (4,), F32)
    out[..., :3] = np.where(valid[..., None], rgb, F32(0.0))
    out[..., 3] = F32(1.0)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
