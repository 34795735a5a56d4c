"""The reference for the moments target (pt_set_moment_target): the oracle's radiance of every draw of a stream
(ptoracle.Scene.gbuffer, columns 8-10: CalculateRadiance's result before the history rule), folded in numpy
float32 by the rule of include/pt.h, frame by frame (test infrastructure).

    h, s as in tests/features_ref.py
    L = (0.2126*r.x + 0.7152*r.y) + 0.0722*r.z
    moments.x = h*old.x + s*L      moments.y = h*old.y + s*(L*L)      moments.z = +0.0      moments.w = h*old.w + s

One float32 operation per product and sum; results are compared as uint32 views."""
import numpy as np

import features_ref as FR

F32 = np.float32


def lum(v):
    return (F32(0.2126) * v[..., 0] + F32(0.7152) * v[..., 1]) + F32(0.0722) * v[..., 2]


def fold(moments, g, frame, moving):
    """One draw's G-buffer dump `g` (h, w, >= 11) folded into the (h, w, 4) float32 target: a new array."""
    g = np.asarray(g, F32)
    reset = float(frame) == 1.0
    s = F32(0.5) if (not reset and moving) else F32(1.0)

    def hist(old):
        return np.zeros_like(old) if reset else s * old

    L = lum(g[..., 8:11])
    m = np.empty_like(moments)
    m[..., 0] = hist(moments[..., 0]) + s * L
    m[..., 1] = hist(moments[..., 1]) + s * (L * L)
    m[..., 2] = F32(0.0)
    m[..., 3] = hist(moments[..., 3]) + s * F32(1.0)
    return m


def accumulate(frames, gbufs, indices, moments=None, keep=()):
    """Fold the frames `indices` (in order) from `moments` (zero when None): the last target, and {i: target}
    after each frame of `keep`."""
    h, w = gbufs[0].shape[:2]
    m = np.zeros((h, w, 4), F32) if moments is None else moments
    kept = {}
    for i in indices:
        fc, moving = FR.frame_state(frames[i])
        m = fold(m, gbufs[i], fc, moving)
        if i in keep:
            kept[i] = m
    return m, kept
