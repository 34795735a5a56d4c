"""The reference for the feature buffers (pt_set_feature_targets): the oracle's G-buffer of every draw of a
stream (ptoracle.Scene.gbuffer: columns 0-2 objectNormal, 3-5 objectColor, 6 objectID), folded in numpy
float32 by the rule of include/pt.h, frame by frame (test infrastructure).

    h = (F == 1) ? 0 : (M ? 0.5 : 1)        at F == 1 the history term is +0.0, still added
    s = (F != 1 && M) ? 0.5 : 1
    normal_id.xyz     = h*old.xyz + s*objectNormal      normal_id.w     = objectID of this draw
    albedo_weight.xyz = h*old.xyz + s*objectColor       albedo_weight.w = h*old.w + s*1.0

One float32 multiply per product and one add per component; results are compared as uint32 views."""
import numpy as np

import helpers as H

F32 = np.float32


def fold(normal_id, albedo_weight, g, frame, moving):
    """One draw's G-buffer `g` (h, w, >= 7) folded into the two (h, w, 4) float32 targets: new arrays."""
    g = np.asarray(g, F32)
    reset = float(frame) == 1.0
    s = F32(0.5) if (not reset and moving) else F32(1.0)

    def hist(old):
        return np.zeros_like(old) if reset else s * old   # (h == s whenever the history counts)

    n, a = np.empty_like(normal_id), np.empty_like(albedo_weight)
    n[..., :3] = hist(normal_id[..., :3]) + s * g[..., 0:3]
    n[..., 3] = g[..., 6]
    a[..., :3] = hist(albedo_weight[..., :3]) + s * g[..., 3:6]
    a[..., 3] = hist(albedo_weight[..., 3]) + s * F32(1.0)
    return n, a


def frame_state(frame):
    """(uFrameCounter, uCameraIsMoving) of a frame's path-tracing call."""
    u = H.path_call(frame)["uniforms"]
    return u["uFrameCounter"][1][0], int(u["uCameraIsMoving"][1][0]) != 0


_GBUF = {}


def gbuffers(key, meta, frames, W, Hh, mesh=None, maps=None):
    """The oracle's G-buffer of every frame of `frames` at W x H, computed once per `key`."""
    k = (key, len(frames), W, Hh)
    if k not in _GBUF:
        sc = H.oracle_scene(meta, W, Hh, mesh, maps)
        _GBUF[k] = [sc.gbuffer(H.with_resolution(H.path_call(f)["uniforms"], W, Hh)) for f in frames]
        for g in _GBUF[k]:
            g.setflags(write=False)
    return _GBUF[k]


def accumulate(frames, gbufs, indices, normal_id=None, albedo_weight=None, keep=()):
    """Fold the frames `indices` (in order) from the given targets (zero when None): the last pair, and
    {i: pair} after each frame of `keep`."""
    h, w = gbufs[0].shape[:2]
    n = np.zeros((h, w, 4), F32) if normal_id is None else normal_id
    a = np.zeros((h, w, 4), F32) if albedo_weight is None else albedo_weight
    kept = {}
    for i in indices:
        fc, moving = frame_state(frames[i])
        n, a = fold(n, a, gbufs[i], fc, moving)
        if i in keep:
            kept[i] = (n, a)
    return (n, a), kept


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
