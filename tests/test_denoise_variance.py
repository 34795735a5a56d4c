"""pt_set_moment_target and pt_denoise_variance on the CPU: hand-checkable cases of the numpy references
(tests/moments_ref.py, tests/denoise_var_ref.py), the filter's quality on the oracle's own renders against the raw
accumulation and against pt_denoise, and the binding of both entry points (no device call)."""
import numpy as np
import pytest

import denoise_ref as DR
import denoise_var_ref as VR
import features_ref as FR
import helpers as H
import moments_ref as MR
from test_denoise import _flat, _noisy, _still_frames, _tm

F32 = np.float32


def _moments(hh, ww, weight, L, var=0.0):
    """Moments of `weight` samples of mean luminance L and variance var: (w L, w (L^2 + var), 0, w)."""
    m = np.zeros((hh, ww, 4), F32)
    wt = F32(weight)
    m[..., 0] = F32(L) * wt
    m[..., 1] = (F32(L) * F32(L) + F32(var)) * wt
    m[..., 3] = wt
    return m


# ------------------------------------------------------------------ the moments fold

def test_moments_fold_rule():
    """Frame 1 resets (history +0.0), a still frame adds, a moving frame halves both: the weights 1, 2, 1.5."""
    g = np.zeros((2, 3, 11), F32)
    g[..., 8:11] = (1.0, 0.5, 0.25)
    L = MR.lum(g[..., 8:11])
    assert np.all(L == F32(F32(F32(0.2126) + F32(0.7152) * F32(0.5)) + F32(0.0722) * F32(0.25)))
    m = MR.fold(np.full((2, 3, 4), np.nan, F32), g, 1.0, True)
    assert DR.same_bits(m[..., 0], L) and DR.same_bits(m[..., 1], L * L)
    assert np.all(m[..., 3] == 1.0) and np.all(m[..., 2] == 0.0) and not np.signbit(m[..., 2]).any()
    m2 = MR.fold(m, g, 2.0, False)
    assert DR.same_bits(m2[..., 0], L + L) and np.all(m2[..., 3] == 2.0)
    m3 = MR.fold(m2, g, 3.0, True)
    assert DR.same_bits(m3[..., 0], F32(0.5) * m2[..., 0] + F32(0.5) * L) and np.all(m3[..., 3] == 1.5)
    assert np.all(m3[..., 2] == 0.0)


# ------------------------------------------------------------------ hand-checkable cases of the filter

@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("weight", [1.0, 4.0, 0.5, 3.0])
def test_flat_regions_come_back_bit_for_bit(weight, iterations, demodulate):
    """tests/test_denoise.py's fixed point with zero-variance moments: var = 0 everywhere, so the luminance term is
    (0 * 0) / 1e-8 = 0, every weight is k * exp(0) = k, and the weights kept sum exactly - dst.xyz == beauty.xyz,
    and nothing bleeds across column 20 of the 33 x 17 frame, in either variance branch (weights below and at 4)."""
    b, n, a = _flat(17, 33, weight, (0.75, 0.75, 0.75), (0.5, 0.5, 0.5), 3.0)
    b2, n2, a2 = _flat(17, 33, weight, (0.25, 0.25, 0.25), (0.125, 0.125, 0.125), 7.0)
    m, m2 = _moments(17, 33, weight, 0.75), _moments(17, 33, weight, 0.25)
    for t, t2 in ((b, b2), (n, n2), (a, a2), (m, m2)):
        t[:, 20:] = t2[:, 20:]
    dst = VR.denoise(b, n, a, m, iterations, demodulate=demodulate)
    assert DR.same_bits(dst[..., :3], b[..., :3])
    assert np.all(dst[..., 3] == 1.0)
    assert np.all(VR.prep(b, n, a, m, demodulate)[6] == 0.0)
    # the one-region frame
    b, n, a = _flat(17, 33, weight, (0.75, 0.75, 0.75), (0.5, 0.5, 0.5), 3.0)
    dst = VR.denoise(b, n, a, _moments(17, 33, weight, 0.75), iterations, demodulate=demodulate)
    assert DR.same_bits(dst[..., :3], b[..., :3]) and np.all(dst[..., 3] == 1.0)


def _noisy_moments(hh, ww, weight=4.0, seed=6):
    rng = np.random.default_rng(seed)
    m = _moments(hh, ww, weight, 0.75, 0.0)
    m[..., 0] += rng.random((hh, ww), dtype=F32)
    m[..., 1] += rng.random((hh, ww), dtype=F32) * F32(4.0) + F32(2.0)   # (second moment > first squared everywhere)
    return m


@pytest.mark.parametrize("which", ["albedo_weight.w", "moments.w"])
@pytest.mark.parametrize("demodulate", [True, False])
def test_weight_zero_pixel_full_of_nan_touches_nothing_else(demodulate, which):
    """A pixel whose four inputs are NaN and whose one weight channel is 0 is invalid, and skipped as a tap in the
    7x7 sums, the 3x3 variance mean and the 5x5 kernel: no other pixel's bits move."""
    b, n, a = _noisy(17, 33)
    m = _noisy_moments(17, 33)
    hole = (8, 11)
    clean_in = [t.copy() for t in (b, n, a, m)]
    for t in clean_in:
        t[hole] = 0.0   # both weights 0, finite data
    for t in (b, n, a, m):
        t[hole] = np.nan
    (a if which == "albedo_weight.w" else m)[hole + (3,)] = 0.0
    clean = VR.denoise(*clean_in, iterations=5, demodulate=demodulate)
    dirty = VR.denoise(b, n, a, m, iterations=5, demodulate=demodulate)
    assert not np.isnan(clean).any() and (clean[..., :3] > 0).sum() > 0
    assert DR.same_bits(clean, dirty)
    assert dirty[hole].tolist() == [0.0, 0.0, 0.0, 1.0]
    # ... and it does change pixels: this is not the identity
    assert not DR.same_bits(clean[..., :3], clean_in[0][..., :3])


def test_never_folded_targets_give_an_empty_frame():
    z = np.zeros((5, 7, 4), F32)
    b = np.ones((5, 7, 4), F32)
    m = _moments(5, 7, 2.0, 0.5, 0.25)
    for nid, alb, mo in ((z, z, z), (z, z, m), (z, np.ones((5, 7, 4), F32), z)):
        dst = VR.denoise(b, nid, alb, mo, 2)
        assert np.all(dst[..., :3] == 0) and np.all(dst[..., 3] == 1) and not np.signbit(dst).any()


def test_checkerboard_of_weights_takes_both_variance_branches():
    """moments.w = 3 on the black squares (the spatial estimate) and 4 on the white ones (the temporal one): the
    two estimates differ and are finite, and the image is filtered."""
    b, n, a = _noisy(17, 33)
    m = _noisy_moments(17, 33)
    yy, xx = np.mgrid[0:17, 0:33]
    black = (yy + xx) % 2 == 0
    m[black] *= F32(0.75)   # weight 3, exactly
    assert np.all(m[black, 3] == 3.0) and np.all(m[~black, 3] == 4.0)
    var, branch = VR.prep(b, n, a, m, True)[6:8]
    assert np.array_equal(branch, black)
    assert np.isfinite(var).all() and (var[black] > 0).all() and (var[~black] > 0).all()
    all_spatial = VR.prep(b, n, a, m * F32(0.5), True)[6]   # every weight < 4: the other branch on the white squares
    assert np.isfinite(all_spatial).all()
    assert (all_spatial[~black] != var[~black] * F32(2.0)).mean() > 0.9   # (the same branch would only halve mw)
    dst = VR.denoise(b, n, a, m)
    assert np.isfinite(dst).all() and not DR.same_bits(dst[..., :3], b[..., :3])


# ------------------------------------------------------------------ quality

@pytest.mark.parametrize("name,W,Hh,count", [("cornell_256", 96, 72, 384), ("gltf_teapot_320x180", 96, 64, 384),
                                             ("quadric_256", 64, 48, 256), ("sky_256", 64, 48, 256)])
def test_variance_guided_is_closer_to_the_converged_image(name, W, Hh, count):
    """At 1, 4 and 16 accumulated samples, default parameters, RMSE of x / (1 + x) against the oracle's `count`-frame
    mean: the variance-guided filter beats the raw accumulation on every case, and pt_denoise (defaults) on every
    case but the sky scene's (about even at 16 spp: not part of the second condition). Measured (ratio to raw,
    pt_denoise | variance-guided): DESIGN.md section 6."""
    meta = H.stream(name)
    sc = H.oracle_scene(meta, W, Hh)
    acc = np.zeros((Hh, W, 4), F32)
    nid = np.zeros((Hh, W, 4), F32)
    alb = np.zeros((Hh, W, 4), F32)
    mom = np.zeros((Hh, W, 4), F32)
    at = {}
    for k, u in enumerate(_still_frames(meta, count)):
        u = H.with_resolution(u, W, Hh)
        acc, _ = sc.path_trace(u, acc)
        if k < 16:
            g = sc.gbuffer(u)
            nid, alb = FR.fold(nid, alb, g, 1.0 + k, False)
            mom = MR.fold(mom, g, 1.0 + k, False)
        if k + 1 in (1, 4, 16):
            at[k + 1] = (acc.copy(), nid, alb, mom)
    ref = _tm(acc[..., :3].astype(np.float64) / count)
    failed = []
    for spp, (b, n, a, m) in at.items():
        assert np.all(a[..., 3] == spp) and np.all(m[..., 3] == spp)

        def rmse(x):
            return np.sqrt(np.mean((_tm(x[..., :3].astype(np.float64) / spp) - ref) ** 2))

        raw, plain, guided = rmse(b), rmse(DR.denoise(b, n, a)), rmse(VR.denoise(b, n, a, m))
        print("%s %d spp: rmse raw %.5f pt_denoise %.5f (ratio %.3f) variance-guided %.5f (ratio %.3f)"
              % (name, spp, raw, plain, plain / raw, guided, guided / raw))
        if not guided / raw < 1.0:
            failed.append((spp, "raw", raw, guided))
        if name != "sky_256" and not guided < plain:
            failed.append((spp, "pt_denoise", plain, guided))
    assert not failed, (name, failed)


# ------------------------------------------------------------------ the binding

def test_binding_declares_the_entry_points():
    import babylon_pt as bp
    assert "pt_set_moment_target" in bp.SYMBOLS and "pt_denoise_variance" in bp.SYMBOLS
    L = bp.lib()
    assert len(L.pt_set_moment_target.argtypes) == 2
    assert len(L.pt_denoise_variance.argtypes) == 10
    assert L.pt_set_moment_target(None, None) == -1   # PT_ERR_ARG for no effect / no context: no device call
    assert L.pt_denoise_variance(None, None, None, None, None, None, 3, 0.5, 4.0, 1) == -1
    assert hasattr(bp.Engine, "denoise_variance") and hasattr(bp.Effect, "setMomentTarget")
