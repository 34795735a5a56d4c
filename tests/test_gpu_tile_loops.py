"""The device loops that no other test enters, bit for bit (uint32) against the references the suite already has.

1. pt_denoise_pass<S,LAST> and pt_dvar_pass<S,LAST> beyond one tile per block: launch_pass / launch_dvar_pass start
   min(ntiles, clamp(ntiles / 4, 4096, 8192)) blocks, so the loop behind the first tile (the next tile's registers
   stored into the one LDS buffer between two barriers) runs only for images of more than 4096 tiles. Thin images
   reach every regime of that formula with few pixels; one image has full-height tiles.
2. One engine denoising several sizes: the slabs' planes lie at the slab's capacity, not the call's pixel count,
   and a slab grows right behind queued calls.
3. pt_blend_w, pt_feature_fold<MOM> and pt_output_w given fewer workgroups than units (PT_MAIN_WAVES below the
   unit count): their grid-stride loops, pt_output_w's two LDS buffers handed over many times.

Seeded inputs written with pt_write_pixels against tests/denoise_ref.py and tests/denoise_var_ref.py (1, 2); the
oracle's replay and the folds of tests/features_ref.py and tests/moments_ref.py (3). No tolerance anywhere.

Run on an MI355X: python -m pytest tests/test_gpu_tile_loops.py -m gpu
"""
import os
import re

import numpy as np
import pytest

import denoise_ref as DR
import denoise_var_ref as VR
import features_ref as FR
import helpers as H
import moments_ref as MR
from test_gpu_compaction import _bits_equal, _diff_report, _issue, _player
from test_gpu_denoise_variance import _seeded

pytestmark = pytest.mark.gpu

F32 = np.float32
CSRC = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "csrc")


# ------------------------------------------------------------------ seeded inputs for thin images

def _seeded_stripes(hh, ww, seed):
    """test_gpu_denoise_variance's _seeded for images a few rows high, where its blocks of ids and its row of
    albedo under the floor (placed by y and the height) would be the whole image: ids that change every 37 columns
    (tiles straddle the borders; on a high image every 29 rows as well), a stripe of albedo below the 1e-3 floor 5
    columns wide every 211, and the huge and the clamped second moments on diagonals, so that a single row has them
    as often as an area. The rest is _seeded's: the checkerboard of weights 3 and 4, zero-variance pixels, and
    NaN-filled pixels whose albedo_weight.w or whose moments.w alone is 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hh, 0:ww]
    wt = np.where((yy + xx) % 2 == 0, F32(3.0), F32(4.0)).astype(F32)
    b = np.zeros((hh, ww, 4), F32)
    n = np.zeros((hh, ww, 4), F32)
    a = np.zeros((hh, ww, 4), F32)
    m = np.zeros((hh, ww, 4), F32)
    b[..., :3] = (rng.random((hh, ww, 3), dtype=F32) + F32(0.25)) * wt[..., None]
    b[..., 3] = 1.0
    nrm = rng.random((hh, ww, 3), dtype=F32) - F32(0.5)
    n[..., :3] = nrm * wt[..., None]
    n[..., 3] = (3.0 + (xx // 37) % 5 + 7 * ((yy // 29) % 2)).astype(F32)
    a[..., :3] = rng.random((hh, ww, 3), dtype=F32) * wt[..., None]
    a[xx % 211 < 5, :3] = 0.0   # below the 1e-3 floor
    a[..., 3] = wt
    L = rng.random((hh, ww), dtype=F32) + F32(0.25)
    m[..., 0] = L * wt
    m[..., 1] = (L * L + rng.random((hh, ww), dtype=F32)) * wt
    m[..., 3] = wt
    zero_var = rng.random((hh, ww)) < 0.15
    m[zero_var, 1] = (L * L * wt)[zero_var]
    m[((yy + xx // 4) % 5 == 0) & (xx % 4 == 0), 1] = F32(1e12)   # huge variance, finite through every product
    m[((yy + xx // 6) % 7 == 3) & (xx % 6 == 1), 1] = 0.0          # a second moment below the first squared: clamped to 0
    holes_a = (rng.random((hh, ww)) < 0.04)
    holes_m = (rng.random((hh, ww)) < 0.04) & ~holes_a
    for t in (b, n, a, m):
        t[holes_a | holes_m] = np.nan
    a[holes_a, 3] = 0.0
    m[holes_m, 3] = 0.0
    assert holes_a.any() and holes_m.any()
    return b, n, a, m


_INPUTS = {}
_REFS = {}

D_DEFAULTS = dict(iterations=3, sigma_normal=0.5, sigma_colour=1.0, demodulate=True)
V_DEFAULTS = dict(iterations=3, sigma_normal=0.5, sigma_luminance=4.0, demodulate=True)


def _inputs(W, Hh):
    """The four seeded arrays of a size, made once and read-only: _seeded's at the sizes of the existing tests,
    the striped ones for everything wider."""
    if (W, Hh) not in _INPUTS:
        arrs = _seeded(Hh, W, 11 + W) if W < 1024 else _seeded_stripes(Hh, W, 11 + W)
        for t in arrs:
            t.setflags(write=False)
        _INPUTS[(W, Hh)] = arrs
    return _INPUTS[(W, Hh)]


def _reference(which, W, Hh, **params):
    """dst of `which` ("denoise" | "variance") over the size's inputs, computed once per set of parameters."""
    p = dict(D_DEFAULTS if which == "denoise" else V_DEFAULTS, **params)
    k = (which, W, Hh, tuple(sorted(p.items())))
    if k not in _REFS:
        b, n, a, m = _inputs(W, Hh)
        ref = DR.denoise(b, n, a, **p) if which == "denoise" else VR.denoise(b, n, a, m, **p)
        assert not np.isnan(ref).any()
        ref.setflags(write=False)
        _REFS[k] = ref
    return p, _REFS[k]


def _textures(e, W, Hh, ndst=1):
    """The four inputs of a size written into render targets of `e`, and `ndst` zero-filled dsts."""
    import babylon_pt as bp
    tex = [bp.RenderTargetTexture("in%d" % k, (W, Hh), e) for k in range(4)]
    for t, arr in zip(tex, _inputs(W, Hh)):
        t.write(arr)
    return tex, [bp.RenderTargetTexture("dst%d" % k, (W, Hh), e) for k in range(ndst)]


def _call(e, which, tex, dst, p):
    if which == "denoise":
        e.denoise(tex[0], tex[1], tex[2], dst, **p)
    else:
        e.denoise_variance(tex[0], tex[1], tex[2], tex[3], dst, **p)


# ------------------------------------------------------------------ 1. the passes beyond 4096 tiles

def _pass_grid(W, Hh):
    """(tiles, blocks, most tiles per block) of launch_pass (csrc/pt_denoise.hip) and launch_dvar_pass
    (csrc/pt_denoise_var.hip) for a W x H image, with the two clamps as those sources state them today."""
    clamps = set()
    for name in ("pt_denoise.hip", "pt_denoise_var.hip"):
        with open(os.path.join(CSRC, name)) as f:
            found = re.findall(r"blocks = ntiles / 4 < (\d+) \? (\d+) : ntiles / 4 > (\d+) \? (\d+) : ntiles / 4;", f.read())
        assert len(found) == 1 and found[0][0] == found[0][1] and found[0][2] == found[0][3], (
            "%s: the grid of the LDS passes is no longer clamp(ntiles / 4, lo, hi): the shapes of this file were "
            "chosen for that formula and must move with it" % name)
        clamps.add((int(found[0][0]), int(found[0][2])))
    assert len(clamps) == 1, clamps
    lo, hi = clamps.pop()
    tiles = ((W + 15) // 16) * ((Hh + 15) // 16)
    blocks = min(tiles, min(max(tiles // 4, lo), hi))
    return tiles, blocks, (tiles + blocks - 1) // blocks


# W, H -> tiles, blocks, most tiles per block: the smallest images that reach each regime of the grid formula
PASS_SHAPES = {
    (65547, 3): (4097, 4096, 2),     # the first image that loops at all: block 0 alone, its second tile 11 columns wide
    (131083, 2): (8193, 4096, 3),    # every block loops, block 0 twice: LDS stored again twice
    (320011, 1): (20001, 5000, 5),   # the grid is ntiles / 4, with a remainder
    (524301, 1): (32769, 8192, 5),   # the upper clamp
    (4099, 249): (4112, 4096, 2),    # full-height tiles: all four waves filter, a block's tiles in tile rows 0 and 15
}
# iterations=3 is S = 1, 2, 4 with LAST on S = 4. On the smallest image also LAST on S = 1 and on S = 2 inside the
# loop, a S = 4 pass that is not the last (the far passes behind it), and no demodulation.
PASS_CASES = [(W, Hh, {}) for (W, Hh) in PASS_SHAPES] + [(65547, 3, p) for p in (
    dict(iterations=1), dict(iterations=2), dict(iterations=5), dict(demodulate=False))]


def _case_id(case):
    W, Hh, p = case
    return "%dx%d" % (W, Hh) + "".join("-%s=%s" % kv for kv in sorted(p.items()))


@pytest.mark.parametrize("which", ["denoise", "variance"])
@pytest.mark.parametrize("case", PASS_CASES, ids=_case_id)
def test_passes_beyond_one_tile_per_block(which, case):
    W, Hh, params = case
    # launch_pass / launch_dvar_pass: if these move, the shapes above must move with them
    grid = _pass_grid(W, Hh)
    assert grid == PASS_SHAPES[(W, Hh)], "%dx%d: (tiles, blocks, most tiles per block) = %s" % (W, Hh, grid)
    assert grid[0] > grid[1] and grid[2] >= 2   # some block walks on to a second tile
    import babylon_pt as bp
    p, ref = _reference(which, W, Hh, **params)
    e = bp.Engine(0)
    try:
        tex, (dst,) = _textures(e, W, Hh)
        _call(e, which, tex, dst, p)
        got = dst.read()
    finally:
        e.dispose()
    assert _bits_equal(ref, got), "%s %dx%d %s: %s" % (which, W, Hh, p, _diff_report(ref, got))
    if which == "variance" and not params:   # what the inputs exercise, as test_seeded_inputs asserts it
        var, branch = VR.prep(*_inputs(W, Hh), True)[6:8]
        assert branch.any() and (~branch).any() and np.isfinite(var).all() and var.max() > 1e9


# ------------------------------------------------------------------ 2. one context, several sizes

def test_one_engine_many_sizes():
    """Both denoisers on one engine, interleaved, at 33x17, 96x64, 33x17 again (on slabs sized for 96x64: the
    planes lie 6144 pixels apart, the image has 561), 65547x3, 96x64 again, 65547x3 again and 131083x2. Every
    call has a dst of its own and nothing is read before the last call is queued, so each growth of a slab
    (DevMem::grow: it waits for the main stream, frees and allocates) comes right behind queued calls that use the
    old one - the last behind the two largest calls of the sequence."""
    import babylon_pt as bp
    steps = [(33, 17), (96, 64), (33, 17), (65547, 3), (96, 64), (65547, 3), (131083, 2)]
    grows, cap = [], 0
    for W, Hh in steps:
        grows.append(W * Hh > cap)
        cap = max(cap, W * Hh)
    assert grows == [True, True, False, True, False, False, True]
    e = bp.Engine(0)
    try:
        sets = {size: _textures(e, *size, ndst=2 * steps.count(size)) for size in dict.fromkeys(steps)}
        free = {size: list(dsts) for size, (_, dsts) in sets.items()}
        queued = []
        for W, Hh in steps:
            for which in ("denoise", "variance"):
                p, ref = _reference(which, W, Hh)
                dst = free[(W, Hh)].pop(0)
                _call(e, which, sets[(W, Hh)][0], dst, p)
                queued.append((which, W, Hh, dst, ref))
        got = [dst.read() for _, _, _, dst, _ in queued]
    finally:
        e.dispose()
    for step, ((which, W, Hh, _, ref), g) in enumerate(zip(queued, got)):
        assert _bits_equal(ref, g), "call %d, %s %dx%d: %s" % (step, which, W, Hh, _diff_report(ref, g))


# ------------------------------------------------------------------ 3. PT_MAIN_WAVES below the unit count

STILL = 8   # still-camera frames after the recorded ones: a buffer set and its fused order build come round again
_STREAM_REF = {}


def _stream_reference(name, meta, frames, W, Hh):
    """Of `frames` at W x H: the oracle's last accumulation and canvas and the reference folds of the three feature
    targets. The same for every PT_MAIN_WAVES, so computed once per stream and size."""
    k = (name, W, Hh)
    if k not in _STREAM_REF:
        acc, can, _ = H.oracle_replay(dict(meta, frames=frames), None, W, Hh, with_output=True)
        gb = FR.gbuffers("loops-" + name, meta, frames, W, Hh)
        feat = FR.accumulate(frames, gb, range(len(frames)))[0]
        mom = MR.accumulate(frames, gb, range(len(frames)))[0]
        _STREAM_REF[k] = dict(acc=acc[-1], can=can[-1], nid=feat[0], alb=feat[1], mom=mom)
    return _STREAM_REF[k]


# stream, W, H, PT_MAIN_WAVES, further knobs -> pt_output_w's tiles, pt_blend_w's and pt_feature_fold's units
# (pt_launch_blend / pt_launch_feature_fold: 64 columns x 4 of a band's row groups)
MAIN_WAVES_CASES = [
    ("gltf_teapot_320x180", 96, 64, 1, {}, 24, 32),     # one wave walks everything
    ("gltf_teapot_320x180", 96, 64, 5, {}, 24, 32),     # remainders: 24 = 4 * 5 + 4, 32 = 6 * 5 + 2
    ("gltf_teapot_320x180", 96, 64, 23, {}, 24, 32),    # exactly one wave takes two tiles
    ("gltf_teapot_320x180", 96, 64, 24, {}, 24, 32),    # output does not loop, blend and fold do
    ("gltf_teapot_320x180", 33, 17, 4, {}, 6, 8),
    ("gltf_teapot_320x180", 203, 117, 7, {}, 104, 128),  # 14 or 15 tiles a wave: the LDS buffers alternate many times
    ("gltf_teapot_320x180", 96, 64, 5, {"PT_FUSE_ORDER": "0"}, 24, 32),   # no order-build block beside the tiles
    ("cornell_256", 48, 32, 3, {}, 6, 8),               # an analytic program
]


def _main_waves_run(monkeypatch, name, W, Hh, waves, env, tiles, units, moments=True):
    """The megakernel's one-wave main kernels with `waves` workgroups, the feature targets (and the moments target)
    bound, the recorded frames and eight still ones with no sync between the draws: the last accumulation and
    canvas against the oracle's, the targets against the reference folds (a moments target left unbound stays 0)."""
    import babylon_pt as bp
    bands = (Hh + 15) // 16
    assert ((W + 15) // 16) * bands == tiles and ((W + 63) // 64) * bands * 4 == units
    assert waves < units and waves <= tiles   # blend and fold loop; output too, unless waves == tiles
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    monkeypatch.setenv("PT_MAIN_WAVES", str(waves))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    meta = H.stream(name)
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb, mom = (bp.RenderTargetTexture(t, (W, Hh), e) for t in ("featureNormalId", "featureAlbedoWeight",
                                                                          "featureMoments"))
        fx = player.wrappers[H.path_call(frames[0])["effect"]].effect
        fx.setFeatureTargets(nid, alb)
        if moments:
            fx.setMomentTarget(mom)
        for calls in frames:
            _issue(e, player, calls, 1)
        got = dict(acc=player.textures["pathTracingRenderTarget"].read(), can=e.read_canvas(W, Hh),
                   nid=nid.read(), alb=alb.read(), mom=mom.read())
    finally:
        e.dispose()
    ref = _stream_reference(name, meta, frames, W, Hh)
    if not moments:
        ref = dict(ref, mom=np.zeros((Hh, W, 4), F32))
    what = "%s %dx%d PT_MAIN_WAVES=%d %s" % (name, W, Hh, waves, env)
    # (pt_output_w also writes the frame's screenCopy, the next blend's history: a tile it leaves out shows in both)
    labels = (("acc", "last accumulation (pt_blend_w)"), ("can", "last canvas (pt_output_w)"),
              ("nid", "normal_id (pt_feature_fold)"), ("alb", "albedo_weight (pt_feature_fold)"),
              ("mom", "moments (pt_feature_fold<MOM>)"))
    bad = ["%s: %s" % (label, _diff_report(ref[part], got[part])) for part, label in labels
           if not _bits_equal(ref[part], got[part])]
    assert not bad, "%s: %s" % (what, "; ".join(bad))


@pytest.mark.parametrize("name,W,Hh,waves,env,tiles,units", MAIN_WAVES_CASES,
                         ids=["%s-%dx%d-%d%s" % (c[0].split("_")[1 if c[0][0] == "g" else 0], c[1], c[2], c[3],
                                                 "-order-alone" if c[4] else "") for c in MAIN_WAVES_CASES])
def test_main_waves_below_the_unit_count(monkeypatch, name, W, Hh, waves, env, tiles, units):
    """pt_blend_w, pt_feature_fold<true> and pt_output_w given fewer workgroups than they have units, all three
    targets bound."""
    _main_waves_run(monkeypatch, name, W, Hh, waves, env, tiles, units)


def test_main_waves_fold_without_moments(monkeypatch):
    """The fold's other instantiation, pt_feature_fold<false>, looping: the feature targets alone."""
    _main_waves_run(monkeypatch, "gltf_teapot_320x180", 96, 64, 5, {}, 24, 32, moments=False)
