"""The moments target (pt_set_moment_target): the accumulated luminance moments of every program, backend, BVH
layout and grid edge, bound alone and beside the feature targets, with frames in flight and late-bounce compaction,
band partitions and a multi-part context, bit for bit against the oracle's radiance folded by the rule of
include/pt.h (tests/moments_ref.py) - and the beauty, the canvas and the statistics, bit for bit what they are
without it. The scaffold is tests/test_gpu_features.py's (same streams and frames: one oracle G-buffer serves both).
No tolerance anywhere.

Run on an MI355X: python -m pytest tests/test_gpu_moments.py -m gpu
"""
import copy

import numpy as np
import pytest

import features_ref as FR
import helpers as H
import moments_ref as MR
from test_gpu_compaction import _bits_equal, _diff_report, _issue, _player
from test_gpu_features import STILL, _check_features, _maps, _path_effect, _targets

pytestmark = pytest.mark.gpu


def _moments_target(e, player):
    import babylon_pt as bp
    return bp.RenderTargetTexture("featureMoments", (player.width, player.height), e)


def _check(what, got, ref):
    assert _bits_equal(ref, got), "%s: moments: %s" % (what, _diff_report(ref, got))


def _run(key, meta, W, Hh, mesh=None, maps=None, backend="megakernel", layout="pairs", devices=None, alone=False):
    """A fresh engine, the moments target bound (`alone`) or all three targets, the stream's frames plus STILL still
    ones with no sync between them; the moments read right after a mid-stream path-tracing draw and after the last
    frame, against the reference fold."""
    import babylon_pt as bp
    e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
    try:
        e.set_backend(backend)
        e.set_bvh_layout(layout)
        player = _player(e, meta, W, Hh, mesh, maps)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        mid = len(frames) - 4
        mom = _moments_target(e, player)
        fx = _path_effect(player, frames)
        fx.setMomentTarget(mom)
        if not alone:
            nid, alb = _targets(e, player)
            fx.setFeatureTargets(nid, alb)
        got = {}

        def read_mid():
            got["mid"] = mom.read()

        for i, calls in enumerate(frames):
            _issue(e, player, calls, 1, read_mid if i == mid else None)
        got["last"] = mom.read()
        if not alone:
            got["feat"] = (nid.read(), alb.read())
        assert e.bvh_layout_used() == layout or meta["scene"] not in ("gltf", "hdri")
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh, mesh, maps)
    last, kept = MR.accumulate(frames, gb, range(len(frames)), keep={mid})
    _check("%s after frame %d's path tracing" % (key, mid), got["mid"], kept[mid])
    _check("%s after the last frame" % key, got["last"], last)
    assert np.all(last[..., 2] == 0.0) and not np.signbit(got["last"][..., 2]).any()
    if not alone:
        _check_features(key, got["feat"], FR.accumulate(frames, gb, range(len(frames)))[0])


# ------------------------------------------------------------------ every program

@pytest.mark.parametrize("name,W,Hh,maps", [("cornell_256", 48, 32, False), ("sky_256", 48, 32, False),
                                             ("quadric_256", 48, 32, False), ("gltf_teapot_320x180", 96, 64, False),
                                             ("hdri_helmet_320x180", 96, 64, True)])
def test_programs(name, W, Hh, maps):
    key = {"gltf_teapot_320x180": "feat-teapot", "hdri_helmet_320x180": "feat-helmet"}.get(name, "feat-" + name)
    _run(key, H.stream(name), W, Hh, maps=_maps() if maps else None)


# ------------------------------------------------------------------ backends x layouts, the moments alone

@pytest.mark.parametrize("layout", ["pairs", "trail", "reference"])
@pytest.mark.parametrize("backend", ["megakernel", "wavefront", "persistent"])
def test_backends_and_layouts(backend, layout):
    """With the moments target alone the megakernel runs its kernels without G-buffer staging, and the queued
    backends' fold reads their per-pixel radiance at the quad-rounded stride."""
    _run("feat-teapot", H.stream("gltf_teapot_320x180"), 96, 64, backend=backend, layout=layout, alone=True)


# ------------------------------------------------------------------ moving frames, a reset, still frames

def test_moving_then_reset_then_still():
    """The teapot stream starts at uFrameCounter 2 with the camera moving (weights 0.5, 1.5, 2.5); then two still
    frames that begin a new accumulation (uFrameCounter 1: the reset, weight 1; then 2). Checked after every frame."""
    import babylon_pt as bp
    meta, W, Hh = H.stream("gltf_teapot_320x180"), 96, 64
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = list(meta["frames"])
        for k in range(2):
            f = copy.deepcopy(player.synth_frame(k))
            u = H.path_call(f)["uniforms"]
            u["uFrameCounter"] = ["f", [1.0 + k]]
            u["uSampleCounter"] = ["f", [1.0 + k]]
            frames.append(f)
        mom = _moments_target(e, player)
        _path_effect(player, frames).setMomentTarget(mom)
        got = []
        for calls in frames:
            _issue(e, player, calls, 1)
            got.append(mom.read())
    finally:
        e.dispose()
    gb = FR.gbuffers("mom-teapot-reset", meta, frames, W, Hh)
    _, kept = MR.accumulate(frames, gb, range(len(frames)), keep=set(range(len(frames))))
    for i, wt in enumerate((0.5, 1.5, 2.5, 1.0, 2.0)):
        assert np.all(kept[i][..., 3] == wt), (i, wt)
        _check("frame %d (weight %g)" % (i, wt), got[i], kept[i])


# ------------------------------------------------------------------ edges of the grid

@pytest.mark.parametrize("name,W,Hh,backend", [("gltf_duck_320x180", 33, 17, "megakernel"),
                                                ("gltf_duck_320x180", 33, 17, "wavefront"),
                                                ("gltf_duck_320x180", 33, 17, "persistent"),
                                                ("gltf_teapot_320x180", 1, 1, "megakernel")])
def test_grid_edges(name, W, Hh, backend):
    _run("feat-edge-" + name, H.stream(name), W, Hh, backend=backend, alone=backend != "megakernel")


# ------------------------------------------------------------------ binding and unbinding; nothing else changes

def _order_run(monkeypatch, bind):
    monkeypatch.setenv("PT_OVERLAP_DEPTH", "3")
    monkeypatch.setenv("PT_CONT", "1")
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    import babylon_pt as bp
    meta, W, Hh = H.stream("gltf_teapot_320x180"), 96, 64
    out = {}
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        mom = _moments_target(e, player)
        if bind:
            _path_effect(player, frames).setMomentTarget(mom)
        for calls in frames:
            _issue(e, player, calls, 1)
        out["mom"] = mom.read()
        out["acc"] = player.textures["pathTracingRenderTarget"].read()
        out["canvas"] = e.read_canvas(W, Hh)
        out["cont"] = e.cont_stats()
        out["qs"] = e.queue_stats()
        out["frames"] = frames
    finally:
        e.dispose()
    return out


def test_only_the_moments_bound_changes_nothing_else(monkeypatch):
    """Three frames in flight and compaction forced: with only the moments target bound, the beauty, the canvas,
    queue_stats and cont_stats are what they are with nothing bound, and the moments are the reference's."""
    a = _order_run(monkeypatch, True)
    b = _order_run(monkeypatch, False)
    assert _bits_equal(b["acc"], a["acc"]), _diff_report(b["acc"], a["acc"])
    assert np.array_equal(a["canvas"], b["canvas"])
    assert a["cont"] == b["cont"] and a["cont"][1] > 0, (a["cont"], b["cont"])
    assert a["qs"] == b["qs"] and a["qs"]["frames_in_flight"] == 3, (a["qs"], b["qs"])
    assert not b["mom"].any()
    frames = a["frames"]
    gb = FR.gbuffers("feat-teapot", H.stream("gltf_teapot_320x180"), frames, 96, 64)
    _check("moments alone, three frames in flight", a["mom"], MR.accumulate(frames, gb, range(len(frames)))[0])


def test_bind_late_unbind_rebind_in_combinations():
    """Frames 0-3: moments + normal_id; 4-7: albedo_weight alone; 8-9: nothing; 10-12: all three, and then the
    moments texture is destroyed while bound (which unbinds it) before a last draw."""
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb = _targets(e, player)
        mom = _moments_target(e, player)
        fx = _path_effect(player, frames)

        def play(lo, hi):
            for calls in frames[lo:hi]:
                _issue(e, player, calls, 1)

        fx.setMomentTarget(mom)
        fx.setFeatureTargets(nid, None)
        play(0, 4)
        got_a = (mom.read(), nid.read(), alb.read())
        fx.setMomentTarget(None)
        fx.setFeatureTargets(None, alb)
        play(4, 8)
        got_b = (mom.read(), nid.read(), alb.read())
        fx.setFeatureTargets(None, None)
        play(8, 10)
        got_c = (mom.read(), nid.read(), alb.read())
        fx.setFeatureTargets(nid, alb)
        fx.setMomentTarget(mom)
        play(10, 12)
        got_d = (mom.read(), nid.read(), alb.read())
        mom.dispose()
        play(12, len(frames))
        got_e = (nid.read(), alb.read())
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    zero = np.zeros((Hh, W, 4), np.float32)
    m03, _ = MR.accumulate(frames, gb, range(0, 4))
    (n03, _), _ = FR.accumulate(frames, gb, range(0, 4))
    (_, a47), _ = FR.accumulate(frames, gb, range(4, 8))
    m_d, _ = MR.accumulate(frames, gb, range(10, 12), moments=m03)
    (n_d, a_d), _ = FR.accumulate(frames, gb, range(10, 12), n03, a47)
    (n_e, a_e), _ = FR.accumulate(frames, gb, range(12, len(frames)), n_d, a_d)
    for what, got, ref in (("moments + normal_id", got_a, (m03, n03, zero)), ("albedo_weight alone", got_b, (m03, n03, a47)),
                           ("nothing bound", got_c, (m03, n03, a47)), ("all three", got_d, (m_d, n_d, a_d))):
        _check(what, got[0], ref[0])
        _check_features(what, got[1:], ref[1:])
    _check_features("after the moments texture was destroyed", got_e, (n_e, a_e))


# ------------------------------------------------------------------ partitions and parts

def test_row_partition():
    """set_row_partition(2, k): each part's draw folds only its 16-row bands and leaves the others untouched; the
    union is the one-part result."""
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        mom = _moments_target(e, player)
        _path_effect(player, frames).setMomentTarget(mom)
        mark = np.full((Hh, W, 4), -3.0, np.float32)
        mom.write(mark)
        seen = []
        for p in range(2):
            e.set_row_partition(2, p)
            player.play_call(frames[0][0])
            seen.append(mom.read())
        e.set_row_partition(1, 0)
        for call in frames[0][1:]:
            player.play_call(call)
        for calls in frames[1:]:
            _issue(e, player, calls, 2)
        got = mom.read()
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    fc, moving = FR.frame_state(frames[0])
    first = MR.fold(mark, gb[0], fc, moving)
    rows0 = bp.owned_rows(Hh, 2, 0)
    want = mark.copy()
    want[rows0] = first[rows0]
    _check("part 0 of 2", seen[0], want)
    _check("part 1 of 2", seen[1], first)
    last, _ = MR.accumulate(frames, gb, range(1, len(frames)), moments=first)
    _check("two row partitions", got, last)


def test_multi_part_context():
    """A two-part context on one device: each part folds its bands of its share; read() assembles the one-part bits."""
    _run("feat-parts", H.stream("gltf_teapot_320x180"), 203, 40, devices=[0, 0])


# ------------------------------------------------------------------ refusals

def test_errors_and_a_draw_after_them():
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    e2 = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb = _targets(e, player)
        mom = _moments_target(e, player)
        fx = _path_effect(player, frames)
        path = frames[0][0]
        # PT_ERR_ARG: the wrong effect kind, a texture that is no render target, a foreign one, no effect
        for call in frames[0][1:]:
            with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
                player.wrappers[call["effect"]].effect.setMomentTarget(mom)
        with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
            fx.setMomentTarget(player.textures["file:BlueNoise_RGBA256.png"])
        foreign = bp.RenderTargetTexture("foreign", (W, Hh), e2)
        with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
            fx.setMomentTarget(foreign)
        assert bp.lib().pt_set_moment_target(None, mom.handle) == -1
        # PT_ERR_STATE from the draw: a size mismatch, the draw target, previousBuffer, another feature target
        small = bp.RenderTargetTexture("small", (W + 1, Hh), e)
        fx.setFeatureTargets(nid, alb)
        for t in (small, player.textures["pathTracingRenderTarget"], player.textures["screenCopyRenderTarget"], nid, alb):
            fx.setMomentTarget(t)
            with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
                player.play_call(path)
        fx.setMomentTarget(mom)
        for calls in frames:
            _issue(e, player, calls, 1)
        got = (mom.read(), nid.read(), alb.read())
    finally:
        e.dispose()
        e2.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    _check("after the refused draws", got[0], MR.accumulate(frames, gb, range(len(frames)))[0])
    _check_features("after the refused draws", got[1:], FR.accumulate(frames, gb, range(len(frames)))[0])
