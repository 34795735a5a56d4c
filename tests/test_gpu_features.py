"""Feature buffers (pt_set_feature_targets): the accumulated G-buffer normal + object id and albedo + weight of
every program, backend, BVH layout and grid edge, with late-bounce compaction, band partitions, multi-part
contexts and counting, bit for bit against the oracle's G-buffer folded by the rule of include/pt.h
(tests/features_ref.py) - and the beauty, bit for bit what it is without features.

The scaffold of a case: a fresh engine, both targets bound to the path-tracing effect, the stream's recorded
frames plus ten still-camera frames (every buffer set comes round at least twice), no sync between frames, one
read of both feature targets right after a mid-stream path-tracing draw and one after the last frame; both
reads, the last accumulation and the last canvas are compared as uint32 / bytes. No tolerance anywhere.

Run on an MI355X: python -m pytest tests/test_gpu_features.py -m gpu
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import features_ref as FR
import helpers as H
from helpers import _with_material
from test_gpu_compaction import _bits_equal, _diff_report, _issue, _oracle, _player

pytestmark = pytest.mark.gpu

STILL = 10   # still-camera frames after the recorded ones

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _maps():
    return _cached("maps256", lambda: H.synthetic_pbr_maps(256))


def _dragon():
    return _cached("dragon64", lambda: H.synthetic_dragon(64, 64))


def _path_effect(player, frames):
    return player.wrappers[H.path_call(frames[0])["effect"]].effect


def _targets(e, player):
    import babylon_pt as bp
    size = (player.width, player.height)
    return bp.RenderTargetTexture("featureNormalId", size, e), bp.RenderTargetTexture("featureAlbedoWeight", size, e)


def _check_features(what, got, ref):
    for name, g, r in (("normal_id", got[0], ref[0]), ("albedo_weight", got[1], ref[1])):
        assert _bits_equal(r, g), "%s: %s: %s" % (what, name, _diff_report(r, g))


def _check_beauty(what, acc, can, ref):
    last = max(ref["acc"])
    assert _bits_equal(ref["acc"][last], acc), "%s: last accumulation: %s" % (what, _diff_report(ref["acc"][last], acc))
    assert _bits_equal(ref["can"], can), "%s: last canvas: %s" % (what, _diff_report(ref["can"], can))


def _run(key, meta, W, Hh, mesh=None, maps=None, backend="megakernel", layout="pairs", parts=1, devices=None,
         counting=False):
    """The scaffold. Returns what the engine reported and the oracle's beauty reference."""
    import babylon_pt as bp
    e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
    try:
        e.set_backend(backend)
        e.set_bvh_layout(layout)
        if counting:
            e.set_counting(True)
            e.reset_counters()
        player = _player(e, meta, W, Hh, mesh, maps)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        mid = len(frames) - 4
        nid, alb = _targets(e, player)
        _path_effect(player, frames).setFeatureTargets(nid, alb)
        got = {}

        def read_mid():
            got["mid"] = (nid.read(), alb.read())

        for i, calls in enumerate(frames):
            _issue(e, player, calls, parts, read_mid if i == mid else None)
        got["last"] = (nid.read(), alb.read())
        got["acc"] = player.textures["pathTracingRenderTarget"].read()
        got["can"] = e.read_canvas(W, Hh)
        rep = {"cs": e.cont_stats(), "layout": e.bvh_layout_used(), "counters": e.counters() if counting else None}
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh, mesh, maps)
    last, kept = FR.accumulate(frames, gb, range(len(frames)), keep={mid})
    _check_features("%s after frame %d's path tracing" % (key, mid), got["mid"], kept[mid])
    _check_features("%s after the last frame" % key, got["last"], last)
    ref = _oracle(key, meta, frames, W, Hh, mesh, maps)
    _check_beauty(key, got["acc"], got["can"], ref)
    return rep, ref


# ------------------------------------------------------------------ every program

@pytest.mark.parametrize("name", ["cornell_256", "quadric_256", "sky_256"])
def test_analytic_programs(name):
    _run("feat-" + name, H.stream(name), 48, 32)


def test_gltf_teapot():
    """The stream that starts at uFrameCounter 2 with the camera moving: the 0.5 / 0.5 branch."""
    rep, _ = _run("feat-teapot", H.stream("gltf_teapot_320x180"), 96, 64)
    assert rep["layout"] == "pairs"


def test_hdri_helmet_with_maps():
    _run("feat-helmet", H.stream("hdri_helmet_320x180"), 96, 64, maps=_maps())


def test_sky_mesh_dragon():
    _run("feat-skymesh", H.sky_mesh_stream(), 96, 64, mesh=_dragon())


# ------------------------------------------------------------------ backends x layouts

@pytest.mark.parametrize("layout", ["pairs", "trail", "reference"])
@pytest.mark.parametrize("backend", ["megakernel", "wavefront", "persistent"])
def test_backends_and_layouts(backend, layout):
    rep, _ = _run("feat-teapot", H.stream("gltf_teapot_320x180"), 96, 64, backend=backend, layout=layout)
    assert rep["layout"] == layout


# ------------------------------------------------------------------ edges of the grid

@pytest.mark.parametrize("name,W,Hh,backend", [("gltf_duck_320x180", 33, 17, "megakernel"),
                                                ("gltf_duck_320x180", 33, 17, "wavefront"),
                                                ("gltf_duck_320x180", 33, 17, "persistent"),
                                                ("gltf_teapot_320x180", 1, 1, "megakernel"),
                                                ("gltf_teapot_320x180", 203, 117, "megakernel")])
def test_grid_edges(name, W, Hh, backend):
    """33x17: odd sizes, quad helpers beyond both edges, a last band of one row (and, on the queued backends,
    a quad-rounded G-buffer whose rows are longer than the target's); one pixel; 203x117."""
    _run("feat-edge-" + name, H.stream(name), W, Hh, backend=backend)


# ------------------------------------------------------------------ late-bounce compaction forced

@pytest.mark.parametrize("material", [1, 2, 3])
def test_with_compaction_forced(monkeypatch, material):
    """Records go through pt_cont while features are bound: the FEAT + CONT variant stages the G-buffer of
    the paths it hands on, too."""
    monkeypatch.setenv("PT_CONT", "1")
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    meta = _with_material(H.stream("gltf_teapot_320x180"), material)
    rep, _ = _run("feat-cont-m%d" % material, meta, 203, 117)
    stored, launched = rep["cs"]
    assert stored > 0 and launched > 0, rep["cs"]


# ------------------------------------------------------------------ binding and unbinding

def test_one_target_then_the_other_then_none():
    """Frames 0-3 fold into normal_id alone, 4-7 into albedo_weight alone, 8-9 into neither; then normal_id is
    destroyed while bound (which unbinds it) and 10-12 fold into albedo_weight again. The beauty stays exact."""
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb = _targets(e, player)
        fx = _path_effect(player, frames)
        zero = np.zeros((Hh, W, 4), np.float32)

        def play(lo, hi):
            for calls in frames[lo:hi]:
                _issue(e, player, calls, 1)

        fx.setFeatureTargets(nid, None)
        play(0, 4)
        got_a = (nid.read(), alb.read())
        fx.setFeatureTargets(None, alb)
        play(4, 8)
        got_b = (nid.read(), alb.read())
        fx.setFeatureTargets(None, None)
        play(8, 10)
        got_c = (nid.read(), alb.read())
        fx.setFeatureTargets(nid, alb)
        nid.dispose()
        play(10, len(frames))
        got_d = alb.read()
        acc = player.textures["pathTracingRenderTarget"].read()
        can = e.read_canvas(W, Hh)
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    (n03, _), _ = FR.accumulate(frames, gb, range(0, 4))
    (_, a47), _ = FR.accumulate(frames, gb, range(4, 8))
    (_, a_end), _ = FR.accumulate(frames, gb, range(10, len(frames)), albedo_weight=a47)
    _check_features("normal_id alone", got_a, (n03, zero))
    _check_features("albedo_weight alone", got_b, (n03, a47))
    _check_features("unbound", got_c, (n03, a47))
    assert _bits_equal(a_end, got_d), "after normal_id was destroyed: %s" % _diff_report(a_end, got_d)
    _check_beauty(key, acc, can, _oracle(key, meta, frames, W, Hh))


# ------------------------------------------------------------------ partitions and parts

@pytest.mark.parametrize("parts", [2, 3])
def test_row_partition(parts):
    """set_row_partition on one engine: each part's draw folds only its 16-row bands (the weight of the first
    frame shows which), and the union is the one-part result."""
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb = _targets(e, player)
        _path_effect(player, frames).setFeatureTargets(nid, alb)
        seen = []

        def first_frame():
            for p in range(parts):
                e.set_row_partition(parts, p)
                player.play_call(frames[0][0])
                seen.append(alb.read()[..., 3] != 0)
            e.set_row_partition(1, 0)
            for call in frames[0][1:]:
                player.play_call(call)

        first_frame()
        for calls in frames[1:]:
            _issue(e, player, calls, parts)
        got = (nid.read(), alb.read())
        acc = player.textures["pathTracingRenderTarget"].read()
    finally:
        e.dispose()
    rows = np.zeros(Hh, bool)
    for p in range(parts):
        rows[bp.owned_rows(Hh, parts, p)] = True
        want = np.repeat(rows[:, None], W, 1)
        assert np.array_equal(seen[p], want), "part %d's fold touched rows it does not own" % p
    assert rows.all()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    last, _ = FR.accumulate(frames, gb, range(len(frames)))
    _check_features("%d row partitions" % parts, got, last)
    ref = _oracle(key, meta, frames, W, Hh)
    assert _bits_equal(ref["acc"][max(ref["acc"])], acc)


@pytest.mark.parametrize("devices", [[0, 0], [0] * 5])
def test_multi_part_context(devices):
    """Each part folds its bands of its share of the targets; read() assembles the one-part result."""
    _run("feat-parts", H.stream("gltf_teapot_320x180"), 203, 40, devices=devices)


# ------------------------------------------------------------------ counting

def test_counting_with_features():
    """The counting kernels stage the G-buffer too (tested at run time): counters and features exact."""
    rep, ref = _run("feat-teapot", H.stream("gltf_teapot_320x180"), 96, 64, counting=True)
    assert rep["counters"] == ref["counters"]


# ------------------------------------------------------------------ errors

def test_errors_and_a_draw_after_them():
    import babylon_pt as bp
    meta, W, Hh, key = H.stream("gltf_teapot_320x180"), 96, 64, "feat-teapot"
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(STILL)]
        nid, alb = _targets(e, player)
        fx = _path_effect(player, frames)
        path = frames[0][0]
        # the wrong effect kind, a texture that is no render target
        for call in frames[0][1:]:
            with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
                player.wrappers[call["effect"]].effect.setFeatureTargets(nid, alb)
        with pytest.raises(bp.PtError, match="PT_ERR_ARG"):
            fx.setFeatureTargets(player.textures["file:BlueNoise_RGBA256.png"], None)
        # a size mismatch, the draw target, previousBuffer, one target twice: refused by the draw
        small = bp.RenderTargetTexture("small", (W + 1, Hh), e)
        for a, b in ((small, None), (None, small), (player.textures["pathTracingRenderTarget"], alb),
                     (nid, player.textures["screenCopyRenderTarget"]), (nid, nid)):
            fx.setFeatureTargets(a, b)
            with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
                player.play_call(path)
        fx.setFeatureTargets(nid, alb)
        for calls in frames:
            _issue(e, player, calls, 1)
        got = (nid.read(), alb.read())
        acc = player.textures["pathTracingRenderTarget"].read()
        can = e.read_canvas(W, Hh)
    finally:
        e.dispose()
    gb = FR.gbuffers(key, meta, frames, W, Hh)
    last, _ = FR.accumulate(frames, gb, range(len(frames)))
    _check_features("after the refused draws", got, last)
    _check_beauty(key, acc, can, _oracle(key, meta, frames, W, Hh))


# ------------------------------------------------------------------ the JavaScript host

@pytest.mark.skipif(not shutil.which("node"), reason="node not installed")
def test_node_feature_targets_match_python(tmp_path):
    """js/replay_features.js replays the teapot stream with feature targets through the shim and the addon:
    byte for byte the Python binding's result (and so the reference's)."""
    import babylon_pt as bp
    meta = H.stream("gltf_teapot_320x180")
    W, Hh = meta["width"], meta["height"]
    H.bluenoise().tofile(tmp_path / "bluenoise.u8")
    for k, v in H.texture_payloads(meta, H.mesh(meta)).items():
        v.tofile(tmp_path / (k + ".f32"))
    out = str(tmp_path / "out")
    script = os.path.join(H.ROOT, "babylon.js-pathtracing-renderer_amd", "js", "replay_features.js")
    subprocess.run(["node", script, os.path.join(H.GOLD, "gltf_teapot_320x180.json"), str(tmp_path), out],
                   check=True, timeout=300)
    js = [np.fromfile(out + s, np.float32).reshape(Hh, W, 4) for s in (".normal_id.f32", ".albedo_weight.f32", ".acc.f32")]
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh)
        nid, alb = _targets(e, player)
        _path_effect(player, meta["frames"]).setFeatureTargets(nid, alb)
        for i in range(len(meta["frames"])):
            player.play_frame(i)
        py = [nid.read(), alb.read(), player.textures["pathTracingRenderTarget"].read()]
    finally:
        e.dispose()
    for name, a, b in zip(("normal_id", "albedo_weight", "accumulation"), js, py):
        assert a.tobytes() == b.tobytes(), name
    gb = FR.gbuffers("feat-teapot-full", meta, meta["frames"], W, Hh)
    last, _ = FR.accumulate(meta["frames"], gb, range(len(meta["frames"])))
    _check_features("node", js[:2], last)
