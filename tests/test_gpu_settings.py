"""The settings a page's GUI reaches, on the GPU: every entry of tests/settings_variants.py (light
planes, light radius, sphere and model materials, sun directions, HDRI exposure and sun power,
epsilon, aperture, model transforms) on every schedule and BVH layout, bit for bit against the CPU
oracle and, where the page has a reference shader, against the frames its transcribed shader text
rendered (tests/golden/xcheck/variants_<scene>.npz). The recorded streams hold one setting per page,
so the branches of setup_scene() and sky_setup() (csrc/pt_capi.cpp: evaluated on the host, once per
draw) that other settings take, and the walks' root-box tests under other model transforms, are
compared here and nowhere else.

Besides per-variant parity: the algorithmic counters under the model transforms (a wrong root-box
cull can give the right pixels for the wrong traversal), late-bounce compaction on four variants,
and settings switched while draws are in flight (a host precomputation cached across draws or
buffer sets would show there).

Run on an MI355X: python -m pytest tests/test_gpu_settings.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import settings_variants as S
from test_gpu_compaction import _assert_compacted, _bits_equal, _diff_report, _run

pytestmark = pytest.mark.gpu

# (schedule, BVH layout): every combination must give the same bits
BACKENDS = [(b, l) for b in ("megakernel", "persistent", "wavefront") for l in ("pairs", "trail", "reference")]

_PLAYERS = {}


@pytest.fixture(scope="module", params=BACKENDS, ids=["-".join(b) for b in BACKENDS])
def backend(request, engine):
    """Module-scoped, so that the tests of one backend run together and share its players."""
    engine.set_backend(request.param[0])
    engine.set_bvh_layout(request.param[1])
    yield request.param
    engine.sync()
    _PLAYERS.clear()
    engine.set_backend("megakernel")
    engine.set_bvh_layout("pairs")


def _new_player(e, base, w, h):
    import babylon_pt as bp
    meta, mesh, maps = S.base_meta(base), S.base_mesh(base), S.base_maps(base)
    player = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh) if mesh is not None else None, w, h)
    if maps:
        for kind, sampler in H.PBR_SAMPLERS.items():
            player.textures[sampler] = bp.Texture(e, maps[kind], name=kind)
    return player


def _player(engine, base, key, w=S.W, h=S.HGT):
    """One StreamPlayer per base stream and backend: its data textures are uploaded once, the variants
    go through play_call's uniform_override. Both render targets are zeroed before a variant, as the
    oracle starts from a zero history (the teapot pages' first recorded frame blends it)."""
    k = (base, key, w, h)
    if k not in _PLAYERS:
        _PLAYERS[k] = _new_player(engine, base, w, h)
    player = _PLAYERS[k]
    zero = np.zeros((h, w, 4), np.float32)
    for name in ("pathTracingRenderTarget", "screenCopyRenderTarget"):
        player.textures[name].write(zero)
    engine.resize_canvas(w, h)
    return player


def _play(engine, player, name):
    """A variant's frames through the player: the accumulation after each frame and the last canvas."""
    base, over, w, h, frames = S.VARIANTS[name]
    accs = []
    for k in range(frames):
        player.play_frame(k, uniform_override=over)
        engine.sync()
        accs.append(player.textures["pathTracingRenderTarget"].read())
    return accs, engine.read_canvas(w, h)


def _check(name, accs, canvas):
    ref = S.oracle(name)
    xref = S.transcribed(name)
    assert (xref is not None) == (S.VARIANTS[name][0] in S.XCHECK_BASES)
    for k, got in enumerate(accs):
        assert _bits_equal(ref["acc"][k], got), "%s frame %d vs the oracle: %s" % (name, k, _diff_report(ref["acc"][k], got))
        if xref is not None:
            assert _bits_equal(xref[k], got), "%s frame %d vs the transcribed shader: %s" % (name, k, _diff_report(xref[k], got))
    assert _bits_equal(ref["canvas"], canvas), "%s canvas: %s" % (name, _diff_report(ref["canvas"], canvas))


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_setting_variant_bitexact(engine, backend, name):
    """Accumulation after each of the two frames (RGBA32F as uint32) and the last canvas (bytes)
    equal the oracle's and the transcribed reference's."""
    base = S.VARIANTS[name][0]
    accs, canvas = _play(engine, _player(engine, base, backend), name)
    if base in S.MESH_BASES:
        assert engine.bvh_layout_used() == backend[1]
    _check(name, accs, canvas)


@pytest.mark.parametrize("name", S.TEAPOT_TRANSFORMS + [S.SKY_MESH_TRANSFORM])
def test_model_transform_counters(engine, backend, name):
    """The counting kernels under the model transforms - model in the wall plane, a speck, a skewed
    model, the camera inside the root box, the composite's moved dragon: node fetches, leaf tests and
    hit lookups equal the oracle's, with the pixels."""
    base = S.VARIANTS[name][0]
    player = _player(engine, base, backend)
    engine.set_counting(True)
    engine.reset_counters()
    try:
        accs, canvas = _play(engine, player, name)
        cnt = engine.counters()
    finally:
        engine.set_counting(False)
    assert engine.bvh_layout_used() == backend[1]
    _check(name, accs, canvas)
    assert cnt == S.oracle(name)["counters"]
    assert cnt["node_fetches"] > 0


@pytest.mark.parametrize("name", ["teapot_plane2_r150", "teapot_camera_in_model_m3", "hdri_exposure005",
                                  "skymesh_sun_below_m2"])
def test_setting_variant_compacted(monkeypatch, name):
    """Late-bounce compaction (fresh engine, PT_CONT=1, no overlap lag, 7 draws with no sync) under a
    side light as large as its wall, rays that start inside the model, a dim environment and a sun
    under the horizon: path records go through pt_cont and every bit stays the oracle's."""
    base, _, w, h, _ = S.VARIANTS[name]
    rep, ref = _run(monkeypatch, "setting-" + name, S.variant_meta(name), w, h, mesh=S.base_mesh(base))
    assert rep["layout"] == "pairs"
    assert ref["counters"]["node_fetches"] > 0
    _assert_compacted(rep, w, h)


# ------------------------------------------------------------------ settings switched in flight

SWITCHES = {
    "cornell_256": ("cornell_plane2_r150_m2", "cornell_plane0_m1"),          # a light, then none
    "gltf_teapot_320x180": ("teapot_plane2_r150", "teapot_model_skewed_m4"),
    "hdri_teapot_320x180": ("hdri_exposure005", "hdri_sun_below"),
    S.SKY_MESH: ("skymesh_sun_below_m2", "skymesh_sun_zenith_m3"),
}


@pytest.mark.parametrize("base", list(SWITCHES))
def test_settings_switched_with_draws_in_flight(engine, base):
    """Nine frames with no sync (the default schedule: three frames in flight), the setting switched
    at frames 3 and 6 to two variants, uCameraIsMoving = 1 on the switching frame as the GUI handlers
    set it and still frames in between. setup_scene() / sky_setup() run on the host per draw: were
    their results shared between draws or buffer sets, a draw in flight would render with its
    neighbour's setting. The accumulation read right after frame 7's path tracing, the last
    accumulation and the last canvas equal the oracle's over the same per-frame uniforms."""
    import ptoracle as po
    w, h = S.W, S.HGT
    player = _player(engine, base, "switch")
    meta = S.base_meta(base)
    frames = meta["frames"] + [player.synth_frame(k) for k in range(9 - len(meta["frames"]))]
    assert len(frames) == 9
    played = []
    for i, calls in enumerate(frames):
        over = {} if i < 3 else dict(S.VARIANTS[SWITCHES[base][0 if i < 6 else 1]][1])
        if i in (3, 6):
            over["uCameraIsMoving"] = ["i", [1]]
        played.append([dict(c, uniforms=dict(c["uniforms"], **over)) if c["shader"] == "pathTracingFragmentShader" else c
                       for c in calls])
    assert [H.path_call(f)["uniforms"]["uCameraIsMoving"][1][0] for f in played] == [1, 0, 0, 1, 0, 0, 1, 0, 0]
    mid, got = 7, {}
    for i, calls in enumerate(played):
        for call in calls:
            player.play_call(call)
            if i == mid and call["shader"] == "pathTracingFragmentShader":
                got["mid"] = player.textures["pathTracingRenderTarget"].read()
    engine.sync()
    got["acc"] = player.textures["pathTracingRenderTarget"].read()
    got["can"] = engine.read_canvas(w, h)

    sc = H.oracle_scene(meta, w, h, S.base_mesh(base), S.base_maps(base))
    acc = np.zeros((h, w, 4), np.float32)
    for i, calls in enumerate(played):
        acc, _ = sc.path_trace(H.with_resolution(H.path_call(calls)["uniforms"], w, h), acc)
        if i == mid:
            want_mid = acc.copy()
    ou = H.output_call(played[-1])["uniforms"]
    want_can = po.screen_output(acc, ou["uOneOverSampleCounter"][1][0], ou.get("uToneMappingExposure", ["f", [0.0]])[1][0])
    assert _bits_equal(want_mid, got["mid"]), "accumulation after frame %d's path tracing: %s" % (mid, _diff_report(want_mid, got["mid"]))
    assert _bits_equal(acc, got["acc"]), "last accumulation: %s" % _diff_report(acc, got["acc"])
    assert _bits_equal(want_can, got["can"]), "last canvas: %s" % _diff_report(want_can, got["can"])
