"""Dead shadow segments (pt_program.h deadShadow): a path that samples the light with a throughput of exactly +0
ends at that shading step in the timed kernels of the room programs (Cornell, quadrics, glTF), its shadow
segment untraced. The radiance and the alpha flag must keep their bits, on every schedule: each case is four frames
from a cleared history, bit-exact against the CPU oracle (accumulation as uint32, canvas bytes) on the scaffold of
tests/test_gpu_compaction.py. The sky programs keep every segment (the rule is off there); their sun-lobe site is
covered all the same, with a sun below two walls' horizons.

That each scene really holds zero-weight light samples is a condition, asserted with the oracle's G-buffer and a
NumPy restatement of the weight: surfaces whose every sample has weight zero are seen at bounce 0 (the ceiling
above the quad light's plane; walls that face away from the sun), and a DIFFUSE surface samples the light at its
first diffuse hit with probability 1/2 per frame.

Run on an MI355X: python -m pytest tests/test_gpu_dead_segments.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import test_gpu_compaction as C
from helpers import _with_material

pytestmark = pytest.mark.gpu

DIFFUSE = 1
FRAMES = 4
f32 = np.float32

# schedule -> (backend, environment)
SCHEDULES = {
    "megakernel": ("megakernel", {"PT_CONT": "0"}),
    "compacted": ("megakernel", {"PT_CONT": "1", "PT_CONT_LANES": "64"}),   # every looping path goes on in pt_cont
    "persistent": ("persistent", {"PT_CONT": "0"}),
    "wavefront": ("wavefront", {"PT_CONT": "0"}),
}

LOW_SUN = [-0.6, 0.35, -0.72]   # normalised below: behind the back wall (normal +z) and the left wall (normal +x)


def _low_sun_direction():
    v = np.array(LOW_SUN, np.float64)
    return [float(c) for c in v / np.linalg.norm(v)]


def _with_sun(meta, sun):
    frames = []
    for f in meta["frames"]:
        frames.append([dict(c, uniforms=dict(c["uniforms"], uSunDirection=["f", list(sun)]))
                       if c["shader"] == "pathTracingFragmentShader" else c for c in f])
    return dict(meta, frames=frames)


def _scene(name):
    """(oracle cache key, stream, mesh) of a case's scene."""
    if name == "gltf":
        return "ds-gltf", _with_material(H.stream("gltf_teapot_320x180"), DIFFUSE), None
    if name == "cornell":
        return "ds-cornell", H.stream("cornell_256"), None
    if name == "sky":
        return "ds-sky", _with_sun(H.stream("sky_256"), _low_sun_direction()), None
    return "ds-skymesh", _with_sun(H.sky_mesh_stream(DIFFUSE), _low_sun_direction()), C._small_dragon()


def _run(monkeypatch, name, size, schedule):
    """Four frames from a cleared history on a fresh engine of `schedule`, compared with the oracle (shared per
    scene and size); returns the compaction statistics."""
    import babylon_pt as bp
    key, meta, mesh = _scene(name)
    W, Hh = size
    backend, env = SCHEDULES[schedule]
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = bp.Engine(0)
    try:
        e.set_backend(backend)
        player = C._player(e, meta, W, Hh, mesh)
        frames = (meta["frames"] + [player.synth_frame(k) for k in range(FRAMES)])[:FRAMES]
        mid = FRAMES - 2
        got = C._draw(e, player, frames, mid)
        rep = {"cs": e.cont_stats(), "qs": e.queue_stats(), "frames": frames}
    finally:
        e.dispose()
    C._compare("%s %dx%d %s" % (key, W, Hh, schedule), got, C._oracle(key, meta, frames, W, Hh, mesh, keep={mid}), mid)
    return rep


def _check_schedule(rep, size, schedule):
    if schedule == "compacted":   # records went through pt_cont: it shaded light-sampling sites
        C._assert_compacted(rep, size[0], size[1])
    else:
        assert rep["cs"] == (0, 0), rep["cs"]


# ------------------------------------------------------------------------------- the condition (CPU only)

def _ids_at_bounce_0(name, size, frame=1):
    _, meta, mesh = _scene(name)
    W, Hh = size
    sc = H.oracle_scene(meta, W, Hh, mesh)
    return sc.gbuffer(H.with_resolution(H.path_call(meta["frames"][frame])["uniforms"], W, Hh))[..., 6], meta


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v * (f32(1.0) / np.sqrt(_dot(v, v)))[..., None]


def _quad_light_weights(uniforms, x, nl):
    """sampleQuadLight's weight (js/PathTracingCommon.js sampleAxisAlignedQuadLight; pt_device.h) in float32 for surface points
    `x` (N, 3) with normal `nl`, over a 5x5 grid of the clamped random numbers: (N, 25) weights."""
    assert uniforms["uQuadLightPlaneSelectionNumber"][1][0] == 6        # the ceiling light, normal (0, -1, 0)
    L = f32(uniforms["uQuadLightRadius"][1][0]) * f32(0.2)
    v0 = np.array([-L, f32(49.0), -L], f32)
    v2 = np.array([L, f32(49.0), L], f32)
    ln = np.array([0.0, -1.0, 0.0], f32)
    r = np.clip(np.linspace(0.0, 1.0, 5, dtype=f32), f32(0.1), f32(0.9))
    rx, rz = np.meshgrid(r, r, indexing="ij")
    q = np.stack([v0[0] * (f32(1) - rx) + v2[0] * rx, np.full_like(rx, f32(49.0)), v0[2] * (f32(1) - rz) + v2[2] * rz],
                 -1).reshape(1, -1, 3)
    d = q - x[:, None, :]
    d2 = _dot(d, d)
    r2 = (f32(2) * L) * (f32(2) * L)   # distance(v0, v1) * distance(v0, v3) of the square light
    cos_a_max = np.sqrt(f32(1) - np.clip(r2 / d2, f32(0), f32(1)))
    d = _normalize(d)
    dot_nl = np.maximum(f32(0), _dot(np.broadcast_to(nl, d.shape), d))
    w = f32(2) * (f32(1) - cos_a_max) * np.maximum(f32(0), -_dot(d, np.broadcast_to(ln, d.shape))) * dot_nl
    assert w.dtype == f32
    return np.clip(w, f32(0), f32(1))


@pytest.mark.parametrize("name,size", [("gltf", (96, 64)), ("gltf", (50, 38)), ("cornell", (96, 64))])
def test_room_scenes_hold_zero_weight_light_samples(name, size):
    """The ceiling (quad 3 of the room, y = 50) lies above the quad light's plane (y = 49, facing down): every light
    sample taken from it has weight exactly zero - and a floor point under the light does not (the restatement is no
    constant zero). The frame shows the ceiling at bounce 0, a DIFFUSE surface."""
    ids, meta = _ids_at_bounce_0(name, size)
    ceiling_id = 2.0 + 3.0
    assert (ids == ceiling_id).sum() >= 10, "the ceiling is not in view"
    u = H.path_call(meta["frames"][1])["uniforms"]
    g = np.linspace(-45.0, 45.0, 7, dtype=f32)
    gx, gz = np.meshgrid(g, g, indexing="ij")
    ceiling = np.stack([gx, np.full_like(gx, f32(50.0)), gz], -1).reshape(-1, 3)
    w = _quad_light_weights(u, ceiling, np.array([0.0, -1.0, 0.0], f32))
    assert w.shape == (49, 25) and (w.view(np.uint32) == 0).all()      # bitwise +0
    floor = np.array([[0.0, -50.0, 0.0]], f32)
    assert (_quad_light_weights(u, floor, np.array([0.0, 1.0, 0.0], f32)) > 0).all()
    if name == "gltf":   # the model is in view too, as a DIFFUSE surface: its hits sample the light
        assert (ids == 8.0).sum() >= 10


def _sun_lobe_dirs(sun, roughness):
    """specularLobeDir(sun, roughness) (js/PathTracingCommon.js randomDirectionInSpecularLobe; pt_device.h) in
    float32 over a 16x16 grid of its two random numbers, [0, 1] and [0, 1): (256, 3) unit directions."""
    sun = np.asarray(sun, f32)
    rough = f32(roughness)
    exponent = f32(7.0) * (f32(1) - np.sqrt(rough))
    r1, r2 = np.meshgrid(np.linspace(0.0, 1.0, 16, dtype=f32), np.linspace(0.0, 0.999, 16, dtype=f32), indexing="ij")
    cos_t = np.power(r1, f32(1) / (np.exp(exponent) + f32(1))).astype(f32)
    sin_t = np.sqrt(np.maximum(f32(0), f32(1) - cos_t * cos_t))
    phi = r2 * f32(6.28318530717958648)
    a = np.array([0.0, 1.0, 0.0], f32) if abs(sun[1]) < 0.9 else np.array([1.0, 0.0, 0.0], f32)
    U = np.cross(a, sun).astype(f32)
    U = U / np.sqrt((U * U).sum())
    V = np.cross(sun, U).astype(f32)
    lobe = (U * np.cos(phi)[..., None]) * sin_t[..., None] + (V * np.sin(phi)[..., None]) * sin_t[..., None] \
        + sun * cos_t[..., None]
    rd = sun * (f32(1) - rough) + lobe.astype(f32) * rough
    return _normalize(rd.astype(f32)).reshape(-1, 3)


@pytest.mark.parametrize("name", ["sky", "skymesh"])
def test_sky_scenes_hold_zero_weight_sun_samples(name):
    """With the sun behind the back wall (quad 0, normal +z) and the left wall (quad 1, normal +x), every direction
    of the sun's lobe (roughness 0.1) has max(0, dot(rd, nl)) * 0.05 exactly zero on both, and a positive weight on
    the floor; both walls are in view at bounce 0."""
    ids, meta = _ids_at_bounce_0(name, (96, 64))
    sun = H.path_call(meta["frames"][1])["uniforms"]["uSunDirection"][1]
    rd = _sun_lobe_dirs(sun, 0.1)
    assert np.isfinite(rd).all()
    for quad, nl in ((0, [0.0, 0.0, 1.0]), (1, [1.0, 0.0, 0.0])):
        assert (ids == 2.0 + quad).sum() >= 10, "quad %d is not in view" % quad
        w = np.maximum(f32(0), _dot(rd, np.array(nl, f32)[None, :])) * f32(0.05)
        assert (w.view(np.uint32) == 0).all()
    assert (np.maximum(f32(0), _dot(rd, np.array([0.0, 1.0, 0.0], f32)[None, :])) * f32(0.05) > 0).all()


# --------------------------------------------------------------------------------------- the frames

@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("size", [(96, 64), (50, 38)], ids=["96x64", "50x38"])
def test_gltf_room_diffuse_model(monkeypatch, size, schedule):
    """The glTF room with a DIFFUSE teapot: mesh, wall and ceiling hits all sample the quad light."""
    _check_schedule(_run(monkeypatch, "gltf", size, schedule), size, schedule)


@pytest.mark.parametrize("schedule", ["megakernel", "persistent", "wavefront"])
def test_cornell_page(monkeypatch, schedule):
    """The Cornell page (no mesh: nothing to compact): the ceiling and the light's own plane."""
    _check_schedule(_run(monkeypatch, "cornell", (96, 64), schedule), (96, 64), schedule)


@pytest.mark.parametrize("schedule", ["megakernel", "persistent", "wavefront"])
def test_sky_low_sun(monkeypatch, schedule):
    _check_schedule(_run(monkeypatch, "sky", (96, 64), schedule), (96, 64), schedule)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_sky_mesh_low_sun(monkeypatch, schedule):
    _check_schedule(_run(monkeypatch, "skymesh", (96, 64), schedule), (96, 64), schedule)


def test_counting_replay_keeps_every_segment(engine):
    """The counting variants price the reference's work: the rule is off there, so one 96x64 frame of the glTF room
    with the DIFFUSE model returns the oracle's counters, segments included."""
    key, meta, _ = _scene("gltf")
    W, Hh = 96, 64
    frames = meta["frames"][:1]
    ref = C._oracle(key + "-count", meta, frames, W, Hh)
    engine.set_backend("megakernel")
    player = C._player(engine, meta, W, Hh)
    engine.set_counting(True)
    engine.reset_counters()
    try:
        for call in frames[0]:
            player.play_call(call)
        engine.sync()
        cnt = engine.counters()
        acc = player.textures["pathTracingRenderTarget"].read()
    finally:
        engine.set_counting(False)
    assert cnt == ref["counters"], (cnt, ref["counters"])
    assert cnt["segments"] > W * Hh
    assert C._bits_equal(ref["acc"][0], acc), C._diff_report(ref["acc"][0], acc)
