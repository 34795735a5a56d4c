"""The settings a reference page's GUI can reach, as one table (test infrastructure).

Every recorded uniform stream holds the one setting its page starts with. VARIANTS lists other
settings of the same pages - light plane, light radius, sphere and model materials, sun direction,
HDRI exposure and sun power, intersection epsilon, aperture, model transforms - as uniform overrides
of the path-tracing call, laid over helpers.with_resolution() the way helpers._with_material and
test_gpu_parity._quadric_variant lay theirs. The fixture generator (oracle/xcheck/run_xcheck.py
--variants), the CPU tests (tests/test_xcheck.py) and the GPU tests (tests/test_gpu_settings.py)
all read this table.

VARIANTS: name -> (base, overrides, width, height, frames). `base` is a recorded stream's name or
SKY_MESH (helpers.sky_mesh_stream on synthetic_dragon(64, 64), which has no reference shader). Every
entry is 32x32 over 2 frames: frame 1 clears the history, frame 2 blends; 32x32 is whole waves and
whole 16x16 tiles.
"""
import json
import os

import numpy as np

import helpers as H

W, HGT, FRAMES = 32, 32, 2
SKY_MESH = "sky_mesh"
HELMET = "gltf_helmet_320x180"

# bases whose page has a shader in the reference that the transcription can replay with the
# committed inputs alone (the helmet runs with the seeded maps, which the transcription is not fed)
XCHECK_BASES = ("cornell_256", "sky_256", "quadric_256", "gltf_teapot_320x180", "hdri_teapot_320x180")
MESH_BASES = ("gltf_teapot_320x180", "hdri_teapot_320x180", HELMET, SKY_MESH)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def base_meta(base):
    return _cached(("meta", base), lambda: H.sky_mesh_stream() if base == SKY_MESH else H.stream(base))


def base_mesh(base):
    """The mesh arrays of a base's model (None for a page without one)."""
    if base not in MESH_BASES:
        return None
    return _cached(("mesh", base), lambda: H.synthetic_dragon(64, 64) if base == SKY_MESH else H.mesh(base_meta(base)))


def base_maps(base):
    return _cached("maps", H.synthetic_pbr_maps) if base == HELMET else None


# ------------------------------------------------------------------------------- model transforms
# A recorded uGLTF_Model_InvMatrix, reshaped (4, 4) in the stream's element order, is the matrix B
# with p_model = p_world @ B (row vectors: the GLSL's mat4 * vec4 over the column-major upload). A
# further world-space transform X of the model (p_world' = p_world @ X) gives inv(X) @ B, composed
# in float64 and rounded to binary32.

def _f32list(a):
    return [float(v) for v in np.asarray(a, np.float64).astype(np.float32).reshape(-1)]


def _translate(x, y, z):
    m = np.eye(4)
    m[3, :3] = [x, y, z]
    return m


def _scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def _rotate(ax, ay, az):
    """Rotations about x, then y, then z, in degrees (row vectors)."""
    a, b, c = np.radians([ax, ay, az])
    rx = np.array([[1, 0, 0, 0], [0, np.cos(a), np.sin(a), 0], [0, -np.sin(a), np.cos(a), 0], [0, 0, 0, 1]])
    ry = np.array([[np.cos(b), 0, -np.sin(b), 0], [0, 1, 0, 0], [np.sin(b), 0, np.cos(b), 0], [0, 0, 0, 1]])
    rz = np.array([[np.cos(c), np.sin(c), 0, 0], [-np.sin(c), np.cos(c), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return rx @ ry @ rz


def _recorded(base, name):
    return np.array(H.path_call(base_meta(base)["frames"][0])["uniforms"][name][1], np.float64).reshape(4, 4)


def _model_inv(base, x):
    return {"uGLTF_Model_InvMatrix": ["f", _f32list(np.linalg.inv(x) @ _recorded(base, "uGLTF_Model_InvMatrix"))]}


def model_centre_world(base):
    """The centre of the model's BVH root box (node 0: min at [1:4], max at [5:8]) in world space."""
    root = np.asarray(base_mesh(base)["bvh"], np.float64).reshape(-1, 8)[0]
    c = np.append((root[1:4] + root[5:8]) * 0.5, 1.0)
    return (c @ np.linalg.inv(_recorded(base, "uGLTF_Model_InvMatrix")))[:3]


def _camera_inside(base):
    """The recorded transform, with uCameraMatrix's translation moved to the model's centre: every
    primary ray starts inside the BVH root box."""
    cam = _recorded(base, "uCameraMatrix")
    cam[3, :3] = model_centre_world(base)
    return {"uCameraMatrix": ["f", _f32list(cam)]}


def model_transforms(base):
    """The four model transforms of a teapot page: in the wall plane, a speck, non-uniform scale
    under a rotation, and the camera origin inside the root box."""
    return {
        "model_in_wall": _model_inv(base, _translate(50.0, 0.0, 0.0)),
        "model_speck": _model_inv(base, _scale(0.01, 0.01, 0.01)),
        "model_skewed": _model_inv(base, _scale(4.0, 1.0, 0.25) @ _rotate(37.0, 115.0, 290.0)),
        "camera_in_model": _camera_inside(base),
    }


TEAPOT_TRANSFORMS = []      # the teapot page's four transform variants, by name (filled below)

# ------------------------------------------------------------------------------------------- suns
# The recorded sky page's sun, turned in its own vertical plane (what the GUI's sunDir_RotateX does):
# elevation e -> horizontal * cos(e) + up * sin(e).
_SKY_SUN = H.path_call(H.stream("sky_256")["frames"][0])["uniforms"]["uSunDirection"][1]
_HORIZ = np.array([_SKY_SUN[0], 0.0, _SKY_SUN[2]]) / np.hypot(_SKY_SUN[0], _SKY_SUN[2])


def _sun(y):
    h = _HORIZ * np.sqrt(1.0 - y * y)
    return {"uSunDirection": ["f", [float(np.float32(h[0])), float(y), float(np.float32(h[2]))]]}


SUNS = {
    "sun_zenith": {"uSunDirection": ["f", [0.0, 1.0, 0.0]]},
    "sun_horizon": _sun(0.0),                 # y == 0 exactly
    "sun_below": _sun(-0.17364818),           # 10 degrees under the horizon
    "sun_low": _sun(0.02),
}


def _f(name, v):
    return {name: ["f", [float(v)]]}


def _i(name, v):
    return {name: ["i", [int(v)]]}


def _light(plane, radius=None):
    u = _f("uQuadLightPlaneSelectionNumber", plane)
    if radius is not None:
        u.update(_f("uQuadLightRadius", radius))
    return u


def _join(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


def _build():
    v = {}

    def add(name, base, *parts):
        assert name not in v, name
        v[name] = (base, _join(*parts), W, HGT, FRAMES)

    # ---- cornell_256: every light plane, both radius ends and an odd radius, every sphere material
    b = "cornell_256"
    add("cornell_plane1_r5_m1", b, _light(1, 5), _i("uRightSphereMatType", 1))
    add("cornell_plane2_r150_m2", b, _light(2, 150), _i("uRightSphereMatType", 2))
    add("cornell_plane3_r37_m4", b, _light(3, 37), _i("uRightSphereMatType", 4))
    add("cornell_plane4_r150", b, _light(4, 150))
    add("cornell_plane5_r5", b, _light(5, 5))
    add("cornell_plane0_m1", b, _light(0), _i("uRightSphereMatType", 1))
    add("cornell_plane6_r5_m2", b, _light(6, 5), _i("uRightSphereMatType", 2))
    add("cornell_plane6_r150_m4", b, _light(6, 150), _i("uRightSphereMatType", 4))

    # ---- sky_256: suns and sphere materials
    b = "sky_256"
    for name, sun in SUNS.items():
        add("sky_" + name, b, sun)
    for m in (1, 2, 4):
        add("sky_m%d" % m, b, _i("uRightSphereMatType", m))

    # ---- quadric_256: light planes 1..5 and the radius ends
    b = "quadric_256"
    for plane, radius in ((1, 5), (2, 150), (3, None), (4, 5), (5, 150)):
        add("quadric_plane%d%s" % (plane, "" if radius is None else "_r%d" % radius), b, _light(plane, radius))

    # ---- gltf_teapot_320x180
    b = "gltf_teapot_320x180"
    for plane, radius in ((1, 5), (2, 150), (3, None), (4, 150), (5, 5), (0, None)):
        add("teapot_plane%d%s" % (plane, "" if radius is None else "_r%d" % radius), b, _light(plane, radius))
    add("teapot_eps1", b, _f("uEPS_intersect", 1.0))
    add("teapot_aperture2_focus40", b, _f("uApertureSize", 2.0), _f("uFocusDistance", 40.0))
    for (name, t), m in zip(model_transforms(b).items(), (1, 2, 4, 3)):
        add("teapot_%s_m%d" % (name, m), b, t, _i("uModelMaterialType", m))
        TEAPOT_TRANSFORMS.append("teapot_%s_m%d" % (name, m))

    # ---- hdri_teapot_320x180
    b = "hdri_teapot_320x180"
    add("hdri_exposure005", b, _f("uHDRExposure", 0.05))
    add("hdri_exposure3", b, _f("uHDRExposure", 3.0))
    add("hdri_sunpower1", b, _f("uSunPower", 1.0))
    add("hdri_sunpower50", b, _f("uSunPower", 50.0))
    add("hdri_sun_other", b, {"uSunDirection": ["f", _f32list([-0.48, 0.6, 0.64])]})
    add("hdri_sun_below", b, {"uSunDirection": ["f", _f32list([0.6, -0.28, -0.75])]})
    add("hdri_transparent", b, _i("uModelMaterialType", 2))
    for (name, t), m in zip(model_transforms(b).items(), (4, 1, 3, 2)):
        add("hdri_%s_m%d" % (name, m), b, t, _i("uModelMaterialType", m))

    # ---- gltf_helmet_320x180 with the seeded PBR maps: the tangent frame under a model matrix
    add("helmet_moved_turned", HELMET, _model_inv(HELMET, _rotate(20.0, 40.0, 60.0) @ _translate(10.0, 5.0, -10.0)))

    # ---- sky + mesh composite
    for (name, sun), m in zip(SUNS.items(), (3, 1, 2, 4)):
        add("skymesh_%s_m%d" % (name, m), SKY_MESH, sun, _i("uModelMaterialType", m))
    add("skymesh_model_skewed", SKY_MESH,
        _model_inv(SKY_MESH, _scale(1.5, 1.0, 0.5) @ _rotate(37.0, 115.0, 290.0) @ _translate(10.0, 5.0, 20.0)))
    return v


VARIANTS = _build()
SKY_MESH_TRANSFORM = "skymesh_model_skewed"


def variants_of(base):
    return [n for n, v in VARIANTS.items() if v[0] == base]


def uniforms(name, k, extra=None):
    """The path-tracing uniforms of variant `name` at its frame k (`extra`: laid over last)."""
    base, over, w, h, _ = VARIANTS[name]
    u = H.with_resolution(H.path_call(base_meta(base)["frames"][k])["uniforms"], w, h)
    u.update(over)
    u.update(extra or {})
    return u


def _replay(base, over, w, h, frames):
    sc = H.oracle_scene(base_meta(base), w, h, base_mesh(base), base_maps(base))
    meta = base_meta(base)
    acc = np.zeros((h, w, 4), np.float32)
    accs, counters = [], []
    for f in meta["frames"][:frames]:
        u = H.with_resolution(H.path_call(f)["uniforms"], w, h)
        u.update(over)
        acc, cnt = sc.path_trace(u, acc)
        accs.append(acc.copy())
        counters.append(cnt)
    ou = H.output_call(meta["frames"][frames - 1])["uniforms"]
    exp = ou.get("uToneMappingExposure", ["f", [0.0]])[1][0]
    canvas = H.po_screen_output(acc, ou["uOneOverSampleCounter"][1][0], exp)
    total = {k: sum(c[k] for c in counters) for k in counters[0]}
    return {"acc": accs, "canvas": canvas, "counters": total}


def oracle(name):
    """The oracle over a variant's frames: {"acc": [after each frame], "canvas": the last frame's,
    "counters": totals}. Computed once and shared; callers leave it unchanged."""
    base, over, w, h, frames = VARIANTS[name]
    return _cached(("oracle", name), lambda: _replay(base, over, w, h, frames))


def oracle_base(base, w=W, h=HGT, frames=FRAMES):
    """The base stream's own setting at a variant's size (what liveness is measured against)."""
    return _cached(("oracle-base", base, w, h, frames), lambda: _replay(base, {}, w, h, frames))


def variant_meta(name):
    """The base stream with a variant's overrides laid over every path-tracing call (what
    helpers._with_material does for one uniform): a stream a StreamPlayer can extend with
    synth_frame(), the setting kept."""
    base, over, _, _, _ = VARIANTS[name]
    meta = base_meta(base)
    frames = [[dict(c, uniforms=dict(c["uniforms"], **over)) if c["shader"] == "pathTracingFragmentShader" else c
               for c in f] for f in meta["frames"]]
    return dict(meta, frames=frames)


XDIR = os.path.join(H.GOLD, "xcheck")


def transcribed(name):
    """The accumulation after each frame of a variant as the reference's transcribed shader text
    rendered it (tests/golden/xcheck/variants_<scene>.npz, written by oracle/xcheck/run_xcheck.py
    --variants), or None for a variant whose page has no reference shader."""
    report = _cached("report", lambda: json.load(open(os.path.join(XDIR, "report.json")))["_variants"])
    if name not in report:
        return None
    r = report[name]
    d = _cached(("npz", r["scene"]), lambda: np.load(os.path.join(XDIR, "variants_%s.npz" % r["scene"])))
    return [d["%s/acc%d" % (name, k)] for k in range(r["frames"])]
