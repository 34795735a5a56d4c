"""The reference's shader text, transcribed mechanically, against the oracle and the HIP path.

oracle/xcheck/transcribe.py turns the GLSL of js/PathTracingCommon.js and each scene's
js/*_FragmentShader.js into C++ by syntax-only rewrites (literal suffixes, swizzle proxies,
braced constructors, out-parameter copies) over a GLSL stand-in (oracle/xcheck/glsl_shim.h) that
shares only the pinned transcendental sequences with the oracle; oracle/xcheck/run_xcheck.py ran
it in the build container on every recorded stream and stored its accumulation after each frame
under tests/golden/xcheck/. Neither the reference nor its transcription (the git-ignored
oracle/_ref/, also listed in .gpurunignore; tests/conftest.py refuses a GPU session that finds
it) travels to the GPU box: there only those committed frames are read. These tests pin the oracle and
the HIP kernels to those frames bit for bit: a misreading of the GLSL (an expression, a branch, a
constant, the order of rng() calls) in the hand-written oracle or kernels would show here, which
the oracle-vs-HIP tests alone cannot see. Radiance parity against a GL driver stays unpinned: the
built-ins' rounding is the pinned one on all three sides.

The recorded streams hold one setting per page. The settings the pages' GUIs reach besides it
(tests/settings_variants.py: light planes, radii, materials, suns, exposure, model transforms) went
through the transcription too (run_xcheck.py --variants -> variants_<scene>.npz, report.json's
"_variants"); the tests at the end of this module pin the oracle to those frames and check that each
variant is a live input, tests/test_gpu_settings.py pins the HIP kernels to them.
"""
import json
import os

import numpy as np
import pytest

import helpers as H
import settings_variants as S

XDIR = os.path.join(H.GOLD, "xcheck")
REPORT = json.load(open(os.path.join(XDIR, "report.json")))
CASES = sorted(n for n in REPORT if not n.startswith("_"))
OUT_CASES = [(name, n) for name in sorted(REPORT["_screen_output"]) for n in (1, 2, 200, 201, 4999, 5001)]


def _fixture(name):
    r = REPORT[name]
    d = np.load(os.path.join(XDIR, "%s_%dx%d.npz" % (name, r["width"], r["height"])))
    return r, [d["acc%d" % k] for k in range(r["frames"])]


def _maps(r):
    return H.helmet_maps() if r["maps"] == "helmet" else None


def _same_bits(want, got, what):
    bad = (want.view(np.uint32) != got.view(np.uint32)).any(-1)
    assert not bad.any(), "%s: %d of %d pixels differ from the transcribed reference" % (what, bad.sum(), bad.size)


def test_report_covers_every_reference_shader():
    """Every scene shader of the reference is transcribed (the sky+model composite has no
    reference shader to transcribe), screenCopy and screenOutput too, and the build-time
    comparison found no differing pixel."""
    assert {REPORT[n]["scene"] for n in CASES} == {"cornell", "gltf", "hdri", "sky", "quadric"}
    for n in CASES:
        for f in REPORT[n]["per_frame"]:
            assert f["pixels_differing"] == 0 and f["max_abs"] == 0.0, n
    for n, r in REPORT["_screen_output"].items():
        assert all(v == 0 for v in r["pixels_differing_by_N"].values()), (n, r)


def _quantize(c):
    """the canvas store of a [0,1] colour: u8 = floor(255 c + 0.5) in binary32"""
    c = np.asarray(c, np.float32)
    return np.floor(c * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def _output_fixture(name, n):
    r = REPORT["_screen_output"][name]
    d = np.load(os.path.join(XDIR, "screen_output_%s_%dx%d.npz" % (name, r["width"], r["height"])))
    return r, d["acc"], _quantize(d["out_%d" % n])


@pytest.mark.parametrize("name,n", OUT_CASES)
def test_oracle_screen_output_matches_transcribed_reference(name, n):
    """screenOutput at N either side of its bypass thresholds, on an accumulation whose alpha
    carries the path tracer's edge flags; includes the frame border, where the GLSL's
    ivec2(gl_FragCoord.xy + vec2(-1, .)) truncates -0.5 to texel 0."""
    r, acc, want = _output_fixture(name, n)
    got = H.po_screen_output(acc, float(np.float32(1.0 / n)), r["exposure"])
    assert np.array_equal(want, got), "%d px differ" % (want != got).any(-1).sum()


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_transcribed_reference(name):
    r, want = _fixture(name)
    meta = H.stream(name)
    got, _, _ = H.oracle_replay(meta, r["frames"], width=r["width"], height=r["height"], maps=_maps(r))
    for k in range(r["frames"]):
        _same_bits(want[k], got[k], "%s frame %d (oracle)" % (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", OUT_CASES)
def test_hip_screen_output_matches_transcribed_reference(engine, name, n):
    import babylon_pt as bp
    r, acc, want = _output_fixture(name, n)
    meta = H.stream(name)
    payload = H.texture_payloads(meta, H.mesh(meta)) if meta["scene"] in ("gltf", "hdri") else None
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), payload, r["width"], r["height"])
    engine.resize_canvas(player.width, player.height)
    player.textures["pathTracingRenderTarget"].write(acc)
    out_call = H.output_call(meta["frames"][0])
    player.play_call(out_call, uniform_override={"uOneOverSampleCounter": ["f", [float(np.float32(1.0 / n))]],
                                                 "uToneMappingExposure": ["f", [r["exposure"]]]})
    got = engine.read_canvas(player.width, player.height)
    assert np.array_equal(want, got), "%d px differ" % (want != got).any(-1).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_matches_transcribed_reference(engine, name):
    import babylon_pt as bp
    r, want = _fixture(name)
    meta = H.stream(name)
    payload = H.texture_payloads(meta, H.mesh(meta)) if meta["scene"] in ("gltf", "hdri") else None
    player = bp.StreamPlayer(engine, meta, H.bluenoise(), payload, r["width"], r["height"])
    maps = _maps(r)
    if maps:
        for kind, sampler in H.PBR_SAMPLERS.items():
            player.textures[sampler] = bp.Texture(engine, maps[kind], name=kind)
    engine.resize_canvas(player.width, player.height)
    for k in range(r["frames"]):
        player.play_frame(k)
        _same_bits(want[k], player.textures["pathTracingRenderTarget"].read(), "%s frame %d (HIP)" % (name, k))


# ------------------------------------------------------------------- settings the GUIs reach
VREPORT = REPORT["_variants"]
XVARIANTS = [n for n, v in S.VARIANTS.items() if v[0] in S.XCHECK_BASES]


def test_variant_report_covers_the_table():
    """Every variant of a page with a reference shader went through the transcription at the table's
    size, and the build-time comparison with the oracle found no differing pixel in any frame."""
    assert sorted(VREPORT) == sorted(XVARIANTS)
    for n, r in VREPORT.items():
        base, _, w, h, frames = S.VARIANTS[n]
        assert (r["base"], r["width"], r["height"], r["frames"]) == (base, w, h, frames), n
        assert len(r["per_frame"]) == frames
        for f in r["per_frame"]:
            assert f["pixels_differing"] == 0 and f["max_abs"] == 0.0, n


@pytest.mark.parametrize("name", XVARIANTS)
def test_oracle_matches_transcribed_variant(name):
    want = S.transcribed(name)
    got = S.oracle(name)["acc"]
    assert len(want) == len(got)
    for k in range(len(want)):
        assert want[k].shape == (S.HGT, S.W, 4)
        _same_bits(want[k], got[k], "%s frame %d (oracle)" % (name, k))


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_variant_is_a_live_input(name):
    """A variant that renders what its base stream renders pins nothing: after frame 2 its
    accumulation differs in bits from the base's, at the same size, in at least 16 of the 1024
    pixels; a mesh variant's walks still fetch BVH nodes. A variant that fails here is a badly
    chosen input: the input changes, not the bound."""
    base = S.VARIANTS[name][0]
    ref, own = S.oracle_base(base), S.oracle(name)
    changed = (ref["acc"][-1].view(np.uint32) != own["acc"][-1].view(np.uint32)).any(-1)
    assert changed.size == 1024 and changed.sum() >= 16, "%s: %d pixels differ from %s" % (name, changed.sum(), base)
    if base in S.MESH_BASES:
        assert own["counters"]["node_fetches"] > 0, own["counters"]


def test_table_covers_the_gui_ranges():
    """Light planes 0..6, materials 1..4 on every page that has them, both ends of the light
    radius, and suns above, on and below the horizon all appear (as the effective setting: the
    recorded value where a variant leaves it alone)."""
    seen = {}
    for name, (base, over, w, h, frames) in S.VARIANTS.items():
        assert (w, h, frames) == (32, 32, 2), name
        u = S.uniforms(name, 0)
        for k, (_, vals) in u.items():
            seen.setdefault((base, k), []).append(vals)
    def values(base, k):
        return {v[0] for v in seen[(base, k)]}
    for base in ("cornell_256", "gltf_teapot_320x180"):
        assert values(base, "uQuadLightPlaneSelectionNumber") == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0}, base
    assert values("quadric_256", "uQuadLightPlaneSelectionNumber") >= {1.0, 2.0, 3.0, 4.0, 5.0}
    for base in ("cornell_256", "gltf_teapot_320x180", "quadric_256"):
        assert values(base, "uQuadLightRadius") >= {5.0, 150.0}, base
    assert 37.0 in values("cornell_256", "uQuadLightRadius")
    for base, k in (("cornell_256", "uRightSphereMatType"), ("sky_256", "uRightSphereMatType"),
                    ("gltf_teapot_320x180", "uModelMaterialType"), ("hdri_teapot_320x180", "uModelMaterialType"),
                    (S.SKY_MESH, "uModelMaterialType")):
        assert values(base, k) == {1, 2, 3, 4}, (base, k)
    for base in ("sky_256", S.SKY_MESH):
        ys = [v[1] for v in seen[(base, "uSunDirection")]]
        assert any(y > 0 for y in ys) and any(y == 0 for y in ys) and any(y < 0 for y in ys), (base, ys)
        assert [0.0, 1.0, 0.0] in seen[(base, "uSunDirection")]
    ys = [v[1] for v in seen[("hdri_teapot_320x180", "uSunDirection")]]
    assert any(y > 0 for y in ys) and any(y < 0 for y in ys), ys
    assert values("hdri_teapot_320x180", "uHDRExposure") >= {0.05, 3.0}
    assert values("hdri_teapot_320x180", "uSunPower") >= {1.0, 50.0}
    assert 1.0 in values("gltf_teapot_320x180", "uEPS_intersect")
    assert 2.0 in values("gltf_teapot_320x180", "uApertureSize") and 40.0 in values("gltf_teapot_320x180", "uFocusDistance")
    # three moved models and a moved camera on both teapot pages, a moved model on the helmet and
    # on the composite
    def moved(base, k):
        rec = tuple(H.path_call(S.base_meta(base)["frames"][0])["uniforms"][k][1])
        return len({tuple(v) for v in seen[(base, k)]} - {rec})
    for base in ("gltf_teapot_320x180", "hdri_teapot_320x180"):
        assert moved(base, "uGLTF_Model_InvMatrix") == 3 and moved(base, "uCameraMatrix") == 1, base
    assert moved(S.HELMET, "uGLTF_Model_InvMatrix") == 1 and moved(S.SKY_MESH, "uGLTF_Model_InvMatrix") == 1


def test_camera_in_model_starts_inside_the_root_box():
    """The camera-inside variants put the ray origin strictly inside the model's BVH root box."""
    for name in ("teapot_camera_in_model_m3", "hdri_camera_in_model_m2"):
        base = S.VARIANTS[name][0]
        u = S.uniforms(name, 0)
        o = np.append(np.array(u["uCameraMatrix"][1][12:15], np.float64), 1.0)
        p = (o @ np.array(u["uGLTF_Model_InvMatrix"][1], np.float64).reshape(4, 4))[:3]
        root = S.base_mesh(base)["bvh"].reshape(-1, 8)[0]
        assert (root[1:4] < p).all() and (p < root[5:8]).all(), (p, root)
