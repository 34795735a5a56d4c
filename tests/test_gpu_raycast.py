"""pt_cast_rays (csrc/pt_raycast.hip) against the restated SceneIntersect (tests/raycast_ref.py): every field of
every record bit for bit, on every program (Cornell, sky, the twelve quadric shapes at both ends of uShapeK, glTF,
HDRI, sky + mesh), every mesh case of tests/raycast_cases.py under all three BVH layouts (each against the
reference, and the three against each other), ray counts around the wave size with the mesh hits in the tail
lanes, the call's place among the draws (a draw, a query, a draw = two draws, with compaction on and three frames
in flight; no counter or statistic moves; a query needs no draw before it), every error, and pick / autofocus.

Run on an MI355X: python -m pytest tests/test_gpu_raycast.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import raycast_cases as C
import raycast_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("t", "object_id", "type", "triangle", "normal", "bary_u", "color", "bary_v", "uv", "reserved")


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 16)


def _same(what, got, ref, skip=()):
    """Every field of every record (but `skip`), as bits; the message names the first ray and field that differ."""
    assert got.dtype == R.RAY_HIT and got.shape == ref.shape, what
    if skip:
        got, ref = got.copy(), ref.copy()
        for f in skip:
            got[f], ref[f] = 0, 0
    if np.array_equal(_words(got), _words(ref)):
        return
    i = int(np.nonzero((_words(got) != _words(ref)).any(1))[0][0])
    bad = [f for f in FIELDS if np.ascontiguousarray(got[f][i:i + 1]).tobytes() != np.ascontiguousarray(ref[f][i:i + 1]).tobytes()]
    n = int((_words(got) != _words(ref)).any(1).sum())
    raise AssertionError("%s: %d of %d records differ, first ray %d in %s: got %s, reference %s" % (what, n, len(ref), i, bad, got[i], ref[i]))


class _Bound:
    """A case's scene on the engine with its uniforms and samplers set on the path-tracing effect, nothing drawn."""

    def __init__(self, engine, name, w=96, h=64):
        import babylon_pt as bp
        stream, _, key = C.CASES[name]
        self.meta = C._meta(stream)
        payload = H.texture_payloads(self.meta, C.mesh_of(key)) if key is not None else None
        self.player = bp.StreamPlayer(engine, self.meta, H.bluenoise(), payload, w, h)
        if name in C.BUMPED:   # the seeded PBR maps, under the names the helmet streams bind
            maps = C._cached("maps", H.synthetic_pbr_maps)
            for kind, sampler in H.PBR_SAMPLERS.items():
                self.player.textures[sampler] = bp.Texture(engine, maps[kind], name=kind)
        call = H.path_call(self.meta["frames"][0])
        self.fx = self.player.wrappers[call["effect"]].effect
        for uname, ent in C.uniforms_of(name).items():
            self.fx._set_entry(uname, ent)
        for sname, tex in call["samplers"].items():
            self.fx.setTexture(sname, self.player.textures.get(tex) if tex else None)

    def dispose(self):
        for raw, kind in (self.meta.get("textures") or {}).items():
            self.player.textures[raw].dispose()


@pytest.fixture
def bound(engine):
    made = []

    def make(name, **kw):
        made.append(_Bound(engine, name, **kw))
        return made[-1]
    yield make
    engine.set_bvh_layout("pairs")
    for b in made:
        b.dispose()


# ------------------------------------------------------------------------------------------ programs and meshes

@pytest.mark.parametrize("name", [n for n in C.CASES if n not in C.MESH_CASES])
def test_room_programs_bitexact(bound, name):
    """Cornell, sky, and the quadric page at uShapeK 0.01 and 1 (the ends its control clamps to): spheres or shapes
    and quads, misses, exact zeros of both signs, a zero, a NaN and an infinite direction."""
    o, d, _ = C.rays_of(name)
    _same(name, bound(name).fx.cast_rays(o, d), C.reference(name))


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_mesh_cases_bitexact_on_every_layout(engine, bound, name):
    """Trees of 1, 2 and 3 triangles, a chain to the trail's depth bound (tight, and with every box the root's: all
    28 levels pending, the slab's last level), the teapot as metal, as glass (the double-sided test), under a skewed
    model matrix, in the HDRI program and in the sky composite: reference, pairs and trail each give the reference's
    records, hence each other's. The helmet cases run the textured program variants, whose mesh hits are
    PBR_MATERIAL and carry a bump-mapped normal: the reference restates no bump map, so against it every field but
    `normal` is compared, and the normals are compared between the three layouts."""
    o, d, _ = C.rays_of(name)
    b = bound(name)
    got = {}
    skip = ("normal",) if name in C.BUMPED else ()
    for layout in C.LAYOUTS:
        engine.set_bvh_layout(layout)
        got[layout] = b.fx.cast_rays(o, d)
        _same("%s, %s" % (name, layout), got[layout], C.reference(name), skip)
    if skip:
        mesh = C.reference(name)["triangle"] >= 0
        assert mesh.sum() > 10 and (C.reference(name)["type"][mesh] == R.PBR_MATERIAL).all()
        assert not np.array_equal(got["pairs"]["normal"][mesh], C.reference(name)["normal"][mesh]), "no bump map applied"
        _same(name + ", what is not a mesh hit", got["pairs"][~mesh], C.reference(name)[~mesh])
    for layout in C.LAYOUTS[1:]:
        _same("%s, %s against %s" % (name, layout, C.LAYOUTS[0]), got[layout], got[C.LAYOUTS[0]])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ray_counts_around_the_wave_size(engine, bound, n):
    """n rays with the mesh hits last, so in the tail lanes of the last wave (n = 1: the one ray hits the mesh):
    records 0 .. n - 1 are the reference's, and the words behind record n - 1 of the caller's buffer stay as they
    were. Per-ray results do not depend on the ray's place, so the reference's records are taken by index."""
    name = "gltf_teapot"
    o, d, _ = C.rays_of(name)
    ref = C.reference(name)
    mesh = np.nonzero(ref["triangle"] >= 0)[0]
    rest = np.nonzero(ref["triangle"] < 0)[0]
    k = min(n, 7)
    idx = np.concatenate([np.resize(rest, n - k), mesh[:k]])   # (the other rays, repeated where n needs more of them)
    assert len(idx) == n and (ref["triangle"][idx[-k:]] >= 0).all()
    b = bound(name)
    import babylon_pt as bp
    for layout in C.LAYOUTS:
        engine.set_bvh_layout(layout)
        _same("n = %d, %s" % (n, layout), b.fx.cast_rays(o[idx], d[idx]), ref[idx])
    # through the C ABI into a buffer with a guard record behind the last one
    oo, dd = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    buf = np.full((n + 1) * 16, 0xA5A5A5A5, np.uint32)
    engine.check(bp.lib().pt_cast_rays(b.fx.handle, oo.ctypes.data, dd.ctypes.data, n, buf.ctypes.data), "pt_cast_rays")
    assert np.array_equal(buf[:n * 16].reshape(n, 16), _words(ref[idx])) and (buf[n * 16:] == 0xA5A5A5A5).all()


def test_a_call_larger_than_a_chunk(bound):
    """More rays than one chunk of the slab (pt_plan.h kRaycastChunk = 262144): the case's rays repeated, every
    copy's records the reference's, across the chunk boundary too."""
    name = "gltf_teapot"
    o, d, _ = C.rays_of(name)
    ref = C.reference(name)
    reps = 262144 // len(o) + 2
    got = bound(name).fx.cast_rays(np.tile(o, (reps, 1)), np.tile(d, (reps, 1)))
    assert len(got) > 262144 + len(o)
    assert np.array_equal(_words(got).reshape(reps, len(o), 16), np.broadcast_to(_words(ref), (reps, len(o), 16)))


# ------------------------------------------------------------------------------------------ the call among the draws

def _fresh(monkeypatch, meta, W, Hh, mesh):
    import babylon_pt as bp
    monkeypatch.setenv("PT_CONT", "1")            # compaction forced on at a small frame, no overlap lag:
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")     # tests/test_gpu_compaction.py's knobs
    e = bp.Engine(0)
    player = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh), W, Hh)
    e.resize_canvas(W, Hh)
    return e, player


def _frames(player, meta, draws=7):
    return meta["frames"] + [player.synth_frame(k) for k in range(draws - len(meta["frames"]))]


def test_a_query_between_draws_changes_no_draw(monkeypatch):
    """Seven frames with no sync between them (three frames in flight, late-bounce compaction on: pt_trace and pt_cont
    use the draws' spill slabs on the side streams) with a query after every path-tracing draw give the accumulation,
    the canvas and the record totals of the same frames without a query; the queries' records are the reference's;
    and no counter, pt_queue_stats, pt_cont_stats or pt_fuse_stats entry, nor pt_bvh_layout_used, moves at a query."""
    name = "gltf_teapot"
    meta, mesh = C._meta(C.CASES[name][0]), C.mesh_of(C.CASES[name][2])
    o, d, _ = C.rays_of(name)
    W, Hh = 160, 90
    out = {}
    for queries in (False, True):
        e, player = _fresh(monkeypatch, meta, W, Hh, mesh)
        try:
            fx = player.wrappers[H.path_call(meta["frames"][0])["effect"]].effect
            hits = []
            for calls in _frames(player, meta):
                player.play_call(calls[0])
                if queries:
                    hits.append(fx.cast_rays(o, d))
                player.play_call(calls[1])
                player.play_call(calls[2])
            e.sync()
            out[queries] = (player.textures["pathTracingRenderTarget"].read(), e.read_canvas(W, Hh), e.cont_stats())
            if queries:
                for h in hits:
                    _same("a query between draws", h, C.reference(name))
                e.set_counting(True)
                player.play_frame(1)
                e.sync()
                before = (e.counters(), e.queue_stats(), e.cont_stats(), e.fuse_stats(), e.bvh_layout_used())
                _same("a query after the draws", fx.cast_rays(o, d), C.reference(name))
                assert (e.counters(), e.queue_stats(), e.cont_stats(), e.fuse_stats(), e.bvh_layout_used()) == before
                assert before[0]["paths"] > 0 and before[4] == "pairs"
        finally:
            e.dispose()
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32)), "accumulation"
    assert np.array_equal(out[True][1], out[False][1]), "canvas"
    assert out[True][2] == out[False][2] and out[False][2][0] > 0, "records through pt_cont: %s / %s" % (out[True][2], out[False][2])


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_a_query_needs_no_draw_target_history_or_blue_noise(layout):
    """A fresh context, an effect with nothing bound but the two data textures, no draw: the first call of the
    context is the query (the child-pair records are built by it)."""
    import babylon_pt as bp
    name = "gltf_chain28"
    o, d, _ = C.rays_of(name)
    e = bp.Engine(0)
    try:
        e.set_bvh_layout(layout)
        u = C.uniforms_of(name)
        payload = H.texture_payloads(C._meta(C.CASES[name][0]), C.mesh_of(C.CASES[name][2]))
        wr = bp.EffectWrapper(e, "gltf", list(u.keys()), ["tAABBTexture", "tTriangleTexture"], "query")
        for uname, ent in u.items():
            wr.effect._set_entry(uname, ent)
        wr.effect.setTexture("tAABBTexture", bp.RawTexture.CreateRGBATexture(payload["bvh"], 2048, 2048, e, name="bvh"))
        wr.effect.setTexture("tTriangleTexture", bp.RawTexture.CreateRGBATexture(payload["tri"], 2048, 2048, e, name="tri"))
        _same("%s before any draw, %s" % (name, layout), wr.effect.cast_rays(o, d), C.reference(name))
    finally:
        e.dispose()


def test_a_texture_write_before_the_query_is_seen(engine, bound):
    """pt_write_pixels into the triangle texture, then the query: the records are the new mesh's."""
    import babylon_pt as bp
    name = "gltf_tiny2"
    o, d, _ = C.rays_of(name)
    b = bound(name)
    _same(name, b.fx.cast_rays(o, d), C.reference(name))
    mesh = C.mesh_of(C.CASES[name][2])
    flipped = dict(mesh, tri=mesh["tri"].copy())
    flipped["tri"][:, 0:9] = mesh["tri"][:, [0, 1, 2, 6, 7, 8, 3, 4, 5]]   # every triangle's winding turned
    raw = next(r for r, kind in b.meta["textures"].items() if kind == "tri")
    payload = H.texture_payloads(b.meta, flipped)["tri"]
    engine.check(bp.lib().pt_write_pixels(engine.ctx, b.player.textures[raw].handle, payload.ctypes.data, payload.nbytes), "pt_write_pixels")
    ref = R.cast("gltf", C.uniforms_of(name), o, d, flipped)
    assert not np.array_equal(ref["triangle"], C.reference(name)["triangle"])
    _same(name + " with its windings turned", b.fx.cast_rays(o, d), ref)


# ------------------------------------------------------------------------------------------ errors

def test_errors(engine, bound):
    import babylon_pt as bp
    L = bp.lib()
    o, d, _ = C.rays_of("cornell")
    o, d = np.ascontiguousarray(o[:4]), np.ascontiguousarray(d[:4])
    hits = np.zeros(4, R.RAY_HIT)
    fx = bound("cornell").fx
    args = (o.ctypes.data, d.ctypes.data, 4, hits.ctypes.data)
    assert L.pt_cast_rays(fx.handle, *args) == 0
    assert L.pt_cast_rays(None, *args) == -1                                           # a bad handle
    assert L.pt_cast_rays(fx.handle, o.ctypes.data, d.ctypes.data, -1, hits.ctypes.data) == -1
    for k in range(3):                                                                 # a NULL pointer with n > 0
        a = list(args)
        a[k if k < 2 else 3] = None
        assert L.pt_cast_rays(fx.handle, *a) == -1
    guard = hits.copy()
    assert L.pt_cast_rays(fx.handle, None, None, 0, None) == 0                         # n == 0 touches nothing
    assert L.pt_cast_rays(fx.handle, o.ctypes.data, d.ctypes.data, 0, hits.ctypes.data) == 0
    assert np.array_equal(_words(hits), _words(guard))
    for prog in ("screenCopy", "screenOutput"):                                        # not a path-tracing effect
        wr = bp.EffectWrapper(engine, prog, [], ["pathTracedImageBuffer", "accumulationBuffer"], prog)
        assert L.pt_cast_rays(wr.effect.handle, *args) == -1
        assert L.pt_cast_rays(wr.effect.handle, None, None, 0, None) == -1
    # a mesh program without its data textures: PT_ERR_STATE, whatever else is bound
    for scene in ("gltf", "hdri", "skymesh"):
        wr = bp.EffectWrapper(engine, scene, ["uGLTF_Model_InvMatrix"], ["tAABBTexture", "tTriangleTexture"], scene)
        with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
            wr.effect.cast_rays(o, d)
    b = bound("gltf_tiny1")
    b.fx.setTexture("tTriangleTexture", None)
    with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
        b.fx.cast_rays(o, d)
    with pytest.raises(ValueError):
        fx.cast_rays(o, d[:3])


def test_multi_part_context_is_unsupported():
    import babylon_pt as bp
    e = bp.Engine(devices=[0, 0])
    try:
        u = C.uniforms_of("cornell")
        wr = bp.EffectWrapper(e, "cornell", list(u.keys()), [], "query")
        o, d, _ = C.rays_of("cornell")
        with pytest.raises(bp.PtError, match="PT_ERR_UNSUPPORTED"):
            wr.effect.cast_rays(o[:4], d[:4])
        # (bad arguments are still bad arguments there, and no rays are no work)
        assert bp.lib().pt_cast_rays(wr.effect.handle, None, None, 4, None) == -1
        assert bp.lib().pt_cast_rays(wr.effect.handle, None, None, 0, None) == 0
    finally:
        e.dispose()


# ------------------------------------------------------------------------------------------ pick and autofocus

def test_pick_and_autofocus(bound):
    """The Cornell view's centre pixel: the record, and autofocus's distance, are the reference's for the ray the
    binding forms on the host; a sky pixel of the sky program is no distance."""
    b = bound("cornell", w=96, h=64)
    o, d = b.fx.camera_ray(48, 32, 96, 64)
    ref = R.cast("cornell", C.uniforms_of("cornell"), o[None], d[None])
    got = b.fx.pick(48, 32, 96, 64)
    _same("pick", np.array([got], R.RAY_HIT), ref)
    assert ref["object_id"][0] >= 0 and b.fx.autofocus(48, 32, 96, 64) == float(ref["t"][0])
    assert 50.0 < float(ref["t"][0]) < 250.0   # the view looks into the room from 120 in front of its centre
    sky = bound("sky", w=96, h=64)
    assert sky.fx.autofocus(48, 63, 96, 64) is None and sky.fx.pick(48, 63, 96, 64)["t"] == R.INF
    assert sky.fx.autofocus(48, 28, 96, 64) is not None   # a little below the horizon: the back wall, or what stands before it
