"""pt_cast_rays_ex (csrc/pt_raycast.hip pt_raycast_q) against the bounded reference (tests/raycast_bounded_ref.py):
the bounded closest hit bit for bit and the occlusion flag, on every case of tests/raycast_cases.py under all three
BVH layouts, with every t_max set of the CPU test carried by one call; ray counts around the wave size with guard
bytes behind the output; t_max = NULL against pt_cast_rays; the device route (torch tensors in and out, no sync, a
call beyond one chunk, a query between draws with three frames in flight); every error; line_of_sight.

Run on an MI355X: python -m pytest tests/test_gpu_raycast_bounded.py -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch   # loaded before libpt.so, as in tests/test_gpu_denoise.py: the device route needs both on one HIP runtime

import helpers as H
import raycast_bounded_ref as B
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
    """A case's scene on the engine with its uniforms and samplers set on the path-tracing effect, nothing drawn
    (tests/test_gpu_raycast.py's helper, copied)."""

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


def _all_sets(name):
    """The case's rays repeated once per given t_max set, the sets' bounds, and the bounded reference's records."""
    o, d, _ = C.rays_of(name)
    k = len(B.GIVEN)
    t = np.concatenate([B.t_max_of(name, w) for w in B.GIVEN])
    ref = np.concatenate([B.reference(name, w) for w in B.GIVEN])
    return np.tile(o, (k, 1)), np.tile(d, (k, 1)), t, ref


def _layouts(name):
    return C.LAYOUTS if name in C.MESH_CASES else ("pairs",)


# ------------------------------------------------------------------------------------------ every case, every layout

@pytest.mark.parametrize("name", list(C.CASES))
def test_bounded_closest_hit_bitexact_on_every_layout(engine, bound, name):
    """One call carries the eleven t_max arrays of the CPU test (NaN, +inf, 2e6, 1000000; 0, -1, t_ref, the float below
    it, half of it; one and a half of it; the float above it), the rays repeated: every field of every record is the
    bounded reference's (`normal` excepted on the bump-mapped cases, compared between the layouts instead), the
    three layouts give each other's records, and the rays pinned at one ulp are misses on the device."""
    o, d, t, ref = _all_sets(name)
    b = bound(name)
    skip = ("normal",) if name in C.BUMPED else ()
    got = {}
    for layout in _layouts(name):
        engine.set_bvh_layout(layout)
        got[layout] = b.fx.cast_rays(o, d, t)
        _same("%s, %s" % (name, layout), got[layout], ref, skip)
    for layout in _layouts(name)[1:]:
        _same("%s, %s against %s" % (name, layout, C.LAYOUTS[0]), got[layout], got[C.LAYOUTS[0]])
    n = len(C.rays_of(name)[0])
    at = B.GIVEN.index("above_t_ref") * n
    for i in B.ONE_ULP_CULLED.get(name, {}):
        for layout in _layouts(name):
            r = got[layout][at + i]
            assert r["object_id"] == -1 and r["t"] == R.INF and r["triangle"] == -1, (layout, i, r)
            assert C.reference(name)["triangle"][i] >= 0
    # the sets did what they are for: the all-miss ones miss, the others hit
    hits = (got[_layouts(name)[0]]["object_id"] >= 0).reshape(len(B.GIVEN), n).sum(1)
    for k, which in enumerate(B.GIVEN):
        assert (hits[k] == 0) == (which in B.ALL_MISS), (which, hits[k])


@pytest.mark.parametrize("name", list(C.CASES))
def test_occluded_flags_on_every_layout(engine, bound, name):
    """The same inputs in the occlusion mode: the flags are object_id >= 0 of the bounded reference on all three
    layouts (the pairs walk stops at the first occluder, the other two run the bounded closest walk), and the
    bytes are exactly 0 or 1. Without a bound the flags are those of the unbounded reference."""
    import babylon_pt as bp
    o, d, t, ref = _all_sets(name)
    b = bound(name)
    oo, dd, _ = C.rays_of(name)
    for layout in _layouts(name):
        engine.set_bvh_layout(layout)
        raw = b.fx._cast_host(o, d, t, bp.RAYS_OCCLUDED)
        assert raw.dtype == np.uint8 and set(np.unique(raw).tolist()) <= {0, 1}, layout
        bad = np.nonzero(raw != B.occluded(ref).astype(np.uint8))[0]
        assert bad.size == 0, "%s, %s: flags differ on rays %s" % (name, layout, bad.tolist()[:10])
        flags = b.fx.occluded(oo, dd)
        assert flags.dtype == np.bool_ and np.array_equal(flags, B.occluded(C.reference(name))), layout
    assert 0 < B.occluded(ref).sum() < len(ref)


# ------------------------------------------------------------------------------------------ ray counts and guards

@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ray_counts_around_the_wave_size(engine, bound, n):
    """n rays with the mesh hits last, in the tail lanes of the last wave, bounded at 1.5 t_ref (and every third ray,
    from the second on, at 0.5 t_ref: a miss), through the C ABI: the records and the flags are the reference's by index, and the guard
    record / guard bytes behind output n - 1 stay as they were."""
    import babylon_pt as bp
    name = "gltf_teapot"
    o, d, _ = C.rays_of(name)
    ref = C.reference(name)
    mesh = np.nonzero(ref["triangle"] >= 0)[0]
    rest = np.nonzero(ref["triangle"] < 0)[0]
    k = min(n, 7)
    idx = np.concatenate([np.resize(rest, n - k), mesh[:k]])
    near = (np.arange(n) % 3 == 1)
    want = np.where(near, B.reference(name, "half")[idx], B.reference(name, "one_and_a_half")[idx])
    t = np.ascontiguousarray(np.where(near, B.t_max_of(name, "half")[idx], B.t_max_of(name, "one_and_a_half")[idx]), np.float32)
    assert (want["triangle"][-k:][~near[-k:]] >= 0).all() and (want["object_id"][near] < 0).all()
    oo, dd = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    b = bound(name)
    L = bp.lib()
    for layout in C.LAYOUTS:
        engine.set_bvh_layout(layout)
        buf = np.full((n + 1) * 16, 0xA5A5A5A5, np.uint32)
        q = bp.RayQuery(oo.ctypes.data, dd.ctypes.data, t.ctypes.data, buf.ctypes.data, n, bp.RAYS_CLOSEST, bp.RAYS_HOST)
        engine.check(L.pt_cast_rays_ex(b.fx.handle, ctypes.byref(q)), "pt_cast_rays_ex")
        assert np.array_equal(buf[:n * 16].reshape(n, 16), _words(want)), layout
        assert (buf[n * 16:] == 0xA5A5A5A5).all(), layout
        flags = np.full(n + 64, 0xA5, np.uint8)
        q = bp.RayQuery(oo.ctypes.data, dd.ctypes.data, t.ctypes.data, flags.ctypes.data, n, bp.RAYS_OCCLUDED, bp.RAYS_HOST)
        engine.check(L.pt_cast_rays_ex(b.fx.handle, ctypes.byref(q)), "pt_cast_rays_ex")
        assert np.array_equal(flags[:n], B.occluded(want).astype(np.uint8)) and (flags[n:] == 0xA5).all(), layout


@pytest.mark.parametrize("name", ["cornell", "gltf_teapot"])
def test_no_bound_through_the_query_is_pt_cast_rays(bound, name):
    """t_max = NULL through pt_cast_rays_ex: pt_cast_rays' records on the same rays, bit for bit."""
    import babylon_pt as bp
    o, d, _ = C.rays_of(name)
    b = bound(name)
    plain = b.fx.cast_rays(o, d)   # (the binding sends t_max = None to pt_cast_rays; the query goes through the C ABI)
    oo, dd = np.ascontiguousarray(o), np.ascontiguousarray(d)
    out = np.zeros(len(o), R.RAY_HIT)
    q = bp.RayQuery(oo.ctypes.data, dd.ctypes.data, None, out.ctypes.data, len(o), bp.RAYS_CLOSEST, bp.RAYS_HOST)
    b.fx.engine.check(bp.lib().pt_cast_rays_ex(b.fx.handle, ctypes.byref(q)), "pt_cast_rays_ex")
    _same(name, out, plain)
    _same(name + " against the reference", out, C.reference(name))


# ------------------------------------------------------------------------------------------ the device route

def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", ["cornell", "gltf_teapot"])
def test_device_route_gives_the_host_routes_bytes(engine, bound, name):
    """torch tensors in and out, closest hit and occlusion, with and without t_max, on every layout: the host route's
    bytes, and the tensors holding the rays are unchanged afterwards."""
    import babylon_pt as bp
    o, d, t, _ = _all_sets(name)
    b = bound(name)
    to, td, tt = _dev(o), _dev(d), _dev(t)
    for layout in _layouts(name):
        engine.set_bvh_layout(layout)
        for bounds, tb in ((None, None), (t, tt)):
            rec = b.fx.cast_rays(to, td, tb)
            occ = b.fx.occluded(to, td, tb)
            assert rec.dtype == torch.float32 and tuple(rec.shape) == (len(o), 16) and rec.device == to.device
            assert occ.dtype == torch.uint8 and tuple(occ.shape) == (len(o),)
            engine.sync()
            _same("%s, %s, records" % (name, layout), bp.ray_hits(rec), b.fx.cast_rays(o, d, bounds))
            assert np.array_equal(occ.cpu().numpy(), b.fx._cast_host(o, d, bounds, bp.RAYS_OCCLUDED)), (layout, bounds is None)
    engine.sync()
    for dev, host in ((to, o), (td, d), (tt, t)):
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32))


def test_device_route_beyond_one_chunk(bound):
    """One device call of more than 262,144 rays (pt_plan.h kRaycastChunk), the case's rays tiled, bounded at the
    float above t_ref and at half of it by turns: every copy's records and flags are the reference's, across the
    chunk boundary too."""
    import babylon_pt as bp
    name = "gltf_teapot"
    o, d, _ = C.rays_of(name)
    n = len(o)
    reps = 262144 // n + 2
    odd = (np.arange(reps) % 2 == 1)[:, None]
    t = np.where(odd, B.t_max_of(name, "half")[None], B.t_max_of(name, "above_t_ref")[None]).astype(np.float32).reshape(-1)
    want = np.where(odd, B.reference(name, "half")[None], B.reference(name, "above_t_ref")[None])
    b = bound(name)
    to, td, tt = _dev(np.tile(o, (reps, 1))), _dev(np.tile(d, (reps, 1))), _dev(t)
    rec = b.fx.cast_rays(to, td, tt)
    occ = b.fx.occluded(to, td, tt)
    b.fx.engine.sync()
    got = bp.ray_hits(rec)
    assert len(got) > 262144 + n
    assert np.array_equal(_words(got).reshape(reps, n, 16), _words(want.reshape(-1)).reshape(reps, n, 16))
    assert np.array_equal(occ.cpu().numpy().reshape(reps, n), B.occluded(want).astype(np.uint8))
    assert np.array_equal(to.cpu().numpy().view(np.uint32).reshape(reps, n, 3), np.broadcast_to(o.view(np.uint32), (reps, n, 3)))


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


def test_a_device_query_between_draws_changes_no_draw(monkeypatch):
    """tests/test_gpu_raycast.py's method on the device route: seven frames with no sync between them (three frames
    in flight, late-bounce compaction on) with a bounded device query and a device occlusion query after every
    path-tracing draw give the accumulation, the canvas and the record totals of the same frames without them; the
    queries' outputs are the reference's; and no counter or statistic moves at a query."""
    import babylon_pt as bp
    name = "gltf_teapot"
    meta, mesh = C._meta(C.CASES[name][0]), C.mesh_of(C.CASES[name][2])
    o, d, _ = C.rays_of(name)
    t = B.t_max_of(name, "one_and_a_half")
    want = B.reference(name, "one_and_a_half")
    to, td, tt = _dev(o), _dev(d), _dev(t)
    W, Hh = 160, 90
    out = {}
    for queries in (False, True):
        e, player = _fresh(monkeypatch, meta, W, Hh, mesh)
        try:
            fx = player.wrappers[H.path_call(meta["frames"][0])["effect"]].effect
            recs, occs = [], []
            for calls in _frames(player, meta):
                player.play_call(calls[0])
                if queries:
                    recs.append(fx.cast_rays(to, td, tt))
                    occs.append(fx.occluded(to, td))
                player.play_call(calls[1])
                player.play_call(calls[2])
            e.sync()
            out[queries] = (player.textures["pathTracingRenderTarget"].read(), e.read_canvas(W, Hh), e.cont_stats())
            if queries:
                for r, f in zip(recs, occs):
                    _same("a device query between draws", bp.ray_hits(r), want)
                    assert np.array_equal(f.cpu().numpy(), B.occluded(C.reference(name)).astype(np.uint8))
                e.set_counting(True)
                player.play_frame(1)
                e.sync()
                before = (e.counters(), e.queue_stats(), e.cont_stats(), e.fuse_stats(), e.bvh_layout_used())
                r, f = fx.cast_rays(to, td, tt), fx.occluded(to, td, tt)
                e.sync()
                _same("a device query after the draws", bp.ray_hits(r), want)
                assert np.array_equal(f.cpu().numpy(), B.occluded(want).astype(np.uint8))
                assert (e.counters(), e.queue_stats(), e.cont_stats(), e.fuse_stats(), e.bvh_layout_used()) == before
                assert before[0]["paths"] > 0 and before[4] == "pairs"
        finally:
            e.dispose()
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32)), "accumulation"
    assert np.array_equal(out[True][1], out[False][1]), "canvas"
    assert out[True][2] == out[False][2] and out[False][2][0] > 0, "records through pt_cont: %s / %s" % (out[True][2], out[False][2])


# ------------------------------------------------------------------------------------------ errors

def test_errors(engine, bound):
    import babylon_pt as bp
    L = bp.lib()
    o, d, _ = C.rays_of("cornell")
    o, d = np.ascontiguousarray(o[:4]), np.ascontiguousarray(d[:4])
    t = np.full(4, 50.0, np.float32)
    hits = np.zeros(4, R.RAY_HIT)
    fx = bound("cornell").fx

    def call(handle, origins=o.ctypes.data, dirs=d.ctypes.data, t_max=t.ctypes.data, out=hits.ctypes.data, n=4,
             mode=bp.RAYS_CLOSEST, memory=bp.RAYS_HOST):
        q = bp.RayQuery(origins, dirs, t_max, out, n, mode, memory)
        return L.pt_cast_rays_ex(handle, ctypes.byref(q))

    assert call(fx.handle) == 0
    assert call(None) == -1                                                    # a bad handle
    assert L.pt_cast_rays_ex(fx.handle, None) == -1                            # a NULL query
    assert call(fx.handle, n=-1) == -1
    assert call(fx.handle, origins=None) == -1 and call(fx.handle, dirs=None) == -1 and call(fx.handle, out=None) == -1
    assert call(fx.handle, t_max=None) == 0                                    # (no bound is no error)
    for mode in (-1, 2):
        assert call(fx.handle, mode=mode) == -1
    for memory in (-1, 2):
        assert call(fx.handle, memory=memory) == -1
    guard = hits.copy()
    assert call(fx.handle, origins=None, dirs=None, t_max=None, out=None, n=0) == 0   # n == 0 touches nothing
    assert call(fx.handle, n=0) == 0
    assert np.array_equal(_words(hits), _words(guard))
    for prog in ("screenCopy", "screenOutput"):                                # not a path-tracing effect
        wr = bp.EffectWrapper(engine, prog, [], ["pathTracedImageBuffer", "accumulationBuffer"], prog)
        assert call(wr.effect.handle) == -1
        assert call(wr.effect.handle, origins=None, dirs=None, t_max=None, out=None, n=0) == -1
    # a mesh program without its data textures: PT_ERR_STATE
    for scene in ("gltf", "hdri", "skymesh"):
        wr = bp.EffectWrapper(engine, scene, ["uGLTF_Model_InvMatrix"], ["tAABBTexture", "tTriangleTexture"], scene)
        with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
            wr.effect.cast_rays(o, d, t)
        with pytest.raises(bp.PtError, match="PT_ERR_STATE"):
            wr.effect.occluded(o, d)
    # the device route's alignment: a record tensor offset by 4 bytes, rays and bounds offset by 2
    to, td, tt = _dev(o), _dev(d), _dev(t)
    rec = torch.zeros(4 * 16 + 4, dtype=torch.float32, device="cuda:0")
    flags = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ok = dict(origins=to.data_ptr(), dirs=td.data_ptr(), t_max=tt.data_ptr(), out=rec.data_ptr(), memory=bp.RAYS_DEVICE)
    assert rec.data_ptr() % 16 == 0 and call(fx.handle, **ok) == 0
    assert call(fx.handle, **dict(ok, out=rec.data_ptr() + 4)) == -1
    assert call(fx.handle, **dict(ok, out=flags.data_ptr() + 1, mode=bp.RAYS_OCCLUDED)) == 0   # (flags are bytes)
    for k in ("origins", "dirs", "t_max"):
        assert call(fx.handle, **dict(ok, **{k: ok[k] + 2})) == -1
    engine.sync()
    assert np.array_equal(rec.cpu().numpy()[:64].view(np.uint32).reshape(4, 16), _words(fx.cast_rays(o, d, t)))
    assert not rec.cpu().numpy()[64:].any() and flags.cpu().numpy()[5:].sum() == 0
    # the binding's own checks
    with pytest.raises(ValueError):
        fx.cast_rays(o, d[:3], t)
    with pytest.raises(ValueError):
        fx.cast_rays(o, d, t[:3])
    with pytest.raises(ValueError):
        fx.cast_rays(to, td.double())                                          # not float32
    with pytest.raises(ValueError):
        fx.cast_rays(_dev(np.zeros((3, 4), np.float32)).t(), td)              # not contiguous
    with pytest.raises(ValueError):
        fx.occluded(to, d)                                                     # a tensor and an array
    with pytest.raises(ValueError):
        fx.cast_rays(to.cpu(), td.cpu())                                       # tensors of another device


def test_multi_part_context_is_unsupported():
    import babylon_pt as bp
    e = bp.Engine(devices=[0, 0])
    try:
        u = C.uniforms_of("cornell")
        wr = bp.EffectWrapper(e, "cornell", list(u.keys()), [], "query")
        o, d, _ = C.rays_of("cornell")
        with pytest.raises(bp.PtError, match="PT_ERR_UNSUPPORTED"):
            wr.effect.cast_rays(o[:4], d[:4], 10.0)
        with pytest.raises(bp.PtError, match="PT_ERR_UNSUPPORTED"):
            wr.effect.occluded(o[:4], d[:4])
        with pytest.raises(bp.PtError, match="PT_ERR_UNSUPPORTED"):
            wr.effect.occluded(_dev(o[:4]), _dev(d[:4]))
        q = bp.RayQuery(None, None, None, None, 4, bp.RAYS_OCCLUDED, bp.RAYS_HOST)   # (bad arguments stay bad arguments)
        assert bp.lib().pt_cast_rays_ex(wr.effect.handle, ctypes.byref(q)) == -1
        q = bp.RayQuery(None, None, None, None, 0, bp.RAYS_OCCLUDED, bp.RAYS_HOST)
        assert bp.lib().pt_cast_rays_ex(wr.effect.handle, ctypes.byref(q)) == 0
    finally:
        e.dispose()


# ------------------------------------------------------------------------------------------ line of sight

def _expect_los(name, p, q, t_max=1.0):
    key = C.CASES[name][2]
    p, q = np.asarray(p, np.float32).reshape(-1, 3), np.asarray(q, np.float32).reshape(-1, 3)
    rec = B.cast(C.scene_of(name), C.uniforms_of(name), p, q - p, np.full(len(p), t_max, np.float32),
                 C.mesh_of(key) if key is not None else None)
    return ~B.occluded(rec)


def test_line_of_sight_in_the_cornell_room(bound):
    """A segment between two points of open air (the first half of a camera ray's way to the left sphere); one through
    that sphere (from 5 in front of the ray's hit to 40 behind it: the sphere's radius is 16); one ending 1 % short of
    the back wall and one ending 1 % beyond it. The expectations are the bounded reference's - and are what the
    geometry says."""
    name = "cornell"
    b = bound(name)
    o, d, _ = C.rays_of(name)
    ref = C.reference(name)
    i = int(np.nonzero(ref["object_id"] == 0)[0][0])          # a camera ray that hits the left sphere
    hit = o[i] + d[i] * ref["t"][i]
    step = d[i] / np.linalg.norm(d[i])
    j = int(np.nonzero(ref["object_id"] == 2)[0][0])          # ... and one that hits the back wall (the first quad)
    wall = o[j].astype(np.float64) + d[j].astype(np.float64) * float(ref["t"][j])
    eye = o[j].astype(np.float64)
    p = np.array([o[i], hit - step * 5.0, eye, eye], np.float32)
    q = np.array([o[i] + d[i] * ref["t"][i] * 0.5, hit + step * 40.0, eye + (wall - eye) * 0.99, eye + (wall - eye) * 1.01], np.float32)
    want = _expect_los(name, p, q)
    assert want.tolist() == [True, False, True, False]
    got = b.fx.line_of_sight(p, q)
    assert got.dtype == np.bool_ and got.tolist() == want.tolist()
    # a shorter segment through t_max: the one that ran into the wall stops short of it
    assert b.fx.line_of_sight(p[3:], q[3:], 0.9).tolist() == _expect_los(name, p[3:], q[3:], 0.9).tolist() == [True]


def test_line_of_sight_past_and_through_the_teapot(engine, bound):
    """A segment through the teapot's body (along a ray aimed at a triangle's interior, to 5 % beyond the hit) and one
    past it (an axis-parallel ray through the model's box that misses the mesh, half way to the wall it hits), on
    every layout."""
    name = "gltf_teapot"
    b = bound(name)
    o, d, kinds = C.rays_of(name)
    ref = C.reference(name)
    a, e = kinds["interior"]
    i = a + int(np.nonzero(ref["triangle"][a:e] >= 0)[0][0])
    a, e = kinds["axis"]
    j = a + int(np.nonzero((ref["triangle"][a:e] < 0) & (ref["object_id"][a:e] >= 0))[0][0])
    p = np.array([o[i], o[j]], np.float32)
    q = np.array([o[i] + d[i] * ref["t"][i] * 1.05, o[j] + d[j] * ref["t"][j] * 0.5], np.float32)
    want = _expect_los(name, p, q)
    assert want.tolist() == [False, True]
    for layout in C.LAYOUTS:
        engine.set_bvh_layout(layout)
        assert b.fx.line_of_sight(p, q).tolist() == want.tolist(), layout
