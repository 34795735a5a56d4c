"""Late-bounce compaction (pt_trace<P,false,true> -> pt_cont_offsets / pt_cont_scatter -> pt_cont) at small
frames: every mesh program, material and BVH layout, the ends of its knobs, frames smaller than a wave,
band partitions that own nothing, a resize with draws in flight, and the auto trial under a moving camera.

Every case is bit-exact against the CPU oracle (RGBA32F accumulation compared as uint32, canvas bytes), and
pt_cont_stats proves that path records really went through pt_cont. The scaffold of a case: a fresh engine
with the case's environment, the stream's recorded frames plus enough still-camera frames that every
buffer set comes round at least twice, no sync between frames, one read of the accumulation right after a
mid-stream path-tracing draw; that read, the last accumulation and the last canvas are compared.

Run on an MI355X: python -m pytest tests/test_gpu_compaction.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
from helpers import _with_material

pytestmark = pytest.mark.gpu

MESH_SCENES = ("gltf", "hdri", "skymesh")


def _bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def _diff_report(a, b):
    if a.shape != b.shape:
        return "shapes %s / %s" % (a.shape, b.shape)
    bad = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
    pix = bad.reshape(bad.shape[0], bad.shape[1], -1).any(-1)
    ys, xs = np.nonzero(pix)
    first = (int(xs[0]), int(ys[0])) if len(xs) else None
    return "mismatching pixels %d / %d, first (x,y)=%s" % (pix.sum(), pix.size, first)


def _exposure(out_uniforms):
    return out_uniforms.get("uToneMappingExposure", ["f", [0.0]])[1][0]


def _still(frames):
    """The frames whose camera stands still: the draws that compact (a moving-camera draw runs alone)."""
    return sum(1 for f in frames if H.path_call(f)["uniforms"]["uCameraIsMoving"][1][0] == 0)


_REF = {}


def _oracle(key, meta, frames, W, Hh, mesh=None, maps=None, keep=()):
    """The oracle over `frames` at W x H from a zero history: the accumulations after the frames in `keep`
    and after the last one, the last canvas, its RGBA32F screenOutput, and the counters' totals. Cached by
    `key`: cases that differ only in how the GPU schedules the same frames share one replay."""
    import ptoracle as po
    k = (key, len(frames), W, Hh, tuple(sorted(keep)))
    if k not in _REF:
        sc = H.oracle_scene(meta, W, Hh, mesh, maps)
        acc = np.zeros((Hh, W, 4), np.float32)
        accs, total = {}, {}
        last = len(frames) - 1
        for i, f in enumerate(frames):
            acc, cnt = sc.path_trace(H.with_resolution(H.path_call(f)["uniforms"], W, Hh), acc)
            for name, v in cnt.items():
                total[name] = total.get(name, 0) + v
            if i in keep or i == last:
                accs[i] = acc.copy()
        ou = H.output_call(frames[-1])["uniforms"]
        inv = ou["uOneOverSampleCounter"][1][0]
        _REF[k] = {"acc": accs, "can": po.screen_output(acc, inv, _exposure(ou)),
                   "f32": po.screen_output_f32(acc, inv, _exposure(ou)), "counters": total}
    return _REF[k]


def _player(e, meta, W, Hh, mesh=None, maps=None):
    import babylon_pt as bp
    payload = None
    if meta["scene"] in MESH_SCENES:
        payload = H.texture_payloads(meta, mesh if mesh is not None else H.mesh(meta))
    player = bp.StreamPlayer(e, meta, H.bluenoise(), payload, W, Hh)
    if maps:
        for kind, sampler in H.PBR_SAMPLERS.items():
            player.textures[sampler] = bp.Texture(e, maps[kind], name=kind)
    e.resize_canvas(W, Hh)
    return player


def _issue(e, player, calls, parts, traced=None):
    """One frame's draws (`traced` is called after its path tracing); with parts > 1 every part traces its
    bands into the same targets, the copy is full-frame and screenOutput goes band by band under the output
    partition."""
    assert [c["shader"][:-len("FragmentShader")] for c in calls] == ["pathTracing", "screenCopy", "screenOutput"]
    if parts == 1:   # (a multi-part context partitions its rows itself)
        player.play_call(calls[0])
    else:
        for p in range(parts):
            e.set_row_partition(parts, p)
            player.play_call(calls[0])
        e.set_row_partition(1, 0)
    if traced:
        traced()
    player.play_call(calls[1])
    if parts == 1:
        player.play_call(calls[2])
        return
    e.set_output_partition(True)
    for p in range(parts):
        e.set_row_partition(parts, p)
        player.play_call(calls[2])
    e.set_output_partition(False)
    e.set_row_partition(1, 0)


def _draw(e, player, frames, mid, parts=1, data_error=False, f32=False):
    """The scaffold's draws: every frame with no sync between them, the accumulation read right after frame
    `mid`'s path-tracing draw, then the last accumulation and canvas (and, for f32, the last screenOutput
    drawn once more into an RGBA32F target)."""
    import babylon_pt as bp
    got = {}

    def read_mid():
        got["mid"] = player.textures["pathTracingRenderTarget"].read()

    for i, calls in enumerate(frames):
        _issue(e, player, calls, parts, read_mid if i == mid else None)
    if data_error:   # reported by the first sync, once
        with pytest.raises(bp.PtError, match="PT_ERR_DATA"):
            e.sync()
    e.sync()
    got["acc"] = player.textures["pathTracingRenderTarget"].read()
    got["can"] = e.read_canvas(player.width, player.height)
    if f32:
        player.textures["outputF32"] = bp.RenderTargetTexture("outputF32", (player.width, player.height), e)
        player.play_call(dict(H.output_call(frames[-1]), target="outputF32"))
        e.sync()
        got["f32"] = player.textures["outputF32"].read()
    return got


def _compare(what, got, ref, mid):
    if "mid" in got:
        assert _bits_equal(ref["acc"][mid], got["mid"]), "%s: accumulation read after frame %d's path tracing: %s" % (
            what, mid, _diff_report(ref["acc"][mid], got["mid"]))
    last = max(ref["acc"])
    assert _bits_equal(ref["acc"][last], got["acc"]), "%s: last accumulation: %s" % (what, _diff_report(ref["acc"][last], got["acc"]))
    assert _bits_equal(ref["can"], got["can"]), "%s: last canvas: %s" % (what, _diff_report(ref["can"], got["can"]))
    if "f32" in got:
        assert _bits_equal(ref["f32"], got["f32"]), "%s: RGBA32F screenOutput: %s" % (what, _diff_report(ref["f32"], got["f32"]))


def _run(monkeypatch, key, meta, W, Hh, env=None, mesh=None, maps=None, layout="pairs", draws=7, parts=1,
         data_error=False, f32=False, devices=None):
    """A case on a fresh engine (`devices`: a multi-part context) with compaction forced on and no overlap
    lag (unless `env` says otherwise): returns what the engine reported, the oracle's reference and the
    frames."""
    import babylon_pt as bp
    monkeypatch.setenv("PT_CONT", "1")
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    e = bp.Engine(0) if devices is None else bp.Engine(devices=devices)
    try:
        e.set_bvh_layout(layout)
        player = _player(e, meta, W, Hh, mesh, maps)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(draws - len(meta["frames"]))]
        mid = len(frames) - 3
        got = _draw(e, player, frames, mid, parts, data_error, f32)
        # (pt_queue_stats describes one part's last draw: not asked of a multi-part context)
        rep = {"qs": e.queue_stats() if devices is None else {"late_bounce_compaction": None},
               "cs": e.cont_stats(), "layout": e.bvh_layout_used(), "frames": frames}
    finally:
        e.dispose()
    print("%s %dx%d: (records stored, draws with pt_cont) = %s of %d still frames, %s" % (
        key, W, Hh, rep["cs"], _still(frames), rep["qs"]["late_bounce_compaction"]))
    ref = _oracle(key, meta, frames, W, Hh, mesh, maps, keep={mid})
    _compare(key, got, ref, mid)
    return rep, ref


def _assert_compacted(rep, W, Hh, bands=1):
    """The draws compacted, and records went through pt_cont: every still-camera draw (of every partition
    that owns rows) launched it, and they stored some records, at most one per traced pixel and draw."""
    still = _still(rep["frames"])
    stored, launched = rep["cs"]
    assert rep["qs"]["late_bounce_compaction"] == "on", rep["qs"]
    assert still > 0 and launched == still * bands, (rep["cs"], still)
    assert rep["qs"]["compacting_draws"] == launched
    assert 0 < stored <= W * Hh * still, rep["cs"]


# ------------------------------------------------------------------ programs x materials x layouts

_CACHE = {}


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _small_dragon():
    return _cached("dragon64", lambda: H.synthetic_dragon(64, 64))


@pytest.mark.parametrize("layout", ["pairs", "trail", "reference"])
@pytest.mark.parametrize("material", [1, 2, 3, 4])
def test_teapot_materials_layouts_compacted(monkeypatch, material, layout):
    """The glTF teapot at 160x90 as Diffuse, Transparent (double-sided leaves), Metal and ClearCoat on each
    BVH layout: `reference` compacts without the record sort (no root box of child pairs)."""
    meta = _with_material(H.stream("gltf_teapot_320x180"), material)
    rep, _ = _run(monkeypatch, "teapot-m%d" % material, meta, 160, 90, layout=layout)
    assert rep["layout"] == layout
    _assert_compacted(rep, 160, 90)


@pytest.mark.parametrize("layout", ["pairs", "trail", "reference"])
@pytest.mark.parametrize("name", ["hdri_helmet_320x180", "gltf_helmet_320x180"])
def test_helmet_with_maps_compacted(monkeypatch, name, layout):
    """The textured program variants (kHasTex): the DamagedHelmet with seeded PBR maps bound - every
    material branch of the PBR decode - at 203x117, in the HDRI and the glTF scene."""
    maps = _cached("maps", H.synthetic_pbr_maps)
    rep, _ = _run(monkeypatch, name, H.stream(name), 203, 117, maps=maps, layout=layout)
    assert rep["layout"] == layout
    _assert_compacted(rep, 203, 117)


@pytest.mark.parametrize("material,layout", [(1, "pairs"), (2, "pairs"), (3, "pairs"), (4, "pairs"),
                                             (3, "trail"), (3, "reference")])
def test_sky_small_dragon_compacted(monkeypatch, material, layout):
    """The sky + mesh composite over an 8,192-triangle dragon stand-in at 160x90, every model material."""
    rep, _ = _run(monkeypatch, "sky-m%d" % material, H.sky_mesh_stream(material), 160, 90, mesh=_small_dragon(),
                  layout=layout)
    assert rep["layout"] == layout
    _assert_compacted(rep, 160, 90)


@pytest.mark.parametrize("layout,used", [("pairs", "pairs"), ("trail", "pairs"), ("reference", "reference")])
def test_bookcase_compacted(monkeypatch, layout, used):
    """The bookcase (150 merged meshes, NaN UVs, a 41-level tree that the restart trail cannot walk, so
    `trail` keeps `pairs`) under the teapot stream at 160x90."""
    rep, ref = _run(monkeypatch, "bookcase", H.stream("gltf_teapot_320x180"), 160, 90, mesh=H.mesh("bookcase"),
                    layout=layout)
    assert rep["layout"] == used
    assert ref["counters"]["hit_lookups"] > 0
    _assert_compacted(rep, 160, 90)


def test_stack_overflow_compacted(monkeypatch):
    """A tree whose walks nest deeper than stackLevels[28], walked by pt_trace and by pt_cont: the dropped
    pushes are the oracle's, the first sync reports PT_ERR_DATA once, and the accumulation is exact."""
    mesh = _cached("knot", lambda: H.synthetic_dragon(128, 128, knot=(2, 3), tube=3.2))
    rep, ref = _run(monkeypatch, "overflow", H.stream("gltf_bunny_1080p"), 160, 90, mesh=mesh, data_error=True)
    assert ref["counters"]["stack_overflow"] > 0
    assert rep["layout"] == "pairs"
    _assert_compacted(rep, 160, 90)


def test_malformed_links_compacted(monkeypatch):
    """Right-child links that are no exact integers cannot be re-packed: the draws fall back to the
    reference walk, compact without the sort, and stay exact."""
    meta = H.stream("gltf_teapot_320x180")
    mesh = H.mesh(meta)
    bvh = mesh["bvh"].copy()
    inner = np.nonzero(bvh[:, 0] < 0)[0]
    bvh[inner[3], 4] += 0.5
    bvh[inner[7], 4] = -3.0
    rep, _ = _run(monkeypatch, "malformed", meta, 160, 90, mesh=dict(mesh, bvh=bvh))
    assert rep["layout"] == "reference"
    _assert_compacted(rep, 160, 90)


def _flat_model():
    """Two triangles in the plane y = 5 that face the teapot stream's camera (it looks up at them from
    y = -20): the model's root box has no height, so the record sort's cell size on that axis is 0."""
    import babylon_pt as bp
    P = np.array([[-30.0, 5.0, -20.0], [30.0, 5.0, -20.0], [30.0, 5.0, 20.0], [-30.0, 5.0, 20.0]])
    tri = np.zeros((2, 32), np.float32)
    for i, t in enumerate(([0, 1, 2], [0, 2, 3])):
        p = P[t]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        tri[i, 0:9] = p.reshape(9)
        tri[i, 9:18] = np.tile(n / np.linalg.norm(n), 3)
        tri[i, 18:24] = -1.0
    p32 = tri[:, 0:9].reshape(2, 3, 3)
    lo, hi = p32.min(1), p32.max(1)
    return {"bvh": bp.bvh_build(np.concatenate([lo, hi, (lo + hi) * 0.5], 1).astype(np.float32)), "tri": tri}


def test_flat_model_compacted(monkeypatch):
    mesh = _flat_model()
    assert mesh["bvh"][0, 2] == mesh["bvh"][0, 6] == 5.0     # the root box: min.y == max.y
    rep, ref = _run(monkeypatch, "flat", H.stream("gltf_teapot_320x180"), 160, 90, mesh=mesh)
    assert rep["layout"] == "pairs"
    assert ref["counters"]["hit_lookups"] > 1000              # the model fills part of the view
    _assert_compacted(rep, 160, 90)


# ------------------------------------------------------------------------------------- knob edges

_ENDS = {
    "lanes-1": {"PT_CONT_LANES": "1"},
    "lanes-64": {"PT_CONT_LANES": "64"},
    "refill-1": {"PT_CONT_REFILL": "1"},
    "refill-64": {"PT_CONT_REFILL": "64"},
    "bounce-5": {"PT_CONT_BOUNCE": "5"},
    "bounce-7": {"PT_CONT_BOUNCE": "7"},            # no path loops that long: pt_cont runs on an empty queue
    "waves-1": {"PT_CONT_WAVES": "1"},
    "waves-3": {"PT_CONT_WAVES": "3"},
    "stored-order": {"PT_CONT_SORT": "0"},
    "grid-1": {"PT_CONT_SORT_GRID": "1"},
    "grid-3": {"PT_CONT_SORT_GRID": "3"},
    "depth-6-lag-6": {"PT_OVERLAP_DEPTH": "6", "PT_OVERLAP_LAG": "6"},
    "depth-2": {"PT_OVERLAP_DEPTH": "2", "PT_OVERLAP_LAG": "0"},
    "serial": {"PT_OVERLAP": "0"},
    # the longest single queue: every lane stores at bounce 2, one wave takes the records one at a time
    "one-long-queue": {"PT_CONT_LANES": "64", "PT_CONT_REFILL": "1", "PT_CONT_WAVES": "1"},
}
_STORED = {}


def _knob_case(monkeypatch, case):
    env = _ENDS[case]
    sets = int(env.get("PT_OVERLAP_DEPTH", "3")) + int(env.get("PT_OVERLAP_LAG", "0"))
    draws = 2 * sets + 1                      # every buffer set twice
    rep, _ = _run(monkeypatch, "knobs", H.stream("gltf_teapot_320x180"), 203, 117, env=env, draws=draws)
    _STORED[case] = rep["cs"][0]
    return rep


@pytest.mark.parametrize("case", list(_ENDS))
def test_knob_ends_compacted(monkeypatch, case):
    """The ends of pt_cont's knobs and of the frames in flight on one scene, the teapot at 203x117 on
    `pairs`: they change which paths are stored, who runs them and in what order, never a bit."""
    rep = _knob_case(monkeypatch, case)
    assert rep["layout"] == "pairs"
    if case == "bounce-7":
        still = _still(rep["frames"])
        assert rep["qs"]["late_bounce_compaction"] == "on" and rep["cs"] == (0, still), (rep["qs"], rep["cs"])
    else:
        _assert_compacted(rep, 203, 117)
    if "PT_OVERLAP_DEPTH" in _ENDS[case]:
        assert rep["qs"]["frames_in_flight"] == int(_ENDS[case]["PT_OVERLAP_DEPTH"]), rep["qs"]


def test_every_lane_stores_at_least_what_the_last_lane_does(monkeypatch):
    """PT_CONT_LANES=64 stores every path that is still looping after bounce 2, PT_CONT_LANES=1 only a
    wave's last one: on the same frames the first count cannot be the smaller."""
    for case in ("lanes-1", "lanes-64"):
        if case not in _STORED:
            _knob_case(monkeypatch, case)
    assert _STORED["lanes-64"] >= _STORED["lanes-1"] > 0, _STORED


# ------------------------------------------------------------------- frame sizes and partitions

SIZES = [(1, 1), (2, 2), (1, 37), (37, 1), (3, 5), (16, 16), (17, 17), (8, 200)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
BACKENDS = [(b, l) for b in ("megakernel", "persistent", "wavefront") for l in ("pairs", "trail", "reference")]


@pytest.fixture(params=BACKENDS, ids=["-".join(b) for b in BACKENDS])
def backend(request, engine):
    engine.set_backend(request.param[0])
    engine.set_bvh_layout(request.param[1])
    yield request.param
    engine.set_backend("megakernel")
    engine.set_bvh_layout("pairs")


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_tiny_frames_bitexact(engine, backend, size):
    """Frames down to one pixel on every schedule and BVH layout (compaction off: the auto default): quad
    helpers of a 1-pixel-wide frame, a frame inside one 8x8 wave tile, the 5x5 output filter on a frame
    smaller than its footprint - the teapot's three recorded frames and four still ones, with the last
    screenOutput also drawn into an RGBA32F target."""
    W, Hh = size
    meta = H.stream("gltf_teapot_320x180")
    player = _player(engine, meta, W, Hh)
    frames = meta["frames"] + [player.synth_frame(k) for k in range(4)]
    mid = len(frames) - 3
    got = _draw(engine, player, frames, mid, f32=True)
    assert engine.bvh_layout_used() == backend[1]
    _compare("%dx%d" % size, got, _oracle("tiny", meta, frames, W, Hh, keep={mid}), mid)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_tiny_frames_compacted(monkeypatch, size):
    """The same frames with compaction forced on: a frame smaller than a wave stores every path that is
    still looping after bounce 2 (its waves never hold more than PT_CONT_LANES live lanes), and pt_cont
    runs as a handful of waves, down to 4."""
    W, Hh = size
    rep, _ = _run(monkeypatch, "tiny", H.stream("gltf_teapot_320x180"), W, Hh, f32=True)
    still = _still(rep["frames"])
    assert rep["qs"]["late_bounce_compaction"] == "on" and rep["cs"][1] == still, (rep["qs"], rep["cs"])
    assert rep["cs"][0] <= W * Hh * still, rep["cs"]


@pytest.mark.parametrize("parts", [3, 8])
def test_band_partitions_compacted(monkeypatch, parts):
    """203x40 is three 16-row bands (the last one 8 rows): as 3 partitions each owns one, as 8 partitions
    five own none and draw nothing. Every part traces into the same targets with compaction on, the copy
    is full-frame and the output goes band by band: the oracle's whole frame."""
    rep, _ = _run(monkeypatch, "bands", H.stream("gltf_teapot_320x180"), 203, 40, parts=parts)
    _assert_compacted(rep, 203, 40, bands=3)


def test_multipart_context_sums_its_parts(monkeypatch):
    """The same 203x40 frames through a context of 2 parts (bands 0 and 2 | band 1) and of 5 parts (two own
    nothing): pt_cont_stats sums the parts. Which paths a wave stores depends on the wave's 8x8 pixels alone,
    so both contexts store the same number of records, whoever traces the band."""
    reps = [_run(monkeypatch, "bands", H.stream("gltf_teapot_320x180"), 203, 40, devices=[0] * n)[0] for n in (2, 5)]
    still = _still(reps[0]["frames"])
    assert [r["cs"][1] for r in reps] == [2 * still, 3 * still], [r["cs"] for r in reps]
    assert reps[0]["cs"][0] == reps[1]["cs"][0] > 0, [r["cs"] for r in reps]
    assert reps[0]["cs"][0] <= 203 * 40 * still


def test_resize_with_draws_in_flight(monkeypatch):
    """96x64 -> 203x117 -> 64x40, four frames each: the two render targets and the canvas are resized while
    a further frame of the old size is queued and not waited for, the record buffers grow for the larger
    frame (cont_reserve), and the running record total survives the reallocation. A resized target's memory
    is zero, so each segment's last accumulation and canvas (read before the queued frame) are the oracle's
    over that segment from a zero history."""
    import babylon_pt as bp
    monkeypatch.setenv("PT_CONT", "1")
    monkeypatch.setenv("PT_OVERLAP_LAG", "0")
    meta = H.stream("gltf_teapot_320x180")
    sizes = [(96, 64), (203, 117), (64, 40)]
    e = bp.Engine(0)
    try:
        player = _player(e, meta, *sizes[0])
        player.override = {}     # (the uniforms of each size come with the calls below)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(11)]
        segments = [frames[0:4], frames[5:9], frames[10:14]]
        queued = [frames[4], frames[9], None]

        def play(calls, W, Hh):
            for call in calls:
                if "uResolution" in call["uniforms"]:
                    call = dict(call, uniforms=H.with_resolution(call["uniforms"], W, Hh))
                player.play_call(call)

        got, stats = [], []
        for s, (W, Hh) in enumerate(sizes):
            if s:
                for name in ("pathTracingRenderTarget", "screenCopyRenderTarget"):
                    player.textures[name].resize((W, Hh))
                e.resize_canvas(W, Hh)
            for calls in segments[s]:
                play(calls, W, Hh)
            got.append((player.textures["pathTracingRenderTarget"].read(), e.read_canvas(W, Hh)))
            stats.append(e.cont_stats())
            if queued[s]:
                play(queued[s], W, Hh)
        qs = e.queue_stats()
    finally:
        e.dispose()
    for s, (W, Hh) in enumerate(sizes):
        ref = _oracle("resize-%d" % s, meta, segments[s], W, Hh)
        _compare("segment %d (%dx%d)" % (s, W, Hh), {"acc": got[s][0], "can": got[s][1]}, ref, None)
    assert qs["late_bounce_compaction"] == "on"
    still = [_still(seg) for seg in segments]
    assert [c[1] for c in stats] == [still[0], still[0] + 1 + still[1], still[0] + 1 + still[1] + 1 + still[2]], stats
    # each segment stored records, counted on top of the ones before the reallocation
    assert 0 < stats[0][0] < stats[1][0] < stats[2][0], stats
    assert stats[2][0] <= sum((n + 1) * W * Hh for n, (W, Hh) in zip(still, sizes)), stats


# ------------------------------------------------------------ the moving camera and the auto trial

def test_moving_camera_draws_stay_out_of_the_auto_trial(monkeypatch):
    """A moving-camera draw runs alone and does not compact (PT_MOVING_SERIAL), so it is no draw of the auto
    mode's trial either: 40 of them leave the trial's draw count untouched and are reported as not
    compacting; the 12 still frames after them are draws 1-12 of the 32 before the trial, which compact by
    the default (PT_CONT_AUTO_PIXELS=0). Counted, the 52 draws would be past the 32 and read "auto: trial"."""
    import babylon_pt as bp
    monkeypatch.delenv("PT_CONT", raising=False)
    monkeypatch.setenv("PT_CONT_AUTO_PIXELS", "0")
    W, Hh = 160, 90
    meta = H.stream("gltf_bunny_1080p")
    mesh = _small_dragon()
    e = bp.Engine(0)
    try:
        player = _player(e, meta, W, Hh, mesh)
        frames = meta["frames"] + [player.synth_frame(k) for k in range(48)]
        for i in range(40):      # (the oracle takes the uniforms as given)
            frames[i] = [dict(c, uniforms=dict(c["uniforms"], uCameraIsMoving=["i", [1]]))
                         if c["shader"] == "pathTracingFragmentShader" else c for c in frames[i]]
        for calls in frames[:40]:
            for call in calls:
                player.play_call(call)
        moving = (e.queue_stats(), e.cont_stats())
        for calls in frames[40:]:
            for call in calls:
                player.play_call(call)
        e.sync()
        acc = player.textures["pathTracingRenderTarget"].read()
        can = e.read_canvas(W, Hh)
        still = (e.queue_stats(), e.cont_stats())
    finally:
        e.dispose()
    assert _still(frames) == 12
    assert moving[0]["late_bounce_compaction"] == "off" and moving[0]["compacting_draws"] == 0, moving
    assert moving[1] == (0, 0), moving
    assert still[0]["late_bounce_compaction"] == "auto: default on", still
    assert still[0]["compacting_draws"] == 12 and still[1][1] == 12, still
    assert 0 < still[1][0] <= 12 * W * Hh, still
    _compare("moving then still", {"acc": acc, "can": can}, _oracle("moving", meta, frames, W, Hh, mesh), None)
