"""Hand-shaped BVH trees (tests/tree_shapes.py) through the child-pair build (pt_pairs_* in csrc/pt_pairs.hip),
the pair walk's stack and the restart trail (bvhWalkPairs, bvhWalkTrail / trailRestart in csrc/pt_device.h).

The builder's trees are tight and balanced, so few far children are ever pending at once. The trees here
are the legal input that is not: chains down to the trail's depth bound of 28 with every box the root's (every
node ties, A is taken and B pushed, so all 28 levels are pending and both LDS rings - 9 and 13 live entries -
run dry and restart through the jump table), 64 chains below a balanced top (many jump-table entries), the
same one level past the bound (the trail is refused; loose, stackLevels[28] overflows as the oracle's),
trees of 1, 2, 3 and 8 triangles, BVH textures without the 2048 x 2048 zero tail, a node with two parents, an
unreachable run and a NaN box. tests/test_tree_shapes.py certifies depth, peak pending and overflow of every
tree used here on the CPU oracle.

Every case compares, with the oracle's replay of the same arrays: every accumulation texel as uint32, the
canvas bytes, and the whole counter dictionary - a restart descent is no node fetch of the reference's - and
asserts the layout the draw really walked. 160x90, two frames.

Run on an MI355X: python -m pytest tests/test_gpu_tree_shapes.py -m gpu
"""
import numpy as np
import pytest

import helpers as H
import tree_shapes as T

pytestmark = pytest.mark.gpu

W, HH, FRAMES = 160, 90, 2
LAYOUTS = ("pairs", "trail", "reference")
SCHEDULES = ("megakernel", "persistent", "wavefront")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def _diff_report(a, b):
    bad = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
    pix = bad.reshape(bad.shape[0], bad.shape[1], -1).any(-1)
    ys, xs = np.nonzero(pix)
    first = (int(xs[0]), int(ys[0])) if len(xs) else None
    return "mismatching pixels %d / %d, first (x,y)=%s" % (pix.sum(), pix.size, first)


def _meta(stream):
    return H.sky_mesh_stream() if stream == "skymesh" else H.stream(stream)


_MAPS = {}


def _maps():
    if not _MAPS:
        _MAPS.update(H.synthetic_pbr_maps())
    return _MAPS


_REF = {}


def _oracle(key, stream, tree, maps=None):
    """The oracle's replay of `tree` under `stream`, once per key: accumulations, canvases, counter sums."""
    if key not in _REF:
        acc, can, cnt = H.oracle_replay(_meta(stream), FRAMES, width=W, height=HH, with_output=True, mesh=tree, maps=maps)
        _REF[key] = {"acc": acc, "can": can, "cnt": {k: sum(c[k] for c in cnt) for k in cnt[0]}}
    return _REF[key]


class _Scene:
    """One tree's textures on the engine under one stream; draw() renders the two frames from a zero history
    with a schedule and a requested layout. `bvh_texture`: (texels, w, h) uploaded in place of the player's
    2048 x 2048 BVH texture."""

    def __init__(self, engine, stream, tree, maps=None, bvh_texture=None):
        import babylon_pt as bp
        self.engine, self.meta = engine, _meta(stream)
        self.player = bp.StreamPlayer(engine, self.meta, H.bluenoise(), H.texture_payloads(self.meta, tree), W, HH)
        self.raw = [raw for raw, kind in self.meta["textures"].items() if kind in ("bvh", "tri")]
        if bvh_texture is not None:
            raw_bvh = next(raw for raw, kind in self.meta["textures"].items() if kind == "bvh")
            arr, w, h = bvh_texture
            self.player.textures[raw_bvh].dispose()
            self.player.textures[raw_bvh] = bp.RawTexture.CreateRGBATexture(arr, w, h, engine, name="bvh")
        for kind, sampler in H.PBR_SAMPLERS.items() if maps else ():
            self.player.textures[sampler] = bp.Texture(engine, maps[kind], name=kind)
        engine.resize_canvas(W, HH)

    def draw(self, schedule, layout, data_error=False):
        import babylon_pt as bp
        e, player = self.engine, self.player
        zero = np.zeros((HH, W, 4), np.float32)
        for name in ("pathTracingRenderTarget", "screenCopyRenderTarget"):
            player.textures[name].write(zero)
        e.set_backend(schedule)
        e.set_bvh_layout(layout)
        e.set_counting(True)
        e.reset_counters()
        got = {"acc": [], "can": []}
        try:
            for i in range(FRAMES):
                player.play_frame(i)
                if data_error:   # reported by the first sync after the draw, once
                    with pytest.raises(bp.PtError, match="PT_ERR_DATA"):
                        e.sync()
                e.sync()
                got["acc"].append(player.textures["pathTracingRenderTarget"].read())
                got["can"].append(e.read_canvas(W, HH))
            got["used"] = e.bvh_layout_used()
            got["cnt"] = e.counters()
        finally:
            e.set_counting(False)
            e.set_backend("megakernel")
            e.set_bvh_layout("pairs")
        return got

    def dispose(self):
        for raw in self.raw:
            self.player.textures[raw].dispose()


def _compare(what, got, ref, used):
    assert got["used"] == used, "%s: walked %s, expected %s" % (what, got["used"], used)
    for i in range(FRAMES):
        assert _bits_equal(ref["acc"][i], got["acc"][i]), "%s frame %d accumulation: %s" % (what, i, _diff_report(ref["acc"][i], got["acc"][i]))
        assert _bits_equal(ref["can"][i], got["can"][i]), "%s frame %d canvas: %s" % (what, i, _diff_report(ref["can"][i], got["can"][i]))
    assert got["cnt"] == ref["cnt"], "%s counters" % what


def _run(engine, key, stream, tree, schedules=("megakernel",), layouts=LAYOUTS, used=None, maps=None, bvh_texture=None,
         oracle_tree=None, data_error=False):
    """The case on every schedule and requested layout (`used`: {requested: walked}, default the requested
    one); returns the oracle's reference."""
    ref = _oracle(key, stream, tree if oracle_tree is None else oracle_tree, maps)
    scene = _Scene(engine, stream, tree, maps, bvh_texture)
    try:
        for schedule in schedules:
            for layout in layouts:
                got = scene.draw(schedule, layout, data_error)
                _compare("%s %s, %s requested" % (key, schedule, layout), got, ref, (used or {}).get(layout, layout))
    finally:
        scene.dispose()
    return ref


# ------------------------------------------------------------------------------------------ shapes x boxes

_SHAPE_CASES = [(shape, boxes, schedule) for shape in T.SHAPES for boxes in T.BOXES for schedule in SCHEDULES]


@pytest.mark.parametrize("shape,boxes,schedule", _SHAPE_CASES, ids=["-".join(c) for c in _SHAPE_CASES])
def test_shaped_teapot_trees_bitexact(engine, shape, boxes, schedule):
    """The teapot's triangles in a balanced tree, a left and a right chain, a zigzag and a left chain of
    one-, two- and three-triangle bundles to depth 28, and 64 chains below six balanced levels, with tight,
    loose and alternating boxes: pairs, trail and reference
    each walk the layout asked for - at depth 28 the trail is used - and give the oracle's bits and counters.
    Loose, the left chain keeps 28 entries pending (stackLevels[28] exactly full, the stack walk's global
    slab filled to its last level, trail bits down to bit 3) and every node ties."""
    tree = T.case_tree("teapot", shape, boxes)
    ref = _run(engine, ("teapot", shape, boxes), "gltf_teapot_320x180", tree, schedules=(schedule,))
    assert ref["cnt"]["stack_overflow"] == 0 and ref["cnt"]["hit_lookups"] > 1000
    if boxes == "loose":
        assert ref["cnt"]["leaf_tests"] > 6000 * 992


# ------------------------------------------------------------------------------------------ the bound

def test_depth_29_tight_keeps_the_pairs(engine):
    """One level past the bound: the trail request yields the pair walk, with no error."""
    tree = T.case_tree("teapot", "left29", "tight")
    ref = _run(engine, ("teapot", "left29", "tight"), "gltf_teapot_320x180", tree, used={"trail": "pairs"})
    assert ref["cnt"]["stack_overflow"] == 0


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_depth_29_loose_overflows_as_the_oracle(engine, schedule):
    """... and with every level pending the 29th push is dropped as the oracle drops it: the first sync after
    each draw reports PT_ERR_DATA once, the accumulation and the counters are still the oracle's."""
    tree = T.case_tree("teapot", "left29", "loose")
    ref = _run(engine, ("teapot", "left29", "loose"), "gltf_teapot_320x180", tree, schedules=(schedule,),
               used={"trail": "pairs"}, data_error=True)
    assert ref["cnt"]["stack_overflow"] > 0


def test_depth_29_right_chain_loose_does_not_overflow(engine):
    """A right chain keeps one entry pending however deep it is: no overflow, but no trail either."""
    tree = T.case_tree("teapot", "right29", "loose")
    ref = _run(engine, ("teapot", "right29", "loose"), "gltf_teapot_320x180", tree, used={"trail": "pairs"})
    assert ref["cnt"]["stack_overflow"] == 0


# ------------------------------------------------------------------------------------------ every trail program

@pytest.mark.parametrize("shape", ["left28", "top6", "bundles28"])
@pytest.mark.parametrize("stream,tris", [("hdri_teapot_320x180", "teapot"), ("skymesh", "teapot"),
                                         ("gltf_helmet_320x180", "helmet1024"), ("hdri_helmet_320x180", "helmet1024")])
def test_ring_dry_trees_on_every_mesh_program(engine, stream, tris, shape):
    """The deep-loose trees (single leaves and bundles pending) and the top-then-chains loose tree under the HDRI and the sky composite (the ring of
    10) and, over 1024 of the helmet's triangles with the seeded PBR maps bound, under the helmet streams:
    the textured programs, whose ring has 14 slots. Every schedule: the wavefront walk has its own ring."""
    maps = _maps() if tris == "helmet1024" else None
    tree = T.case_tree(tris, shape, "loose")
    ref = _run(engine, (stream, tris, shape), stream, tree, schedules=SCHEDULES, maps=maps)
    assert ref["cnt"]["stack_overflow"] == 0 and ref["cnt"]["hit_lookups"] > 0
    assert ref["cnt"]["leaf_tests"] > 1000 * tree["tri"].shape[0]


# ------------------------------------------------------------------------------------------ compaction

@pytest.mark.parametrize("shape", ["left28", "top6", "bundles28"])
@pytest.mark.parametrize("layout", ["trail", "pairs"])
def test_ring_dry_trees_through_late_bounce_compaction(monkeypatch, layout, shape):
    """The same trees walked by pt_trace's first bounces and by pt_cont's late ones (PT_CONT=1, a fresh
    engine, seven draws with no sync between them: tests/test_gpu_compaction.py's scaffold), and path records
    really went through pt_cont."""
    import test_gpu_compaction as C
    tree = T.case_tree("teapot", shape, "loose")
    rep, ref = C._run(monkeypatch, "shaped-%s-loose" % shape, H.stream("gltf_teapot_320x180"), W, HH, mesh=tree, layout=layout)
    assert rep["layout"] == layout
    assert ref["counters"]["stack_overflow"] == 0 and ref["counters"]["hit_lookups"] > 1000
    C._assert_compacted(rep, W, HH)


# ------------------------------------------------------------------------------------------ tiny and odd trees

@pytest.mark.parametrize("boxes", ["tight", "loose"])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_tiny_trees_bitexact(engine, k, boxes):
    """1, 2, 3 and 8 big triangles: a root that is a leaf (no inner record, a root code with the leaf bit, an
    all-zero jump table), and trees whose jump-table paths meet a leaf first; on every schedule and all three layouts, the
    one asked for."""
    tree = T.tiny_tree(k, boxes)
    ref = _run(engine, ("tiny", k, boxes), "gltf_teapot_320x180", tree, schedules=SCHEDULES)
    assert 10 * ref["cnt"]["hit_lookups"] >= ref["cnt"]["paths"]


@pytest.mark.parametrize("upload", ["exact", "odd", "usual"])
def test_bvh_textures_without_the_zero_tail(engine, upload):
    """The balanced teapot tree in a BVH texture of exactly 2 x nodes texels (the records are the nodes, one
    scan block, the last inner node against the end), of an odd texel count (the record count is rounded up,
    the last record has one texel) and in the usual 2048 x 2048 one: pairs and trail, the same bits."""
    tree = T.case_tree("teapot", "balanced", "tight")
    tex = {"exact": T.exact_texture, "odd": T.odd_texture, "usual": lambda t: None}[upload](tree)
    if tex is not None:
        assert tex[1] * tex[2] == 2 * 1983 + (upload == "odd") and tex[0].size == 4 * tex[1] * tex[2]
    _run(engine, ("teapot-texture", upload), "gltf_teapot_320x180", tree, schedules=SCHEDULES, layouts=("pairs", "trail"),
         bvh_texture=tex,
         oracle_tree=None if tex is None else dict(tree, bvh=tex[0]))


# ------------------------------------------------------------------------------------------ refusals

def _good_tree_gets_its_layout_back(engine, layout):
    tree = T.case_tree("teapot", "balanced", "tight")
    _run(engine, ("teapot", "balanced", "tight"), "gltf_teapot_320x180", tree, layouts=(layout,))


@pytest.mark.parametrize("layout", ["trail", "pairs"])
def test_shared_subtree_refuses_the_trail_and_keeps_the_pairs(engine, layout):
    """A node linked from two parents (and, with it, a run that no link reaches): the records still express
    it, so the pair walk is used and prices the subtree twice as the oracle does; the trail's one path per
    node does not hold, so the trail is refused. A good tree drawn next gets the layout asked for."""
    tree = T.share_subtree(T.case_tree("teapot", "balanced", "tight"))
    assert T.tree_stats(tree["bvh"])["parents_max"] == 2
    _run(engine, "teapot-shared", "gltf_teapot_320x180", tree, schedules=SCHEDULES, layouts=(layout,), used={"trail": "pairs"})
    _good_tree_gets_its_layout_back(engine, layout)


@pytest.mark.parametrize("layout", ["trail", "pairs"])
def test_unreachable_run_leaves_the_trail_on(engine, layout):
    """Nodes behind the tree that no link reaches - here a run as deep as the bound allows - are no
    part of it: same bits as without them."""
    bal = T.case_tree("teapot", "balanced", "tight")
    tree = T.orphan_run(bal, T.case_tree("teapot", "right28", "tight"))
    ref = _run(engine, "teapot-orphan", "gltf_teapot_320x180", tree, layouts=(layout,))
    assert ref["cnt"] == _oracle(("teapot", "balanced", "tight"), "gltf_teapot_320x180", bal)["cnt"]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("layout", ["trail", "pairs"])
def test_nan_box_falls_back_to_the_reference_walk(engine, layout, schedule):
    """A NaN coordinate in a reachable node's box (the records' box test needs NaN-free boxes): the draw walks
    the reference layout, exactly; a good tree drawn next gets the layout asked for."""
    tree = T.nan_box(T.case_tree("teapot", "balanced", "tight"))
    _run(engine, "teapot-nan", "gltf_teapot_320x180", tree, schedules=(schedule,), layouts=(layout,),
         used={"trail": "reference", "pairs": "reference"})
    _good_tree_gets_its_layout_back(engine, layout)
