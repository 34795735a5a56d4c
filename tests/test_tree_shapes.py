"""The hand-shaped tree generator (tests/tree_shapes.py) and the facts tests/test_gpu_tree_shapes.py rests on,
on the CPU oracle: the generator rebuilds the native builder's trees bit for bit, every shape the GPU file
draws has the depth and the peak number of pending entries it is meant to have, the depth-28 shapes fill the
reference's stackLevels[28] without overflowing it and the loose left chain to depth 29 overflows it, the
ring-dry cases keep more entries pending than either LDS ring holds, the top-then-chains trees reach many
entries of the jump table, and every tree the generator or an editor returns keeps every link pointing at a
higher node id (so every walk ends). Host code: runs on the CPU."""
import os

import numpy as np
import pytest

import helpers as H
import tree_shapes as T

W, HH, FRAMES = 160, 90, 2

_REPLAY = {}


def _replay(stream, tree_key, tree, maps=None):
    """The oracle's two frames at 160x90 of `tree` under `stream`: (last accumulation, counter sums)."""
    key = (stream, tree_key)
    if key not in _REPLAY:
        meta = H.sky_mesh_stream() if stream == "skymesh" else H.stream(stream)
        acc, _, cnt = H.oracle_replay(meta, FRAMES, width=W, height=HH, mesh=tree, maps=maps)
        _REPLAY[key] = (acc[-1], {k: sum(c[k] for c in cnt) for k in cnt[0]})
    return _REPLAY[key]


def _case(tris, shape, boxes, stream="gltf_teapot_320x180", maps=None):
    return _replay(stream, (tris, shape, boxes), T.case_tree(tris, shape, boxes), maps)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------ the generator

@pytest.mark.parametrize("key", ["teapot", "duck"])
def test_generator_rebuilds_the_builders_tree_bit_for_bit(key):
    """With the builder's own split counts and its leaves' triangle order, tight boxes: the committed tree."""
    m = np.load(os.path.join(H.GOLD, "mesh_%s.npz" % key))
    rule, order = T.split_counts(m["bvh"])
    got = T.shaped_tree(m["tri"], rule, "tight", order)["bvh"]
    assert _same_bits(got, m["bvh"])


def test_rules_split_as_described():
    assert T.balanced(7, 0) == 4 and T.balanced(2, 5) == 1
    assert [T.left_chain(2)(9, d) for d in range(3)] == [8, 8, 5]
    assert [T.right_chain(2)(9, d) for d in range(3)] == [1, 1, 5]
    assert [T.top_then_chains(2)(9, d) for d in range(4)] == [5, 5, 8, 8]
    assert [T.zigzag(6)(9, d) for d in range(7)] == [8, 8, 1, 8, 8, 1, 5]
    assert [T.left_bundles(3)(9, d) for d in range(4)] == [8, 7, 6, 5] and T.left_bundles(3)(2, 2) == 1
    assert T.chain_levels(992, 28) == 18 and T.chain_levels(1024, 28) == 18 and T.chain_levels(992, 29) == 19
    assert T.chain_levels(992, 28, lambda level: 1 + level % 3) == 18


def test_box_modes():
    tri = T.teapot_triangles()
    root = (tri[:, 0:9].reshape(-1, 3).min(0), tri[:, 0:9].reshape(-1, 3).max(0))
    depth = {}
    for mode in T.BOXES:
        bvh = T.case_tree("teapot", "zigzag28", mode)["bvh"]
        if not depth:   # every node's depth, by one ascending pass (links name higher ids)
            depth = {0: 0}
            for n in range(bvh.shape[0]):
                if bvh[n, 0] < 0:
                    depth[n + 1] = depth[int(bvh[n, 4])] = depth[n] + 1
        for n in range(bvh.shape[0]):
            loose = mode == "loose" or (mode == "even" and depth[n] % 2 == 0)
            is_root_box = np.array_equal(bvh[n, 1:4], root[0]) and np.array_equal(bvh[n, 5:8], root[1])
            if loose:
                assert is_root_box
            elif not bvh[n, 0] < 0:   # a tight leaf: its triangle's own float32 bounds
                p = tri[int(bvh[n, 0]), 0:9].reshape(3, 3)
                assert np.array_equal(bvh[n, 1:4], p.min(0)) and np.array_equal(bvh[n, 5:8], p.max(0))
    t = T.case_tree("teapot", "zigzag28", "tight")["bvh"]
    inner = np.nonzero(t[:, 0] < 0)[0]   # a tight inner box is its children's union
    for n in inner:
        a, b = t[n + 1], t[int(t[n, 4])]
        assert np.array_equal(t[n, 1:4], np.minimum(a[1:4], b[1:4])) and np.array_equal(t[n, 5:8], np.maximum(a[5:8], b[5:8]))


# ------------------------------------------------------------------------------------------ the shapes' numbers
# 992 teapot triangles: a balanced tree is ceil(log2 992) = 10 deep; an 18-level chain leaves 974 triangles,
# again 10 levels; 64 subtrees of 15 or 16 triangles chained are 15 deep below level 6; the zigzag turns left
# on 12 of its 18 levels; 18 levels of bundles peel off 36 triangles and leave 956, 10 levels. The helmet
# subset's 1024 triangles: 10, 18 + 10 (1006 triangles), 6 + 15, 12 + 10, 18 + 10 (988 triangles).
EXPECT = {"balanced": (10, 10), "left28": (28, 28), "right28": (28, 10), "top6": (21, 21), "zigzag28": (28, 22),
          "bundles28": (28, 28), "left29": (29, 29), "right29": (29, 10)}


@pytest.mark.parametrize("tris,n", [("teapot", 992), ("helmet1024", 1024)])
@pytest.mark.parametrize("shape", list(EXPECT))
def test_depth_and_peak_pending_of_every_shape(tris, n, shape):
    for boxes in T.BOXES:
        s = T.tree_stats(T.case_tree(tris, shape, boxes)["bvh"])
        assert (s["depth"], s["left_turns"]) == EXPECT[shape]
        assert s["nodes"] == 2 * n - 1 and s["leaves"] == n and s["parents_max"] == 1


@pytest.mark.parametrize("boxes", T.BOXES)
@pytest.mark.parametrize("shape", T.SHAPES)
def test_shapes_within_the_bound_never_overflow_and_render_the_builders_image(shape, boxes):
    """Depth <= 28: at most 28 entries pending, stackLevels[28] exactly full at worst. The boxes bound their
    subtrees in every mode, so the image is the builder tree's, bit for bit; loose boxes test every leaf."""
    acc, cnt = _case("teapot", shape, boxes)
    ref_acc, ref_cnt = _replay("gltf_teapot_320x180", "builder", H.mesh("teapot"))
    assert cnt["stack_overflow"] == 0
    assert _same_bits(acc, ref_acc)
    assert cnt["hit_lookups"] == ref_cnt["hit_lookups"] == 1887
    if boxes == "loose":
        assert cnt["leaf_tests"] == 6562080 and cnt["leaf_tests"] % 992 == 0


def test_depth_29_overflows_only_with_every_level_pending():
    assert _case("teapot", "left29", "loose")[1]["stack_overflow"] == 6615
    assert _case("teapot", "left29", "tight")[1]["stack_overflow"] == 0
    assert _case("teapot", "right29", "loose")[1]["stack_overflow"] == 0   # one entry pending at a time


@pytest.mark.parametrize("tris", ["teapot", "helmet1024"])
@pytest.mark.parametrize("shape", T.RING_DRY)
def test_ring_dry_cases_keep_more_pending_than_either_ring_holds(tris, shape):
    s = T.tree_stats(T.case_tree(tris, shape, "loose")["bvh"])
    assert s["left_turns"] >= 14 > T.RING_LIVE and s["depth"] <= T.TRAIL_DEPTH


@pytest.mark.parametrize("tris", ["teapot", "helmet1024"])
def test_top_then_chains_reaches_many_jump_table_entries(tris):
    """64 chains hang below level 6, each down the left children: 64 distinct dir-bit prefixes at the jump
    table's deepest level, and 64 at level 6 (the chains' root paths)."""
    bvh = T.case_tree(tris, "top6", "loose")["bvh"]
    assert len(T.table_paths(bvh, 6)) == 64
    deep = T.table_paths(bvh, T.TABLE_LEVELS)
    assert len(deep) >= 32
    assert {p >> (T.TABLE_LEVELS - 6) for p in deep} == set(range(64))
    # the deep chains reach one entry only
    assert len(T.table_paths(T.case_tree(tris, "left28", "loose")["bvh"], T.TABLE_LEVELS)) == 1


@pytest.mark.parametrize("stream,tris", [("hdri_teapot_320x180", "teapot"), ("skymesh", "teapot"),
                                         ("gltf_helmet_320x180", "helmet1024"), ("hdri_helmet_320x180", "helmet1024")])
def test_other_programs_cases_test_every_leaf(stream, tris):
    """The deep-loose and top-then-chains trees under the other streams: same counters for both shapes (every
    ray that meets the root box tests every leaf), some hits, no overflow."""
    maps = H.synthetic_pbr_maps() if tris == "helmet1024" else None
    a, ca = _case(tris, "left28", "loose", stream, maps)
    b, cb = _case(tris, "top6", "loose", stream, maps)
    n = T.case_tree(tris, "left28", "loose")["tri"].shape[0]
    assert ca == cb and _same_bits(a, b)
    assert ca["stack_overflow"] == 0 and ca["hit_lookups"] > 0
    assert ca["leaf_tests"] > 1000 * n and ca["leaf_tests"] % n == 0
    if tris == "helmet1024":
        assert ca["rgba8_taps"] > ca["paths"]   # the PBR maps are sampled: the textured programs


# ------------------------------------------------------------------------------------------ tiny trees

@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_tiny_trees_cover_the_view(k):
    tree = T.tiny_tree(k)
    assert tree["bvh"].shape == (2 * k - 1, 8) and tree["tri"].shape == (k, 32)
    if k == 1:
        assert tree["bvh"][0, 0] == 0.0 and tree["bvh"][0, 4] == -1.0   # the root is a leaf
    _, cnt = _replay("gltf_teapot_320x180", ("tiny", k), tree)
    assert cnt["paths"] == FRAMES * W * HH
    assert 10 * cnt["hit_lookups"] >= cnt["paths"]
    for boxes in ("loose", "even"):
        acc, c2 = _replay("gltf_teapot_320x180", ("tiny", k, boxes), T.tiny_tree(k, boxes))
        assert c2["hit_lookups"] == cnt["hit_lookups"]


def test_big_triangles_span_the_box_with_both_windings():
    lo, hi = np.array([-3.0, -2.0, -1.0]), np.array([5.0, 2.0, 7.0])
    tri = T.big_triangles(8, lo, hi)
    p = tri[:, 0:9].reshape(8, 3, 3)
    assert np.array_equal(p[..., 0].min(1), np.full(8, lo[0])) and np.array_equal(p[..., 0].max(1), np.full(8, hi[0]))
    assert np.array_equal(p[..., 1].min(1), np.full(8, lo[1])) and np.array_equal(p[..., 1].max(1), np.full(8, hi[1]))
    assert p[..., 2].min() >= lo[2] and p[..., 2].max() <= hi[2]
    nz = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2]
    assert (np.sign(nz) == [1, -1, 1, -1, 1, -1, 1, -1]).all()
    assert np.all(tri[:, 18:24] == -1.0)


# ------------------------------------------------------------------------------------------ editors

def _edited():
    bal = T.case_tree("teapot", "balanced", "tight")
    return {"share": T.share_subtree(bal), "nan": T.nan_box(bal),
            "orphan": T.orphan_run(bal, T.case_tree("teapot", "right28", "tight"))}


def test_editors_keep_the_invariant_and_replay():
    bal = T.case_tree("teapot", "balanced", "tight")
    base = T.tree_stats(bal["bvh"])
    ed = _edited()
    for tree in ed.values():
        T.check_links(tree["bvh"])
    s = T.tree_stats(ed["share"]["bvh"])
    # node 1's right link names the root's right child: two parents, one level deeper through node 1, and
    # node 1's old right subtree is a run that no link reaches
    assert ed["share"]["bvh"][1, 4] == bal["bvh"][0, 4] != bal["bvh"][1, 4]
    assert s["parents_max"] == 2 and s["depth"] == base["depth"] + 1 and s["nodes"] < base["nodes"]
    _, c_share = _replay("gltf_teapot_320x180", "share", ed["share"])
    _, c_bal = _case("teapot", "balanced", "tight")
    assert c_share["stack_overflow"] == 0 and 0 < c_share["hit_lookups"] < c_bal["hit_lookups"]
    # a NaN coordinate in a reachable node's box changes what the walk finds
    assert np.isnan(ed["nan"]["bvh"][2]).sum() == 1
    _, c_nan = _replay("gltf_teapot_320x180", "nan", ed["nan"])
    assert 0 < c_nan["hit_lookups"] != c_bal["hit_lookups"]
    # an unreachable run (here one as deep as the bound) changes nothing
    s = T.tree_stats(ed["orphan"]["bvh"])
    assert ed["orphan"]["bvh"].shape[0] == 2 * 1983 and s["nodes"] == 1983 and s["depth"] == 10
    a_orp, c_orp = _replay("gltf_teapot_320x180", "orphan", ed["orphan"])
    assert c_orp == c_bal and _same_bits(a_orp, _case("teapot", "balanced", "tight")[0])


def test_small_textures_hold_the_same_tree():
    bal = T.case_tree("teapot", "balanced", "tight")
    ref_acc, ref_cnt = _case("teapot", "balanced", "tight")
    arr, w, h = T.exact_texture(bal)
    assert w * h == 2 * 1983 and arr.size == 4 * w * h
    acc, cnt = _replay("gltf_teapot_320x180", "exact", dict(bal, bvh=arr))
    assert _same_bits(acc, ref_acc) and cnt == ref_cnt
    arr, w, h = T.odd_texture(bal)
    assert w * h == 2 * 1983 + 1 and arr.size == 4 * w * h
    acc, cnt = _replay("gltf_teapot_320x180", "odd", dict(bal, bvh=arr))
    assert _same_bits(acc, ref_acc) and cnt == ref_cnt


@pytest.mark.parametrize("link", [0, 1, 2, 5.5, 99])
def test_check_links_refuses_links_that_do_not_go_forward(link):
    """A link to the root, to the node itself, to its own left child's id or below, a fractional one, one past
    the tree: refused before anything walks it."""
    bvh = T.tiny_tree(3)["bvh"].copy()
    assert bvh[1, 0] < 0
    T.check_links(bvh)
    bvh[1, 4] = link
    if link == 2:          # node 1's left child: a higher id, legal (and finite)
        T.check_links(bvh)
        return
    with pytest.raises(AssertionError):
        T.check_links(bvh)
