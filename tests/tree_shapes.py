"""Hand-shaped BVH trees in the reference's layout (test infrastructure, host only).

The native builder's trees are tight and balanced; the trees here are legal input of the shapes it never
makes: chains down to the restart trail's depth bound, loose boxes that tie at every node and keep every
level pending, tiny trees, shared and unreachable subtrees, a NaN box, and BVH textures that are not the
2048 x 2048 zero-tailed one. tests/test_tree_shapes.py checks the generator on the CPU oracle,
tests/test_gpu_tree_shapes.py draws the trees on the device.

The layout (js/BVH_Fast_Builder.js): node n is the texel pair (2n, 2n + 1), eight floats. Nodes are numbered
depth-first, left subtree first, so an inner node's left child is n + 1. An inner node holds [0] = -1 and
[4] = its right child's id, a leaf [0] = its triangle's index and [4] = -1; the box is [1:4] (min), [5:8] (max).

One invariant holds for everything this module returns (check_links): every link of every inner node names a
higher node id. Every walk of such a tree is finite, on the oracle and on the device alike; a link to the
root, to an ancestor or to the node itself would make a walk that never ends.
"""
import numpy as np

import helpers as H


# ------------------------------------------------------------------------------------------ rules
# rule(n, depth) -> how many of a node's n >= 2 triangles go to its left child (1 .. n - 1)

def balanced(n, depth):
    return (n + 1) // 2


def left_chain(k):
    """One triangle peeled off to the right per level for k levels (the chain runs down the left children),
    then balanced."""
    return lambda n, depth: n - 1 if depth < k else balanced(n, depth)


def left_bundles(k):
    """A left chain of k levels that peels off 1, 2, 3, 1, 2, 3, ... triangles to the right: the pending far
    children are subtrees of different sizes, so a walk that takes one for another counts other leaves."""
    return lambda n, depth: max(1, n - 1 - depth % 3) if depth < k else balanced(n, depth)


def right_chain(k):
    """One triangle peeled off to the left per level for k levels (the chain runs down the right links)."""
    return lambda n, depth: 1 if depth < k else balanced(n, depth)


def top_then_chains(b):
    """Balanced for b levels, then every subtree a left chain to its last triangle."""
    return lambda n, depth: balanced(n, depth) if depth < b else n - 1


def zigzag(k):
    """A chain of k levels that runs left, left, right, repeated; then balanced."""
    return lambda n, depth: (n - 1 if depth % 3 < 2 else 1) if depth < k else balanced(n, depth)


def chain_levels(n, depth, peel=lambda level: 1):
    """The k for which a k-level chain over n triangles (level d peels off peel(d) of them) followed by a
    balanced tree has its deepest leaf `depth` links below the root."""
    left = n
    for k in range(0, n - 1):
        if k + int(np.ceil(np.log2(left))) == depth:
            return k
        left -= peel(k)
    raise ValueError("no chain over %d triangles reaches depth %d" % (n, depth))


# ------------------------------------------------------------------------------------------ the generator

def check_links(bvh):
    """The invariant: every link of every inner node (its left child n + 1, its right link [4]) names a
    higher node id inside the tree, as an exact integer."""
    bvh = np.asarray(bvh)
    n = bvh.shape[0]
    inner = np.nonzero(bvh[:, 0] < 0)[0]
    right = bvh[inner, 4]
    assert np.all(right == np.floor(right)), "a right link is no integer"
    assert np.all(inner + 1 < n), "a left child lies past the tree"
    assert np.all(right > inner) and np.all(right < n), "a right link does not name a higher node of the tree"
    assert n == 1 or bvh[0, 0] < 0
    return bvh


def shaped_tree(tri, rule, boxes="tight", order=None):
    """A tree over the triangle records `tri` (n, 32): {"bvh": (2n - 1, 8) float32, "tri": tri}.
    rule(n, depth) splits a node's triangles; they keep list order (`order`: the list, a permutation of the
    triangle indices, default 0 .. n - 1; a leaf names its triangle's index in `tri`).
    boxes: "tight" the float32 min / max of the subtree's vertices, "loose" every node carries the root's
    box, "even" loose on even depths and tight on odd ones."""
    assert boxes in ("tight", "loose", "even")
    tri = np.asarray(tri, np.float32)
    n = tri.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    assert sorted(order.tolist()) == list(range(n))
    pos = tri[:, 0:9].reshape(n, 3, 3)
    lo, hi = pos.min(1)[order], pos.max(1)[order]          # per list entry
    root = (lo.min(0), hi.max(0))
    bvh = np.zeros((2 * n - 1, 8), np.float32)
    nxt = [0]

    def build(first, count, depth):
        me = nxt[0]
        nxt[0] += 1
        tight = (lo[first:first + count].min(0), hi[first:first + count].max(0))
        loose = boxes == "loose" or (boxes == "even" and depth % 2 == 0)
        bvh[me, 1:4], bvh[me, 5:8] = root if loose else tight
        if count == 1:
            bvh[me, 0], bvh[me, 4] = order[first], -1.0
            return
        left = int(rule(count, depth))
        assert 1 <= left < count, "rule(%d, %d) = %d" % (count, depth, left)
        bvh[me, 0] = -1.0
        build(first, left, depth + 1)
        bvh[me, 4] = nxt[0]
        build(first + left, count - left, depth + 1)

    build(0, n, 0)
    assert nxt[0] == 2 * n - 1
    return {"bvh": check_links(bvh), "tri": tri}


def split_counts(bvh):
    """The rule that rebuilds a depth-first tree's shape, and its leaves' triangle list: (rule, order).
    The rule is keyed by the order in which shaped_tree asks, which is the node numbering."""
    bvh = np.asarray(bvh)
    inner = bvh[:, 0] < 0
    counts = [int(bvh[n, 4] - n) // 2 for n in range(bvh.shape[0]) if inner[n]]
    it = iter(counts)
    return (lambda n, depth: next(it)), bvh[~inner, 0].astype(np.int64)


def tree_stats(bvh):
    """Of the nodes the root reaches: {"nodes", "depth": the deepest leaf's links below the root,
    "left_turns": the most left children on any root-to-leaf path - with loose boxes every box ties, A is
    taken and B is pushed, so this is exactly the walk's peak number of pending entries -, "leaves",
    "parents_max": the most links that name one node}. Links name higher ids, so one ascending pass does it."""
    bvh = check_links(bvh)
    n = bvh.shape[0]
    depth = np.full(n, -1, np.int64)
    turns = np.zeros(n, np.int64)
    refs = np.zeros(n, np.int64)
    depth[0] = 0
    for m in range(n):
        if depth[m] < 0 or not bvh[m, 0] < 0:
            continue
        for child, turn in ((m + 1, 1), (int(bvh[m, 4]), 0)):
            refs[child] += 1
            depth[child] = max(depth[child], depth[m] + 1)
            turns[child] = max(turns[child], turns[m] + turn)
    reached = depth >= 0
    leaves = reached & ~(bvh[:, 0] < 0)
    return {"nodes": int(reached.sum()), "depth": int(depth[leaves].max()), "left_turns": int(turns[leaves].max()),
            "leaves": int(leaves.sum()), "parents_max": int(refs.max()) if n > 1 else 0}


def table_paths(bvh, level):
    """The distinct root paths (dir bits, 1 = the right link) of the reachable inner nodes `level` links
    below the root: the entries of the restart trail's jump table at that depth that hold a record."""
    bvh = check_links(bvh)
    paths, front = set(), [(0, 0, 0)]
    while front:
        m, d, bits = front.pop()
        if not bvh[m, 0] < 0:
            continue
        if d == level:
            paths.add(bits)
            continue
        front.append((m + 1, d + 1, bits << 1))
        front.append((int(bvh[m, 4]), d + 1, (bits << 1) | 1))
    return paths


# ------------------------------------------------------------------------------------------ editors

def _subtree_end(bvh, n):
    """One past the last node of the depth-first run that starts at n (of an unedited tree)."""
    end = n + 1
    while n < end:
        if bvh[n, 0] < 0:
            end = max(end, int(bvh[n, 4]) + 1)
        n += 1
    return end


def share_subtree(tree, node=1, target=None):
    """The inner node `node`'s right link redirected to an inner node with a higher id outside its own
    subtree (default: the first one behind it): that node then has two parents and its subtree is walked,
    and priced, twice; `node`'s old right subtree becomes a run that no link reaches."""
    bvh = tree["bvh"].copy()
    assert bvh[node, 0] < 0
    end = _subtree_end(bvh, node)
    if target is None:
        target = next(m for m in range(end, bvh.shape[0]) if bvh[m, 0] < 0)
    assert target >= end and bvh[target, 0] < 0
    bvh[node, 4] = target
    return dict(tree, bvh=check_links(bvh))


def orphan_run(tree, other):
    """`other`'s nodes (a tree over the same triangle records) appended behind `tree`'s as a run that no
    link reaches."""
    base = tree["bvh"].shape[0]
    run = other["bvh"].copy()
    inner = run[:, 0] < 0
    run[inner, 4] += base
    return dict(tree, bvh=check_links(np.concatenate([tree["bvh"], run])))


def nan_box(tree, node=2, lane=1):
    """One coordinate of a node's box made NaN."""
    bvh = tree["bvh"].copy()
    assert lane in (1, 2, 3, 5, 6, 7)
    bvh[node, lane] = np.nan
    return dict(tree, bvh=check_links(bvh))


def _sides(texels):
    h = max(d for d in range(1, int(texels ** 0.5) + 1) if texels % d == 0)
    return texels // h, h


def exact_texture(tree):
    """The BVH texture with no tail: (texels as a flat float32 array, width, height), exactly two texels
    per node."""
    flat = np.ascontiguousarray(tree["bvh"], np.float32).reshape(-1)
    return (flat,) + _sides(flat.size // 4)


def odd_texture(tree):
    """... and with one zero texel behind the last node: an odd texel count."""
    flat = np.concatenate([np.ascontiguousarray(tree["bvh"], np.float32).reshape(-1), np.zeros(4, np.float32)])
    assert (flat.size // 4) % 2 == 1
    return (flat,) + _sides(flat.size // 4)


# ------------------------------------------------------------------------------------------ triangles

def big_triangles(k, lo, hi):
    """k hand-made triangle records that span the box lo .. hi: triangle i stands across the box at z slice
    i of k, tilted a little about the vertical, two corners on the box's floor and one on its ceiling (or,
    every other pair, the other way round), its x and y extent the box's; wound alternately one way and
    the other, so that a single-sided test sees some of them from +z and some from -z. Flat normals, no
    UVs."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, r = (lo + hi) * 0.5, (hi - lo) * 0.5
    tri = np.zeros((k, 32), np.float32)
    for i in range(k):
        z = np.array([0.0, 0.0, lo[2] + (hi[2] - lo[2]) * (i + 0.5) / k - c[2]])
        d = np.array([r[0], 0.0, r[2] / (2 * k)])
        up = np.array([0.0, r[1], 0.0]) * (1.0 if i % 4 < 2 else -1.0)
        p = np.stack([c + z - d - up, c + z + d - up, c + z + 0.25 * d * (-1.0) ** i + up])
        if (i % 2 == 1) != (i % 4 >= 2):
            p = p[::-1]
        p = p.astype(np.float32).astype(np.float64)
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        tri[i, 0:9] = p.reshape(9)
        tri[i, 9:18] = np.tile(nrm / np.linalg.norm(nrm), 3)
        tri[i, 18:24] = -1.0
    return tri


def teapot_triangles():
    return H.mesh("teapot")["tri"]


def helmet_subset():
    """A fixed 1024-triangle subset of the DamagedHelmet's records, UVs intact: every 15th triangle. A loose
    tree over it costs a ray about a thousand leaf tests, as the teapot's does."""
    return np.ascontiguousarray(H.mesh("helmet")["tri"][::15][:1024])


# ------------------------------------------------------------------------------------------ the cases
# shared by the CPU file (which certifies depth, peak pending and overflow on the oracle) and the GPU file

BOXES = ("tight", "loose", "even")
TRAIL_DEPTH = 28      # pt_plan.h kTrailMaxDepth == the reference's stackLevels[28]
TABLE_LEVELS = 11     # pt_plan.h kTopLevels
RING_LIVE = 13        # live entries of the larger ring (pt_device.h kRingOf: 10 / 14 slots, one always free)


def shape_rule(shape, n):
    """The rules of the GPU file's shapes over n triangles; the chains end `TRAIL_DEPTH` links below the root."""
    k = chain_levels(n, TRAIL_DEPTH)
    return {"balanced": balanced, "left28": left_chain(k), "right28": right_chain(k), "top6": top_then_chains(6),
            "zigzag28": zigzag(k), "left29": left_chain(k + 1), "right29": right_chain(k + 1),
            "bundles28": left_bundles(chain_levels(n, TRAIL_DEPTH, lambda level: 1 + level % 3))}[shape]


SHAPES = ("balanced", "left28", "right28", "top6", "zigzag28", "bundles28")
# the shapes whose loose trees keep more entries pending than either ring holds
RING_DRY = ("left28", "top6", "zigzag28", "bundles28")

_TREES = {}


def case_tree(tris, shape, boxes):
    """The tree of a case, built once: tris "teapot" or "helmet1024"."""
    key = (tris, shape, boxes)
    if key not in _TREES:
        tri = teapot_triangles() if tris == "teapot" else helmet_subset()
        _TREES[key] = shaped_tree(tri, shape_rule(shape, tri.shape[0]), boxes)
    return _TREES[key]


def tiny_tree(k, boxes="tight"):
    """1, 2, 3 or 8 big triangles over three times the teapot's box (a good part of the teapot stream's
    view), balanced."""
    key = ("tiny", k, boxes)
    if key not in _TREES:
        root = H.mesh("teapot")["bvh"][0].astype(np.float64)
        _TREES[key] = shaped_tree(big_triangles(k, 3.0 * root[1:4], 3.0 * root[5:8]), balanced, boxes)
    return _TREES[key]
