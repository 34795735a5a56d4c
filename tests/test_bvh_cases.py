"""Both BVH builders (pt_bvh_build, csrc/pt_bvh_build.cpp; pt_bvh_build_gpu, csrc/pt_bvh_gpu.hip) on
directed inputs, against what the reference's own BVH_Build_Iterative made of the same inputs:
tests/golden/bvh_cases.npz, written by tests/golden/gen/make_bvh_cases.py (which describes the cases).
Every comparison is bit for bit. The 199-level chains pin the builders only; they are not drawn (the
walk's trail ends at depth 28)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

PATH = os.path.join(H.GOLD, "bvh_cases.npz")
PINF, NINF = 0x7F800000, 0xFF800000


def _load():
    d = np.load(PATH)
    tris, works = d["tris"].astype(np.int64), d["works"].astype(np.int64)
    t0 = np.concatenate([[0], np.cumsum(tris)])
    w0 = np.concatenate([[0], np.cumsum(works)])
    n0 = np.concatenate([[0], np.cumsum(2 * works - 1)])
    cases = {}
    for i, name in enumerate(d["names"]):
        cases[name.decode()] = (np.ascontiguousarray(d["aabb_in"][t0[i]:t0[i + 1]]),
                                np.ascontiguousarray(d["work"][w0[i]:w0[i + 1]]),
                                np.ascontiguousarray(d["nodes"][n0[i]:n0[i + 1]]))
    assert t0[-1] == len(d["aabb_in"]) and w0[-1] == len(d["work"]) and n0[-1] == len(d["nodes"])
    return cases


CASES = _load()
NAMES = list(CASES)
SLOTS = ["idObject", "min.x", "min.y", "min.z", "idRightChild", "max.x", "max.y", "max.z"]


def _assert_same_bits(got, want, what):
    got = np.ascontiguousarray(got, np.float32).view(np.uint32)
    assert got.shape == want.shape, "%s: %s nodes, the reference has %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        n, s = bad[0]
        raise AssertionError("%s: %d of %d nodes differ, the first at node %d, %s: 0x%08x, the reference has 0x%08x"
                             % (what, len(np.unique(bad[:, 0])), len(want), n, SLOTS[s], got[n, s], want[n, s]))


def _floats(u):
    return u.view(np.float32)


def _inner(nodes):
    return nodes[_floats(nodes)[:, 0] < 0]


def _leaves_below(nodes):
    """Per node: the number of leaves of its subtree (left child = node + 1, right = slot 4)."""
    f = _floats(nodes)
    count = np.zeros(len(nodes), np.int64)
    for n in range(len(nodes) - 1, -1, -1):   # children come after their parent
        count[n] = 1 if f[n, 0] >= 0 else count[n + 1] + count[int(f[n, 4])]
    return count


def _depth(nodes):
    f = _floats(nodes)
    depth = np.ones(len(nodes), np.int64)
    for n in range(len(nodes)):
        if f[n, 0] < 0:
            depth[n + 1] = depth[int(f[n, 4])] = depth[n] + 1
    return int(depth.max())


# ---- the fixture itself

def test_fixture_holds_the_cases_and_stays_small():
    for stem in ("zeros_plane", "zeros_plane_permuted", "zeros_plane_subset", "nan_bounds", "extent_ties_4x3x2",
                 "extent_ties_4x4x4", "adjacent_floats_one", "adjacent_floats_neg3", "adjacent_floats_tiny",
                 "fallback_axes_shortest", "fallback_axes_deal", "fallback_axes_block", "chain_left", "chain_right",
                 "infinities", "work_duplicates", "tiny_1", "tiny_2", "tiny_3"):
        assert stem in CASES
    assert sum(n.startswith("extent_ties_") and "slab" not in n for n in NAMES) == 13
    for name, (aabb, work, nodes) in CASES.items():
        assert aabb.shape[1] == 9 and nodes.shape == (2 * len(work) - 1, 8), name
        assert 1 <= len(work) <= 520 and len(aabb) <= 520 and int(work.max()) < len(aabb), name
        # every triangle of the work list is a leaf once per mention; links stay inside the array
        f = _floats(nodes)
        leaf = f[:, 0] >= 0
        assert sorted(f[leaf, 0].astype(np.int64).tolist()) == sorted(work.tolist()), name
        assert (f[~leaf, 4] > np.nonzero(~leaf)[0] + 1).all() and (f[~leaf, 4] < len(nodes)).all(), name
    assert len(CASES["zeros_plane_subset"][1]) == 131
    assert len(CASES["work_duplicates"][1]) == 150 and len(np.unique(CASES["work_duplicates"][1])) == 50
    assert os.path.getsize(PATH) < os.path.getsize(os.path.join(H.GOLD, "mesh_teapot.npz"))


def test_fixture_zero_signs_follow_the_work_order():
    """The first zero in work order decides an inner box's zero sign: the same boxes under two work
    orders give the same tree with other signs."""
    a, wa, na = CASES["zeros_plane"]
    b, wb, nb = CASES["zeros_plane_permuted"]
    assert np.array_equal(a, b) and not np.array_equal(wa, wb) and sorted(wa.tolist()) == sorted(wb.tolist())
    inner = _floats(na)[:, 0] < 0
    assert np.array_equal(inner, _floats(nb)[:, 0] < 0)
    assert np.array_equal(na[inner][:, [0, 4]], nb[inner][:, [0, 4]])          # the same links
    assert np.array_equal(_floats(na[inner]), _floats(nb[inner]))              # the same values (-0 == +0)
    box = [1, 2, 3, 5, 6, 7]
    za, zb = na[inner][:, box], nb[inner][:, box]
    zero = (za & 0x7FFFFFFF) == 0
    assert zero.any(1).all()                                                    # z is a zero in every box
    assert ((za != zb) & zero).sum() >= 1
    # both signs occur among the inner boxes' zeros, in both orders
    for z in (za, zb):
        assert (z[zero] == 0).any() and (z[zero] == 0x80000000).any()


def test_fixture_nan_bounds_stay_out_of_inner_boxes():
    aabb, work, nodes = CASES["nan_bounds"]
    nan_in = np.isnan(_floats(aabb))
    assert set(np.unique(aabb[nan_in]).tolist()) == {0x7FC00000}
    assert nan_in[:, 0:3].any() and nan_in[:, 3:6].any() and nan_in[:, 6:9].any()
    inner = _inner(nodes)
    assert not np.isnan(_floats(inner)).any()
    # the cluster whose min.x is NaN throughout is a run of its own: its box's min.x stays +Infinity
    cluster = np.nonzero(nan_in[:, 0] & (_floats(aabb)[:, 6] > 50.0))[0]
    assert len(cluster) == 40
    leaves = _leaves_below(nodes)
    runs = np.nonzero((nodes[:, 1] == PINF) & (_floats(nodes)[:, 0] < 0) & (leaves == 40))[0]
    assert len(runs) == 1
    below = nodes[runs[0]:runs[0] + 79]
    assert sorted(_floats(below)[_floats(below)[:, 0] >= 0, 0].astype(int).tolist()) == cluster.tolist()
    for name in NAMES:   # and nowhere else in the fixture either
        assert not np.isnan(_floats(_inner(CASES[name][2]))).any(), name


def test_fixture_chains_are_deep():
    for name in ("chain_left", "chain_right"):
        assert _depth(CASES[name][2]) >= 150, name
    assert _depth(CASES["chain_left"][2]) == 200 and _depth(CASES["chain_right"][2]) == 200


def test_fixture_infinities_give_infinite_boxes():
    aabb, work, nodes = CASES["infinities"]
    root = nodes[0]
    assert root[1:4].tolist() == [NINF] * 3 and root[5:8].tolist() == [PINF] * 3


REF = os.environ.get("PT_REFERENCE", "/root/reference")


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "js")) and shutil.which("node")),
                    reason="needs the reference scripts and node (build container)")
def test_fixture_is_what_the_generator_writes(tmp_path):
    """Regenerated from the reference builder, the cases are the committed file, byte for byte."""
    out = str(tmp_path / "bvh_cases.npz")
    subprocess.run([sys.executable, os.path.join(H.GOLD, "gen", "make_bvh_cases.py"), out], check=True,
                   capture_output=True, timeout=300)
    with open(out, "rb") as f, open(PATH, "rb") as g:
        assert f.read() == g.read()


# ---- the host builder

@pytest.mark.parametrize("name", NAMES)
def test_host_builder_matches_the_reference(name):
    import babylon_pt as bp
    aabb, work, nodes = CASES[name]
    _assert_same_bits(bp.bvh_build(_floats(aabb), work), nodes, name)


def test_gpu_builder_refuses_bad_arguments_before_any_device_call():
    import babylon_pt as bp
    build = bp.lib().pt_bvh_build_gpu
    aabb = np.zeros((2, 9), np.float32); work = np.arange(2, dtype=np.uint32); out = np.zeros((3, 8), np.float32)
    a, w, o = aabb.ctypes.data, work.ctypes.data, out.ctypes.data
    ARG = -1
    assert bp.ERRORS[ARG] == "PT_ERR_ARG"
    assert build(0, None, w, 2, o, 3, None) == ARG
    assert build(0, a, None, 2, o, 3, None) == ARG
    assert build(0, a, w, 2, None, 3, None) == ARG
    assert build(0, a, w, 0, o, 3, None) == ARG
    assert build(0, a, w, -1, o, 3, None) == ARG
    assert build(0, a, w, 2, o, 2, None) == ARG                               # max_nodes < 2n - 1
    assert build(0, a, w, (1 << 24) + 1, o, 2 * ((1 << 24) + 1) - 1, None) == ARG   # node ids past exact floats
    assert build(0, a, w, (1 << 30) + 7, o, 0x7FFFFFFF, None) == ARG          # 2n - 1 past an int
    assert not out.any()


# ---- the device builder

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_builder_matches_the_reference(name):
    import babylon_pt as bp
    aabb, work, nodes = CASES[name]
    got, _ = bp.bvh_build_gpu(_floats(aabb), work)
    _assert_same_bits(got, nodes, name)


@pytest.mark.gpu
def test_gpu_builder_matches_host_around_wave_and_block_sizes():
    """Random boxes at run lengths either side of a 64-lane wave, a 256-thread block and two blocks,
    the largest first, so that a small build follows a large one in freshly freed memory."""
    import babylon_pt as bp
    rng = np.random.default_rng(11)
    for n in sorted((63, 64, 65, 255, 256, 257, 511, 513), reverse=True):
        lo = rng.normal(size=(n, 3)).astype(np.float32)
        hi = lo + rng.random((n, 3)).astype(np.float32)
        aabb = np.concatenate([lo, hi, (lo + hi) * np.float32(0.5)], 1).astype(np.float32)
        for work in (None, rng.permutation(n).astype(np.uint32)):
            want = bp.bvh_build(aabb, work)
            got, _ = bp.bvh_build_gpu(aabb, work)
            _assert_same_bits(got, want.view(np.uint32), "n = %d%s" % (n, "" if work is None else ", permuted"))
