"""The bounded ray-query reference (tests/raycast_bounded_ref.py) on every case of tests/raycast_cases.py, on the CPU.

With t_ref the unbounded reference's t of each ray:
  * no bound - t_max None, NaN, +inf, 2e6, 1000000.0 - gives raycast_ref.cast's records to the bit;
  * 0, -1, t_ref itself, the float below t_ref and 0.5 t_ref miss on every ray (every test is `d < hitT`, strict);
  * 1.5 t_ref gives the unbounded records on every ray;
  * the float above t_ref gives the unbounded records, except the rays raycast_bounded_ref.ONE_ULP_CULLED pins by case
    and index, each a mesh hit of the unbounded reference whose leaf box the bounded walk culls (checked);
  * against a brute-force minimum over all triangles closer than the bound (raycast_ref.brute(..., t_max=)), on the
    0.5 and 1.5 sets, the mesh part disagrees on at most 1 % of a case's rays, each listed: none at 0.5, and at 1.5
    the grazing vertex rays raycast_cases.EXCEPTIONS already lists for the unbounded walk. The one-ulp set is exempt:
    it exists to sit on the culling edge.
"""
import numpy as np
import pytest

import raycast_bounded_ref as B
import raycast_cases as C
import raycast_ref as R


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 16)


def _differing(a, b):
    return np.nonzero((_words(a) != _words(b)).any(1))[0].tolist()


def _is_miss(rec):
    w = _words(rec)
    return (rec["t"] == R.INF) & (rec["object_id"] == -1) & (rec["type"] == -100) & (rec["triangle"] == -1) & ~w[:, 4:].any(1)


@pytest.mark.parametrize("name", list(C.CASES))
def test_no_bound_is_the_unbounded_reference(name):
    for which in B.NO_BOUND:
        assert _differing(B.reference(name, which), C.reference(name)) == [], which


@pytest.mark.parametrize("name", list(C.CASES))
def test_bounds_at_or_below_the_hit_miss(name):
    assert (C.reference(name)["object_id"] >= 0).sum() > 10
    for which in B.ALL_MISS:
        got = B.reference(name, which)
        assert _is_miss(got).all(), "%s: rays %s are no miss" % (which, np.nonzero(~_is_miss(got))[0].tolist())
        assert not B.occluded(got).any()


@pytest.mark.parametrize("name", list(C.CASES))
def test_a_bound_well_beyond_the_hit_changes_nothing(name):
    assert _differing(B.reference(name, "one_and_a_half"), C.reference(name)) == []


def _leaf_of(bvh, triangle):
    return int(np.nonzero((bvh[:, 0] == triangle) & (bvh[:, 4] == -1.0))[0][0])


@pytest.mark.parametrize("name", list(C.CASES))
def test_a_bound_one_ulp_beyond_the_hit(name):
    ref, got = C.reference(name), B.reference(name, "above_t_ref")
    pinned = B.ONE_ULP_CULLED.get(name, {})
    assert _differing(got, ref) == sorted(pinned)
    if not pinned:
        return
    o, d, _ = C.rays_of(name)
    u, m = C.uniforms_of(name), C.mesh_of(C.CASES[name][2])
    bvh = np.asarray(m["bvh"], np.float32).reshape(-1, 8)
    ro, rd = R._rays(o, d)
    t_max = B.t_max_of(name, "above_t_ref")
    with np.errstate(all="ignore"):
        _, mo, md = R.model_space(u, ro, rd)
    for i in pinned:
        assert ref["triangle"][i] >= 0 and ref["t"][i] < t_max[i], "ray %d is no mesh hit of the unbounded reference" % i
        assert _is_miss(got[i:i + 1])[0] or got["triangle"][i] < 0
        # the reason, checked: the leaf's slab test gives a distance that is not below the bound
        leaf = bvh[_leaf_of(bvh, ref["triangle"][i])]
        with np.errstate(all="ignore"):
            inv = tuple(R.F(1.0) / c[i] for c in md)
            box_t = R.bounding_box(leaf[1:4], leaf[5:8], tuple(c[i] for c in mo), inv)
        assert not box_t < t_max[i], "ray %d: the leaf's box is not culled at the bound" % i


def _agrees(rec, start, i, ts, ties):
    if rec["triangle"][i] >= 0:
        return ts[i].view(np.uint32) == rec["t"][i].view(np.uint32) and rec["triangle"][i] in ties[i]
    return not ts[i] < (rec["t"][i] if rec["object_id"][i] >= 0 else start[i])


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_bounded_walk_agrees_with_the_bounded_brute_force_minimum(name):
    o, d, _ = C.rays_of(name)
    u, m = C.uniforms_of(name), C.mesh_of(C.CASES[name][2])
    for which, listed in (("half", {}), ("one_and_a_half", C.EXCEPTIONS.get(name, {}))):
        rec = B.reference(name, which)
        start = B.start_of(B.t_max_of(name, which), len(o))
        ts, ids, ties = R.brute(u, o, d, m, t_max=start)
        assert len(listed) <= len(o) // 100, "at most 1 %% of %d rays may be listed" % len(o)
        bad = [i for i in range(len(o)) if not _agrees(rec, start, i, ts, ties)]
        assert bad == sorted(listed), "%s: bounded walk and brute force disagree on rays %s, listed %s" % (which, bad, sorted(listed))
    assert (B.reference(name, "one_and_a_half")["triangle"] >= 0).sum() >= 5


def test_min_is_the_glsls():
    t = np.array([np.nan, np.inf, -np.inf, 2e6, 1000000.0, 999999.9375, 0.0, -1.0], np.float32)
    s = B.start_of(t, len(t))
    assert np.array_equal(s[:5].view(np.uint32), np.array([R.INF, R.INF, -np.inf, R.INF, R.INF], np.float32).view(np.uint32))
    assert np.array_equal(s[5:], t[5:]) and (B.start_of(None, 3) == R.INF).all() and (B.start_of(5.0, 2) == 5.0).all()
