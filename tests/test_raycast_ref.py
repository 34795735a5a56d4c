"""The ray-query reference (tests/raycast_ref.py) checked against something that is not a walk.

On every mesh case of tests/raycast_cases.py the reference's walk is compared, ray by ray, with a brute-force
minimum of the same triangle test over all triangle records (raycast_ref.brute): a mesh hit has the brute minimum's
t to the bit and a triangle that attains it (several may, through a shared edge or vertex: the walk keeps the first
it meets in its own order), and where the walk reports no mesh hit no triangle is closer than what it did hit. The
only rays excused are those the case table lists by index with a reason, at most 1 % of a case's rays, and the
reason is checked too. The non-finite rays' walks end, and the records have the layout of pt_ray_hit."""
import numpy as np
import pytest

import raycast_cases as C
import raycast_ref as R


def _agrees(ref, i, ts, ties):
    if ref["triangle"][i] >= 0:
        return ts[i].view(np.uint32) == ref["t"][i].view(np.uint32) and ref["triangle"][i] in ties[i]
    return not ts[i] < ref["t"][i]


def _leaf_of(bvh, triangle):
    return int(np.nonzero((bvh[:, 0] == triangle) & (bvh[:, 4] == -1.0))[0][0])


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_walk_agrees_with_the_brute_force_minimum(name):
    o, d, _ = C.rays_of(name)
    ref = C.reference(name)
    u, m = C.uniforms_of(name), C.mesh_of(C.CASES[name][2])
    ts, ids, ties = R.brute(u, o, d, m)
    listed = C.EXCEPTIONS.get(name, {})
    assert len(listed) <= len(o) // 100, "at most 1 %% of %d rays may be listed" % len(o)
    bad = [i for i in range(len(o)) if not _agrees(ref, i, ts, ties)]
    assert bad == sorted(listed), "walk and brute force disagree on rays %s, listed %s" % (bad, sorted(listed))
    assert (ref["triangle"] >= 0).sum() >= 5, "the case's rays hardly hit its mesh"
    # the reason, checked: brute force found a nearer triangle whose leaf box the slab test culls for this ray
    bvh = np.asarray(m["bvh"], np.float32).reshape(-1, 8)
    ro, rd = R._rays(o, d)
    with np.errstate(all="ignore"):
        _, mo, md = R.model_space(u, ro, rd)
    for i in listed:
        assert ts[i] < ref["t"][i]
        leaf = bvh[_leaf_of(bvh, ids[i])]
        with np.errstate(all="ignore"):
            inv = tuple(R.F(1.0) / c[i] for c in md)
            box_t = R.bounding_box(leaf[1:4], leaf[5:8], tuple(c[i] for c in mo), inv)
        assert not box_t < ref["t"][i], "ray %d: the nearer triangle's leaf box is not culled" % i


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_every_kind_of_ray_is_there(name):
    """Interiors, edges and vertices are hit; rays looking away from the mesh and out of the room hit no triangle;
    the axis rays carry exact zeros of both signs; the degenerate rays are the last three."""
    o, d, kinds = C.rays_of(name)
    ref = C.reference(name)
    for kind in ("interior", "edge", "vertex"):
        a, b = kinds[kind]
        assert (ref["triangle"][a:b] >= 0).any(), kind
    # (the tiny trees' box is wider than the room: their rays start inside it, and "behind" may look at a triangle)
    for kind in ("away",) if C.CASES[name][2][0] == "tiny" else ("behind", "away"):
        a, b = kinds[kind]
        assert (ref["triangle"][a:b] < 0).all(), kind
    a, b = kinds["away"]
    assert (ref["object_id"][a:b] < 0).any(), "no ray misses everything"
    a, b = kinds["axis"]
    zeros = d[a:b][d[a:b] == 0.0]
    assert zeros.size == 2 * (b - a) and (len(zeros) < 12 or (np.signbit(zeros).any() and not np.signbit(zeros).all()))
    a, b = kinds["degenerate"]
    assert b == len(o) and not d[a].any() and np.isnan(d[a + 1]).sum() == 1 and np.isinf(d[a + 2]).sum() == 1


def test_a_miss_is_the_documented_record():
    ref = C.reference("sky")
    miss = ref[ref["object_id"] < 0]
    assert len(miss) > 10
    assert (miss["t"] == R.INF).all() and (miss["type"] == -100).all() and (miss["triangle"] == -1).all()
    rest = np.ascontiguousarray(miss).view(np.uint32).reshape(len(miss), 16)[:, 4:]
    assert not rest.any(), "every other field of a miss is +0.0"


def test_room_programs_find_their_objects():
    """Cornell and sky: both spheres and the walls; quadrics: all twelve shapes at both ends of uShapeK but the two
    that vanish at the small end."""
    for name, ids in (("cornell", range(8)), ("sky", range(6))):
        assert set(ids) <= set(C.reference(name)["object_id"].tolist()), name
    assert len(set(C.reference("quadric_k1")["object_id"].tolist()) & set(range(12))) >= 10
    a, b = C.reference("quadric_k001"), C.reference("quadric_k1")
    assert not np.array_equal(a["t"], b["t"]), "uShapeK changes nothing"


def test_record_layout_is_pt_ray_hit():
    import babylon_pt as bp
    assert R.RAY_HIT == bp.RAY_HIT and R.RAY_HIT.itemsize == 64
    assert [R.RAY_HIT.fields[f][1] for f in ("t", "object_id", "type", "triangle", "normal", "bary_u", "color", "bary_v",
                                              "uv", "reserved")] == [0, 4, 8, 12, 16, 28, 32, 44, 48, 56]
    assert np.float32(R.INF) == bp.RAY_MISS_T


def test_camera_ray_is_the_shaders_pinhole_ray():
    """Effect.camera_ray without a device: the origin is the camera's position, and a pixel's direction is main()'s
    float32 sequence for the pixel's centre, normalised."""
    import babylon_pt as bp
    fx = bp.Effect(None, None)
    u = C.uniforms_of("cornell")
    for name in ("uCameraMatrix", "uULen", "uVLen"):
        fx._cache[name] = np.array(u[name][1], np.float32).tobytes()
    f = np.float32
    cam = np.array(u["uCameraMatrix"][1], np.float32)
    o, d = fx.camera_ray(1, 2, 8, 8)
    assert np.array_equal(o, cam[12:15])
    ppx, ppy = (f(1.5) / f(8)) * f(2) - f(1), (f(2.5) / f(8)) * f(2) - f(1)
    v = (cam[0:3] * ppx) * f(u["uULen"][1][0]) + (cam[4:7] * ppy) * f(u["uVLen"][1][0]) + cam[8:11]
    v = v * (f(1) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    assert np.array_equal(d.view(np.uint32), v.astype(np.float32).view(np.uint32))
    assert abs(float(np.linalg.norm(d.astype(np.float64))) - 1.0) < 1e-6
