"""The ray-query cases (test infrastructure, host only): scenes, meshes and seeded ray sets shared by
tests/test_raycast_ref.py (the reference against a brute-force minimum, on the CPU) and tests/test_gpu_raycast.py
(pt_cast_rays against the reference, on the device). A case's reference is computed once and shared; callers leave
it unchanged.

A mesh case's rays, a few hundred at most (the reference's walk is Python):
  * aimed at triangle interiors, edge midpoints and vertices of seeded triangles, from seeded origins around the model;
  * axis-parallel, with exact +0 and -0 components, through seeded points of the root box;
  * from inside the root box (its centre), and from beyond the mesh looking away from it;
  * out of the room's open side (and, without a ceiling, up): they miss everything;
  * a zero direction, one with a NaN component, one with an infinite component.
Directions are not normalised: t is in units of their length.
"""
import numpy as np

import helpers as H
import raycast_ref as R
import tree_shapes as T

IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
LAYOUTS = ("reference", "pairs", "trail")
K_ENDS = (0.01, 1.0)   # uShapeK's ends: what the reference page's control clamps it to (js/Transformed_Quadric_Geometry.js:893-902)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _meta(stream):
    return H.sky_mesh_stream() if stream == "skymesh" else H.stream(stream)


def _skewed():
    """A non-identity model transform: scale (1.5, 1, 0.5), rotations about all three axes and a translation, composed
    in float64 with settings_variants' helpers (as its skymesh_model_skewed); the uniform is its inverse in float32."""
    import settings_variants as S
    x = S._scale(1.5, 1.0, 0.5) @ S._rotate(37.0, 115.0, 290.0) @ S._translate(3.0, -2.0, 5.0)
    return [float(v) for v in np.linalg.inv(x).astype(np.float32).reshape(-1)]


# name -> (stream, uniform overrides, mesh key or None)
CASES = {
    "cornell": ("cornell_256", {}, None),
    "sky": ("sky_256", {}, None),
    "quadric_k001": ("quadric_256", {"uShapeK": ["f", [K_ENDS[0]]]}, None),
    "quadric_k1": ("quadric_256", {"uShapeK": ["f", [K_ENDS[1]]]}, None),
    "gltf_tiny1": ("gltf_teapot_320x180", {"uGLTF_Model_InvMatrix": ["f", IDENTITY]}, ("tiny", 1)),
    "gltf_tiny2": ("gltf_teapot_320x180", {"uGLTF_Model_InvMatrix": ["f", IDENTITY]}, ("tiny", 2)),
    "gltf_tiny3": ("gltf_teapot_320x180", {"uGLTF_Model_InvMatrix": ["f", IDENTITY]}, ("tiny", 3)),
    "gltf_chain28": ("gltf_teapot_320x180", {}, ("chain", "tight")),
    "gltf_chain28_loose": ("gltf_teapot_320x180", {}, ("chain", "loose")),
    "gltf_teapot": ("gltf_teapot_320x180", {}, ("teapot",)),
    "gltf_teapot_glass": ("gltf_teapot_320x180", {"uModelMaterialType": ["i", [R.TRANSPARENT]]}, ("teapot",)),
    "gltf_teapot_skewed": ("gltf_teapot_320x180", {"uGLTF_Model_InvMatrix": ["f", _skewed()]}, ("teapot",)),
    "hdri_teapot": ("hdri_teapot_320x180", {}, ("teapot",)),
    "skymesh_teapot": ("skymesh", {}, ("teapot",)),
    # the textured program variants: 1024 of the helmet's triangles with the seeded PBR maps bound (PBR_MATERIAL, and a
    # bump map, which the reference does not restate: BUMPED cases compare every field but `normal`)
    "gltf_helmet_maps": ("gltf_helmet_320x180", {}, ("helmet",)),
    "hdri_helmet_maps": ("hdri_helmet_320x180", {}, ("helmet",)),
}
BUMPED = ("gltf_helmet_maps", "hdri_helmet_maps")
MESH_CASES = tuple(n for n, c in CASES.items() if c[2] is not None)
# rays per case: the loose chain costs a ray about a thousand leaf tests in the reference
RAYS_PER_KIND = {"gltf_chain28_loose": 2}


# The seed of every mesh case's rays, chosen (tests/test_raycast_ref.py holds the choice to it) so that the
# reference's walk and a brute-force minimum over all triangles disagree on at most 1 % of the case's rays, and the
# rays on which they do, by index, with the reason.
SEEDS = {name: 1 for name in MESH_CASES}
GRAZING = ("a ray aimed at a vertex: a neighbour of the triangle the walk returns also passes the triangle test, a few "
           "ulps nearer, but the ray grazes that neighbour's leaf box and the slab test culls it, so the walk never "
           "tests it; the GLSL's walk does the same")
EXCEPTIONS = {
    "gltf_chain28": {49: GRAZING}, "gltf_teapot": {49: GRAZING}, "gltf_teapot_glass": {49: GRAZING},
    "gltf_teapot_skewed": {57: GRAZING}, "hdri_teapot": {49: GRAZING}, "skymesh_teapot": {49: GRAZING},
    "gltf_helmet_maps": {65: GRAZING}, "hdri_helmet_maps": {65: GRAZING},
}


def mesh_of(key):
    if key[0] == "tiny":
        return T.tiny_tree(key[1])
    if key[0] == "chain":
        return T.case_tree("teapot", "left28", key[1])
    if key[0] == "helmet":
        return T.case_tree("helmet1024", "balanced", "tight")
    return _cached("teapot-mesh", lambda: H.mesh("teapot"))


def scene_of(name):
    return _meta(CASES[name][0])["scene"]


def uniforms_of(name):
    stream, over, _ = CASES[name]
    u = dict(H.path_call(_meta(stream)["frames"][0])["uniforms"])
    u.update(over)
    return u


def _world_from_model(u):
    """p_world = p_model @ this (row vectors), in float64: the inverse of the recorded uGLTF_Model_InvMatrix."""
    return np.linalg.inv(np.array(u["uGLTF_Model_InvMatrix"][1], np.float64).reshape(4, 4))


def mesh_rays(name):
    """The seeded ray set of a mesh case: (origins, dirs) float32 (n, 3), and the index ranges by kind."""
    u = uniforms_of(name)
    m = mesh_of(CASES[name][2])
    rng = np.random.default_rng(SEEDS[name])
    per = RAYS_PER_KIND.get(name, 24)
    tri = np.asarray(m["tri"], np.float64)
    pos = tri[:, 0:9].reshape(-1, 3, 3)
    root = np.asarray(m["bvh"], np.float64).reshape(-1, 8)[0]
    lo, hi = root[1:4], root[5:8]
    to_world = _world_from_model(u)

    def world(p):
        p = np.atleast_2d(p)
        return (np.concatenate([p, np.ones((p.shape[0], 1))], 1) @ to_world)[:, :3]

    centre = world((lo + hi) * 0.5)[0]
    radius = float(np.linalg.norm(world(hi)[0] - centre))
    # origins on a sphere about the model: outside its box, but inside the room (the tiny trees' box is wider than it)
    far = 0.45 if CASES[name][2][0] == "tiny" else 1.6
    sets, kinds = [], {}

    def put(kind, o, d):
        o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        start = sum(len(s[0]) for s in sets)
        sets.append((o, d))
        kinds[kind] = (start, start + len(o))

    def around(n):
        v = rng.normal(size=(n, 3))
        return centre + v / np.linalg.norm(v, axis=1, keepdims=True) * radius * far

    pick = rng.integers(0, pos.shape[0], per)
    b = rng.dirichlet([1.0, 1.0, 1.0], per)
    inner = np.einsum("nk,nkc->nc", b, pos[pick])
    o = around(per)
    put("interior", o, world(inner) - o)
    edge = (pos[pick, np.arange(per) % 3] + pos[pick, (np.arange(per) + 1) % 3]) * 0.5
    o = around(per)
    put("edge", o, world(edge) - o)
    vert = pos[pick, np.arange(per) % 3]
    o = around(per)
    put("vertex", o, world(vert) - o)
    # axis-parallel through seeded points of the root box, both signs of each axis; the other two components are
    # exact zeros of either sign
    through = world(lo + rng.random((per, 3)) * (hi - lo))
    axis = np.arange(per) % 3
    sign = np.where((np.arange(per) // 3) % 2 == 0, 1.0, -1.0)
    d = np.where((np.arange(per) // 6) % 2 == 0, 0.0, -0.0)[:, None] * np.ones((per, 3))
    d[np.arange(per), axis] = sign * 3.0
    put("axis", through - d * radius, d)
    v = rng.normal(size=(per, 3))
    put("inside", np.tile(centre, (per, 1)), v)
    o = around(per)
    put("behind", o, o - centre)
    # out of the room's open side (-z), and up
    miss = np.column_stack([rng.uniform(-0.3, 0.3, per), rng.uniform(0.0, 0.3, per), -np.ones(per)])
    miss[::2] = np.column_stack([rng.uniform(-0.1, 0.1, per), np.ones(per), rng.uniform(-0.1, 0.1, per)])[::2]
    put("away", np.tile(centre + [0.0, 0.0, -60.0], (per, 1)), miss)
    o = around(3)
    d = world(inner[:1]) - o
    d[0] = 0.0
    d[1, 1] = np.nan
    d[2, 0] = np.inf
    put("degenerate", o, d)
    origins = np.concatenate([s[0] for s in sets]).astype(np.float32)
    dirs = np.concatenate([s[1] for s in sets]).astype(np.float32)
    return origins, dirs, kinds


def room_rays(name):
    """A program without a mesh: camera rays of a 16 x 12 grid over the recorded view (they find every sphere or shape
    and the walls), rays from the room's centre in seeded directions, axis-parallel rays with exact zeros of either
    sign, rays up to the ceiling's quad light, and the three degenerate directions."""
    u = uniforms_of(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    cam = np.array(u["uCameraMatrix"][1], np.float64)
    ul, vl = u["uULen"][1][0], u["uVLen"][1][0]
    xs, ys = np.meshgrid((np.arange(16) + 0.5) / 16 * 2 - 1, (np.arange(12) + 0.5) / 12 * 2 - 1)
    d = (cam[0:3][None] * (xs.reshape(-1, 1) * ul) + cam[4:7][None] * (ys.reshape(-1, 1) * vl) + cam[8:11][None]) * 7.0
    o = np.tile(cam[12:15], (d.shape[0], 1))
    v = rng.normal(size=(48, 3))
    o, d = np.concatenate([o, np.zeros((48, 3))]), np.concatenate([d, v])
    ax = np.where(np.arange(12)[:, None] // 6 % 2 == 0, 0.0, -0.0) * np.ones((12, 3))
    ax[np.arange(12), np.arange(12) % 3] = np.where(np.arange(12) // 3 % 2 == 0, 2.0, -2.0)
    o, d = np.concatenate([o, rng.uniform(-30.0, 30.0, (12, 3))]), np.concatenate([d, ax])
    up = np.column_stack([rng.uniform(-0.02, 0.02, 8), np.ones(8), rng.uniform(-0.02, 0.02, 8)])   # to the ceiling's light
    o, d = np.concatenate([o, rng.uniform(-3.0, 3.0, (8, 3))]), np.concatenate([d, up])
    deg = rng.normal(size=(3, 3))
    deg[0] = 0.0
    deg[1, 2] = np.nan
    deg[2, 1] = -np.inf
    o, d = np.concatenate([o, rng.uniform(-30.0, 30.0, (3, 3))]), np.concatenate([d, deg])
    return o.astype(np.float32), d.astype(np.float32), {}


def rays_of(name):
    return _cached(("rays", name), lambda: (mesh_rays if CASES[name][2] is not None else room_rays)(name))


def reference(name):
    """The reference's records for the case's rays, once."""
    def make():
        o, d, _ = rays_of(name)
        key = CASES[name][2]
        return R.cast(scene_of(name), uniforms_of(name), o, d, mesh_of(key) if key is not None else None)
    return _cached(("ref", name), make)
