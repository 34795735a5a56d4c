"""SceneIntersect with a bound on hitT, for the bounded ray queries (test infrastructure, host only).

pt_cast_rays_ex (include/pt.h) is SceneIntersect with hitT starting at min(INFINITY, t_max) instead of INFINITY, the
GLSL's min (y < x ? y : x: a NaN, an infinite or any t_max >= 1000000.0 is no bound). This file composes that from
tests/raycast_ref.py's pieces, without changing them:

  1. raycast_ref.analytic, unbounded;
  2. every ray whose analytic t is not < the start is reset to a miss, and its hit_t set to the start;
  3. raycast_ref.walk(m, o, d, hit_t, dbl) and raycast_ref.mesh_attributes, as raycast_ref.cast does;
  4. t = INFINITY where object_id < 0 (the miss record carries INFINITY, not t_max);
  5. occluded() is object_id >= 0 of that.

Why step 2 is the GLSL with a lower start. The analytic part of SceneIntersect is a running minimum under a strict
`<`: hitT starts at s, and each object in turn does `if (d < hitT) { hitT = d; take it }`. Its final holder is the
first object, in the GLSL's order, that attains the minimum m of all the d's, whenever m < s, and nothing when not -
for any s: an object is taken iff its d is below every earlier d and below s, so the last one taken is the first
to attain m, provided m < s, and none is taken otherwise. With s = INFINITY that holder is what raycast_ref.analytic
returns; with a lower s the holder is the same object if m < s and nothing if not. The mesh is different: the walk
compares box distances with hitT as well, so a lower start culls boxes too, and the walk has to be run with it
(step 3) - filtering the unbounded record by t < t_max is not the same thing (ONE_ULP_CULLED below).

The t_max sets every bounded test uses, for a case of tests/raycast_cases.py whose unbounded reference has the
distances t_ref: SETS below. reference(name) computes each set's records once; callers leave them unchanged.
"""
import numpy as np

import raycast_cases as C
import raycast_ref as R

F = np.float32
INF = R.INF


def start_of(t_max, n):
    """min(INFINITY, t_max) per ray, the GLSL's min: (n,) float32. None is no bound."""
    if t_max is None:
        return np.full(n, INF, np.float32)
    t = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    return np.where(t < INF, t, INF).astype(np.float32)


def cast(scene, u, origins, dirs, t_max=None, mesh=None):
    """raycast_ref.cast with hitT starting at min(INFINITY, t_max[i]): RAY_HIT records."""
    ro, rd = R._rays(origins, dirs)
    n = ro[0].shape[0]
    start = start_of(t_max, n)
    out = np.zeros(n, R.RAY_HIT)
    out["object_id"], out["type"], out["triangle"] = -1, -100, -1
    with np.errstate(all="ignore"):
        count = R.analytic(scene, u, ro, rd, out)
        beyond = ~(out["t"] < start)
        miss = np.zeros(1, R.RAY_HIT)
        miss["object_id"], miss["type"], miss["triangle"] = -1, -100, -1
        out[beyond] = miss[0]
        hit_t = np.where(beyond, start, out["t"]).astype(np.float32)
        out["t"] = hit_t
        if scene in R.MESH_SCENES:
            m = R.Mesh(mesh)
            M, mo, md = R.model_space(u, ro, rd)
            dbl = R.double_sided(u)
            kind = R.PBR_MATERIAL if R._ui(u, "uModelUsesAlbedoTexture") else R._ui(u, "uModelMaterialType")
            for i in range(n):
                o, d = tuple(c[i] for c in mo), tuple(c[i] for c in md)
                t, tri_id, tu, tv, lookup = R.walk(m, o, d, hit_t[i], dbl)
                if not lookup:
                    continue
                normal, uv = R.mesh_attributes(m, M, tri_id, tu, tv)
                out[i] = (t, count, kind, int(tri_id) // 8, normal, tu, (1.0, 1.0, 1.0), tv, uv, (0.0, 0.0))
    out["t"][out["object_id"] < 0] = INF
    return out


def occluded(records):
    return records["object_id"] >= 0


# ------------------------------------------------------------------------------------------ the t_max sets

NO_BOUND = ("none", "nan", "inf", "2e6", "1e6")               # the unbounded records, to the bit
ALL_MISS = ("zero", "minus_one", "t_ref", "below_t_ref", "half")   # every ray misses
SETS = NO_BOUND + ALL_MISS + ("one_and_a_half", "above_t_ref")
GIVEN = SETS[1:]   # the sets that are an array: one call can carry them all, the rays repeated


def t_max_of(name, which):
    """The set's t_max for the case's rays: None or (n,) float32. t_ref is the unbounded reference's t."""
    t_ref = C.reference(name)["t"]
    n = len(t_ref)
    with np.errstate(all="ignore"):
        return {
            "none": lambda: None,
            "nan": lambda: np.full(n, np.nan, np.float32),
            "inf": lambda: np.full(n, np.inf, np.float32),
            "2e6": lambda: np.full(n, 2e6, np.float32),
            "1e6": lambda: np.full(n, 1000000.0, np.float32),
            "zero": lambda: np.zeros(n, np.float32),
            "minus_one": lambda: np.full(n, -1.0, np.float32),
            "t_ref": lambda: t_ref.copy(),
            "below_t_ref": lambda: np.nextafter(t_ref, F(-np.inf)),
            "half": lambda: F(0.5) * t_ref,
            "one_and_a_half": lambda: F(1.5) * t_ref,
            "above_t_ref": lambda: np.nextafter(t_ref, F(np.inf)),
        }[which]()


def reference(name, which):
    """The bounded reference's records for the case's rays under the set's t_max, once."""
    def make():
        o, d, _ = C.rays_of(name)
        key = C.CASES[name][2]
        return cast(C.scene_of(name), C.uniforms_of(name), o, d, t_max_of(name, which), C.mesh_of(key) if key is not None else None)
    return C._cached(("bounded", name, which), make)


# With t_max one ulp above the unbounded hit's t the records are the unbounded ones, but for these rays, by case and
# index: mesh hits of the unbounded reference that the bounded walk misses.
CULLED = ("the triangle's t is below the bound, but the slab test of its leaf's box gives a distance that is not (the "
          "box test and the triangle test round differently, and here the box's entry comes out an ulp or more "
          "beyond the triangle's t), so the walk with that start culls the leaf before it tests the triangle; the GLSL "
          "with that start does the same")
ONE_ULP_CULLED = {
    "gltf_teapot_skewed": {60: CULLED, 69: CULLED},
}
