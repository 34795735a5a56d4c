"""SceneIntersect restated for ray queries (test infrastructure, host only).

An independent restatement, in numpy float32, of what the reference's fragment programs compute in
SceneIntersect for one ray - js/BabylonPathTracing_FragmentShader.js:47-112 (Cornell),
js/PhysicalSkyModel_FragmentShader.js:48-113 (sky), js/GLTFModelPathTracing_FragmentShader.js:116-346 (glTF; the
HDRI program's is the same text over four quads), js/TransformedQuadricGeometry_FragmentShader.js:77-317 (the
twelve shapes) and SetupScene() of each - written from the GLSL, not from the HIP kernels. One IEEE binary32
operation per GLSL operation, in the GLSL's order (DESIGN.md "Parity": products and sums left to right, cross as
a.y b.z - b.y a.z, min(x, y) = y < x ? y : x, normalize(v) = v * (1 / sqrt(dot(v, v))), '/' and sqrt correctly
rounded). The sky + mesh composite has no shader of its own in the reference: it is the sky program's spheres and
quads with the glTF program's model block appended.

The analytic objects are evaluated for all rays at once (numpy arrays, one rounding per operation, selects in
place of branches); the BVH walk is the GLSL's stack walk, ray by ray. The twelve quadric intersectors are the
oracle's (ptoracle.quadric_probe), fed rays this file has moved to object space itself.

cast(scene, uniforms, origins, dirs, mesh=None) returns records with the fields of pt_ray_hit (include/pt.h).
Bump-mapped normals are not restated: with uModelUsesBumpTexture set, `normal` holds the interpolated normal
under the model transform, and the caller compares every field but that one.

brute(...) is the same triangle test over every triangle, without a tree: what the walk is checked against.
"""
import numpy as np

F = np.float32
INF = F(1000000.0)                 # #define INFINITY 1000000.0
LIGHT, DIFFUSE, TRANSPARENT, METAL, CLEARCOAT_DIFFUSE, PBR_MATERIAL = 0, 1, 2, 3, 4, 10

RAY_HIT = np.dtype([("t", "<f4"), ("object_id", "<i4"), ("type", "<i4"), ("triangle", "<i4"), ("normal", "<f4", (3,)),
                    ("bary_u", "<f4"), ("color", "<f4", (3,)), ("bary_v", "<f4"), ("uv", "<f4", (2,)),
                    ("reserved", "<f4", (2,))])

MESH_SCENES = ("gltf", "hdri", "skymesh")
QUADRIC_MATRICES = ("uSphereInvMatrix", "uCylinderInvMatrix", "uConeInvMatrix", "uParaboloidInvMatrix",
                    "uHyperboloidInvMatrix", "uCapsuleInvMatrix", "uFlattenedRingInvMatrix", "uBoxInvMatrix",
                    "uPyramidFrustumInvMatrix", "uDiskInvMatrix", "uRectangleInvMatrix", "uTorusInvMatrix")
QUADRIC_COLORS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (1.0, 0.1, 0.0), (0.5, 1.0, 0.0),
                  (0.0, 0.4, 1.0), (0.0, 0.0, 1.0), (0.2, 0.0, 1.0), (0.0, 1.0, 0.5), (1.0, 0.3, 0.0), (0.5, 0.0, 1.0))


# ------------------------------------------------------------------------------------------ GLSL built-ins
# a vec3 is a tuple of three float32 scalars or three float32 arrays

def vec(x, y, z):
    return (F(x), F(y), F(z))


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def gmin(x, y):
    return np.where(y < x, y, x)


def gmax(x, y):
    return np.where(x < y, y, x)


def normalize(a):
    inv = F(1.0) / np.sqrt(dot(a, a))
    return scale(a, inv)


def mat_point(m, v, w):
    """vec3(M * vec4(v, w)) for a column-major mat4 of 16 float32."""
    w = F(w)
    return tuple(m[r] * v[0] + m[4 + r] * v[1] + m[8 + r] * v[2] + m[12 + r] * w for r in range(3))


def mat3_transposed(m, n):
    """transpose(mat3(M)) * n."""
    return tuple(m[4 * r] * n[0] + m[4 * r + 1] * n[1] + m[4 * r + 2] * n[2] for r in range(3))


# ------------------------------------------------------------------------------------------ intersectors

def unit_sphere(ro, rd):
    """UnitSphereIntersect with solveQuadratic (js/PathTracingCommon.js:631-685): (t, n)."""
    a = dot(rd, rd)
    b = F(2.0) * dot(rd, ro)
    c = dot(ro, ro) - F(1.0)
    inv_a = F(1.0) / a
    b = b * inv_a
    c = c * inv_a
    neg_half_b = -b * F(0.5)
    u2 = neg_half_b * neg_half_b - c
    neg = u2 < F(0.0)
    neg_half_b = np.where(neg, F(0.0), neg_half_b)
    u = np.where(neg, F(0.0), np.sqrt(np.where(neg, F(0.0), u2)))
    t0 = neg_half_b - u
    t1 = neg_half_b + u
    t = np.where(t0 > F(0.0), t0, np.where(t1 > F(0.0), t1, INF))
    hit = add(ro, scale(rd, t))
    return t, (F(2.0) * hit[0], F(2.0) * hit[1], F(2.0) * hit[2])


def triangle(v0, v1, v2, ro, rd, double_sided):
    """TriangleIntersect / BVH_TriangleIntersect / BVH_DoubleSidedTriangleIntersect
    (js/PathTracingCommon.js:1168-1182, 1214-1245): (t, u, v). The single-sided forms differ only in where they test
    det < 0; both give INFINITY for it."""
    edge1 = sub(v1, v0)
    edge2 = sub(v2, v0)
    pvec = cross(rd, edge2)
    det = F(1.0) / dot(edge1, pvec)
    tvec = sub(ro, v0)
    u = dot(tvec, pvec) * det
    qvec = cross(tvec, edge1)
    v = dot(rd, qvec) * det
    t = dot(edge2, qvec) * det
    miss = (u < F(0.0)) | (u > F(1.0)) | (v < F(0.0)) | (u + v > F(1.0)) | (t <= F(0.0))
    if not double_sided:
        miss = miss | (det < F(0.0))
    return np.where(miss, INF, t), u, v


def quad(q, ro, rd):
    """QuadIntersect(v0, v1, v2, v3, ro, rd, false)."""
    t1, _, _ = triangle(q["v0"], q["v1"], q["v2"], ro, rd, False)
    t2, _, _ = triangle(q["v0"], q["v2"], q["v3"], ro, rd, False)
    return gmin(t1, t2)


def bounding_box(mn, mx, ro, inv):
    """BoundingBoxIntersect (js/PathTracingCommon.js:1194-1207)."""
    near = tuple((mn[k] - ro[k]) * inv[k] for k in range(3))
    far = tuple((mx[k] - ro[k]) * inv[k] for k in range(3))
    tmin = tuple(gmin(near[k], far[k]) for k in range(3))
    tmax = tuple(gmax(near[k], far[k]) for k in range(3))
    t0 = gmax(gmax(tmin[0], tmin[1]), tmin[2])
    t1 = gmin(gmin(tmax[0], tmax[1]), tmax[2])
    return np.where(gmax(t0, F(0.0)) > t1, INF, t0)


# ------------------------------------------------------------------------------------------ SetupScene

def _uf(u, name, k=0):
    e = u.get(name)
    return F(e[1][k]) if e is not None and k < len(e[1]) else F(0.0)


def _ui(u, name):
    e = u.get(name)
    return int(e[1][0]) if e is not None else 0


def _um4(u, name):
    e = u.get(name)
    return np.array(e[1], np.float32) if e is not None else np.zeros(16, np.float32)


def _quad(normal, v0, v1, v2, v3, color, kind):
    return {"normal": vec(*normal), "v0": vec(*v0), "v1": vec(*v1), "v2": vec(*v2), "v3": vec(*v3),
            "color": vec(*color), "type": kind}


def setup_scene(scene, u):
    """SetupScene() of the scene's shader: (spheres, quads). The quad light needs a uQuadLightPlaneSelectionNumber
    of 1..6 (the GLSL leaves quads[5] unset otherwise)."""
    W = F(50.0)
    spheres = [{"color": vec(1.0, 1.0, 0.0), "type": CLEARCOAT_DIFFUSE},
               {"color": vec(1.0, 1.0, 1.0), "type": METAL if scene in ("gltf", "hdri") else _ui(u, "uRightSphereMatType")}]
    white = (1.0, 1.0, 1.0)
    back = _quad((0, 0, 1), (-W, W, W), (W, W, W), (W, -W, W), (-W, -W, W), white, DIFFUSE)
    left = _quad((1, 0, 0), (-W, -W, W), (-W, -W, -W), (-W, W, -W), (-W, W, W), (0.7, 0.05, 0.05), DIFFUSE)
    right = _quad((-1, 0, 0), (W, -W, -W), (W, -W, W), (W, W, W), (W, W, -W), (0.05, 0.05, 0.7), DIFFUSE)
    ceiling = _quad((0, -1, 0), (-W, W, -W), (W, W, -W), (W, W, W), (-W, W, W), white, DIFFUSE)
    floor = _quad((0, 1, 0), (-W, -W, W), (W, -W, W), (W, -W, -W), (-W, -W, -W), white, DIFFUSE)
    if scene in ("hdri", "sky", "skymesh"):   # N_QUADS 4: no ceiling, no quad light
        return spheres, [back, left, right, floor]
    L = _uf(u, "uQuadLightRadius") * F(0.2)
    E = tuple(F(1.0) * F(10.0) for _ in range(3))
    wm, wp = W - F(1.0), -W + F(1.0)
    sel = float(_uf(u, "uQuadLightPlaneSelectionNumber"))
    light = {
        1.0: ((-1, 0, 0), (wm, -L, L), (wm, L, L), (wm, L, -L), (wm, -L, -L)),
        2.0: ((1, 0, 0), (wp, -L, -L), (wp, L, -L), (wp, L, L), (wp, -L, L)),
        3.0: ((0, 0, 1), (-L, -L, wp), (L, -L, wp), (L, L, wp), (-L, L, wp)),
        4.0: ((0, 0, -1), (-L, -L, wm), (-L, L, wm), (L, L, wm), (L, -L, wm)),
        5.0: ((0, 1, 0), (-L, wp, -L), (-L, wp, L), (L, wp, L), (L, wp, -L)),
        6.0: ((0, -1, 0), (-L, wm, -L), (L, wm, -L), (L, wm, L), (-L, wm, L)),
    }[sel]
    return (spheres if scene != "quadric" else []), [back, left, right, ceiling, floor, _quad(*light, E, LIGHT)]


# ------------------------------------------------------------------------------------------ the model block

class Mesh:
    """tAABBTexture / tTriangleTexture as texelFetch sees them: texel i of the 2048-wide texture is floats
    4 i .. 4 i + 3 of the flat upload, zero outside it."""

    def __init__(self, mesh):
        self.bvh = np.ascontiguousarray(mesh["bvh"], np.float32).reshape(-1, 4)
        self.tri = np.ascontiguousarray(mesh["tri"], np.float32).reshape(-1, 4)

    @staticmethod
    def _fetch(tex, i):
        i = float(i)
        if not (0.0 <= i < tex.shape[0]):
            return np.zeros(4, np.float32)
        return tex[int(i)]

    def node(self, i):
        """GetBoxNodeData(i): the two texels of node i."""
        ix2 = F(i) * F(2.0)
        return self._fetch(self.bvh, ix2), self._fetch(self.bvh, ix2 + F(1.0))

    def tri_texel(self, i):
        return self._fetch(self.tri, i)


def walk(m, ro, rd, hit_t, double_sided):
    """The stack walk of js/GLTFModelPathTracing_FragmentShader.js:201-298 for one model-space ray:
    (hitT, triangleID, triangleU, triangleV, triangleLookupNeeded). stackLevels holds 28 entries; a walk that
    would need more is refused (the GLSL writes past the array)."""
    with np.errstate(all="ignore"):
        inv = tuple(F(1.0) / c for c in rd)
        stack = [None] * 28
        stackptr = 0
        cur0, cur1 = m.node(F(0.0))
        cur = (F(0.0), bounding_box(cur0[1:4], cur1[1:4], ro, inv))
        stack[0] = cur
        skip = bool(cur[1] < hit_t)
        tri_id, tri_u, tri_v, lookup = F(0.0), F(0.0), F(0.0), False
        while True:
            if not skip:
                stackptr -= 1
                if stackptr < 0:
                    break
                cur = stack[stackptr]
                if cur[1] >= hit_t:
                    continue
                cur0, cur1 = m.node(cur[0])
            skip = False
            if cur0[0] < F(0.0):
                id_a, id_b = cur[0] + F(1.0), cur1[0]
                a0, a1 = m.node(id_a)
                b0, b1 = m.node(id_b)
                sa = (id_a, bounding_box(a0[1:4], a1[1:4], ro, inv))
                sb = (id_b, bounding_box(b0[1:4], b1[1:4], ro, inv))
                if sb[1] < sa[1]:
                    sa, sb = sb, sa
                    a0, a1, b0, b1 = b0, b1, a0, a1
                if sb[1] < hit_t:
                    cur, cur0, cur1 = sb, b0, b1
                    skip = True
                if sa[1] < hit_t:
                    if skip:
                        if stackptr >= 28:
                            raise OverflowError("the walk needs more than stackLevels[28]")
                        stack[stackptr] = sb
                        stackptr += 1
                    cur, cur0, cur1 = sa, a0, a1
                    skip = True
                continue
            tid = F(8.0) * cur0[0]
            vd0, vd1, vd2 = m.tri_texel(tid), m.tri_texel(tid + F(1.0)), m.tri_texel(tid + F(2.0))
            d, tu, tv = triangle(tuple(vd0[0:3]), (vd0[3], vd1[0], vd1[1]), (vd1[2], vd1[3], vd2[0]), ro, rd, double_sided)
            if d < hit_t:
                hit_t, tri_id, tri_u, tri_v, lookup = F(d), tid, F(tu), F(tv), True
        return hit_t, tri_id, tri_u, tri_v, lookup


def mesh_attributes(m, model, tri_id, u, v):
    """The triangle lookup (js/GLTFModelPathTracing_FragmentShader.js:302-344): (hitNormal, hitUV), without the
    bump map."""
    with np.errstate(all="ignore"):
        vd = [m.tri_texel(tri_id + F(k)) for k in range(6)]
        w = F(1.0) - u - v
        n = add(add(scale(tuple(vd[2][1:4]), w), scale(tuple(vd[3][0:3]), u)), scale((vd[3][3], vd[4][0], vd[4][1]), v))
        n = normalize(n)
        uv = (w * vd[4][2] + u * vd[5][0] + v * vd[5][2], w * vd[4][3] + u * vd[5][1] + v * vd[5][3])
        return normalize(mat3_transposed(model, n)), uv


# ------------------------------------------------------------------------------------------ SceneIntersect

def _rays(origins, dirs):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    assert o.shape == d.shape
    return tuple(o[:, k].copy() for k in range(3)), tuple(d[:, k].copy() for k in range(3))


def analytic(scene, u, ro, rd, out):
    """The spheres (or the twelve shapes) and the quads, for all rays at once, into the records `out`."""
    n = out.shape[0]
    spheres, quads = setup_scene(scene, u)
    t = np.full(n, INF, np.float32)
    count = 0

    def take(d, normal, color, kind, oid):
        nonlocal t
        closer = d < t
        t = np.where(closer, d, t)
        for k in range(3):
            out["normal"][:, k] = np.where(closer, normal[k], out["normal"][:, k])
            out["color"][:, k] = np.where(closer, F(color[k]), out["color"][:, k])
        out["type"] = np.where(closer, kind, out["type"])
        out["object_id"] = np.where(closer, oid, out["object_id"])

    if scene == "quadric":
        import ptoracle as po
        k = float(_uf(u, "uShapeK"))
        for s, name in enumerate(QUADRIC_MATRICES):
            M = _um4(u, name)
            o, d = mat_point(M, ro, 1.0), mat_point(M, rd, 0.0)
            dist, nrm = po.quadric_probe(s, k, np.stack(o, -1), np.stack(d, -1))
            hn = vec(0.0, -1.0, 0.0) if s in (9, 10) else normalize(tuple(nrm[:, c] for c in range(3)))
            hn = tuple(np.broadcast_to(c, (n,)) for c in hn)
            take(dist, normalize(mat3_transposed(M, hn)), QUADRIC_COLORS[s], _ui(u, "uAllShapesMatType"), count)
            count += 1
    else:
        for s, name in enumerate(("uLeftSphereInvMatrix", "uRightSphereInvMatrix")):
            M = _um4(u, name)
            dist, nrm = unit_sphere(mat_point(M, ro, 1.0), mat_point(M, rd, 0.0))
            take(dist, normalize(mat3_transposed(M, normalize(nrm))), spheres[s]["color"], spheres[s]["type"], count)
            count += 1
    for q in quads:
        take(quad(q, ro, rd), tuple(np.broadcast_to(c, (n,)) for c in normalize(q["normal"])), q["color"], q["type"], count)
        count += 1
    out["t"] = t
    return count


def model_space(u, ro, rd):
    M = _um4(u, "uGLTF_Model_InvMatrix")
    return M, mat_point(M, ro, 1.0), mat_point(M, rd, 0.0)


def double_sided(u):
    return not _ui(u, "uModelUsesAlbedoTexture") and _ui(u, "uModelMaterialType") == TRANSPARENT


def cast(scene, u, origins, dirs, mesh=None):
    """SceneIntersect of `scene` ("cornell", "sky", "quadric", "gltf", "hdri", "skymesh") under the path-tracing
    uniforms `u` (a recorded call's {name: [kind, values]}) for every ray: RAY_HIT records."""
    ro, rd = _rays(origins, dirs)
    n = ro[0].shape[0]
    out = np.zeros(n, RAY_HIT)
    out["object_id"], out["type"], out["triangle"] = -1, -100, -1
    with np.errstate(all="ignore"):
        count = analytic(scene, u, ro, rd, out)
        if scene not in MESH_SCENES:
            return out
        m = Mesh(mesh)
        M, mo, md = model_space(u, ro, rd)
        dbl = double_sided(u)
        kind = PBR_MATERIAL if _ui(u, "uModelUsesAlbedoTexture") else _ui(u, "uModelMaterialType")
        for i in range(n):
            o, d = tuple(c[i] for c in mo), tuple(c[i] for c in md)
            t, tri_id, tu, tv, lookup = walk(m, o, d, out["t"][i], dbl)
            if not lookup:
                continue
            normal, uv = mesh_attributes(m, M, tri_id, tu, tv)
            out[i] = (t, count, kind, int(tri_id) // 8, normal, tu, (1.0, 1.0, 1.0), tv, uv, (0.0, 0.0))
    return out


def brute(u, origins, dirs, mesh, t_max=None):
    """The mesh alone, without a tree: per ray the minimum of the walk's triangle test over every triangle record,
    closer than `t_max` (default INFINITY): (t, triangle, ties). Where several triangles share the minimum to the
    bit - a ray through a shared edge or vertex - `triangle` is the first in record order and ties[i] lists them all:
    the walk keeps the first it meets in its own, near-first order. INFINITY, -1 and an empty list where nothing is
    closer."""
    ro, rd = _rays(origins, dirs)
    n = ro[0].shape[0]
    tri = np.ascontiguousarray(mesh["tri"], np.float32).reshape(-1, 32)
    v0, v1, v2 = (tuple(tri[:, 3 * k + c] for c in range(3)) for k in range(3))
    ts = np.full(n, INF, np.float32) if t_max is None else np.array(t_max, np.float32)
    ids = np.full(n, -1, np.int32)
    ties = [np.zeros(0, np.int64)] * n
    with np.errstate(all="ignore"):
        _, mo, md = model_space(u, ro, rd)
        dbl = double_sided(u)
        for i in range(n):
            d, _, _ = triangle(v0, v1, v2, tuple(c[i] for c in mo), tuple(c[i] for c in md), dbl)
            d = np.where(d == d, d, INF)   # a NaN distance (a degenerate ray) is closer than nothing, as in the walk
            j = int(np.argmin(d))          # (the first of equal minima)
            if d[j] < ts[i]:
                ts[i], ids[i], ties[i] = d[j], j, np.nonzero(d == d[j])[0]
    return ts, ids, ties
