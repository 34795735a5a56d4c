"""Directed inputs for the BVH builders, with the reference builder's own answer (build container only).

Builds small box sets that reach the builder's edges (signed zeros whose winner depends on the work
order, NaN bounds, every tie of the three extents, centroids exactly on a split, a split between two
adjacent floats, the second and third axis, the alternate deal, 199-level chains, infinities, a work
list with repeats, one to three boxes), runs each through the reference's unmodified
BVH_Build_Iterative under node (bvh_cases.js: js/babylon.js and js/BVH_Fast_Builder.js are loaded
from PT_REFERENCE at run time) and writes tests/golden/bvh_cases.npz:

  names, tris, works  per case: its name, its triangle count and the length m of its work list
  aabb_in  (sum tris, 9) uint32: the float32 bits of min.xyz, max.xyz, centroid.xyz per triangle
  work     (sum m,) uint32: the work lists
  nodes    (sum (2m - 1), 8) uint32: the float32 bits of the node arrays the reference leaves

The cases lie one after another in the three arrays (forty small cases as members of their own would
spend a third of the file on zip and .npy headers); tests/test_bvh_cases.py cuts them apart again.
Bits, not floats, so that NaNs and the signs of zeros survive. The file is written with fixed zip
dates: the same inputs give the same bytes (tests/test_bvh_cases.py regenerates and compares).

usage: python tests/golden/gen/make_bvh_cases.py [output .npz]
"""
import io
import itertools
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
QNAN = 0x7FC00000   # the canonical quiet NaN: the only one a JS engine is sure to write back unchanged
F = np.float32


def boxes(lo, hi, c=None):
    lo = np.asarray(lo, F); hi = np.asarray(hi, F)
    c = (lo + hi) * F(0.5) if c is None else np.asarray(c, F)
    return np.ascontiguousarray(np.concatenate([lo, hi, c], 1).astype(F))


def points(c):
    c = np.asarray(c, F)
    return boxes(c, c, c)


def dyadic(rng, shape, scale=1.0, bits=4):
    """Uniform in [0, scale) on a grid of 2^-bits * scale: exact in float32, and the file stays small."""
    return (rng.integers(0, 1 << bits, shape).astype(F) / F(1 << bits)) * F(scale)


def set_bits(a, row, col, value):
    a.view(np.uint32)[row, col] = value


def zeros_plane(cases):
    """196 thin boxes on a 14 x 14 lattice in the plane z = 0: min.z and max.z are +0 or -0 by the
    RNG, and so are min.x and min.y of the column and the row at the lattice's edge, on x = 0 and y = 0."""
    rng = np.random.default_rng(101)
    i, j = np.meshgrid(np.arange(14), np.arange(14), indexing="ij")
    x = i.ravel().astype(F) * F(0.5); y = j.ravel().astype(F) * F(0.5)
    z = np.zeros_like(x)
    a = boxes(np.stack([x, y, z], 1), np.stack([x + F(0.5), y + F(0.5), z], 1))
    u = a.view(np.uint32)
    for col in (0, 1, 2, 3, 4, 5, 8):   # every bound (and the z centroid) that is a zero gets a random sign
        zero = (u[:, col] & 0x7FFFFFFF) == 0
        u[:, col] = np.where(zero, rng.integers(0, 2, len(a)).astype(np.uint32) << 31, u[:, col])
    assert ((u[:, 0] & 0x7FFFFFFF) == 0).sum() == 14 and ((u[:, 1] & 0x7FFFFFFF) == 0).sum() == 14
    perm = rng.permutation(len(a)).astype(np.uint32)
    cases.append(("zeros_plane", a, np.arange(len(a), dtype=np.uint32)))
    cases.append(("zeros_plane_permuted", a, perm))
    cases.append(("zeros_plane_subset", a, rng.permutation(len(a))[:131].astype(np.uint32)))


def nan_bounds(cases):
    """150 boxes: 110 in the unit cube and a cluster of 40 far out on x, which the root split isolates
    as a run. Single NaN mins, single NaN maxes, one NaN centroid, and the cluster's whole min.x."""
    rng = np.random.default_rng(102)
    lo = dyadic(rng, (150, 3)); lo[110:, 0] += F(100.0)
    hi = lo + dyadic(rng, (150, 3), 0.25) + F(1.0 / 64)
    a = boxes(lo, hi)                       # centroids from the clean bounds
    order = rng.permutation(150)
    a = a[order]
    cluster = np.nonzero(order >= 110)[0]
    free = np.nonzero(order < 110)[0]
    for n, row in enumerate(free[:12]):     # single mins: x, y, z in turn
        set_bits(a, row, n % 3, QNAN)
    for n, row in enumerate(free[12:24]):   # single maxes
        set_bits(a, row, 3 + n % 3, QNAN)
    set_bits(a, free[24], 7, QNAN)          # a centroid (y: the x split must still isolate the cluster)
    set_bits(a, free[25], 1, QNAN); set_bits(a, free[25], 4, QNAN)   # min.y and max.y of one box
    for row in cluster:
        set_bits(a, row, 0, QNAN)
    set_bits(a, cluster[3], 5, QNAN)        # and one max inside the cluster
    cases.append(("nan_bounds", a, np.arange(150, dtype=np.uint32)))


def lattice(k, rng):
    g = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3).astype(F)
    return g[rng.permutation(len(g))]


def extent_ties(cases):
    """Lattices of unit cubes: every ordering and every tie of the three extents, with centroids
    exactly on a split wherever a run is an odd number of cubes long. A lattice of cubes separates
    on its first axis whenever that axis is two or more cubes long, so the second and third entries
    of the axis order decide nothing there; the slabs do that: every box spans one axis in full (so
    all centroids agree on it, and it is the longest or tied for the longest), and the other two
    axes are a lattice."""
    rng = np.random.default_rng(103)
    dims = list(itertools.permutations((4, 3, 2))) + [(4, 4, 2), (4, 2, 4), (2, 4, 4), (4, 2, 2), (2, 4, 2),
                                                      (2, 2, 4), (4, 4, 4)]
    for k in dims:
        lo = lattice(k, rng)
        a = boxes(lo, lo + F(1.0))
        cases.append(("extent_ties_%dx%dx%d" % k, a, np.arange(len(a), dtype=np.uint32)))
    for axis in range(3):
        for p, q in ((2, 4), (4, 2), (2, 2), (4, 4)):
            k = [p, q]; k.insert(axis, 1)
            lo = lattice(k, rng)
            hi = lo + F(1.0)
            hi[:, axis] = F(4.0)
            a = boxes(lo, hi)
            cases.append(("extent_ties_slab%s_%dx%d" % ("xyz"[axis], p, q), a, np.arange(len(a), dtype=np.uint32)))


def adjacent_floats(cases):
    """130 point boxes on two adjacent floats of one axis: only the double midpoint separates them
    (the float sum rounds to the even neighbour, and nothing is below that)."""
    rng = np.random.default_rng(104)
    for name, axis, v0, toward in (("one", 0, 1.0, 2.0), ("neg3", 1, -3.0, 0.0), ("tiny", 2, 2.0 ** -126, 1.0)):
        v0 = F(v0); v1 = np.nextafter(v0, F(toward))
        lo_v, hi_v = (v0, v1) if v0 < v1 else (v1, v0)
        assert F(F(lo_v + hi_v) * F(0.5)) == lo_v          # a float midpoint puts nothing on the left
        assert float(lo_v) < (float(lo_v) + float(hi_v)) * 0.5 < float(hi_v)    # the double midpoint does
        pick = rng.random(130) < rng.uniform(0.3, 0.7)
        assert 0 < pick.sum() < 130
        c = np.zeros((130, 3), F)
        c[:, axis] = np.where(pick, v1, v0)
        cases.append(("adjacent_floats_" + name, points(c), np.arange(130, dtype=np.uint32)))


def fallback_axes(cases):
    rng = np.random.default_rng(105)
    # centroids all equal on the longest (x) and the middle (y) axis, distinct on the shortest (z)
    w = F(5.0) + dyadic(rng, 100, 5.0); h = F(2.0) + dyadic(rng, 100, 1.0)
    z = (rng.permutation(128)[:100].astype(F)) / F(128)
    lo = np.stack([-w, -h, z], 1); hi = np.stack([w, h, z + F(1.0 / 256)], 1)
    cases.append(("fallback_axes_shortest", boxes(lo, hi), np.arange(100, dtype=np.uint32)))
    # centroids beyond the box on every axis: no axis has anything on the left, the list is dealt
    lo = dyadic(rng, (100, 3)); hi = lo + dyadic(rng, (100, 3), 0.5)
    cases.append(("fallback_axes_deal", boxes(lo, hi, F(1000.0) + dyadic(rng, (100, 3), 8.0)),
                  np.arange(100, dtype=np.uint32)))
    # 129 identical boxes from row 77 on, inside 300 others
    lo = dyadic(rng, (429, 3), 8.0, 4); hi = lo + dyadic(rng, (429, 3), 0.5, 1) + F(1.0 / 4)
    lo[77:77 + 129] = lo[77]; hi[77:77 + 129] = hi[77]
    cases.append(("fallback_axes_block", boxes(lo, hi), np.arange(429, dtype=np.uint32)))


def chains(cases):
    """200 point boxes at c_k = 2^k * (1 + (k + 100) / 256), k = -100..99: every split takes one box
    off the far end, 199 levels deep. (Bare powers of two stop short of that: once the run spans more
    than 53 binades the double sum min + max drops the min, the split is exactly c_(k-1), and that
    box goes right with c_k; the growing mantissa keeps c_(k-1) strictly below c_k / 2.)"""
    rng = np.random.default_rng(106)
    k = np.arange(-100, 100)
    ck = np.ldexp(1.0 + (k + 100) / 256.0, k)
    assert (ck.astype(F) == ck).all() and (ck[:-1] < ck[1:] * 0.5).all()
    for name, sign in (("chain_left", 1.0), ("chain_right", -1.0)):
        c = np.zeros((200, 3), F)
        c[:, 0] = (sign * ck[rng.permutation(200)]).astype(F)
        cases.append((name, points(c), np.arange(200, dtype=np.uint32)))


def infinities(cases):
    rng = np.random.default_rng(107)
    lo = dyadic(rng, (80, 3), 4.0); hi = lo + dyadic(rng, (80, 3), 0.5) + F(1.0 / 64)
    a = boxes(lo, hi)                       # finite centroids
    for n, row in enumerate(range(0, 24, 3)):      # both on one axis: the split is NaN, the extent infinite
        a[row, n % 3] = -np.inf; a[row, 3 + n % 3] = np.inf
    for n, row in enumerate(range(30, 48, 3)):     # one infinity only
        a[row, n % 6] = np.inf if n % 6 >= 3 else -np.inf
    a[60, 6] = np.inf; a[63, 7] = -np.inf          # and two infinite centroids
    cases.append(("infinities", a, np.arange(80, dtype=np.uint32)))


def work_duplicates(cases):
    rng = np.random.default_rng(108)
    lo = dyadic(rng, (70, 3), 4.0); hi = lo + dyadic(rng, (70, 3), 0.5) + F(1.0 / 64)
    named = rng.permutation(70)[:50]
    work = np.repeat(named, 3)[rng.permutation(150)].astype(np.uint32)
    cases.append(("work_duplicates", boxes(lo, hi), work))


def tiny(cases):
    rng = np.random.default_rng(109)
    for n in (1, 2, 3):
        lo = dyadic(rng, (n, 3), 4.0); hi = lo + dyadic(rng, (n, 3), 0.5) + F(1.0 / 64)
        cases.append(("tiny_%d" % n, boxes(lo, hi), np.arange(n, dtype=np.uint32)))


def inputs():
    cases = []
    for make in (zeros_plane, nan_bounds, extent_ties, adjacent_floats, fallback_axes, chains, infinities,
                 work_duplicates, tiny):
        make(cases)
    assert all(len(w) <= 520 and len(a) <= 520 for _, a, w in cases)
    return cases


def run_reference(cases):
    """{name: nodes as uint32 bits} from the reference builder under node."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, a, w in cases:
            a.view("<u4").tofile(os.path.join(tmp, name + ".aabb.u32"))
            w.astype("<u4").tofile(os.path.join(tmp, name + ".work.u32"))
        with open(os.path.join(tmp, "cases.json"), "w") as f:
            json.dump([{"name": name, "tris": len(a), "work": len(w)} for name, a, w in cases], f)
        subprocess.run(["node", os.path.join(HERE, "bvh_cases.js"), tmp], check=True, stdout=subprocess.DEVNULL)
        for name, a, w in cases:
            out[name] = np.fromfile(os.path.join(tmp, name + ".nodes.u32"), dtype="<u4").reshape(2 * len(w) - 1, 8)
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that equal arrays give equal bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, arr in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asfortranarray(arr), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "bvh_cases.npz")
    cases = inputs()
    nodes = run_reference(cases)
    arrays = [("names", np.array([name for name, _, _ in cases], dtype="S")),
              ("tris", np.array([len(a) for _, a, _ in cases], np.uint32)),
              ("works", np.array([len(w) for _, _, w in cases], np.uint32)),
              ("aabb_in", np.concatenate([a.view(np.uint32) for _, a, _ in cases])),
              ("work", np.concatenate([w for _, _, w in cases])),
              ("nodes", np.concatenate([nodes[name] for name, _, _ in cases]))]
    write_npz(path, arrays)
    print("%d cases, %d bytes" % (len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
