#!/usr/bin/env python3
"""What pt_cast_rays delivers: primary-ray queries per second on a bench workload's scene, for the pixel-centre
camera rays of the bench's view at --size, in row-major order and in 8x8-tile order (the order the path-tracing
kernel's waves take their pixels in: a wave's 64 rays then cover one 8x8 block instead of a 64-pixel run of a row).

Two figures per order and BVH layout, each the median of --reps calls after --warmup calls:
  kernel   the pt_raycast launches of a call (a call of this size runs in chunks), between HIP events recorded
           around each launch on the context's stream (PT_RAYCAST_EVENTS=1, pt_debug_raycast_ms): Mrays/s of the
           kernel alone;
  call     Effect.cast_rays as a host sees it, by the host clock (the call ends in a device synchronise): staging
           24 B per ray in, the kernel, 64 B per ray out, the record array's allocation.
Prints one JSON line. A measurement path that finds no GPU fails.

usage: raycast_rate.py [--workload dragon] [--size 1920x1080] [--layouts pairs,trail,reference] [--reps 9] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["PT_RAYCAST_EVENTS"] = "1"   # (read at the library's first query)

import ctypes            # noqa: E402
import numpy as np       # noqa: E402
import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="dragon", choices=sorted(H.WORKLOADS))
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--layouts", default="pairs,trail,reference")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

W, Hh = (int(v) for v in a.size.lower().split("x"))
meta, mesh_arrays, maps, _ = H.workload(a.workload)
e = bp.Engine(0)
player = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
if maps:
    for kind, sampler in H.PBR_SAMPLERS.items():
        player.textures[sampler] = bp.Texture(e, maps[kind], name=kind)
call = H.path_call(meta["frames"][0])
fx = player.wrappers[call["effect"]].effect
uniforms = dict(call["uniforms"])
uniforms.update({k: v for k, v in player.override.items() if k in uniforms})   # uResolution, uULen at --size
for name, ent in uniforms.items():
    fx._set_entry(name, ent)
for name, tex in call["samplers"].items():
    fx.setTexture(name, player.textures.get(tex) if tex else None)

# Effect.camera_ray for every pixel at once: the same float32 sequence
f = np.float32
m = fx._uniform("uCameraMatrix", 16)
ulen, vlen = fx._uniform("uULen", 1)[0], fx._uniform("uVLen", 1)[0]
ys, xs = np.mgrid[0:Hh, 0:W].astype(np.float32)
ppx = ((xs + f(0.5)) / f(W)) * f(2.0) - f(1.0)
ppy = ((ys + f(0.5)) / f(Hh)) * f(2.0) - f(1.0)
d = (m[0:3] * ppx[..., None]) * ulen + (m[4:7] * ppy[..., None]) * vlen + m[8:11]
d = d * (f(1.0) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
assert d.dtype == np.float32
o0, d0 = fx.camera_ray(W // 3, Hh // 3, W, Hh)
assert np.array_equal(d[Hh // 3, W // 3].view(np.uint32), d0.view(np.uint32))


def tiled(img):
    """(H, W, 3) -> rays in 8x8-tile order, tiles row-major, pixels row-major inside a tile (edge tiles clipped)."""
    order = []
    for ty in range(0, Hh, 8):
        for tx in range(0, W, 8):
            yy, xx = np.mgrid[ty:min(ty + 8, Hh), tx:min(tx + 8, W)]
            order.append((yy * W + xx).reshape(-1))
    return np.ascontiguousarray(img.reshape(-1, 3)[np.concatenate(order)])


orders = {"row_major": np.ascontiguousarray(d.reshape(-1, 3)), "tiles_8x8": tiled(d)}
n = W * Hh
origins = np.ascontiguousarray(np.tile(m[12:15], (n, 1)))
kernel_ms = bp.lib().pt_debug_raycast_ms
kernel_ms.restype = ctypes.c_float
kernel_ms.argtypes = []

out = {"workload": a.workload, "size": "%dx%d" % (W, Hh), "rays": n, "reps": a.reps, "warmup": a.warmup, "layouts": {}}
for layout in a.layouts.split(","):
    e.set_bvh_layout(layout)
    row = {}
    for oname, dirs in orders.items():
        hits = None
        for _ in range(a.warmup):
            hits = fx.cast_rays(origins, dirs)
        ks, cs = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            hits = fx.cast_rays(origins, dirs)
            cs.append((time.perf_counter() - t0) * 1e3)
            ms = float(kernel_ms())
            if not ms > 0.0:
                raise SystemExit("no kernel time: PT_RAYCAST_EVENTS was not read")
            ks.append(ms)
        k, c = statistics.median(ks), statistics.median(cs)
        row[oname] = {"kernel_ms": round(k, 4), "kernel_ms_min_max": [round(min(ks), 4), round(max(ks), 4)],
                      "kernel_mrays_s": round(n / k / 1e3, 1), "call_ms": round(c, 2), "call_mrays_s": round(n / c / 1e3, 1),
                      "mesh_hits": int((hits["triangle"] >= 0).sum()), "misses": int((hits["object_id"] < 0).sum())}
    out["layouts"][layout] = row
e.sync()
e.dispose()
print(json.dumps(out), flush=True)
