#!/usr/bin/env python3
"""What pt_cast_rays_ex delivers beside pt_cast_rays (tools/raycast_rate.py, whose method this is): the pixel-centre
camera rays of a bench workload's view at --size, in row-major order, per BVH layout, as

  closest                 pt_cast_rays itself (pt_raycast): the figure raycast_rate.py reports
  closest_half            the bounded closest hit, t_max = 0.5 t_ref (every ray misses: the bound culls the walk)
  occluded                the occlusion query without a bound
  occluded_one_and_a_half ... with t_max = 1.5 t_ref (the flags of the unbounded query)

each on the host route and on the device route (torch tensors in and out). Two figures per entry, each the median
of --reps calls after --warmup calls, with the least and the most:
  kernel   the launches of a call between HIP events on the context's stream (PT_RAYCAST_EVENTS=1,
           pt_debug_raycast_ms; a device call's events are read after the sync);
  call     by the host clock: the host route's call (it ends in a synchronise), the device route from the enqueue to
           the end of a pt_sync.
and the bytes each call moves between host and device. Prints one JSON line. A measurement path that finds no GPU fails.

usage: raycast_query_rate.py [--workload dragon] [--size 1920x1080] [--layouts pairs,trail,reference] [--reps 9] [--warmup 3]"""
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
import torch             # noqa: E402  (before libpt.so: both on one HIP runtime)
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
torch.cuda.init()
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
dirs = np.ascontiguousarray(d.reshape(-1, 3))
n = W * Hh
origins = np.ascontiguousarray(np.tile(m[12:15], (n, 1)))
kernel_ms = bp.lib().pt_debug_raycast_ms
kernel_ms.restype = ctypes.c_float
kernel_ms.argtypes = []


def stats(v, digits):
    return {"median": round(statistics.median(v), digits), "min_max": [round(min(v), digits), round(max(v), digits)]}


out = {"workload": a.workload, "size": "%dx%d" % (W, Hh), "rays": n, "reps": a.reps, "warmup": a.warmup, "layouts": {}}
for layout in a.layouts.split(","):
    e.set_bvh_layout(layout)
    t_ref = fx.cast_rays(origins, dirs)["t"]
    bounds = {"closest": None, "closest_half": f(0.5) * t_ref, "occluded": None, "occluded_one_and_a_half": f(1.5) * t_ref}
    to, td = torch.from_numpy(origins).to("cuda:0"), torch.from_numpy(dirs).to("cuda:0")
    torch.cuda.synchronize()
    row = {}
    for query, t in bounds.items():
        host_fn = fx.occluded if query.startswith("occluded") else fx.cast_rays
        tt = None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
        torch.cuda.synchronize()
        per_ray_out = 1 if query.startswith("occluded") else 64
        for route in ("host", "device"):
            ks, cs, res = [], [], None
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                if route == "host":
                    res = host_fn(origins, dirs, t)
                else:
                    res = host_fn(to, td, tt)
                    e.sync()
                c = (time.perf_counter() - t0) * 1e3
                ms = float(kernel_ms())
                if not ms > 0.0:
                    raise SystemExit("no kernel time: PT_RAYCAST_EVENTS was not read")
                if k >= a.warmup:
                    ks.append(ms)
                    cs.append(c)
            flags = res if query.startswith("occluded") else None
            if route == "device":
                res = res.cpu().numpy()
                hit = int(res.sum()) if flags is not None else int((bp.ray_hits(res)["object_id"] >= 0).sum())
            else:
                hit = int(res.sum()) if flags is not None else int((res["object_id"] >= 0).sum())
            row["%s_%s" % (query, route)] = {
                "kernel_ms": stats(ks, 4), "kernel_mrays_s": round(n / statistics.median(ks) / 1e3, 1),
                "call_ms": stats(cs, 3), "call_mrays_s": round(n / statistics.median(cs) / 1e3, 1), "rays_with_an_object": hit,
                "bytes_host_to_device": 0 if route == "device" else n * (24 + (4 if t is not None else 0)),
                "bytes_device_to_host": 0 if route == "device" else n * per_ray_out}
    out["layouts"][layout] = row
e.sync()
e.dispose()
print(json.dumps(out), flush=True)
