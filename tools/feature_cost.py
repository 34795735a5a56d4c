#!/usr/bin/env python3
"""What the feature buffers cost: ms per frame of a bench workload with both feature targets bound
(Effect.setFeatureTargets) against unbound, on one engine and one build, alternating, `rounds` rounds, the
least of the rounds (the whole-frame A/B of tools/gpu_frame_ab.sh, with the binding as the variable). A frame is
pathTracing + screenCopy + screenOutput, driven as bench.py drives it; wall clock between two syncs. Prints one
JSON line. Under a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/feature_cost.py
--only on) the trace's pt_feature_fold row is the fold kernel's own time.

usage: feature_cost.py [--workload dragon] [--size 1920x1080] [--steps 200] [--warmup 20] [--rounds 3] [--only on|off]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="dragon", choices=sorted(H.WORKLOADS))
ap.add_argument("--size", default=None)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only", choices=("on", "off"), default=None, help="one arm only (for a kernel trace)")
a = ap.parse_args()

meta, mesh_arrays, maps, (W, Hh) = H.workload(a.workload)
if a.size:
    W, Hh = (int(v) for v in a.size.lower().split("x"))
e = bp.Engine(0)
p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
for kind, sampler in (H.PBR_SAMPLERS.items() if maps else ()):
    p.textures[sampler] = bp.Texture(e, maps[kind], name=kind)
e.resize_canvas(W, Hh)
fx = p.wrappers[H.path_call(meta["frames"][0])["effect"]].effect
targets = (bp.RenderTargetTexture("featureNormalId", (W, Hh), e), bp.RenderTargetTexture("featureAlbedoWeight", (W, Hh), e))
k = 0


def run(n):
    global k
    for _ in range(n):
        for call in p.synth_frame(k):
            p.play_call(call)
        k += 1


ms = {"off": [], "on": []}
for _ in range(a.rounds):
    for arm in ("off", "on"):
        if a.only and arm != a.only:
            continue
        fx.setFeatureTargets(*(targets if arm == "on" else (None, None)))
        run(a.warmup)
        e.sync()
        t0 = time.perf_counter()
        run(a.steps)
        e.sync()
        ms[arm].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
best = {arm: min(v) for arm, v in ms.items() if v}
out = {"workload": a.workload, "size": [W, Hh], "steps": a.steps, "rounds_ms": ms, "ms_per_frame": best,
       "bytes_per_frame": 128 * W * Hh, "byte_floor_us_at_8TBps": round(128 * W * Hh / 8e12 * 1e6, 1)}
if len(best) == 2:
    out["on_over_off"] = round(best["on"] / best["off"], 4)
    out["added_us"] = round((best["on"] - best["off"]) * 1e3, 1)
print(json.dumps(out), flush=True)
e.dispose()
