#!/usr/bin/env python3
"""What serving every frame costs the render loop: frames per second of bench.py's step loop (the dragon stand-in,
still camera, one step = pathTracing + screenCopy + screenOutput) at 1920x1080 and 3840x2160 in three shapes:

  none   no encode: the loop as bench.py times it;
  sync   Engine.encode_canvas_jpeg after every step: the call waits for the stream twice and runs the deferred
         screenCopy, so no second frame is ever queued;
  job    Engine.encode_canvas_jpeg_begin after every step, the job finished two steps later: two jobs pending
         while the frames run.

Quality 90, 4:2:0 by default. A round is `steps` steps of each shape between two syncs after `warmup` steps; the
shapes' order is reversed every round. Beside frames per second a round reports pt_fuse_stats' stale copies per step
(0 in a loop that stays fused) and, for `job`, pt_job_stats.

With --parent-lib the shapes none and sync are also measured with that libpt.so (a build of the parent commit, loaded
through PT_LIBPT; it has no jobs), each library in a fresh child process per round, the libraries' order reversed
every round. Prints one JSON line: per size, shape and library the rounds' frames per second and their range.

usage: encode_jobs_cost.py [--sizes 1920x1080,3840x2160] [--quality 90] [--subsampling 2] [--steps 300] [--warmup 30]
                           [--rounds 3] [--lag 2] [--parent-lib PATH]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--subsampling", type=int, default=2)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--lag", type=int, default=2, help="a job is finished this many steps after it began")
ap.add_argument("--shapes", default="none,sync,job")
ap.add_argument("--parent-lib", default=None, help="a libpt.so built from the parent commit, for none and sync")
ap.add_argument("--reverse", action="store_true", help="(a child's) run the shapes in reverse order")
a = ap.parse_args()


def measure():
    """one process, one library: every size, `rounds` rounds (one in a child), the shapes' order reversed each"""
    import babylon_pt as bp
    import helpers as H
    meta, mesh_arrays, _, _ = H.workload("dragon")
    shapes = [s for s in a.shapes.split(",") if s != "job" or hasattr(bp.lib(), "pt_job_finish")]
    out = {}
    for size in a.sizes.split(","):
        W, Hh = (int(v) for v in size.lower().split("x"))
        e = bp.Engine(0)
        p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
        e.resize_canvas(W, Hh)
        k = 0

        def run(shape, n):
            nonlocal k
            pending, nbytes = [], 0
            for _ in range(n):
                for call in p.synth_frame(k):
                    p.play_call(call)
                k += 1
                if shape == "sync":
                    nbytes += len(e.encode_canvas_jpeg(a.quality, a.subsampling, False))
                elif shape == "job":
                    pending.append(e.encode_canvas_jpeg_begin(a.quality, a.subsampling, False))
                    if len(pending) > a.lag:
                        nbytes += len(pending.pop(0).result())
            for j in pending:
                nbytes += len(j.result())
            e.sync()
            return nbytes

        res = {s: {"fps": [], "stale_copies_per_step": [], "file_bytes": None} for s in shapes}
        for r in range(a.rounds):
            order = shapes[::-1] if (r % 2 == 1) != a.reverse else shapes
            for s in order:
                run(s, a.warmup)
                stale0 = e.fuse_stats()[1]
                t0 = time.perf_counter()
                nbytes = run(s, a.steps)
                dt = time.perf_counter() - t0
                res[s]["fps"].append(round(a.steps / dt, 1))
                if stale0 is not None:
                    res[s]["stale_copies_per_step"].append(round((e.fuse_stats()[1] - stale0) / a.steps, 3))
                if s != "none":
                    res[s]["file_bytes"] = nbytes // a.steps
        if "job" in shapes:
            res["job"]["job_stats"] = e.job_stats()
        out[size] = res
        e.dispose()
    return out


def spread(v):
    return {"rounds": v, "least": min(v), "most": max(v)}


if a.parent_lib is None:
    got = measure()
    for size in got.values():
        for s in size.values():
            s["fps"] = spread(s["fps"])
    print(json.dumps({"workload": "dragon", "quality": a.quality, "subsampling": a.subsampling, "steps": a.steps,
                      "lag": a.lag, "this": got}))
else:
    merged = {"this": {}, "parent": {}}
    for r in range(a.rounds):
        for lib in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            env = dict(os.environ)
            env.pop("PT_LIBPT", None)
            if lib == "parent":
                env["PT_LIBPT"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--sizes", a.sizes, "--quality", str(a.quality),
                   "--subsampling", str(a.subsampling), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--rounds", "1", "--lag", str(a.lag), "--shapes", a.shapes if lib == "this" else "none,sync"]
            if r % 2 == 1:
                cmd.append("--reverse")
            line = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env).stdout.strip().splitlines()[-1]
            for size, shapes in json.loads(line)["this"].items():
                for s, v in shapes.items():
                    m = merged[lib].setdefault(size, {}).setdefault(s, {"fps": [], "stale_copies_per_step": []})
                    m["fps"] += v["fps"]["rounds"]
                    m["stale_copies_per_step"] += v["stale_copies_per_step"]
                    m["file_bytes"] = v["file_bytes"]
                    if "job_stats" in v:
                        m["job_stats"] = v["job_stats"]
    for lib in merged.values():
        for size in lib.values():
            for s in size.values():
                s["fps"] = spread(s["fps"])
    print(json.dumps({"workload": "dragon", "quality": a.quality, "subsampling": a.subsampling, "steps": a.steps,
                      "lag": a.lag, "rounds": a.rounds, **merged}))
