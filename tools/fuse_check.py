#!/usr/bin/env python3
"""The render loop's fused pass on bench.py's own route (its player, its step loop, default arguments' workload and
size, no PT_* setting): after K frames pt_fuse_stats must show K fused accumulate-and-output passes and no
screenCopy kernel, and one such kernel once the frame is read. Exits non-zero otherwise."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench             # noqa: E402
import babylon_pt as bp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="dragon")
ap.add_argument("--size", default=None, help="WxH (default: the workload's bench size)")
ap.add_argument("--frames", type=int, default=30)
a = ap.parse_args()
for k in [k for k in os.environ if k.startswith("PT_") and k != "PT_LIBPT"]:
    del os.environ[k]
import helpers as H      # noqa: E402
W, Hh = [int(v) for v in a.size.split("x")] if a.size else H.WORKLOADS[a.workload][3]
engine = bp.Engine(0)
player = bench.make_player(engine, a.workload, W, Hh)[0]
engine.resize_canvas(W, Hh)
engine.set_row_partition(1, 0)
for k in range(a.frames):
    for call in player.synth_frame(k):   # bench.py's step(): pathTracing, screenCopy, screenOutput
        player.play_call(call)
loop = engine.fuse_stats()   # (host counters: no synchronisation, which would bring the stale texture up to date)
engine.sync()
engine.read_canvas(W, Hh)
after = engine.fuse_stats()
print("%s %dx%d, %d frames: fused passes %d, screenCopy kernels %d (after reading the canvas: %d)" % (
    a.workload, W, Hh, a.frames, loop[0], loop[1], after[1]))
engine.dispose()
sys.exit(0 if loop == (a.frames, 0) and after == (a.frames, 1) else 1)
