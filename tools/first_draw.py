"""First-draw cost of a fresh context (tools/README.md): wall clock from context creation to the first sync
after one frame of a workload - the context, the texture uploads, and the first mesh draw with the child-pair
build of its BVH (csrc/pt_pairs.hip). The mesh arrays are made on the CPU before the clock starts. One fresh
process per figure.

usage: python tools/first_draw.py [--workload W] [--size WxH]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package and tests/helpers.py on the path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    import babylon_pt as bp
    import helpers as H
    W, Hh = (int(v) for v in args.size.lower().split("x"))
    meta, mesh_arrays, _, _ = H.workload(args.workload)
    payloads, noise = H.texture_payloads(meta, mesh_arrays), H.bluenoise()
    bp.lib()
    t0 = time.perf_counter()
    engine = bp.Engine(0)
    player = bp.StreamPlayer(engine, meta, noise, payloads, W, Hh)
    engine.resize_canvas(W, Hh)
    t1 = time.perf_counter()
    player.play_frame(0)
    engine.sync()
    t2 = time.perf_counter()
    layout = engine.bvh_layout_used()
    player.play_frame(1)
    engine.sync()
    t3 = time.perf_counter()
    print("context to first sync ms %.2f (context + uploads %.2f, first frame with the %s build %.2f; second frame %.2f)"
          % (1e3 * (t2 - t0), 1e3 * (t1 - t0), layout, 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
    engine.dispose()


if __name__ == "__main__":
    main()
