#!/usr/bin/env python3
"""What pt_canvas_encode_png costs: time per Engine.encode_canvas_png call on the canvas of rendered dragon stand-in
frames (after each of --samples still frames) and on a flat canvas, at each --filters value and --colour, with the
file's size, beside the host route measured in the same run on one thread: a pt_read_pixels of the same canvas, Pillow's
default PNG save of those pixels, and zlib.compress at level 1 of the same filtered bytes (tests/png_enc_ref.py's
filters are not timed: a host encoder filters in C). The engine runs on a torch stream. The call synchronises twice
(it reads the IDATs' length, then the IDATs), so it is timed two ways: `call_us` the host's clock around the call,
and `stream_us` two events on the stream around `reps` calls, both the least of `rounds` rounds. The split per kernel
comes from a kernel trace of this program (rocprofv3 --kernel-trace --stats -- python tools/png_encode_cost.py).
Prints one JSON line.

usage: png_encode_cost.py [--size 1920x1080] [--samples 1,64] [--filters none,paeth,adaptive] [--colour rgb]
                          [--reps 10] [--rounds 3]"""
import argparse
import io
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np       # noqa: E402
import torch             # noqa: E402
import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402
import png_enc_ref as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--samples", default="1,64", help="still frames accumulated before the calls are timed")
ap.add_argument("--filters", default="none,paeth,adaptive")
ap.add_argument("--colour", default="rgb")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
W, Hh = (int(v) for v in a.size.lower().split("x"))
stream = torch.cuda.Stream(device=0)


def timed(fn):
    """(us per call by the host's clock, us per call between two events on the stream): the least of the rounds"""
    wall, dev = None, None
    for _ in range(a.rounds):
        for _ in range(2):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        t1 = time.perf_counter()
        ev1.record(stream)
        ev1.synchronize()
        w, d = (t1 - t0) / a.reps * 1e6, ev0.elapsed_time(ev1) / a.reps * 1e3
        wall, dev = (w if wall is None else min(wall, w)), (d if dev is None else min(dev, d))
    return round(wall, 1), round(dev, 1)


def host_us(fn, n=3):
    best, res = None, None
    for _ in range(n):
        t0 = time.perf_counter()
        res = fn()
        us = (time.perf_counter() - t0) * 1e6
        best = us if best is None else min(best, us)
    return round(best, 1), res


def pillow_png(pixels):
    from PIL import Image
    img = Image.fromarray(pixels, "RGBA" if pixels.shape[2] == 4 else "RGB")
    buf = io.BytesIO()
    img.save(buf, "PNG")
    return buf.getvalue()


def measure(e, label):
    wall, dev = timed(lambda: e.read_canvas(W, Hh))
    row = {"read_pixels_us": {"call": wall, "stream": dev, "bytes": 4 * W * Hh}}
    canvas = e.read_canvas(W, Hh)
    top = np.ascontiguousarray(canvas[::-1] if a.colour == "rgba" else canvas[::-1, :, :3])
    us, png = host_us(lambda: pillow_png(top))
    row["pillow_default"] = {"us": us, "file_bytes": len(png)}
    for f in a.filters.split(","):
        wall, dev = timed(lambda: e.encode_canvas_png(a.colour, f))
        data = e.encode_canvas_png(a.colour, f)
        filtered = P.filtered_stream(top, bp.Engine.PNG_FILTERS[f])[0]
        us, z = host_us(lambda: zlib.compress(filtered, 1))
        row[f] = {"call_us": wall, "stream_us": dev, "file_bytes": len(data), "idats": data.count(b"IDAT"),
                  "filtered_bytes": len(filtered), "zlib_level1_us": us, "zlib_level1_bytes": len(z),
                  "zlib_level6_bytes": len(zlib.compress(filtered, 6))}
    print(label, json.dumps(row), file=sys.stderr, flush=True)
    return row


out = {"workload": "dragon", "size": "%dx%d" % (W, Hh), "colour": a.colour, "reps": a.reps, "rounds": a.rounds, "canvases": {}}
e = bp.Engine(0)
e.set_stream(stream.cuda_stream)
e.resize_canvas(W, Hh)
out["canvases"]["flat"] = measure(e, "flat")
meta, mesh_arrays, maps, _ = H.workload("dragon")
p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
done = 0
for call in meta["frames"][0]:
    p.play_call(call)
done = 1
for want in sorted(int(v) for v in a.samples.split(",")):
    while done < want:
        for call in p.synth_frame(done - 1):
            p.play_call(call)
        done += 1
    e.sync()
    out["canvases"]["samples_%d" % want] = measure(e, "samples %d" % want)
e.sync()
e.set_stream(None)
e.dispose()
print(json.dumps(out), flush=True)
