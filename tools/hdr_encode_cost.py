#!/usr/bin/env python3
"""What pt_target_encode_hdr costs: time per call on the rendered accumulation of the Cornell box and of the sky
program (after --samples still frames, scale 1 / samples) at each of --sizes, with the file's size and its ratio to
the 16 W H bytes of the texels, beside, in the same run, a pt_read_pixels of the same RGBA32F target. Both C calls
write into host buffers allocated once; the Python binding's call (one buffer kept per engine, the file copied out of
it into a bytes object) is timed beside them. The file is first held against the definition: its decode
(pt_assets.decode_hdr) must equal tests/hdr_enc_ref.py's RGBE of the texels read back. The engine runs on a torch
stream. All calls synchronise (the encode twice: it reads the length, then the bytes), so each is timed two ways:
`call_us` the host's clock around the call, and `stream_us` two events on the stream around `reps` calls. A round
times `reps` reads, then `reps` encodes, then `reps` binding calls, so the three alternate; the least of `rounds`
rounds is reported. The split per kernel comes from a kernel trace of this program (rocprofv3 --kernel-trace --stats
-- python tools/hdr_encode_cost.py). Prints one JSON line.

usage: hdr_encode_cost.py [--sizes 1920x1080,3840x2160] [--samples 8] [--reps 200] [--rounds 3] [--no-check]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np       # noqa: E402
import torch             # noqa: E402
import babylon_pt as bp  # noqa: E402
import hdr_enc_ref as R  # noqa: E402
import helpers as H      # noqa: E402
import pt_assets          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--samples", type=int, default=8, help="still frames accumulated before the calls are timed")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-check", action="store_true", help="do not hold the file against the reference first")
a = ap.parse_args()
stream = torch.cuda.Stream(device=0)


def timed(fns):
    """per function (us per call by the host's clock, us per call between two events on the stream): the least of
    the rounds, each of which times the functions in turn"""
    best = [[None, None] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
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
            for m, v in enumerate(((t1 - t0) / a.reps * 1e6, ev0.elapsed_time(ev1) / a.reps * 1e3)):
                best[k][m] = v if best[k][m] is None else min(best[k][m], v)
    return [(round(w, 1), round(d, 1)) for w, d in best]


out = {"samples": a.samples, "reps": a.reps, "rounds": a.rounds, "runs": {}}
for size in a.sizes.split(","):
    W, Hh = (int(v) for v in size.lower().split("x"))
    for name in ("cornell_256", "sky_256"):
        e = bp.Engine(0)
        e.set_stream(stream.cuda_stream)
        e.resize_canvas(W, Hh)
        meta = H.stream(name)
        p = bp.StreamPlayer(e, meta, H.bluenoise(), None, W, Hh)
        for call in meta["frames"][0]:
            p.play_call(call)
        for k in range(a.samples - 1):
            for call in p.synth_frame(k):
                p.play_call(call)
        e.sync()
        acc = p.textures["pathTracingRenderTarget"]
        scale = 1.0 / a.samples
        texels = np.empty((Hh, W, 4), np.float32)   # (allocated once: the readback alone is timed)
        texels.fill(0)
        lib = bp.lib()
        e.check(lib.pt_read_pixels(e.ctx, acc.handle, texels.ctypes.data, texels.nbytes), "read")
        data = acc.encode_hdr(scale)
        if not a.no_check:   # the file timed below is the definition's: its decode against the reference's RGBE
            want = R.decoded(R.scanlines(texels, scale))
            assert np.array_equal(pt_assets.decode_hdr(data)[..., :3].astype(np.float64), want), (name, size)
        buf, got = (ctypes.c_uint8 * len(data))(), ctypes.c_size_t(0)
        (rwall, rdev), (wall, dev), (bwall, bdev) = timed([
            lambda: e.check(lib.pt_read_pixels(e.ctx, acc.handle, texels.ctypes.data, texels.nbytes), "read"),
            lambda: e.check(lib.pt_target_encode_hdr(e.ctx, acc.handle, scale, buf, len(data), ctypes.byref(got)),
                            "encode"),
            lambda: acc.encode_hdr(scale)])
        assert bytes(buf) == data
        row = {"read_pixels": {"call_us": rwall, "stream_us": rdev, "bytes": 16 * W * Hh},
               "encode_hdr": {"call_us": wall, "stream_us": dev, "file_bytes": len(data),
                              "binding_call_us": bwall, "binding_stream_us": bdev,
                              "bytes_per_texel": round(len(data) / (W * Hh), 3),
                              "of_texels": round(len(data) / (16.0 * W * Hh), 4),
                              "checked": not a.no_check},
               "encode_over_read": round(wall / rwall, 3)}
        print(name, size, json.dumps(row), file=sys.stderr, flush=True)
        out["runs"]["%s_%s" % (name.split("_")[0], size)] = row
        e.sync()
        e.set_stream(None)
        e.dispose()
print(json.dumps(out), flush=True)
