#!/usr/bin/env python3
"""What pt_targets_encode_exr costs: time per call and the file's size on the rendered dragon stand-in at --size after
--frames still frames with the feature buffers bound, for two channel sets - `rgb`, the beauty's R G B as HALF at
1 / weight, and `aov`, the ten channels of Engine.exr_aov_channels (beauty, albedo and normal as HALF, id as FLOAT) -
under each of NONE, ZIPS and ZIP, beside, in the same run, the pt_read_pixels of the textures the set names (one for
rgb, three for aov: what a caller who writes the file on the CPU pays before it starts). The C calls write into host
buffers allocated once. Each file is first held against the definition: tests/exr_enc_ref.py's decode of it must
return the reference's samples of the texels read back (--check-bytes compares the whole file with the reference's,
which deflates on the CPU and takes a while at 1080p). The engine runs on a torch stream. Every call synchronises,
so each is timed two ways: `call_us` the host's clock around the call, `stream_us` two events on the stream around
`reps` calls; a round times the readback and then every file in turn, and the least of `rounds` rounds is reported.
The split per kernel comes from a kernel trace of this program (rocprofv3 --kernel-trace --stats -- python
tools/exr_encode_cost.py). Prints one JSON line.

usage: exr_encode_cost.py [--size 1920x1080] [--frames 16] [--reps 20] [--rounds 3] [--check-bytes]"""
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
import exr_enc_ref as R  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--frames", type=int, default=16, help="still frames accumulated before the calls are timed")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--check-bytes", action="store_true", help="compare every file with the reference's, byte for byte")
a = ap.parse_args()
W, Hh = (int(v) for v in a.size.lower().split("x"))
stream = torch.cuda.Stream(device=0)
TYPES = {"half": R.HALF, "float": R.FLOAT}
NUMBER = {"none": R.NONE, "zips": R.ZIPS, "zip": R.ZIP}


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


meta, mesh_arrays, maps, _ = H.workload("dragon")
e = bp.Engine(0)
e.set_stream(stream.cuda_stream)
p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
e.resize_canvas(W, Hh)
nid, alb = (bp.RenderTargetTexture(n, (W, Hh), e) for n in ("featureNormalId", "featureAlbedoWeight"))
p.wrappers[H.path_call(meta["frames"][0])["effect"]].effect.setFeatureTargets(nid, alb)
for call in meta["frames"][0]:
    p.play_call(call)
for k in range(a.frames - 1):
    for call in p.synth_frame(k):
        p.play_call(call)
e.sync()
beauty = p.textures["pathTracingRenderTarget"]
lib = bp.lib()
host = {t: np.zeros((Hh, W, 4), np.float32) for t in (beauty, nid, alb)}   # (allocated once: the readback alone is timed)


def read(texs):
    for t in texs:
        e.check(lib.pt_read_pixels(e.ctx, t.handle, host[t].ctypes.data, host[t].nbytes), "read")


read(host)
weight = float(host[alb][0, 0, 3])
assert weight >= 1.0 and (host[alb][..., 3] == weight).all(), "the weight is uniform over a frame"
sets = {"rgb": ([(n, beauty, k, 1.0 / weight, "half") for k, n in enumerate("RGB")], [beauty]),
        "aov": (bp.Engine.exr_aov_channels(beauty, nid, alb, weight), [beauty, nid, alb])}
out = {"workload": "dragon", "size": a.size, "frames": a.frames, "weight": weight, "reps": a.reps, "rounds": a.rounds,
       "checked": "bytes" if a.check_bytes else "decode", "sets": {}}
for name, (chans, texs) in sets.items():
    ref = [(n, host[t], k, s, TYPES[kind]) for n, t, k, s, kind in chans]
    files, calls = {}, []
    for z in ("none", "zips", "zip"):
        data = e.encode_targets_exr(chans, z)
        got, _ = R.decode(data)   # the file timed below is the definition's
        for n, tex, k, s, kind in ref:
            assert np.array_equal(got[n], R.samples(tex, k, s, kind)[::-1]), (name, z, n)
        if a.check_bytes:
            assert data == R.encode(ref, NUMBER[z]), (name, z)
        files[z] = data
        arr, _names = e._exr_channels(chans)
        buf, size = (ctypes.c_uint8 * len(data))(), ctypes.c_size_t(0)
        calls.append((arr, _names, buf, size, NUMBER[z], len(chans)))
    fns = [lambda: read(texs)]
    for arr, _names, buf, size, number, n in calls:
        fns.append(lambda arr=arr, buf=buf, size=size, number=number, n=n: e.check(
            lib.pt_targets_encode_exr(e.ctx, arr, n, number, buf, len(buf), ctypes.byref(size)), "encode"))
    times = timed(fns)
    raw = sum(2 if kind == "half" else 4 for *_x, kind in chans) * W * Hh
    row = {"channels": len(chans), "sample_bytes": raw,
           "read_pixels": {"call_us": times[0][0], "stream_us": times[0][1], "bytes": 16 * W * Hh * len(texs)}}
    for (z, data), (wall, dev), call in zip(files.items(), times[1:], calls):
        assert bytes(call[2]) == data
        row[z] = {"call_us": wall, "stream_us": dev, "file_bytes": len(data), "of_samples": round(len(data) / raw, 4),
                  "bytes_per_texel": round(len(data) / (W * Hh), 3), "encode_over_read": round(wall / times[0][0], 3)}
    print(name, json.dumps(row), file=sys.stderr, flush=True)
    out["sets"][name] = row
e.sync()
e.set_stream(None)
e.dispose()
print(json.dumps(out), flush=True)
