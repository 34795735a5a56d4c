#!/usr/bin/env python3
"""What pt_denoise costs: device time per Engine.denoise call at 1..5 iterations on dragon stand-in frames with
feature targets bound, at 1920x1080 and 3840x2160, beside its two yardsticks measured in the same run: the byte
floor (prep reads 48 B and writes 32 B per pixel; a pass reads 32 B and writes 32 B, the last one reads 48 B
and writes 16 B; at 8 TB/s) and pt_output's own time (screenOutput, the project's 25-tap tile kernel) on
the same frames (its per-draw events in the engine's timing window). The engine runs on a torch stream; a round
is `reps` calls between two events on that stream, the figure the least of `rounds` rounds. The difference
between k and k - 1 iterations is the pass at spacing 2^(k-1) (each is also the last pass of its call, so the
remodulation rides along in both). Prints one JSON line.

usage: denoise_cost.py [--sizes 1920x1080,3840x2160] [--frames 8] [--reps 20] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch             # noqa: E402
import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--frames", type=int, default=8, help="still frames accumulated before the calls are timed")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

meta, mesh_arrays, maps, _ = H.workload("dragon")
stream = torch.cuda.Stream(device=0)


def timed(fn):
    """us per call of fn: the least of the rounds."""
    best = None
    for _ in range(a.rounds):
        for _ in range(3):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(a.reps):
            fn()
        ev1.record(stream)
        ev1.synchronize()
        us = ev0.elapsed_time(ev1) / a.reps * 1e3
        best = us if best is None else min(best, us)
    return round(best, 1)


def output_us(e, p, output):
    """us per screenOutput draw, from the engine's own per-draw events (its host side sets uniforms per draw, so
    back-to-back draws would leave gaps between two outer events): the least of the rounds."""
    best = None
    for _ in range(a.rounds):
        e.timing_begin()
        for _ in range(a.reps):
            p.play_call(output)
        ms, n = e.timing_end("screenOutput")
        best = ms / n * 1e3 if best is None else min(best, ms / n * 1e3)
    return round(best, 1)


def floor_us(px, iterations):
    return round((80 + 64 * iterations) * px / 8e12 * 1e6, 1)


out = {"workload": "dragon", "reps": a.reps, "rounds": a.rounds, "sizes": {}}
for size in a.sizes.split(","):
    W, Hh = (int(v) for v in size.lower().split("x"))
    e = bp.Engine(0)
    e.set_stream(stream.cuda_stream)
    p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
    e.resize_canvas(W, Hh)
    nid, alb, dst = (bp.RenderTargetTexture(n, (W, Hh), e) for n in ("featureNormalId", "featureAlbedoWeight", "denoised"))
    p.wrappers[H.path_call(meta["frames"][0])["effect"]].effect.setFeatureTargets(nid, alb)
    for call in meta["frames"][0]:
        p.play_call(call)
    for k in range(a.frames):
        for call in p.synth_frame(k):
            p.play_call(call)
    e.sync()
    beauty = p.textures["pathTracingRenderTarget"]
    output = H.output_call(p.synth_frame(a.frames))
    p.play_call(output)   # (a deferred copy or order build rides along with this one, not with the timed ones)
    row = {"pt_output_us": output_us(e, p, output), "denoise_us": {}, "byte_floor_us": {}, "pass_us": {}}
    prev = None
    for it in (1, 2, 3, 4, 5):
        us = timed(lambda: e.denoise(beauty, nid, alb, dst, iterations=it))
        row["denoise_us"][str(it)] = us
        row["byte_floor_us"][str(it)] = floor_us(W * Hh, it)
        if prev is not None:
            row["pass_us"]["spacing_%d" % (1 << (it - 1))] = round(us - prev, 1)
        prev = us
    row["pass_over_pt_output"] = {k: round(v / row["pt_output_us"], 2) for k, v in row["pass_us"].items()}
    out["sizes"]["%dx%d" % (W, Hh)] = row
    e.sync()
    e.set_stream(None)
    e.dispose()
print(json.dumps(out), flush=True)
