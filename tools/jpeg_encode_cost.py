#!/usr/bin/env python3
"""What pt_canvas_encode_jpeg_opt costs: time per Engine.encode_canvas_jpeg call on the canvas of rendered dragon
stand-in frames at 1920x1080 and 3840x2160, quality 75 and 90, at each --subsampling asked for (0 4:4:4, the
default, 1 4:2:2, 2 4:2:0; the keys of the others are "q<quality>_s<subsampling>") and each --optimize (0 the
Annex K Huffman tables, the default; 1 tables built for the frame, key suffix "_opt"), with the file's size, beside
its yardsticks
measured in the same run: pt_output on the same frames (its per-draw events in the engine's timing window), a
pt_read_pixels of the same canvas (what a host that encodes on a CPU core must fetch first), and, where Pillow
is installed, its one-thread encode of the same pixels with the same settings (the work the call replaces).
The engine runs on a torch stream. The call synchronises twice (it reads the stream's length, then the stream),
so it is timed two ways: `call_us` the host's clock around the call, and `stream_us` two events on the stream
around `reps` calls, both the least of `rounds` rounds. The split per kernel comes from a kernel trace of this
program (rocprofv3 --kernel-trace --stats -- python tools/jpeg_encode_cost.py): the six pt_jpeg_* kernels, nine
with --optimize 1. With --denoise the canvas is the tone-mapped output of Engine.denoise over the same frames
(feature targets bound), the clean frame a host serves most often.
`bytes` is what the kernels move at least: the canvas read (4 B per pixel), the coefficients written and read
(2 x 128 B per block) and the file; `kernel_bytes` the same per kernel and `kernel_floor_us` that at 8 TB/s.
Prints one JSON line.

usage: jpeg_encode_cost.py [--sizes 1920x1080,3840x2160] [--qualities 75,90] [--subsampling 0,1,2] [--optimize 0,1]
                           [--denoise] [--frames 8] [--reps 20] [--rounds 3]"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch             # noqa: E402
import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--qualities", default="75,90")
ap.add_argument("--subsampling", default="0", help="0 4:4:4, 1 4:2:2, 2 4:2:0 (Pillow's numbering), comma-separated")
ap.add_argument("--optimize", default="0", help="0 the Annex K tables, 1 tables built for the frame, comma-separated")
ap.add_argument("--denoise", action="store_true", help="encode the denoised frame (Engine.denoise, default parameters)")
ap.add_argument("--frames", type=int, default=8, help="still frames accumulated before the calls are timed")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

meta, mesh_arrays, maps, _ = H.workload("dragon")
stream = torch.cuda.Stream(device=0)


def timed(fn):
    """(us per call by the host's clock, us per call between two events on the stream): the least of the rounds"""
    wall, dev = None, None
    for _ in range(a.rounds):
        for _ in range(3):
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


def output_us(e, p, output):
    best = None
    for _ in range(a.rounds):
        e.timing_begin()
        for _ in range(a.reps):
            p.play_call(output)
        ms, n = e.timing_end("screenOutput")
        best = ms / n * 1e3 if best is None else min(best, ms / n * 1e3)
    return round(best, 1)


def pillow_us(rgb, q, ss, opt):
    try:
        from PIL import Image, ImageFile
    except ImportError:
        return None
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 4 * rgb.size)   # (an optimised save writes the file in one piece)
    img = Image.fromarray(rgb, "RGB")
    best = None
    for _ in range(3):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        img.save(buf, "JPEG", quality=q, subsampling=ss, restart_marker_rows=1, optimize=bool(opt))
        us = (time.perf_counter() - t0) * 1e6
        best = us if best is None else min(best, us)
    return round(best, 1), buf.getvalue()


def block_counts(W, Hh, ss):
    """(blocks, MCU rows): an MCU is 8 hs x 8 vs pixels and hs vs + 2 blocks"""
    hs, vs = ((1, 1), (2, 1), (2, 2))[ss]
    mcus_x, rows = -(-W // (8 * hs)), -(-Hh // (8 * vs))
    return mcus_x * rows * (hs * vs + 2), rows


def kernel_bytes(W, Hh, file_len, ss):
    """the bytes each kernel reads and writes at least: per block 128 B of coefficients and a 4 B
    offset, per MCU row three 4 B words and an 8 B offset, the bit buffer about the file's length (stream)"""
    blocks, rows = block_counts(W, Hh, ss)
    stream = file_len - 629
    return {"pt_jpeg_dct": 4 * W * Hh + blocks * (128 + 4),            # canvas in; coefficients, AC bit counts out
            "pt_jpeg_scan_blocks": blocks * (2 + 4 + 4) + stream,      # a block's DC and count in, offset out; zeroes
            "pt_jpeg_emit": blocks * (128 + 4) + 2 * stream,           # coefficients, offsets in; the bits ORed
            "pt_jpeg_count_ff": stream + rows * 8,                     # the bits in; tile counts, row length out
            "pt_jpeg_scan_rows": rows * 12,
            "pt_jpeg_pack": 2 * stream + rows * 16}                    # the bits in, the stream out


out = {"workload": "dragon", "frames": a.frames, "denoised": a.denoise, "reps": a.reps, "rounds": a.rounds, "sizes": {}}
for size in a.sizes.split(","):
    W, Hh = (int(v) for v in size.lower().split("x"))
    e = bp.Engine(0)
    e.set_stream(stream.cuda_stream)
    p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh_arrays), W, Hh)
    e.resize_canvas(W, Hh)
    if a.denoise:
        nid, alb, clean = (bp.RenderTargetTexture(n, (W, Hh), e) for n in ("featureNormalId", "featureAlbedoWeight", "denoised"))
        p.wrappers[H.path_call(meta["frames"][0])["effect"]].effect.setFeatureTargets(nid, alb)
    for call in meta["frames"][0]:
        p.play_call(call)
    for k in range(a.frames):
        for call in p.synth_frame(k):
            p.play_call(call)
    e.sync()
    output = H.output_call(p.synth_frame(a.frames))
    if a.denoise:   # screenOutput with the filtered accumulation bound as its sampler: a plain tone map of it
        p.textures["denoised"] = clean
        e.denoise(p.textures["pathTracingRenderTarget"], nid, alb, clean)
        output = dict(output)
        output["samplers"] = {k: "denoised" for k in output["samplers"]}
    p.play_call(output)   # (a deferred copy or order build rides along with this one, not with the timed ones)
    row = {"pt_output_us": output_us(e, p, output)}
    wall, dev = timed(lambda: e.read_canvas(W, Hh))
    row["read_pixels_us"] = {"call": wall, "stream": dev, "bytes": 4 * W * Hh}
    canvas = e.read_canvas(W, Hh)
    rgb = canvas[::-1, :, :3].copy()
    for q, ss, opt in ((int(v), int(s), int(o)) for v in a.qualities.split(",") for s in a.subsampling.split(",")
                       for o in a.optimize.split(",")):
        wall, dev = timed(lambda: e.encode_canvas_jpeg(q, subsampling=ss, optimize=opt))
        data = e.encode_canvas_jpeg(q, subsampling=ss, optimize=opt)
        blocks = block_counts(W, Hh, ss)[0]
        moved = 4 * W * Hh + 2 * 128 * blocks + len(data)
        r = {"call_us": wall, "stream_us": dev, "file_bytes": len(data), "blocks": blocks, "bytes": moved,
             "byte_floor_us": round(moved / 8e12 * 1e6, 1), "kernel_bytes": kernel_bytes(W, Hh, len(data), ss),
             "kernel_floor_us": {k: round(v / 8e12 * 1e6, 2) for k, v in kernel_bytes(W, Hh, len(data), ss).items()}}
        pil = pillow_us(rgb, q, ss, opt)
        if pil is None:
            r["pillow_us"] = None   # Pillow is not installed here
        else:
            r["pillow_us"], r["same_bytes_as_pillow"] = pil[0], pil[1] == data
        row[("q%d" % q if ss == 0 else "q%d_s%d" % (q, ss)) + ("_opt" if opt else "")] = r
    out["sizes"]["%dx%d" % (W, Hh)] = row
    e.sync()
    e.set_stream(None)
    e.dispose()
print(json.dumps(out), flush=True)
