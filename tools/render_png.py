#!/usr/bin/env python3
"""Render K progressive frames of a bench workload through the C ABI and save the displayed canvas
(screenOutput: 5x5 denoise, 1/N, Reinhard, gamma) as a PNG - a visual check of the converged image
(BASELINE configs[4]-style: many samples + the output filter). Prints Mpaths/s over the run.

With --features DIR the accumulated G-buffer (Effect.setFeatureTargets) is saved beside it: normal.png
(xyz / weight * 0.5 + 0.5), albedo.png (xyz / weight) and id.png (the last frame's object id, modulo a small
palette).

With --denoise the accumulation is also filtered by Engine.denoise (pt_denoise, default parameters) over the feature
buffers and drawn by the same screenOutput with the result bound as its accumulation sampler - a plain tone map of
it; saved beside the plain image as <out>_denoised.png.

With --hdr PATH the accumulation itself, scaled by 1 / sample count (the page's uOneOverSampleCounter), is written as
a Radiance .hdr file encoded on the device (Engine.encode_target_hdr): the linear radiance the PNG is a tone map of.

usage: render_png.py [--workload dragon|bunny|helmet] [--size WxH] [--frames K] [--features DIR] [--denoise]
                     [--hdr PATH] --out PATH"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import babylon_pt as bp  # noqa: E402
import helpers as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=("dragon", "bunny", "helmet"), default="dragon")
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--out", required=True)
ap.add_argument("--features", metavar="DIR", help="also save normal.png, albedo.png and id.png there")
ap.add_argument("--denoise", action="store_true", help="also save the denoised image as <out>_denoised.png")
ap.add_argument("--hdr", metavar="PATH", help="also save the accumulation / sample count as a Radiance .hdr file")
a = ap.parse_args()
W, Hh = (int(v) for v in a.size.lower().split("x"))
meta = H.stream("hdri_helmet_320x180" if a.workload == "helmet" else "gltf_bunny_1080p")
mesh = H.synthetic_dragon() if a.workload == "dragon" else H.mesh(meta)
e = bp.Engine(0)
p = bp.StreamPlayer(e, meta, H.bluenoise(), H.texture_payloads(meta, mesh), W, Hh)
if a.workload == "helmet":
    maps = H.synthetic_pbr_maps(2048)
    for kind, sampler in H.PBR_SAMPLERS.items():
        p.textures[sampler] = bp.Texture(e, maps[kind], name=kind)
e.resize_canvas(W, Hh)
feat = None
if a.features or a.denoise:
    feat = (bp.RenderTargetTexture("featureNormalId", (W, Hh), e), bp.RenderTargetTexture("featureAlbedoWeight", (W, Hh), e))
    p.wrappers[H.path_call(p.meta["frames"][0])["effect"]].effect.setFeatureTargets(*feat)
for call in p.meta["frames"][0]:
    p.play_call(call)
e.sync()
t0 = time.perf_counter()
for k in range(a.frames):
    for call in p.synth_frame(k):
        p.play_call(call)
e.sync()
dt = time.perf_counter() - t0
img = e.read_canvas(W, Hh)[::-1, :, :3]          # GL rows bottom-up -> image rows top-down
from PIL import Image                             # noqa: E402
Image.fromarray(np.ascontiguousarray(img)).save(a.out)
if a.hdr:
    last = H.output_call(p.synth_frame(a.frames - 1) if a.frames else p.meta["frames"][0])
    one_over_n = float(last["uniforms"]["uOneOverSampleCounter"][1][0])
    data = p.textures["pathTracingRenderTarget"].encode_hdr(one_over_n)
    with open(a.hdr, "wb") as f:
        f.write(data)
    print("hdr: scale 1/%.0f, %d bytes (%.2f B per texel), saved %s" % (1.0 / one_over_n, len(data), len(data) / (W * Hh), a.hdr))
if a.features:
    PALETTE = np.array([[0, 0, 0], [230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48],
                        [145, 30, 180], [70, 240, 240], [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128]], np.uint8)
    nid, alb = (t.read()[::-1] for t in feat)
    wgt = np.maximum(alb[..., 3:4], np.float32(1e-20))   # (the weight is one value for the whole frame, > 0)

    def u8(x):
        return np.ascontiguousarray(np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8))

    os.makedirs(a.features, exist_ok=True)
    Image.fromarray(u8(nid[..., :3] / wgt * 0.5 + 0.5)).save(os.path.join(a.features, "normal.png"))
    Image.fromarray(u8(alb[..., :3] / wgt)).save(os.path.join(a.features, "albedo.png"))
    Image.fromarray(np.ascontiguousarray(PALETTE[nid[..., 3].astype(np.int64) % len(PALETTE)])).save(os.path.join(a.features, "id.png"))
    print("features: weight %.1f, %d object ids, saved normal.png albedo.png id.png in %s" % (
        float(alb[0, 0, 3]), len(np.unique(nid[..., 3])), a.features))
if a.denoise:
    p.textures["denoised"] = bp.RenderTargetTexture("denoised", (W, Hh), e)
    e.denoise(p.textures["pathTracingRenderTarget"], feat[0], feat[1], p.textures["denoised"])
    output = dict(H.output_call(p.synth_frame(a.frames - 1)))
    output["samplers"] = {k: "denoised" for k in output["samplers"]}
    p.play_call(output)
    stem, ext = os.path.splitext(a.out)
    Image.fromarray(np.ascontiguousarray(e.read_canvas(W, Hh)[::-1, :, :3])).save(stem + "_denoised" + ext)
    print("denoised: saved %s" % (stem + "_denoised" + ext))
print("%s %dx%d %d frames: %.1f Mpaths/s, mean %.1f, saved %s" % (a.workload, W, Hh, a.frames,
      W * Hh * a.frames / dt / 1e6, img.mean(), a.out))
