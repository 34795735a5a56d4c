// replay_raycast.js — sets the first frame's uniforms and samplers of a recorded draw stream (tests/golden/*.json)
// on its path-tracing effect through the Babylon-shaped shim and the N-API addon, draws nothing, and casts rays
// against the bound scene (Effect.castRays / Effect.pick -> pt_cast_rays). The JavaScript host's view of a ray
// query; tests compare its records byte for byte with the Python binding's.
//
// usage: node replay_raycast.js <stream.json> <payload_dir> <out_prefix> [px py]
//   payload_dir as for replay_stream.js (bluenoise.u8 and, for glTF streams, bvh.f32 / tri.f32, hdr.f32), plus
//   origins.f32 and dirs.f32: three floats per ray each
//   writes <out_prefix>.hits.bin (64 bytes per ray, include/pt.h pt_ray_hit) and <out_prefix>.pick.json, the record
//   under pixel (px, py) of the stream's frame (default: its centre)
'use strict';
const fs = require('fs');
const path = require('path');
const { install } = require('./babylon_pt.js');

const [streamPath, payloadDir, outPrefix, pxArg, pyArg] = process.argv.slice(2);
const meta = JSON.parse(fs.readFileSync(streamPath, 'utf8'));
const BABYLON = {};
const errors = [];
const size = { width: meta.width, height: meta.height };
install(BABYLON, { width: meta.width, height: meta.height, onError: (m) => errors.push(m) });
const PROGRAMS = { cornell: 3, gltf: 4, hdri: 5, sky: 6, quadric: 7, skymesh: 8 };

const engine = new BABYLON.Engine(size);
const f32 = (f) => { const b = fs.readFileSync(path.join(payloadDir, f)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const tex = {
  'file:BlueNoise_RGBA256.png': BABYLON.RawTexture.CreateRGBATexture(new Uint8Array(fs.readFileSync(path.join(payloadDir, 'bluenoise.u8'))), 256, 256, engine, false, false, 1, 0),
};
for (const [raw, kind] of Object.entries(meta.textures || {})) {
  tex[raw] = kind === 'hdr'
    ? BABYLON.RawTexture.CreateRGBATexture(f32('hdr.f32'), meta.hdr.width, meta.hdr.height, engine, false, meta.hdr.invertY, 3, 1)
    : BABYLON.RawTexture.CreateRGBATexture(f32(kind + '.f32'), 2048, 2048, engine, false, false, 1, 1);
}
const call = meta.frames[0].find((c) => c.shader === 'pathTracingFragmentShader');
const w = new BABYLON.EffectWrapper({ engine, name: call.effect, uniformNames: Object.keys(call.uniforms),
  samplerNames: Object.keys(call.samplers), ptProgram: PROGRAMS[meta.scene] });
for (const [n, [kind, v]] of Object.entries(call.uniforms)) {
  if (kind === 'i') w.effect.setInt(n, v[0]);
  else if (v.length === 16) w.effect.setMatrix(n, { m: v });
  else if (v.length === 1) w.effect.setFloat(n, v[0]);
  else if (v.length === 2) w.effect.setFloat2(n, v[0], v[1]);
  else w.effect.setFloat3(n, v[0], v[1], v[2]);
}
// (the render targets of the stream are not created: a query needs neither a target nor a history)
for (const [n, t] of Object.entries(call.samplers)) if (t && tex[t]) w.effect.setTexture(n, tex[t]);

const hits = w.effect.castRays(f32('origins.f32'), f32('dirs.f32'));
if (hits) fs.writeFileSync(outPrefix + '.hits.bin', Buffer.from(hits));
const px = pxArg !== undefined ? parseInt(pxArg, 10) : meta.width >> 1;
const py = pyArg !== undefined ? parseInt(pyArg, 10) : meta.height >> 1;
fs.writeFileSync(outPrefix + '.pick.json', JSON.stringify(w.effect.pick(px, py, meta.width, meta.height)));
if (errors.length || !hits) { console.error(errors.join('\n')); process.exit(2); }
engine.dispose();
