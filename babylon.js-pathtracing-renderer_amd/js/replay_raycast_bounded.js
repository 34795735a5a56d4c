// replay_raycast_bounded.js — js/replay_raycast.js's setup (the first frame's uniforms and samplers of a recorded draw
// stream on its path-tracing effect, nothing drawn), then the bounded queries of the shim: Effect.castRays with
// { tMax }, with { tMax, occluded } and Effect.lineOfSight (-> pt_cast_rays_ex, host memory). Tests compare what it
// writes byte for byte with the Python binding's results.
//
// usage: node replay_raycast_bounded.js <stream.json> <payload_dir> <out_prefix>
//   payload_dir as for replay_raycast.js (bluenoise.u8, bvh.f32 / tri.f32, hdr.f32, origins.f32, dirs.f32), plus
//   tmax.f32: one float per ray, and p.f32, q.f32: three floats per segment end each
//   writes <out_prefix>.hits.bin (64 bytes per ray, include/pt.h pt_ray_hit), <out_prefix>.occluded.bin (one byte
//   per ray) and <out_prefix>.los.json (an array of booleans)
'use strict';
const fs = require('fs');
const path = require('path');
const { install } = require('./babylon_pt.js');

const [streamPath, payloadDir, outPrefix] = process.argv.slice(2);
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
for (const [n, t] of Object.entries(call.samplers)) if (t && tex[t]) w.effect.setTexture(n, tex[t]);

const origins = f32('origins.f32'), dirs = f32('dirs.f32'), tMax = f32('tmax.f32');
const hits = w.effect.castRays(origins, dirs, { tMax });
if (hits) fs.writeFileSync(outPrefix + '.hits.bin', Buffer.from(hits));
const occluded = w.effect.castRays(origins, dirs, { tMax, occluded: true });
if (occluded) fs.writeFileSync(outPrefix + '.occluded.bin', Buffer.from(occluded));
const los = w.effect.lineOfSight(f32('p.f32'), f32('q.f32'));
if (los) fs.writeFileSync(outPrefix + '.los.json', JSON.stringify(los));
if (errors.length || !hits || !occluded || !los) { console.error(errors.join('\n')); process.exit(2); }
engine.dispose();
