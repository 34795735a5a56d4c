// replay_encode_exr.js — replays a recorded per-frame draw stream (tests/golden/*.json) through the
// Babylon-shaped shim and the N-API addon, then encodes the accumulation on the device as an OpenEXR file
// (Engine.encodeTargetsEXR -> pt_targets_encode_exr): B G R as HALF at scale 1 / frames, given out of order, and the
// alpha as a FLOAT channel A at scale 1, ZIP; with `jobs` the same through encodeTargetsEXRBegin, begun before the
// synchronous call and finished after it. The JavaScript host's view of the EXR encoder. Tests compare it byte for
// byte with the Python binding's and with the reference encoder over the texels written beside it.
//
// usage: node replay_encode_exr.js <stream.json> <payload_dir> <out_prefix> [frames] [jobs]
//   payload_dir as for replay_stream.js: bluenoise.u8 and, for glTF streams, bvh.f32 / tri.f32, hdr.f32
//   writes <out_prefix>.exr and <out_prefix>.acc.f32 (RGBA32F, rows bottom-up); with jobs also <out_prefix>.job.exr
'use strict';
const fs = require('fs');
const path = require('path');
const { install } = require('./babylon_pt.js');

const [streamPath, payloadDir, outPrefix, framesArg, jobsArg] = process.argv.slice(2);
const meta = JSON.parse(fs.readFileSync(streamPath, 'utf8'));
const nFrames = framesArg ? parseInt(framesArg, 10) : meta.frames.length;
const BABYLON = {};
const errors = [];
const size = { width: meta.width, height: meta.height };
install(BABYLON, { width: meta.width, height: meta.height, onError: (m) => errors.push(m) });
const PROGRAMS = { cornell: 3, gltf: 4, hdri: 5, sky: 6, quadric: 7, skymesh: 8 };
const SHADER_PROGRAM = { screenCopyFragmentShader: 1, screenOutputFragmentShader: 2 };

const engine = new BABYLON.Engine(size);
const f32 = (f) => { const b = fs.readFileSync(path.join(payloadDir, f)); return new Float32Array(b.buffer, b.byteOffset, b.byteLength / 4); };
const tex = {
  pathTracingRenderTarget: new BABYLON.RenderTargetTexture('pathTracingRenderTarget', size, engine),
  screenCopyRenderTarget: new BABYLON.RenderTargetTexture('screenCopyRenderTarget', size, engine),
  'file:BlueNoise_RGBA256.png': BABYLON.RawTexture.CreateRGBATexture(new Uint8Array(fs.readFileSync(path.join(payloadDir, 'bluenoise.u8'))), 256, 256, engine, false, false, 1, 0),
};
for (const [raw, kind] of Object.entries(meta.textures || {})) {
  tex[raw] = kind === 'hdr'
    ? BABYLON.RawTexture.CreateRGBATexture(f32('hdr.f32'), meta.hdr.width, meta.hdr.height, engine, false, meta.hdr.invertY, 3, 1)
    : BABYLON.RawTexture.CreateRGBATexture(f32(kind + '.f32'), 2048, 2048, engine, false, false, 1, 1);
}
const renderer = new BABYLON.EffectRenderer(engine);
const wrappers = {};
for (const call of meta.frames[0]) {
  wrappers[call.effect] = new BABYLON.EffectWrapper({ engine, name: call.effect, uniformNames: Object.keys(call.uniforms),
    samplerNames: Object.keys(call.samplers), ptProgram: SHADER_PROGRAM[call.shader] || PROGRAMS[meta.scene] });
}
for (let i = 0; i < nFrames; i++) {
  for (const call of meta.frames[i]) {
    const w = wrappers[call.effect];
    for (const [n, [kind, v]] of Object.entries(call.uniforms)) {
      if (kind === 'i') w.effect.setInt(n, v[0]);
      else if (v.length === 16) w.effect.setMatrix(n, { m: v });
      else if (v.length === 1) w.effect.setFloat(n, v[0]);
      else if (v.length === 2) w.effect.setFloat2(n, v[0], v[1]);
      else w.effect.setFloat3(n, v[0], v[1], v[2]);
    }
    for (const [n, t] of Object.entries(call.samplers)) w.effect.setTexture(n, t ? tex[t] : null);
    renderer.render(w, call.target ? tex[call.target] : null);
  }
}
const acc = tex.pathTracingRenderTarget;
const channels = [
  { name: 'B', rt: acc, component: 2, scale: 1 / nFrames, type: 'half' },
  { name: 'G', rt: acc, component: 1, scale: 1 / nFrames, type: 'half' },
  { name: 'R', rt: acc, component: 0, scale: 1 / nFrames, type: 'half' },
  { name: 'A', rt: acc, component: 3, scale: 1.0, type: 'float' },
];
if (jobsArg === 'jobs') {   // begun before the synchronous call, finished after it
  const job = engine.encodeTargetsEXRBegin(channels, 'zip');
  fs.writeFileSync(outPrefix + '.exr', engine.encodeTargetsEXR(channels, 'zip'));
  fs.writeFileSync(outPrefix + '.job.exr', job.finish());
} else {
  fs.writeFileSync(outPrefix + '.exr', engine.encodeTargetsEXR(channels, 'zip'));
}
fs.writeFileSync(outPrefix + '.acc.f32', Buffer.from(acc.readPixels().buffer));
if (errors.length) { console.error(errors.join('\n')); process.exit(2); }
engine.dispose();
