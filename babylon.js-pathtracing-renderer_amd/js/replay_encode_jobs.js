// replay_encode_jobs.js — replays a recorded per-frame draw stream (tests/golden/*.json) through the
// Babylon-shaped shim and the N-API addon as a Node host that serves every frame does: after each frame's draws
// it begins an encode job (Engine.encodeCanvasJPEGBegin -> pt_canvas_encode_jpeg_begin) and goes on to the next
// frame; a job is finished two frames after it began, so two are pending while the frames run, and the files are
// written at the end. Tests compare every file byte for byte with the Python binding's.
//
// usage: node replay_encode_jobs.js <stream.json> <payload_dir> <out_prefix> [frames] [quality] [subsampling] [optimize]
//   as replay_encode.js; writes <out_prefix>.<frame>.jpg for every frame and <out_prefix>.stats.json (engine.jobStats())
'use strict';
const fs = require('fs');
const path = require('path');
const { install } = require('./babylon_pt.js');

const [streamPath, payloadDir, outPrefix, framesArg, qualityArg, subsamplingArg, optimizeArg] = process.argv.slice(2);
const meta = JSON.parse(fs.readFileSync(streamPath, 'utf8'));
const nFrames = framesArg ? parseInt(framesArg, 10) : meta.frames.length;
const quality = qualityArg ? parseInt(qualityArg, 10) : 90;
const subsampling = subsamplingArg ? parseInt(subsamplingArg, 10) : 0;
const optimize = optimizeArg ? parseInt(optimizeArg, 10) !== 0 : false;
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
const pending = [], files = [];
for (let i = 0; i < nFrames; i++) {
  if (pending.length === 2) files.push(pending.shift().finish());
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
  pending.push(engine.encodeCanvasJPEGBegin(quality, subsampling, optimize));
}
while (pending.length) files.push(pending.shift().finish());
files.forEach((f, i) => fs.writeFileSync(outPrefix + '.' + i + '.jpg', f));
fs.writeFileSync(outPrefix + '.stats.json', JSON.stringify(engine.jobStats()));
if (errors.length) { console.error(errors.join('\n')); process.exit(2); }
engine.dispose();
