// babylon_pt.js — the drop-in: Babylon's effect API (EffectWrapper / EffectRenderer /
// RenderTargetTexture / RawTexture / Texture / Engine render loop) implemented over libpt.so through
// the N-API addon, so the reference's unmodified js/*_Path_Tracing.js setup scripts render on an
// MI355X. Everything else those scripts use (Vector3, Matrix, TransformNode, UniversalCamera,
// SceneLoader, Mesh.MergeMeshes, the glTF loader) stays the real Babylon running on NullEngine:
// the scene graph is host-side bookkeeping, the pixels are produced by the gfx950 kernels.
//
//   const BABYLON = require('babylonjs');              // the vendored build the page loads
//   require('.../js/babylon_pt.js').install(BABYLON, { width: 1920, height: 1080 });
//   // ...then load js/PathTracingCommon.js, the scene shader and the setup script unchanged.
//
// Boundary map (reference call -> C ABI, include/pt.h):
//   new BABYLON.Engine(canvas)                    -> pt_ctx_create           (js/GLTF_Model_Path_Tracing.js:189)
//   new BABYLON.RenderTargetTexture(n,{w,h},...)  -> pt_render_target_create (:762-768), .resize -> pt_render_target_resize
//   BABYLON.RawTexture.CreateRGBATexture(...)     -> pt_texture_create_rgba32f / _rgba8 (:466-487)
//   new BABYLON.Texture(url, ...)                 -> host PNG / JPEG decode + pt_texture_create_rgba8 (:749-758);
//   Texture.updateURL(url, bytes) (glTF loader)   -> the same, for the models' PBR maps
//                                                    '*.hdr' -> host RGBE decode, readPixels() (js/HDRI_Environment_Path_Tracing.js:764-823)
//   new BABYLON.EffectWrapper({...})              -> pt_effect_create (GLSL text -> program) (:773-811)
//   effect.setFloat/.../setMatrix/setTexture      -> pt_set_float / pt_set_int / pt_set_texture (:813-848)
//   new BABYLON.EffectRenderer(engine).render()   -> pt_render (:1230-1235)
//   effect.setFeatureTargets(normalRT, albedoRT)  -> pt_set_feature_targets (extension: accumulated G-buffer)
//   engine.denoise(beautyRT, normalRT, albedoRT, dstRT, opts) -> pt_denoise (extension: a-trous filter over them)
//   effect.setMomentTarget(momentsRT)             -> pt_set_moment_target (extension: accumulated luminance moments)
//   effect.castRays(origins, dirs) / effect.pick(x, y) -> pt_cast_rays (extension: ray queries against the bound scene)
//   effect.castRays(origins, dirs, {tMax, occluded}) / effect.lineOfSight(p, q) -> pt_cast_rays_ex (a bound, occlusion)
//   engine.denoiseVariance(beautyRT, normalRT, albedoRT, momentsRT, dstRT, opts) -> pt_denoise_variance
//   engine.encodeCanvasJPEG(quality, subsampling, optimize) -> pt_canvas_encode_jpeg_opt (extension: the canvas as a JPEG file)
//   engine.encodeCanvasPNG(colour, filter) -> pt_canvas_encode_png (extension: the canvas as a PNG file, lossless)
//   engine.encodeTargetHDR(rt, scale)      -> pt_target_encode_hdr (extension: a render target as a Radiance .hdr file)
//   engine.encodeTargetHDRBegin(rt, scale) / encodeCanvasPNGBegin(colour, filter) -> their job forms
//   engine.encodeTargetsEXR(channels, compression) / encodeTargetsEXRBegin(...) -> pt_targets_encode_exr and its job
//                                (extension: render targets as one multi-channel OpenEXR file)
//   engine.encodeCanvasJPEGBegin(q, s, o) / readCanvasBegin() -> pt_canvas_encode_jpeg_begin / pt_canvas_read_begin
//                                (extension: the same without a host wait; a job with done(), finish(), cancel())
'use strict';
const fs = require('fs');
const path = require('path');
const zlib = require('zlib');

const ERR = { 0: 'PT_OK', '-1': 'PT_ERR_ARG', '-2': 'PT_ERR_HIP', '-3': 'PT_ERR_SHADER', '-4': 'PT_ERR_STATE',
  '-5': 'PT_ERR_OOM', '-6': 'PT_ERR_DEVICE', '-7': 'PT_ERR_UNSUPPORTED', '-8': 'PT_ERR_DATA' };
const TEXTURETYPE_UNSIGNED_BYTE = 0;

function loadAddon() {
  return require(path.join(__dirname, '..', 'napi', 'pt_napi.node'));
}

// ---------------------------------------------------------------------------------- Radiance .hdr
// The HDRI scene loads its environment with new BABYLON.Texture('*.hdr', ..., onLoad) and reads it
// back with readPixels() (js/HDRI_Environment_Path_Tracing.js:764-823). RGBE -> float as Babylon's
// HDRTools: value = mantissa * 2^(exponent - 136), exponent 0 -> 0; scanlines in file order (the
// usual "-Y H +X W" orientation: first scanline = top row = first row of the returned data), alpha 1.
// Both the flat layout and the adaptive run-length scanlines (2,2,hi,lo header) are read.
function decodeHDR(buf) {
  let pos = 0;
  const line = () => { const e = buf.indexOf(10, pos); const l = buf.toString('latin1', pos, e); pos = e + 1; return l; };
  const magic = line();
  if (!magic.startsWith('#?')) throw new Error('not a Radiance HDR file');
  let fmt = '';
  for (let l = line(); l !== ''; l = line()) if (l.startsWith('FORMAT=')) fmt = l.slice(7);
  if (fmt && fmt !== '32-bit_rle_rgbe') throw new Error('unsupported HDR format ' + fmt);
  const m = /^-Y (\d+) \+X (\d+)$/.exec(line().trim());
  if (!m) throw new Error('unsupported HDR orientation');
  const h = parseInt(m[1], 10), w = parseInt(m[2], 10);
  const data = new Float32Array(w * h * 4);
  const rgbe = new Uint8Array(w * 4);
  for (let y = 0; y < h; y++) {
    if (w >= 8 && w < 0x8000 && buf[pos] === 2 && buf[pos + 1] === 2 && ((buf[pos + 2] << 8) | buf[pos + 3]) === w) {
      pos += 4;
      for (let c = 0; c < 4; c++) {
        for (let x = 0; x < w;) {
          let n = buf[pos++];
          if (n > 128) { n -= 128; const v = buf[pos++]; for (let k = 0; k < n; k++) rgbe[4 * (x++) + c] = v; }
          else for (let k = 0; k < n; k++) rgbe[4 * (x++) + c] = buf[pos++];
        }
      }
    } else {
      for (let x = 0; x < 4 * w; x++) rgbe[x] = buf[pos++];
    }
    for (let x = 0; x < w; x++) {
      const e = rgbe[4 * x + 3], o = 4 * (y * w + x);
      const f = e ? Math.pow(2, e - 136) : 0;
      data[o] = rgbe[4 * x] * f; data[o + 1] = rgbe[4 * x + 1] * f; data[o + 2] = rgbe[4 * x + 2] * f; data[o + 3] = 1;
    }
  }
  return { width: w, height: h, data };
}

// ---------------------------------------------------------------------------------- PNG (RGBA8/16)
// The blue-noise texture is a 16-bit RGBA PNG; WebGL samples it as 8-bit. Pinned: high byte.
function decodePNG(buf) {
  if (buf.readUInt32BE(0) !== 0x89504e47) throw new Error('not a PNG');
  let pos = 8, w = 0, h = 0, bd = 0, ct = 0;
  const idat = [];
  while (pos < buf.length) {
    const len = buf.readUInt32BE(pos), type = buf.toString('ascii', pos + 4, pos + 8);
    const body = buf.slice(pos + 8, pos + 8 + len);
    if (type === 'IHDR') { w = body.readUInt32BE(0); h = body.readUInt32BE(4); bd = body[8]; ct = body[9]; if (body[12]) throw new Error('interlaced PNG'); }
    else if (type === 'IDAT') idat.push(body);
    pos += 12 + len;
  }
  const ch = { 6: 4, 2: 3, 0: 1, 4: 2 }[ct];
  if (!ch || (bd !== 8 && bd !== 16)) throw new Error('unsupported PNG format');
  const bpp = ch * bd / 8, stride = w * bpp;
  const raw = zlib.inflateSync(Buffer.concat(idat));
  const cur = Buffer.alloc(stride), prev = Buffer.alloc(stride);
  const out = new Uint8Array(w * h * 4);
  for (let y = 0, p = 0; y < h; y++) {
    const ft = raw[p++];
    for (let x = 0; x < stride; x++) {
      const a = x >= bpp ? cur[x - bpp] : 0, b = prev[x], c = x >= bpp ? prev[x - bpp] : 0;
      let v = raw[p++];
      if (ft === 1) v += a; else if (ft === 2) v += b; else if (ft === 3) v += (a + b) >> 1;
      else if (ft === 4) { const pa = Math.abs(b - c), pb = Math.abs(a - c), pc = Math.abs(a + b - 2 * c); v += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
      cur[x] = v & 255;
    }
    for (let x = 0; x < w; x++) {
      const px = [0, 0, 0, 255];
      for (let k = 0; k < ch; k++) px[k] = cur[x * bpp + k * (bd / 8)];   // 16-bit: high byte
      if (ch === 1) { px[1] = px[2] = px[0]; }
      if (ch === 2) { px[3] = px[1]; px[1] = px[2] = px[0]; }
      out.set(px, 4 * (y * w + x));
    }
    cur.copy(prev);
  }
  return { width: w, height: h, data: out };
}

// ---------------------------------------------------------------------------------- JPEG (host)
// JPEG maps (the glTF models' PBR textures) are decoded by libpt (pt_jpeg_decode_rgba8,
// csrc/pt_jpeg.cpp: libjpeg-turbo's default decompression reproduced bit for bit), through the addon.
function decodeImage(buf, addon) {
  buf = Buffer.from(buf.buffer ? Buffer.from(buf.buffer, buf.byteOffset, buf.byteLength) : buf);
  if (buf.length >= 4 && buf.readUInt32BE(0) === 0x89504e47) return decodePNG(buf);
  if (!(buf.length >= 2 && buf[0] === 0xff && buf[1] === 0xd8)) throw new Error('not a PNG or JPEG image');
  addon = addon || loadAddon();
  const wh = addon.pt_jpeg_size(buf);
  if (typeof wh === 'number') throw new Error('JPEG: ' + (ERR[wh] || wh));
  const data = new Uint8Array(4 * wh[0] * wh[1]);
  const rc = addon.pt_jpeg_decode_rgba8(buf, data);
  if (rc < 0) throw new Error('JPEG: ' + (ERR[rc] || rc));
  return { width: wh[0], height: wh[1], data };
}

function install(BABYLON, opts) {
  opts = Object.assign({ device: 0, width: 1920, height: 1080, baseDir: process.cwd(), addon: null, onError: null,
                        label: null }, opts || {});
  const addon = opts.addon || loadAddon();
  // opts.label(handle, name): optional debug hook naming each native handle (tracing tools)
  const label = (h, name) => { if (opts.label && h && typeof h !== 'number') opts.label(h, name); return h; };
  const report = opts.onError || ((msg) => console.error('[babylon_pt] ' + msg));
  // with the real Babylon loaded, the scene graph runs on its NullEngine; without it (e.g. a replay
  // host on the GPU box) a minimal base keeps the render-size bookkeeping
  const RealNull = BABYLON.NullEngine || class {
    constructor(o) { this._options = o; }
    getRenderWidth() { return this._options.renderWidth; }
    getRenderHeight() { return this._options.renderHeight; }
    dispose() {}
  };
  const set = (k, v) => { try { BABYLON[k] = v; } catch (e) { Object.defineProperty(BABYLON, k, { value: v, writable: true, configurable: true }); } };
  let current = null;   // the engine whose context owns textures created without an engine argument

  function check(ctx, rc, what) {
    if (typeof rc === 'number' && rc !== 0) report(what + ': ' + (ERR[rc] || rc) + ' ' + addon.pt_last_error(ctx));
    return rc;
  }
  // the addon's arguments of pt_targets_encode_exr behind the context: five parallel arrays and the compression
  function exrArgs(channels, compression) {
    const types = { half: 1, float: 2 };
    const compressions = { none: 0, zips: 2, zip: 3 };
    const z = typeof compression === 'string' ? compressions[compression] : compression | 0;
    if (z === undefined) throw new Error('encodeTargetsEXR: unknown compression');
    const list = Array.from(channels || []);
    return [list.map((c) => String(c.name)), list.map((c) => (c.rt ? c.rt._pt : null)), list.map((c) => c.component | 0),
      list.map((c) => (c.scale === undefined ? 1.0 : +c.scale)),
      list.map((c) => (typeof c.type === 'string' ? types[c.type] | 0 : c.type | 0)), z];
  }
  function ctxOf(sceneOrEngine) {
    if (sceneOrEngine && sceneOrEngine._pt) return sceneOrEngine._pt;
    if (sceneOrEngine && sceneOrEngine.getEngine && sceneOrEngine.getEngine()._pt) return sceneOrEngine.getEngine()._pt;
    return current._pt;
  }

  class Engine extends RealNull {
    constructor(canvas, antialias, options) {
      const w = (canvas && canvas.width) || opts.width, h = (canvas && canvas.height) || opts.height;
      super({ renderWidth: w, renderHeight: h, textureSize: 512, deterministicLockstep: false, lockstepMaxSteps: 1 });
      // the devices of the context: opts.devices, else PT_DEVICES ("0,1,2,3"; a device may repeat),
      // else opts.device - with several, every draw fans out over them inside libpt (pt.h)
      const devs = opts.devices || (process.env.PT_DEVICES ? process.env.PT_DEVICES.split(',').map((d) => parseInt(d, 10)) : null);
      const c = devs ? addon.pt_ctx_create_devices(devs) : addon.pt_ctx_create(opts.device);
      if (typeof c === 'number') throw new Error('pt_ctx_create: ' + (ERR[c] || c));
      this._pt = c;
      this._renderLoop = null;
      this.isPointerLock = false;
      addon.pt_canvas_resize(c, w, h);
      current = this;
    }
    runRenderLoop(fn) { this._renderLoop = fn; }
    // the browser calls the loop from requestAnimationFrame; a Node host steps it explicitly
    stepFrame() { if (this._renderLoop) this._renderLoop(); }
    enterPointerlock() {}
    exitPointerlock() {}
    setHardwareScalingLevel(l) { this._scaling = l; }
    getDeltaTime() { return opts.deltaTimeMs || 1000 / 60; }
    resize() { addon.pt_canvas_resize(this._pt, this.getRenderWidth(), this.getRenderHeight()); }
    readCanvas() {
      const out = new Uint8Array(this.getRenderWidth() * this.getRenderHeight() * 4);
      check(this._pt, addon.pt_read_pixels(this._pt, null, out), 'readPixels');
      return out;
    }
    // MI355X extension (pt_canvas_encode_jpeg_opt): the canvas as a baseline JPEG file (a restart interval per MCU
    // row) encoded on the device, as a Buffer; the bytes are libjpeg-turbo's for the same pixels, quality and
    // subsampling (0 4:4:4, 1 4:2:2, 2 4:2:0), with `optimize` those of its optimize_coding: Huffman tables built
    // on the device for this canvas, a shorter file of the same pixels. The buffer starts at the last call's
    // length; the call is repeated once when it answers that it is too small.
    encodeCanvasJPEG(quality = 90, subsampling = 0, optimize = false) {
      const opt = optimize ? 1 : 0;
      let buf = Buffer.allocUnsafe(this._jpegCapacity || 65536);
      let [rc, size] = addon.pt_canvas_encode_jpeg_opt(this._pt, quality | 0, subsampling | 0, opt, buf);
      if (rc !== 0 && size > buf.length) {
        buf = Buffer.allocUnsafe(size);
        [rc, size] = addon.pt_canvas_encode_jpeg_opt(this._pt, quality | 0, subsampling | 0, opt, buf);
      }
      check(this._pt, rc, 'encodeCanvasJPEG');
      this._jpegCapacity = Math.max(buf.length, size);
      return buf.subarray(0, size);
    }
    // MI355X extension (pt_canvas_encode_png): the canvas as a PNG file, lossless, encoded on the device, as a
    // Buffer. colour 'rgb' (alpha ignored) or 'rgba'; filter 'none', 'sub', 'up', 'average', 'paeth' on every row or
    // 'adaptive' (per row the least sum of |byte as int8|); the numbers of include/pt.h are taken too. One IDAT per
    // 16,320 filtered bytes, each what zlib 1.2.11 writes for that chunk under Z_RLE at level 6 with a full flush.
    encodeCanvasPNG(colour = 'rgb', filter = 'adaptive') {
      const colours = { rgb: 0, rgba: 1 };
      const filters = { none: 0, sub: 1, up: 2, average: 3, paeth: 4, adaptive: 5 };
      const c = typeof colour === 'string' ? colours[colour] : colour | 0;
      const f = typeof filter === 'string' ? filters[filter] : filter | 0;
      if (c === undefined || f === undefined) throw new Error('encodeCanvasPNG: unknown colour or filter');
      let buf = Buffer.allocUnsafe(this._pngCapacity || 65536);
      let [rc, size] = addon.pt_canvas_encode_png(this._pt, c, f, buf);
      if (rc !== 0 && size > buf.length) {
        buf = Buffer.allocUnsafe(size);
        [rc, size] = addon.pt_canvas_encode_png(this._pt, c, f, buf);
      }
      check(this._pt, rc, 'encodeCanvasPNG');
      this._pngCapacity = Math.max(buf.length, size);
      return buf.subarray(0, size);
    }
    // MI355X extension (pt_target_encode_hdr): the RGBA32F RenderTargetTexture `rt` times `scale` as a Radiance .hdr
    // file (RGBE, scanlines run-length coded plane by plane), encoded on the device, as a Buffer: the accumulation
    // with scale = 1 / sample count, a denoised frame, a feature buffer. decodeHDR reads it back.
    encodeTargetHDR(rt, scale = 1.0) {
      const t = rt ? rt._pt : null;
      let buf = Buffer.allocUnsafe(this._hdrCapacity || 65536);
      let [rc, size] = addon.pt_target_encode_hdr(this._pt, t, +scale, buf);
      if (rc !== 0 && size > buf.length) {
        buf = Buffer.allocUnsafe(size);
        [rc, size] = addon.pt_target_encode_hdr(this._pt, t, +scale, buf);
      }
      check(this._pt, rc, 'encodeTargetHDR');
      this._hdrCapacity = Math.max(buf.length, size);
      return buf.subarray(0, size);
    }
    // MI355X extension (pt_target_encode_hdr_begin): encodeTargetHDR without the host wait; what is deferred is
    // queued first, never waited for. `rt` must outlive the job.
    encodeTargetHDRBegin(rt, scale = 1.0) {
      const h = addon.pt_target_encode_hdr_begin(this._pt, rt ? rt._pt : null, +scale);
      if (typeof h === 'number') { check(this._pt, h, 'encodeTargetHDRBegin'); return null; }
      return new Job(this, h);
    }
    // MI355X extension (pt_targets_encode_exr): render targets as one multi-channel OpenEXR file, encoded on the
    // device, as a Buffer. `channels` is an array of { name, rt, component 0..3, scale, type 'half' | 'float' }: each
    // stores one component of one RGBA32F RenderTargetTexture times its scale; `compression` 'none', 'zips' or 'zip'.
    encodeTargetsEXR(channels, compression = 'zip') {
      const a = exrArgs(channels, compression);
      let buf = Buffer.allocUnsafe(this._exrCapacity || 65536);
      let [rc, size] = addon.pt_targets_encode_exr(this._pt, ...a, buf);
      if (rc !== 0 && size > buf.length) {
        buf = Buffer.allocUnsafe(size);
        [rc, size] = addon.pt_targets_encode_exr(this._pt, ...a, buf);
      }
      check(this._pt, rc, 'encodeTargetsEXR');
      this._exrCapacity = Math.max(buf.length, size);
      return buf.subarray(0, size);
    }
    // MI355X extension (pt_targets_encode_exr_begin): encodeTargetsEXR without the host wait; what is deferred is
    // queued first, never waited for. The targets must outlive the job.
    encodeTargetsEXRBegin(channels, compression = 'zip') {
      const h = addon.pt_targets_encode_exr_begin(this._pt, ...exrArgs(channels, compression));
      if (typeof h === 'number') { check(this._pt, h, 'encodeTargetsEXRBegin'); return null; }
      return new Job(this, h);
    }
    // MI355X extension (pt_canvas_encode_png_begin): encodeCanvasPNG without the host wait
    encodeCanvasPNGBegin(colour = 'rgb', filter = 'adaptive') {
      const colours = { rgb: 0, rgba: 1 };
      const filters = { none: 0, sub: 1, up: 2, average: 3, paeth: 4, adaptive: 5 };
      const c = typeof colour === 'string' ? colours[colour] : colour | 0;
      const f = typeof filter === 'string' ? filters[filter] : filter | 0;
      if (c === undefined || f === undefined) throw new Error('encodeCanvasPNGBegin: unknown colour or filter');
      const h = addon.pt_canvas_encode_png_begin(this._pt, c, f);
      if (typeof h === 'number') { check(this._pt, h, 'encodeCanvasPNGBegin'); return null; }
      return new Job(this, h);
    }
    // MI355X extension (pt_canvas_encode_jpeg_begin): encodeCanvasJPEG without the host wait. Everything is queued
    // behind the draws so far; the returned job's finish() is the file the synchronous call would have returned
    // now, whatever is drawn in between. At most 4 jobs are pending; no deferred screenCopy runs.
    encodeCanvasJPEGBegin(quality = 90, subsampling = 0, optimize = false) {
      const h = addon.pt_canvas_encode_jpeg_begin(this._pt, quality | 0, subsampling | 0, optimize ? 1 : 0);
      if (typeof h === 'number') { check(this._pt, h, 'encodeCanvasJPEGBegin'); return null; }
      return new Job(this, h);
    }
    // MI355X extension (pt_canvas_read_begin): readCanvas without the host wait; finish() is the RGBA8 canvas, rows
    // bottom-up, as of this call
    readCanvasBegin() {
      const h = addon.pt_canvas_read_begin(this._pt);
      if (typeof h === 'number') { check(this._pt, h, 'readCanvasBegin'); return null; }
      return new Job(this, h);
    }
    // [jobs begun, finished, of those through the slow copy, cancelled] since the engine was created
    jobStats() { return addon.pt_job_stats(this._pt); }
    // MI355X extension (pt_denoise): the edge-avoiding a-trous filter of the RenderTargetTexture `beauty`, guided
    // by the feature targets accumulated beside it (effect.setFeatureTargets), into `dst`: the accumulation's
    // scale, sharpness flags 1, so screenOutput with `dst` as its accumulationBuffer tone-maps it unchanged.
    // o: { iterations = 3, sigmaNormal = 0.5, sigmaColour = 1.0, demodulate = true }. Asynchronous.
    denoise(beauty, normalRT, albedoRT, dst, o) {
      o = o || {};
      const pt = (t) => (t ? t._pt : null);
      return check(this._pt, addon.pt_denoise(this._pt, pt(beauty), pt(normalRT), pt(albedoRT), pt(dst),
        o.iterations === undefined ? 3 : o.iterations | 0, o.sigmaNormal === undefined ? 0.5 : +o.sigmaNormal,
        o.sigmaColour === undefined ? 1.0 : +o.sigmaColour, o.demodulate === undefined || o.demodulate ? 1 : 0), 'denoise');
    }
    // MI355X extension (pt_denoise_variance): the same filter with a luminance edge-stop scaled by each pixel's
    // own variance, from the moments accumulated by effect.setMomentTarget; `dst` as for denoise.
    // o: { iterations = 3, sigmaNormal = 0.5, sigmaLuminance = 4.0, demodulate = true }. Asynchronous.
    denoiseVariance(beauty, normalRT, albedoRT, momentsRT, dst, o) {
      o = o || {};
      const pt = (t) => (t ? t._pt : null);
      return check(this._pt, addon.pt_denoise_variance(this._pt, pt(beauty), pt(normalRT), pt(albedoRT), pt(momentsRT), pt(dst),
        o.iterations === undefined ? 3 : o.iterations | 0, o.sigmaNormal === undefined ? 0.5 : +o.sigmaNormal,
        o.sigmaLuminance === undefined ? 4.0 : +o.sigmaLuminance, o.demodulate === undefined || o.demodulate ? 1 : 0), 'denoiseVariance');
    }
    dispose() { if (this._pt) { addon.pt_ctx_destroy(this._pt); this._pt = null; } super.dispose(); }
  }

  // A pending encode or read job (engine.encodeCanvasJPEGBegin, readCanvasBegin): done() never blocks, finish()
  // waits for this job only and returns its bytes as a Buffer, cancel() gives the slot back without them. Dead
  // after finish() or cancel(), and with its engine.
  class Job {
    constructor(engine, handle) { this._engine = engine; this._pt = handle; }
    done() {
      const [rc, flag] = addon.pt_job_poll(this._pt);
      check(this._engine._pt, rc, 'job.done');
      return flag === 1;
    }
    finish() {
      let buf = Buffer.allocUnsafe(this._engine._jobCapacity || 65536);
      let [rc, size] = addon.pt_job_finish(this._pt, buf);
      if (rc !== 0 && size > buf.length) {   // (the job stays valid: once more with the length it reported)
        buf = Buffer.allocUnsafe(size);
        [rc, size] = addon.pt_job_finish(this._pt, buf);
      }
      check(this._engine._pt, rc, 'job.finish');
      this._engine._jobCapacity = Math.max(buf.length, size);
      this._pt = null;
      return buf.subarray(0, size);
    }
    cancel() { check(this._engine._pt, addon.pt_job_cancel(this._pt), 'job.cancel'); this._pt = null; }
  }

  class RenderTargetTexture {
    constructor(name, size, scene) {
      this.name = name;
      this._ctx = ctxOf(scene);
      const h = addon.pt_render_target_create(this._ctx, size.width, size.height);
      if (typeof h === 'number') throw new Error('RenderTargetTexture: ' + (ERR[h] || h));
      this._pt = label(h, name);
    }
    getSize() { const s = addon.pt_texture_size(this._pt); return { width: s[0], height: s[1] }; }
    resize(size) { check(this._ctx, addon.pt_render_target_resize(this._pt, size.width, size.height), 'resize'); }
    readPixels() {
      const s = this.getSize(), out = new Float32Array(s.width * s.height * 4);
      check(this._ctx, addon.pt_read_pixels(this._ctx, this._pt, out), 'readPixels');
      return out;
    }
    dispose() { if (this._pt) addon.pt_texture_destroy(this._pt); this._pt = null; }
  }

  const RawTexture = {
    CreateRGBATexture(data, w, h, scene, generateMipMaps, invertY, samplingMode, type) {
      const ctx = ctxOf(scene);
      const t = { name: 'RawTexture', _ctx: ctx };
      const sampling = samplingMode === undefined ? 3 : samplingMode;
      const handle = type === TEXTURETYPE_UNSIGNED_BYTE || data instanceof Uint8Array
        ? addon.pt_texture_create_rgba8(ctx, w, h, data, sampling, invertY ? 1 : 0)
        : addon.pt_texture_create_rgba32f(ctx, w, h, data, sampling, invertY ? 1 : 0);
      if (typeof handle === 'number') { report('CreateRGBATexture: ' + (ERR[handle] || handle)); return null; }
      t._pt = label(handle, 'RawTexture');
      t.dispose = () => { if (t._pt) addon.pt_texture_destroy(t._pt); t._pt = null; };
      return t;
    },
  };

  function adoptForeign(ctx, t) {
    t._ptForeign = null;
    const bytes = t._buffer;
    if (!bytes || typeof bytes === 'string') return;
    try {
      const img = decodeImage(bytes, addon);
      const sm = typeof t.samplingMode === 'number' ? t.samplingMode : 3;
      const h = addon.pt_texture_create_rgba8(ctx, img.width, img.height, img.data, sm, t._invertY ? 1 : 0);
      if (typeof h !== 'number') t._ptForeign = label(h, t.name || t.url || 'texture');
    } catch (e) {
      report('texture ' + (t.name || t.url) + ': ' + e.message + ' (left unbound)');
    }
  }

  class Texture {
    // new Texture(url, scene, noMipmap, invertY, samplingMode, onLoad) or, as the glTF loader calls
    // it, new Texture(null, scene, { invertY, samplingMode, onLoad, ... }) then updateURL(url, bytes)
    constructor(url, scene, noMipmap, invertY, samplingMode, onLoad) {
      if (noMipmap && typeof noMipmap === 'object') {
        const o = noMipmap;
        invertY = o.invertY; samplingMode = o.samplingMode; onLoad = o.onLoad;
      }
      this._name = url || '';
      this._ctx = ctxOf(scene);
      this._pt = null;
      this._size = { width: 0, height: 0 };
      this._pixels = null;
      this._invertY = invertY === undefined ? true : !!invertY;
      this._sampling = samplingMode === undefined ? 3 : samplingMode;
      this._onLoad = onLoad;
      if (url === null || url === undefined) return;   // bytes follow through updateURL
      // page-relative URLs resolve against baseDir, then the extra opts.assetDirs
      const dirs = [opts.baseDir].concat(opts.assetDirs || []);
      const file = path.isAbsolute(url) ? url
        : (dirs.map((d) => path.join(d, url)).find((f) => fs.existsSync(f)) || path.join(opts.baseDir, url));
      if (/\.hdr$/i.test(url)) {
        // an environment: decoded on the host, handed back through readPixels(); the setup script
        // re-uploads it as a RawTexture (so nothing is bound here)
        try {
          const img = decodeHDR(fs.readFileSync(file));
          this._size = { width: img.width, height: img.height };
          this._pixels = img.data;
          if (onLoad) setImmediate(onLoad);
        } catch (e) {
          report('Texture(' + url + '): ' + e.message + ' (not loaded)');
        }
        return;
      }
      let bytes;
      try { bytes = fs.readFileSync(file); } catch (e) { report('Texture(' + url + '): ' + e.message + ' (left unbound)'); return; }
      this._upload(bytes, url);
    }
    // the glTF loader's path: the image file's bytes (Babylon's Texture.updateURL(url, buffer))
    updateURL(url, buffer) {
      if (!this._name || this._name.startsWith('data:')) this._name = url;
      if (this._pt) { addon.pt_texture_destroy(this._pt); this._pt = null; }
      if (buffer) this._upload(buffer, url);
      else report('Texture.updateURL(' + url + '): no image bytes (left unbound)');
    }
    _upload(bytes, what) {
      try {
        const img = decodeImage(bytes, addon);
        this._size = { width: img.width, height: img.height };
        const h = addon.pt_texture_create_rgba8(this._ctx, img.width, img.height, img.data, this._sampling, this._invertY ? 1 : 0);
        if (typeof h !== 'number') this._pt = label(h, this._name || what);
        if (this._onLoad) setImmediate(this._onLoad);
      } catch (e) {
        report('Texture(' + what + '): ' + e.message + ' (left unbound)');
      }
    }
    get name() { return this._name; }
    set name(v) { this._name = v; if (this._pt) label(this._pt, v); }
    getSize() { return this._size; }
    readPixels() { return Promise.resolve(this._pixels); }
    dispose() { if (this._pt) addon.pt_texture_destroy(this._pt); this._pt = null; }
  }

  class Effect {
    constructor(ctx, handle) { this._ctx = ctx; this._pt = handle; this._cam = {}; }
    isReady() { return this._pt !== null; }
    _f(name, arr) { if (CAMERA_UNIFORMS.has(name)) this._cam[name] = Float32Array.from(arr); if (this._pt) check(this._ctx, addon.pt_set_float(this._pt, name, arr), 'set ' + name); return this; }
    setFloat(n, v) { return this._f(n, [v]); }
    setFloat2(n, a, b) { return this._f(n, [a, b]); }
    setFloat3(n, a, b, c) { return this._f(n, [a, b, c]); }
    setFloat4(n, a, b, c, d) { return this._f(n, [a, b, c, d]); }
    setVector2(n, v) { return this._f(n, [v.x, v.y]); }
    setVector3(n, v) { return this._f(n, [v.x, v.y, v.z]); }
    setMatrix(n, m) { return this._f(n, Array.from(m.m !== undefined ? m.m : m.toArray())); }
    setInt(n, v) { if (this._pt) check(this._ctx, addon.pt_set_int(this._pt, n, v | 0), 'setInt ' + n); return this; }
    setBool(n, v) { return this.setInt(n, v ? 1 : 0); }
    setTexture(n, t) {
      // an unloaded Babylon texture (null / undefined, e.g. a model without albedo map) binds
      // nothing; a texture Babylon itself created (the glTF loader's PBR maps) is uploaded once,
      // from the image bytes it keeps (Texture.updateURL(url, buffer))
      if (t && !t._pt && t._ptForeign === undefined) adoptForeign(this._ctx, t);
      const h = t ? (t._pt || t._ptForeign || null) : null;
      if (this._pt) check(this._ctx, addon.pt_set_texture(this._pt, n, h), 'setTexture ' + n);
      return this;
    }
    // MI355X extension (pt_set_feature_targets): while RenderTargetTextures are bound here, every draw of
    // this path-tracing effect also accumulates its G-buffer into them in place, by the beauty's history
    // rule: normalRT = (sum of objectNormal, this draw's objectID), albedoRT = (sum of objectColor, weight).
    // null / undefined: that buffer is not produced; both: the feature is off
    setFeatureTargets(normalRT, albedoRT) {
      if (this._pt) {
        check(this._ctx, addon.pt_set_feature_targets(this._pt, normalRT ? normalRT._pt : null, albedoRT ? albedoRT._pt : null),
          'setFeatureTargets');
      }
      return this;
    }
    // MI355X extension (pt_set_moment_target): while a RenderTargetTexture is bound here, every draw of this
    // path-tracing effect also accumulates the luminance L of its radiance into it in place, by the beauty's
    // history rule: momentsRT = (sum of L, sum of L^2, 0, weight). null / undefined unbinds it
    setMomentTarget(momentsRT) {
      if (this._pt) check(this._ctx, addon.pt_set_moment_target(this._pt, momentsRT ? momentsRT._pt : null), 'setMomentTarget');
      return this;
    }
    // MI355X extension (pt_cast_rays): SceneIntersect of this path-tracing effect's program, with the uniforms and
    // data textures bound now, on world-space rays (3 floats per ray each). Returns an ArrayBuffer of 64-byte records
    // (include/pt.h pt_ray_hit: t, object_id, type, triangle | normal.xyz, bary_u | color.xyz, bary_v | uv.xy, 0, 0),
    // or null when the call fails (reported through onError)
    // With `opts` (pt_cast_rays_ex, host memory): { tMax: Float32Array, one per ray } bounds each ray - hitT starts at
    // min(INFINITY, tMax), so nothing at tMax or beyond is taken (the walk's bound, INTEGRATION.md "Ray queries") -
    // and { occluded: true } returns one byte per ray instead, 1 where the bounded query reports an object.
    castRays(origins, dirs, opts) {
      if (!this._pt) return null;
      const tMax = opts && opts.tMax !== undefined ? opts.tMax : null, occluded = !!(opts && opts.occluded);
      const r = tMax === null && !occluded ? addon.pt_cast_rays(this._pt, origins, dirs)
        : addon.pt_cast_rays_ex(this._pt, origins, dirs, tMax, occluded);
      if (typeof r === 'number') { check(this._ctx, r, 'castRays'); return null; }
      return r;
    }
    // ... whether nothing occludes the open segment from p[i] to q[i] (3 floats per point each): castRays with
    // dirs = q - p formed in float32, tMax = 1 and occluded. Returns an Array of booleans, or null on failure.
    lineOfSight(p, q) {
      const n = Math.floor(p.length / 3);
      const d = new Float32Array(p.length), t = new Float32Array(n).fill(1);
      for (let i = 0; i < p.length; i++) d[i] = Math.fround(Math.fround(q[i]) - Math.fround(p[i]));
      const r = this.castRays(Float32Array.from(p), d, { tMax: t, occluded: true });
      return r ? Array.from(new Uint8Array(r), (v) => v === 0) : null;
    }
    // ... the pinhole ray through the centre of pixel (x, y) (row 0 the bottom one, as gl_FragCoord; width x height
    // default to uResolution), formed in float32 from uCameraMatrix, uULen and uVLen as the shaders' main() forms its
    // direction - no jitter, no aperture - then normalised: { t, objectId, type, triangle, normal, baryU, baryV,
    // color, uv, hit }, t a valid uFocusDistance when `hit`
    pick(x, y, width, height) {
      const f = Math.fround, c = this._cam;
      const m = c.uCameraMatrix || new Float32Array(16);
      const ulen = c.uULen ? c.uULen[0] : 0, vlen = c.uVLen ? c.uVLen[0] : 0;
      const w = width !== undefined ? width : (c.uResolution ? c.uResolution[0] : 0);
      const h = height !== undefined ? height : (c.uResolution ? c.uResolution[1] : 0);
      const ppx = f(f(f(f(x) + 0.5) / f(w)) * 2 - 1), ppy = f(f(f(f(y) + 0.5) / f(h)) * 2 - 1);
      const d = [0, 1, 2].map((k) => f(f(f(f(m[k] * ppx) * ulen) + f(f(m[4 + k] * ppy) * vlen)) + m[8 + k]));
      const inv = f(1 / f(Math.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))));
      const buf = this.castRays(new Float32Array([m[12], m[13], m[14]]), new Float32Array(d.map((v) => f(v * inv))));
      if (!buf) return null;
      const F = new Float32Array(buf), I = new Int32Array(buf);
      return { t: F[0], objectId: I[1], type: I[2], triangle: I[3], normal: [F[4], F[5], F[6]], baryU: F[7],
        color: [F[8], F[9], F[10]], baryV: F[11], uv: [F[12], F[13]], hit: I[1] >= 0 };
    }
  }

  class EffectWrapper {
    constructor(o) {
      this.name = o.name;
      const ctx = ctxOf(o.engine);
      // o.ptProgram (extension): name the program directly when the GLSL text is not at hand
      const h = o.ptProgram
        ? addon.pt_effect_create_program(ctx, o.ptProgram, o.uniformNames || [], o.samplerNames || [])
        : addon.pt_effect_create(ctx, o.fragmentShader || '', o.uniformNames || [], o.samplerNames || []);
      label(h, o.name);
      if (typeof h === 'number') report('EffectWrapper(' + o.name + '): ' + (ERR[h] || h) + ' ' + addon.pt_last_error(ctx));
      this.effect = new Effect(ctx, typeof h === 'number' ? null : h);
      this._observers = [];
      this.onApplyObservable = { add: (f) => { this._observers.push(f); return f; }, clear: () => { this._observers = []; } };
    }
    dispose() { if (this.effect._pt) addon.pt_effect_destroy(this.effect._pt); this.effect._pt = null; }
  }

  class EffectRenderer {
    constructor(engine) { this.engine = engine; }
    // Babylon skips a non-ready effect silently; so does this
    render(wrapper, target) {
      if (!wrapper.effect.isReady()) return;
      wrapper._observers.forEach((f) => f());
      check(wrapper.effect._ctx, addon.pt_render(wrapper.effect._pt, target ? target._pt : null), 'render ' + wrapper.name);
    }
    dispose() {}
  }

  set('Engine', Engine);
  set('RenderTargetTexture', RenderTargetTexture);
  set('RawTexture', RawTexture);
  set('Texture', Texture);
  set('EffectWrapper', EffectWrapper);
  set('EffectRenderer', EffectRenderer);
  return { addon, Engine, decodePNG, decodeHDR, decodeImage, nativeBVH: (device) => nativeBVH(addon, device) };
}

// BVH_Build_Iterative(workList, aabb_array) (js/BVH_Fast_Builder.js:320-406) over libpt's native
// builder (same tree, same bits); with a device number, over the device build (pt_bvh_build_gpu,
// same bits again). A host installs it after loading BVH_Fast_Builder.js:
//   globalThis.BVH_Build_Iterative = require('.../babylon_pt.js').nativeBVH(addon[, device]);
function nativeBVH(addon, device) {
  return function BVH_Build_Iterative(workList, aabbArray) {
    const n = workList.length;
    const out = new Float32Array(8 * (2 * n - 1));
    const work = Uint32Array.from(workList);
    const rc = device === undefined || device === null
      ? addon.pt_bvh_build(aabbArray.subarray(0, 9 * n), work, out)
      : addon.pt_bvh_build_gpu(device, aabbArray, work, out);
    if (rc < 0) throw new Error('pt_bvh_build: ' + (ERR[rc] || rc));
    aabbArray.set(out, 0);
  };
}

// the float uniforms Effect.pick forms its ray from (the shim keeps their last values)
const CAMERA_UNIFORMS = new Set(['uCameraMatrix', 'uULen', 'uVLen', 'uResolution']);

module.exports = { install, decodePNG, decodeHDR, decodeImage, nativeBVH, loadAddon };
