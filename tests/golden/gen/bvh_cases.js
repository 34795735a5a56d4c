// bvh_cases.js — runs the reference's own, unmodified BVH_Build_Iterative (js/BVH_Fast_Builder.js
// over the vendored js/babylon.js, both loaded at run time from PT_REFERENCE) on the directed
// inputs that make_bvh_cases.py writes, and writes back the node array it leaves. Build container
// only, like make_fixtures.js; nothing of the reference is copied.
//
// usage: node bvh_cases.js <dir>
//   <dir>/cases.json          [{name, tris, work}]: triangle count and work-list length per case
//   <dir>/<name>.aabb.u32     tris x 9 float32 as raw little-endian bits (NaN and zero signs kept)
//   <dir>/<name>.work.u32     the work list
//   -> <dir>/<name>.nodes.u32 (2 * work - 1) x 8 float32 as raw bits
'use strict';
const fs = require('fs');
const path = require('path');
const vm = require('vm');

const REF = process.env.PT_REFERENCE || '/root/reference';
const dir = process.argv[2];
require('./browser_env.js').setup(REF, 64, 64, 1);
vm.runInThisContext(fs.readFileSync(path.join(REF, 'js/BVH_Fast_Builder.js'), 'utf8'), { filename: 'js/BVH_Fast_Builder.js' });
const build = vm.runInThisContext('BVH_Build_Iterative');

// the array the setup scripts hand to the builder (2048 x 2048 RGBA floats): the per-triangle
// boxes go in at 9 floats each and the nodes come back at 8 floats each, in the same array
const arr = new Float32Array(2048 * 2048 * 4);
const bits = new Uint32Array(arr.buffer);
function readU32(file) {
  const b = fs.readFileSync(file);
  return new Uint32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength));
}
for (const c of JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))) {
  const aabb = readU32(path.join(dir, c.name + '.aabb.u32'));
  const work = readU32(path.join(dir, c.name + '.work.u32'));
  if (aabb.length !== 9 * c.tris || work.length !== c.work) throw new Error('bad input for ' + c.name);
  const used = Math.max(aabb.length, 8 * (2 * work.length - 1));
  bits.fill(0, 0, used);
  bits.set(aabb);
  build(work, arr);
  fs.writeFileSync(path.join(dir, c.name + '.nodes.u32'), Buffer.from(arr.buffer, 0, 8 * (2 * work.length - 1) * 4));
}
process.stdout.write('ok\n');
