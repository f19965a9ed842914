'use strict';
/* Node-side tests of the sums and the neighbour rows from one pass (Simulation.prototype.splitLists, addon.splitLists,
 * neighborSchemeFused), driven by tests/test_split_lists_node.py.
 *   node tests/js/node_split_lists_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_split_lists_tests.js gpu <dir>   -> splitLists() on tests/golden/plummer1024_bodies0.f32 / _vel0.f32 at the bodies and
 *                                                          at 300 points; the raw outputs go to <dir>, where the Python test compares
 *                                                          them with the bytes of its own binding
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throws(fn, re) { try { fn(); } catch (e) { return re.test(String(e.message) + ' ' + String(e.code)); } return false; }
function dump(dir, name, a) { fs.writeFileSync(path.join(dir, name + '.bin'), Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function golden(name) {
  const raw = fs.readFileSync(path.join(ROOT, 'tests', 'golden', name));
  return new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
}
function dumpAll(dir, pre, o) {
  dump(dir, pre + 'accel_irr', o.accelIrr); dump(dir, pre + 'accel_reg', o.accelReg); dump(dir, pre + 'jerk_irr', o.jerkIrr);
  dump(dir, pre + 'jerk_reg', o.jerkReg); dump(dir, pre + 'list', o.list); dump(dir, pre + 'count', o.count);
}

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_splitLists', typeof addon.splitLists === 'function' && typeof addon.neighborSchemeFused === 'function');
  check('wrapper_has_splitLists', typeof nb.Simulation.prototype.splitLists === 'function' &&
        typeof nb.Simulation.prototype.neighborSchemeFused === 'function');
  check('splitLists_before_init_throws', throws(function () { new nb.Simulation().splitLists(null, { bodies: [0, 1], radius: 0.5 }); },
                                                 /call init\(particles\) first/));
  check('splitLists_wants_a_handle', throws(function () {
    addon.splitLists({}, null, null, 0, 1, null, 0.5, new Float32Array(4), null, null, null, 4, new Uint32Array(4), null);
  }, /./));
} else {
  const dir = process.argv[3];
  const b0 = golden('plummer1024_bodies0.f32'), v0 = golden('plummer1024_vel0.f32'), n = b0.length / 4, cap = 24;
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  const own = sim.splitLists(null, { bodies: [0, n], radius: 0.25, cap: cap });
  check('gpu_splitLists_shapes', own.accelIrr instanceof Float32Array && own.accelIrr.length === 4 * n && own.jerkReg.length === 4 * n &&
        own.list instanceof Uint32Array && own.list.length === n * cap && own.count instanceof Uint32Array && own.count.length === n && own.cap === cap);
  dumpAll(dir, 'own_', own);
  const m = 300, pts = new Float32Array(4 * m), pv = new Float32Array(4 * m), radii = new Float32Array(m);
  for (let r = 0; r < m; r++) {
    for (let c = 0; c < 3; c++) { pts[4 * r + c] = 0.5 * b0[4 * ((7 * r) % n) + c] + 0.125; pv[4 * r + c] = v0[4 * ((11 * r) % n) + c]; }
    radii[r] = 0.0625 * (r % 8);
  }
  const at = sim.splitLists(pts, { pointVel: pv, radii: radii, cap: cap });
  dump(dir, 'points', pts); dump(dir, 'point_vel', pv); dump(dir, 'radii', radii);
  dumpAll(dir, 'at_', at);
  const acc = sim.splitLists(null, { bodies: [0, n], radius: 0.25, jerk: false });
  check('gpu_splitLists_without_the_jerk', acc.jerkIrr === null && acc.jerkReg === null && acc.accelIrr.length === 4 * n && acc.list.length === 64 * n);
  check('gpu_splitLists_range_error', throws(function () { sim.splitLists(null, { bodies: [1000, 25], radius: 0.25 }); }, /first_body.*NB_1|NB_1/));
  check('gpu_splitLists_needs_a_radius', throws(function () { sim.splitLists(null, { bodies: [0, n] }); }, /radius.*NB_1|NB_1/));
  check('gpu_splitLists_needs_pointVel', throws(function () { sim.splitLists(pts, { radius: 0.25 }); }, /point_vel.*NB_1|NB_1/));
  check('gpu_splitLists_cap_range', throws(function () { sim.splitLists(null, { bodies: [0, n], radius: 0.25, cap: 4097 }); }, /cap/));
  check('gpu_no_scheme_is_not_fused', sim.neighborSchemeFused() === false);
  sim.setNeighborScheme({ radius: 0.1, substeps: 2, cap: 128 });
  check('gpu_scheme_is_fused', sim.neighborSchemeFused() === true);
  sim.destroy();
  const two = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4', flags: 4096 });
  two.init([b0, v0]);
  two.setNeighborScheme({ radius: 0.1, substeps: 2, cap: 128 });
  check('gpu_two_calls_flag_is_not_fused', two.neighborSchemeFused() === false);
  two.destroy();
  const leap = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  leap.init([b0, v0]);
  check('gpu_splitLists_jerk_needs_hermite', throws(function () { leap.splitLists(null, { bodies: [0, n], radius: 0.25, jerk: true }); }, /Hermite.*NB_4|NB_4/));
  const la = leap.splitLists(null, { bodies: [0, n], radius: 0.25 });
  check('gpu_splitLists_leapfrog_defaults_to_accel', la.jerkIrr === null && la.accelIrr.length === 4 * n && la.count.length === n);
  leap.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
