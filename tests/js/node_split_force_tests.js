'use strict';
/* Node-side tests of the regular / irregular force+jerk pass (Simulation.prototype.splitForce, addon.splitForce), driven by
 * tests/test_split_force_node.py.
 *   node tests/js/node_split_force_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_split_force_tests.js gpu <dir>   -> splitForce() on tests/golden/plummer1024_bodies0.f32 / _vel0.f32 at the bodies and
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
function same(a, b) { return a.length === b.length && a.every(function (x, t) { return Object.is(x, b[t]); }); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_splitForce', typeof addon.splitForce === 'function');
  check('wrapper_has_splitForce', typeof nb.Simulation.prototype.splitForce === 'function');
  check('splitForce_before_init_throws', throws(function () { new nb.Simulation().splitForce(null, { bodies: [0, 1], radius: 0.5 }); },
                                                 /call init\(particles\) first/));
  check('splitForce_wants_a_handle', throws(function () { addon.splitForce({}, null, null, 0, 1, null, 0.5, new Float32Array(4), null, null, null); }, /./));
} else {
  const dir = process.argv[3];
  const b0 = golden('plummer1024_bodies0.f32'), v0 = golden('plummer1024_vel0.f32'), n = b0.length / 4;
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  const own = sim.splitForce(null, { bodies: [0, n], radius: 0.25 });
  check('gpu_splitForce_shapes', own.accelIrr instanceof Float32Array && own.accelIrr.length === 4 * n && own.accelReg.length === 4 * n &&
        own.jerkIrr.length === 4 * n && own.jerkReg.length === 4 * n);
  dump(dir, 'own_accel_irr', own.accelIrr); dump(dir, 'own_accel_reg', own.accelReg);
  dump(dir, 'own_jerk_irr', own.jerkIrr); dump(dir, 'own_jerk_reg', own.jerkReg);
  const m = 300, pts = new Float32Array(4 * m), pv = new Float32Array(4 * m), radii = new Float32Array(m);
  for (let r = 0; r < m; r++) {
    for (let c = 0; c < 3; c++) { pts[4 * r + c] = 0.5 * b0[4 * ((7 * r) % n) + c] + 0.125; pv[4 * r + c] = v0[4 * ((11 * r) % n) + c]; }
    radii[r] = 0.0625 * (r % 8);
  }
  const at = sim.splitForce(pts, { pointVel: pv, radii: radii });
  dump(dir, 'points', pts); dump(dir, 'point_vel', pv); dump(dir, 'radii', radii);
  dump(dir, 'at_accel_irr', at.accelIrr); dump(dir, 'at_accel_reg', at.accelReg); dump(dir, 'at_jerk_irr', at.jerkIrr); dump(dir, 'at_jerk_reg', at.jerkReg);
  const acc = sim.splitForce(null, { bodies: [0, n], radius: 0.25, jerk: false });
  check('gpu_splitForce_without_the_jerk', acc.jerkIrr === null && acc.jerkReg === null && acc.accelIrr.length === 4 * n);
  check('gpu_splitForce_range_error', throws(function () { sim.splitForce(null, { bodies: [1000, 25], radius: 0.25 }); }, /first_body.*NB_1|NB_1/));
  check('gpu_splitForce_needs_a_radius', throws(function () { sim.splitForce(null, { bodies: [0, n] }); }, /radius.*NB_1|NB_1/));
  check('gpu_splitForce_needs_pointVel', throws(function () { sim.splitForce(pts, { radius: 0.25 }); }, /point_vel.*NB_1|NB_1/));
  sim.destroy();
  const leap = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  leap.init([b0, v0]);
  check('gpu_splitForce_jerk_needs_hermite', throws(function () { leap.splitForce(null, { bodies: [0, n], radius: 0.25, jerk: true }); }, /Hermite.*NB_4|NB_4/));
  const la = leap.splitForce(null, { bodies: [0, n], radius: 0.25 });
  check('gpu_splitForce_leapfrog_defaults_to_accel', la.jerkIrr === null && la.jerkReg === null && same(la.accelIrr, acc.accelIrr) && same(la.accelReg, acc.accelReg));
  leap.destroy();
}
console.log(JSON.stringify({ ok: ok, mode: mode, results: results }));
process.exit(ok ? 0 : 1);
