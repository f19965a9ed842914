'use strict';
/* Node-side tests of the 6th-order Hermite scheme (setHermiteOrder, hermiteOrder, readSnap, uploadDerivs6), driven by
 * tests/test_hermite6_node.py.
 *   node tests/js/node_hermite6_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_hermite6_tests.js gpu <dir>   -> reads <dir>/bodies0.f32 and vel0.f32 (N = 257), runs 5 steps (dt 2^-6, G 1) at
 *                                                       order 6 through the wrapper and writes bodies / vel / accel / jerk / snap /
 *                                                       crackle .f32 into <dir> for the caller to compare with the Python binding,
 *                                                       then checks a checkpoint round trip and the state errors
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throwsA(fn, ctor, re) { try { fn(); } catch (e) { return e instanceof ctor && re.test(String(e.message)); } return false; }
function code(fn) { try { fn(); } catch (e) { return e.code; } return null; }
function loadF32(p) { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); }
function saveF32(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function same(a, b) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  for (const k of ['setHermiteOrder', 'hermiteOrder', 'downloadSnap', 'uploadDerivs6']) check('addon_exports_' + k, typeof addon[k] === 'function');
  for (const k of ['setHermiteOrder', 'hermiteOrder', 'readSnap', 'uploadDerivs6']) check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
  check('readSnap_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).readSnap(); }, Error, /call init\(particles\) first/));
  check('setHermiteOrder_wants_a_handle', throwsA(function () { addon.setHermiteOrder({}, 6); }, Error, /./));
} else {
  const dir = process.argv[3];
  const H = 1 / 64;
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
  const sim = new nb.Simulation({ dt: H, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  check('order_defaults_to_4', sim.hermiteOrder() === 4);
  check('readSnap_at_order_4_is_a_state_error', code(function () { sim.readSnap(); }) === 'NB_4');
  check('order_5_is_invalid', code(function () { sim.setHermiteOrder(5); }) === 'NB_1');
  sim.setHermiteOrder(6);
  check('order_is_6', sim.hermiteOrder() === 6);
  check('variant_is_hermite6', /^hermite6_/.test(sim.variant()), sim.variant());
  check('crackle_is_zero_after_the_start', sim.readSnap().crackle.every(function (x) { return x === 0; }));
  check('setBlockSteps_at_order_6_is_a_state_error', code(function () { sim.setBlockSteps({ eta: 0.02 }); }) === 'NB_4');
  sim.simulate(5);
  const s = sim.read(), j = sim.readJerk(), sc = sim.readSnap();
  for (const k of ['bodies', 'vel', 'accel']) saveF32(path.join(dir, k + '.f32'), s[k]);
  saveF32(path.join(dir, 'jerk.f32'), j);
  saveF32(path.join(dir, 'snap.f32'), sc.snap);
  saveF32(path.join(dir, 'crackle.f32'), sc.crackle);
  check('crackle_is_not_zero_after_steps', sc.crackle.some(function (x) { return x !== 0; }));
  // checkpoint: a second simulation restored from the six arrays continues with the same bits
  const twin = new nb.Simulation({ dt: H, G: 1.0, integrator: 'hermite4' });
  twin.init([b0, v0]);
  twin.restore({ bodies: s.bodies, vel: s.vel });
  twin.setHermiteOrder(6);
  twin.uploadDerivs6(s.accel, j, sc.snap, sc.crackle);
  sim.simulate(3); twin.simulate(3);
  const a = sim.read(), b = twin.read(), as = sim.readSnap(), bs = twin.readSnap();
  check('restore_with_derivs6_continues_bit_identically', same(a.bodies, b.bodies) && same(a.vel, b.vel) && same(a.accel, b.accel) &&
    same(sim.readJerk(), twin.readJerk()) && same(as.snap, bs.snap) && same(as.crackle, bs.crackle));
  check('uploadDerivs_at_order_6_is_a_state_error', code(function () { twin.restore({ bodies: s.bodies, vel: s.vel, accel: s.accel, jerk: j }); }) === 'NB_4');
  const lf = new nb.Simulation({ dt: H, G: 1.0 });
  lf.init([b0, v0]);
  check('setHermiteOrder_on_leapfrog_is_a_state_error', code(function () { lf.setHermiteOrder(6); }) === 'NB_4');
  check('readSnap_on_leapfrog_is_a_state_error', code(function () { lf.readSnap(); }) === 'NB_4');
  lf.destroy(); twin.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
