'use strict';
/* Node-side tests of the start mode of order-6 handles (setStart6, start6), driven by tests/test_start6_node.py.
 *   node tests/js/node_start6_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_start6_tests.js gpu <dir>   -> reads <dir>/bodies0.f32 and vel0.f32, makes the start of an order-6 simulation
 *                                                     (dt 2^-6, G 1) in both modes through the wrapper and writes snap / crackle .f32
 *                                                     into <dir> for the caller to compare with the Python binding
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
function save(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_setStart6', typeof addon.setStart6 === 'function' && typeof addon.start6 === 'function');
  const d = Object.getOwnPropertyDescriptor(nb.Simulation.prototype, 'start6');
  check('wrapper_has_setStart6', typeof nb.Simulation.prototype.setStart6 === 'function' && d && typeof d.get === 'function');
  check('setStart6_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).setStart6(1); }, Error, /call init\(particles\) first/));
  check('setStart6_wants_a_handle', throwsA(function () { addon.setStart6({}, 1); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
  const sim = new nb.Simulation({ dt: 1 / 64, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  check('setStart6_at_order_4_is_a_state_error', code(function () { sim.setStart6(1); }) === 'NB_4');
  sim.setHermiteOrder(6);
  check('default_mode_is_0', sim.start6 === 0);
  const zero = sim.readSnap();
  check('default_crackle_is_0', zero.crackle.every(function (x) { return x === 0; }));
  check('bad_mode_is_an_argument_error', code(function () { sim.setStart6(2); }) === 'NB_1');
  check('setter_returns_the_simulation', sim.setStart6(1) === sim && sim.start6 === 1);
  const sc = sim.readSnap();
  check('snap_is_shared', Buffer.compare(Buffer.from(sc.snap.buffer), Buffer.from(zero.snap.buffer)) === 0);
  save(path.join(dir, 'snap.f32'), sc.snap);
  save(path.join(dir, 'crackle.f32'), sc.crackle);
  sim.setHermiteOrder(4); sim.setHermiteOrder(6);
  check('order_4_returns_the_mode_to_0', sim.start6 === 0);
  const lf = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  lf.init([b0, v0]);
  check('setStart6_on_leapfrog_is_a_state_error', code(function () { lf.setStart6(1); }) === 'NB_4');
  lf.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
