'use strict';
/* Node-side tests of the forces over neighbour rows (Simulation.prototype.listForce, addon.listForce), driven by
 * tests/test_list_force_node.py.
 *   node tests/js/node_list_force_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_list_force_tests.js gpu <dir>   -> listForce() on tests/golden/plummer1024_bodies0.f32 / _vel0.f32 with the rows of
 *                                                         neighborLists() and knn(); the raw outputs go to <dir>, where the Python
 *                                                         test compares them with the bytes of its own binding
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

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_listForce', typeof addon.listForce === 'function');
  check('wrapper_has_listForce', typeof nb.Simulation.prototype.listForce === 'function');
  check('listForce_before_init_throws', throws(function () { new nb.Simulation().listForce(new Uint32Array(8), { cap: 8, bodies: [0, 1] }); },
                                                /call init\(particles\) first/));
  check('listForce_wants_a_handle', throws(function () { addon.listForce({}, new Uint32Array(8), 8, null, null, 0, null, new Float32Array(4), null, null); }, /./));
} else {
  const dir = process.argv[3];
  const b0 = golden('plummer1024_bodies0.f32'), v0 = golden('plummer1024_vel0.f32'), n = b0.length / 4;
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  const cap = 32, nl = sim.neighborLists(null, { bodies: [0, n], radius: 0.25, cap: cap });
  const own = sim.listForce(nl.list, { cap: cap, bodies: [0, n], count: nl.count, jerk: true, phi: true });
  check('gpu_listForce_shapes', own.accel instanceof Float32Array && own.accel.length === 4 * n && own.jerk.length === 4 * n && own.phi.length === n);
  dump(dir, 'lists', nl.list); dump(dir, 'count', nl.count);
  dump(dir, 'own_accel', own.accel); dump(dir, 'own_jerk', own.jerk); dump(dir, 'own_phi', own.phi);
  const def = sim.listForce(nl.list, { cap: cap, bodies: [0, n] });
  check('gpu_listForce_defaults_to_accel', def.jerk === null && def.phi === null && def.accel.every(function (x, t) { return x === own.accel[t]; }));
  const m = 300, pts = new Float32Array(4 * m), pv = new Float32Array(4 * m);
  for (let r = 0; r < m; r++) for (let c = 0; c < 3; c++) { pts[4 * r + c] = 0.5 * b0[4 * ((7 * r) % n) + c] + 0.125; pv[4 * r + c] = v0[4 * ((11 * r) % n) + c]; }
  const kn = sim.knn(pts, { k: 16, dist2: false });
  const at = sim.listForce(kn.index, { cap: 16, points: pts, pointVel: pv, jerk: true, phi: true });
  dump(dir, 'points', pts); dump(dir, 'point_vel', pv); dump(dir, 'knn_index', kn.index);
  dump(dir, 'at_accel', at.accel); dump(dir, 'at_jerk', at.jerk); dump(dir, 'at_phi', at.phi);
  check('gpu_listForce_range_error', throws(function () { sim.listForce(nl.list.subarray(0, 25 * cap), { cap: cap, bodies: [1000, 25] }); }, /first_body.*NB_1|NB_1/));
  check('gpu_listForce_cap_range', throws(function () { sim.listForce(nl.list, { cap: 0, bodies: [0, n] }); }, /options\.cap/) &&
        throws(function () { sim.listForce(nl.list, { bodies: [0, n] }); }, /options\.cap/));
  check('gpu_listForce_needs_pointVel', throws(function () { sim.listForce(kn.index, { cap: 16, points: pts, jerk: true }); }, /point_vel.*NB_1|NB_1/));
  sim.destroy();
  const leap = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  leap.init([b0, v0]);
  check('gpu_listForce_jerk_needs_hermite', throws(function () { leap.listForce(nl.list, { cap: cap, bodies: [0, n], jerk: true }); }, /Hermite.*NB_4|NB_4/));
  const la = leap.listForce(nl.list, { cap: cap, bodies: [0, n], phi: true });
  check('gpu_listForce_leapfrog_has_the_same_bits', la.accel.every(function (x, t) { return x === own.accel[t]; }) && la.phi.every(function (x, t) { return x === own.phi[t]; }));
  leap.destroy();
}
console.log(JSON.stringify({ ok: ok, mode: mode, results: results }));
process.exit(ok ? 0 : 1);
