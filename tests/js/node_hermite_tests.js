'use strict';
/* Node-side tests of the Hermite integrator ({integrator: 'hermite4'}, readJerk, restore with {accel, jerk}), driven by
 * tests/test_hermite_node.py.
 *   node tests/js/node_hermite_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_hermite_tests.js gpu <dir>   -> reads <dir>/bodies0.f32 and vel0.f32, runs 5 steps (dt 1e-3, G 1) through the
 *                                                      wrapper and writes bodies / vel / accel / jerk .f32 into <dir> for the caller
 *                                                      to compare with the Python binding, then checks a checkpoint round trip
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throwsA(fn, ctor, re) { try { fn(); } catch (e) { return e instanceof ctor && re.test(String(e.message)); } return false; }
function loadF32(p) { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); }
function saveF32(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function same(a, b) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_downloadJerk', typeof addon.downloadJerk === 'function');
  check('addon_exports_uploadDerivs', typeof addon.uploadDerivs === 'function');
  check('wrapper_has_readJerk', typeof nb.Simulation.prototype.readJerk === 'function');
  check('integrator_defaults_to_leapfrog', new nb.Simulation().integrator === 'leapfrog');
  check('hermite4_is_accepted', new nb.Simulation({ integrator: 'hermite4' }).integrator === 'hermite4');
  // refused by the wrapper's constructor: nothing has been created, no device has been asked for
  check('unknown_integrator_throws_RangeError', throwsA(function () { new nb.Simulation({ integrator: 'rk4' }); }, RangeError, /integrator/));
  check('readJerk_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).readJerk(); }, Error, /call init\(particles\) first/));
  check('downloadJerk_wants_a_handle', throwsA(function () { addon.downloadJerk({}, new Float32Array(4)); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  check('variant_is_hermite4', /^hermite4_/.test(sim.variant()), sim.variant());
  sim.simulate(5);
  const s = sim.read(), j = sim.readJerk();
  for (const k of ['bodies', 'vel', 'accel']) saveF32(path.join(dir, k + '.f32'), s[k]);
  saveF32(path.join(dir, 'jerk.f32'), j);
  // checkpoint: a second simulation restored from {bodies, vel, accel, jerk} continues with the same bits
  const twin = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  twin.init([b0, v0]);
  twin.restore({ bodies: s.bodies, vel: s.vel, accel: s.accel, jerk: j });
  sim.simulate(3); twin.simulate(3);
  const a = sim.read(), b = twin.read();
  check('restore_with_derivs_continues_bit_identically', same(a.bodies, b.bodies) && same(a.vel, b.vel) && same(a.accel, b.accel) && same(sim.readJerk(), twin.readJerk()));
  const lf = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  lf.init([b0, v0]);
  check('readJerk_on_leapfrog_is_a_state_error', (function () { try { lf.readJerk(); } catch (e) { return e.code === 'NB_4'; } return false; })());
  lf.destroy(); twin.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
