'use strict';
/* Node-side tests of the guarded sums of the mixed pass (setPassGuard / passGuard), driven by tests/test_guard_node.py.
 *   node tests/js/node_guard_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_guard_tests.js gpu <dir>   -> reads <dir>/bodies0.f64 and vel0.f64, makes an f64 'hermite4' simulation with
 *                                                    eps2 1e-8, setPassPrecision('mixed') and setPassGuard(0.01), and writes the
 *                                                    accel / jerk .f64 of the start into <dir> for the caller to hold to the
 *                                                    barycentre bound
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
function loadF64(p) { const b = fs.readFileSync(p); return new Float64Array(b.buffer, b.byteOffset, b.length / 8).slice(); }
function saveF64(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_setPassGuard', typeof addon.setPassGuard === 'function');
  check('addon_exports_passGuard', typeof addon.passGuard === 'function');
  check('wrapper_has_setPassGuard', typeof nb.Simulation.prototype.setPassGuard === 'function');
  check('wrapper_has_passGuard', typeof nb.Simulation.prototype.passGuard === 'function');
  // refused by the wrapper before anything has been created: no device has been asked for
  check('a_string_throws_TypeError', throwsA(function () { new nb.Simulation({ integrator: 'hermite4', f64: true }).setPassGuard('near'); }, TypeError, /rNear/));
  check('setPassGuard_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4', f64: true }).setPassGuard(0.01); }, Error, /call init\(particles\) first/));
  check('setPassGuard_wants_a_handle', throwsA(function () { addon.setPassGuard({}, 0.01); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF64(path.join(dir, 'bodies0.f64')), v0 = loadF64(path.join(dir, 'vel0.f64'));
  const sim = new nb.Simulation({ dt: Math.pow(2, -7), G: 1.0, eps2: 1e-8, integrator: 'hermite4', f64: true });
  sim.init([b0, v0]);
  check('off_by_default', sim.passGuard() === 0);
  check('native_handle_is_a_state_error', code(function () { sim.setPassGuard(0.01); }) === 'NB_4');
  sim.setPassPrecision('mixed');
  check('negative_is_invalid', code(function () { sim.setPassGuard(-1); }) === 'NB_1');
  check('nan_is_invalid', code(function () { sim.setPassGuard(NaN); }) === 'NB_1');
  sim.setPassGuard(0.01);
  check('getter_returns_what_was_set', sim.passGuard() === 0.01);
  check('variant_is_hermite4_f64mxg', /^hermite4_f64mxg_/.test(sim.variant()), sim.variant());
  const s = sim.read(), j = sim.readJerk();
  saveF64(path.join(dir, 'accel.f64'), s.accel);
  saveF64(path.join(dir, 'jerk.f64'), j);
  sim.setPassPrecision('native');
  check('native_again_drops_the_guard', sim.passGuard() === 0 && /^hermite4_f64_/.test(sim.variant()), sim.variant());
  sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
