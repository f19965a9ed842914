'use strict';
/* Node-side tests of the mixed-precision force+jerk pass (setPassPrecision / passPrecision), driven by tests/test_mixed_node.py.
 *   node tests/js/node_mixed_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_mixed_tests.js gpu <dir>   -> reads <dir>/bodies0.f64 and vel0.f64, runs 5 steps (dt 2^-7, G 1) of an f64
 *                                                    'hermite4' simulation with setPassPrecision('mixed') and writes bodies / vel /
 *                                                    accel / jerk .f64 into <dir> for the caller to compare with the Python binding
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throwsA(fn, ctor, re) { try { fn(); } catch (e) { return e instanceof ctor && re.test(String(e.message)); } return false; }
function loadF64(p) { const b = fs.readFileSync(p); return new Float64Array(b.buffer, b.byteOffset, b.length / 8).slice(); }
function saveF64(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_setPassPrecision', typeof addon.setPassPrecision === 'function');
  check('addon_exports_passPrecision', typeof addon.passPrecision === 'function');
  check('wrapper_has_setPassPrecision', typeof nb.Simulation.prototype.setPassPrecision === 'function');
  check('wrapper_has_passPrecision', typeof nb.Simulation.prototype.passPrecision === 'function');
  // refused by the wrapper before anything has been created: no device has been asked for
  check('unknown_mode_throws_RangeError', throwsA(function () { new nb.Simulation({ integrator: 'hermite4', f64: true }).setPassPrecision('double'); }, RangeError, /mode/));
  check('setPassPrecision_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4', f64: true }).setPassPrecision('mixed'); }, Error, /call init\(particles\) first/));
  check('setPassPrecision_wants_a_handle', throwsA(function () { addon.setPassPrecision({}, 1); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF64(path.join(dir, 'bodies0.f64')), v0 = loadF64(path.join(dir, 'vel0.f64'));
  const sim = new nb.Simulation({ dt: Math.pow(2, -7), G: 1.0, integrator: 'hermite4', f64: true });
  sim.init([b0, v0]);
  check('native_by_default', sim.passPrecision() === 'native');
  sim.setPassPrecision('mixed');
  check('mode_is_mixed', sim.passPrecision() === 'mixed');
  check('variant_is_hermite4_f64mx', /^hermite4_f64mx_/.test(sim.variant()), sim.variant());
  sim.simulate(5);
  const s = sim.read(), j = sim.readJerk();
  for (const k of ['bodies', 'vel', 'accel']) saveF64(path.join(dir, k + '.f64'), s[k]);
  saveF64(path.join(dir, 'jerk.f64'), j);
  sim.setPassPrecision(0);
  check('back_to_native', sim.passPrecision() === 'native' && /^hermite4_f64_/.test(sim.variant()), sim.variant());
  const f32 = new nb.Simulation({ dt: 1e-3, G: 1.0, integrator: 'hermite4' });
  f32.init([new Float32Array(b0), new Float32Array(v0)]);
  check('f32_handle_is_a_state_error', (function () { try { f32.setPassPrecision('mixed'); } catch (e) { return e.code === 'NB_4'; } return false; })());
  f32.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
