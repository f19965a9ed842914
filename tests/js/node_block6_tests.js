'use strict';
/* Node-side tests of block individual time steps on order-6 handles (setBlockSteps6), driven by tests/test_block6_node.py.
 *   node tests/js/node_block6_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_block6_tests.js gpu <dir>   -> reads <dir>/bodies0.f32, vel0.f32 and levels0.u8, runs one frozen outer step (dt 2^-4,
 *                                                     G 1, maxLevel 3) through the wrapper and writes bodies / vel / accel / jerk / snap /
 *                                                     crackle .f32, levels.u8 and stats.json into <dir> for the caller to compare with the
 *                                                     Python binding
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
  check('addon_exports_setBlockSteps6', typeof addon.setBlockSteps6 === 'function');
  check('wrapper_has_setBlockSteps6', typeof nb.Simulation.prototype.setBlockSteps6 === 'function');
  check('setBlockSteps6_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).setBlockSteps6({}); }, Error, /call init\(particles\) first/));
  check('setBlockSteps6_wants_a_handle', throwsA(function () { addon.setBlockSteps6({}, null); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
  const lev0 = new Uint8Array(fs.readFileSync(path.join(dir, 'levels0.u8')));
  const sim = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  check('setBlockSteps6_at_order_4_is_a_state_error', code(function () { sim.setBlockSteps6({ frozen: true }); }) === 'NB_4');
  sim.setHermiteOrder(6);
  check('dynamic_levels_on_f32_are_a_state_error', code(function () { sim.setBlockSteps6({ eta: 0.02 }); }) === 'NB_4');
  sim.setBlockSteps6({ maxLevel: 3, frozen: true });
  sim.uploadLevels(lev0);
  sim.simulate(1);
  const s = sim.read(), j = sim.readJerk(), sc = sim.readSnap(), lv = sim.readLevels(), st = sim.blockStats();
  check('stats_enabled', st.enabled === true && st.outerSteps === 1 && st.blockSteps === 8, st);
  for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
  save(path.join(dir, 'jerk.f32'), j);
  save(path.join(dir, 'snap.f32'), sc.snap);
  save(path.join(dir, 'crackle.f32'), sc.crackle);
  save(path.join(dir, 'levels.u8'), lv);
  fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
  sim.setBlockSteps6(null);
  check('switched_off', sim.blockStats().enabled === false && sim.hermiteOrder() === 6);
  sim.simulate(1);
  const lf = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  lf.init([b0, v0]);
  check('setBlockSteps6_on_leapfrog_is_a_state_error', code(function () { lf.setBlockSteps6({}); }) === 'NB_4');
  lf.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
