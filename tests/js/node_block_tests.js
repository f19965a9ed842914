'use strict';
/* Node-side tests of block individual time steps (setBlockSteps, blockStats, readLevels, uploadLevels), driven by
 * tests/test_block_cpu.py and tests/test_block_node.py.
 *   node tests/js/node_block_tests.js cpu         -> the surface, no GPU
 *   node tests/js/node_block_tests.js gpu <dir>   -> reads <dir>/bodies0.f32 and vel0.f32, runs one outer step (dt 2^-4, G 1, eta 0.02,
 *                                                    maxLevel 12) through the wrapper and writes bodies / vel / accel / jerk .f32,
 *                                                    levels.u8 and stats.json into <dir> for the caller to compare with the Python binding
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
function save(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  for (const k of ['setBlockSteps', 'blockStats', 'downloadLevels', 'uploadLevels']) check('addon_exports_' + k, typeof addon[k] === 'function');
  for (const k of ['setBlockSteps', 'blockStats', 'readLevels', 'uploadLevels']) check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
  check('setBlockSteps_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).setBlockSteps({}); }, Error, /call init\(particles\) first/));
  check('setBlockSteps_wants_a_handle', throwsA(function () { addon.setBlockSteps({}, null); }, Error, /./));
} else {
  const dir = process.argv[3];
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
  const sim = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4' });
  sim.init([b0, v0]);
  sim.setBlockSteps({ eta: 0.02, maxLevel: 12 });
  sim.simulate(1);
  const s = sim.read(), j = sim.readJerk(), lv = sim.readLevels(), st = sim.blockStats();
  check('stats_enabled', st.enabled === true && st.outerSteps === 1 && st.blockSteps > 1, st);
  for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
  save(path.join(dir, 'jerk.f32'), j);
  save(path.join(dir, 'levels.u8'), lv);
  fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
  // checkpoint from JavaScript: the twin continues with the same bits
  const twin = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4' });
  twin.init([b0, v0]);
  twin.restore({ bodies: s.bodies, vel: s.vel, accel: s.accel, jerk: j });
  twin.setBlockSteps({ eta: 0.02, maxLevel: 12 });
  twin.uploadLevels(lv);
  sim.simulate(1); twin.simulate(1);
  const a = sim.read(), b = twin.read();
  check('checkpoint_with_levels_continues_bit_identically',
    Buffer.from(a.bodies.buffer).equals(Buffer.from(b.bodies.buffer)) && Buffer.from(a.vel.buffer).equals(Buffer.from(b.vel.buffer)) &&
    Buffer.from(sim.readLevels().buffer).equals(Buffer.from(twin.readLevels().buffer)));
  sim.setBlockSteps(null);
  check('switched_off', sim.blockStats().enabled === false);
  const lf = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  lf.init([b0, v0]);
  check('setBlockSteps_on_leapfrog_is_a_state_error', (function () { try { lf.setBlockSteps({}); } catch (e) { return e.code === 'NB_4'; } return false; })());
  lf.destroy(); twin.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
