'use strict';
/* Node-side tests of the Ahmad-Cohen neighbour scheme (setNeighborScheme, neighborSchemeStats, downloadNeighborScheme), driven by
 * tests/test_ac_scheme_node.py.
 *   node tests/js/node_ac_scheme_tests.js cpu                  -> the surface, no GPU
 *   node tests/js/node_ac_scheme_tests.js gpu <dir> <json>     -> reads <dir>/bodies0.f32 and vel0.f32 and the parameters <json>
 *        ({dt, G, radius, cap, substeps, steps}); checks the start against splitForce, runs `steps` regular steps through the
 *        wrapper and writes bodies / vel / accel / jerk .f32 and stats.json into <dir> for the caller to compare; then provokes the
 *        overflow error with cap 1
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
function same(a, b) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  for (const k of ['setNeighborScheme', 'neighborSchemeStats', 'downloadNeighborScheme']) {
    check('addon_exports_' + k, typeof addon[k] === 'function');
    check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
  }
  check('setNeighborScheme_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' }).setNeighborScheme({ radius: 0.1 }); }, Error, /call init\(particles\) first/));
  check('setNeighborScheme_wants_a_handle', throwsA(function () { addon.setNeighborScheme({}, null); }, Error, /./));
} else {
  const dir = process.argv[3], P = JSON.parse(process.argv[4]);
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32')), n = b0.length / 4;
  const sim = new nb.Simulation({ dt: P.dt, G: P.G, integrator: 'hermite4' });
  sim.init([b0, v0]);
  const want = sim.splitForce(null, { bodies: [0, n], radius: P.radius });
  sim.setNeighborScheme({ radius: P.radius, cap: P.cap, substeps: P.substeps });
  const d = sim.downloadNeighborScheme();
  check('start_equals_splitForce', same(d.accelIrr, want.accelIrr) && same(d.jerkIrr, want.jerkIrr) && same(d.accelReg, want.accelReg) && same(d.jerkReg, want.jerkReg));
  check('list_shape', d.list.length === n * P.cap && d.count.length === n && d.cap === P.cap);
  sim.simulate(P.steps);
  const s = sim.read(), j = sim.readJerk(), st = sim.neighborSchemeStats();
  check('stats', st.enabled === true && st.regularSteps === P.steps && st.substeps === P.steps * P.substeps && st.builds === P.steps + 1 && st.overflowed === 0, st);
  for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
  save(path.join(dir, 'jerk.f32'), j);
  fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
  // an overflow is an ordinary error: NB_4 with the numbers, and setting the scheme again clears it
  sim.setNeighborScheme({ radius: 0.5, cap: 1 });
  let err = null;
  try { sim.simulate(1); } catch (e) { err = e; }
  check('overflow_is_a_state_error', err !== null && err.code === 'NB_4' && /rows hold more than cap members \(largest count \d+, cap 1\)/.test(String(err.message)), err && String(err.message));
  sim.setNeighborScheme(null);
  check('switched_off', sim.neighborSchemeStats().enabled === false);
  check('download_without_the_scheme_throws', throwsA(function () { sim.downloadNeighborScheme(); }, Error, /not switched on/));
  sim.simulate(1);
  const lf = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  lf.init([b0, v0]);
  check('setNeighborScheme_on_leapfrog_is_a_state_error', (function () { try { lf.setNeighborScheme({ radius: 0.1 }); } catch (e) { return e.code === 'NB_4'; } return false; })());
  lf.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
