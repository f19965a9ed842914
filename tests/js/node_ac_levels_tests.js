'use strict';
/* Node-side tests of the neighbour scheme's block individual irregular steps (setNeighborLevels, neighborLevelStats,
 * downloadNeighborLevels, uploadNeighborLevels), driven by tests/test_ac_levels_node.py.
 *   node tests/js/node_ac_levels_tests.js cpu                  -> the surface, no GPU
 *   node tests/js/node_ac_levels_tests.js gpu <dir> <json>     -> reads <dir>/bodies0.f32 and vel0.f32 and the parameters <json>
 *        ({dt, G, radius, cap, substeps, minLevel, eta, steps}); runs `steps` regular steps with dynamic levels through the wrapper,
 *        checkpoints into a second simulation, runs `steps` more on both and compares every array; writes bodies / vel / accel /
 *        jerk .f32, levels.u8 and stats.json of the first `steps` into <dir> for the caller to compare with the Python binding
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throwsA(fn, ctor, re) { try { fn(); } catch (e) { return e instanceof ctor && re.test(String(e.message)); } return false; }
function code(fn) { try { fn(); } catch (e) { return e.code + ' ' + String(e.message); } return 'no error'; }
function loadF32(p) { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); }
function save(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function same(a, b) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }
const CALLS = ['setNeighborLevels', 'neighborLevelStats', 'downloadNeighborLevels', 'uploadNeighborLevels'];

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  for (const k of CALLS) {
    check('addon_exports_' + k, typeof addon[k] === 'function');
    check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
    check(k + '_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' })[k]({ minLevel: 1 }); }, Error, /call init\(particles\) first/));
  }
  check('setNeighborLevels_wants_a_handle', throwsA(function () { addon.setNeighborLevels({}, null); }, Error, /./));
  check('setNeighborLevels_wants_two_arguments', throwsA(function () { addon.setNeighborLevels({}); }, TypeError, /setNeighborLevels\(handle/));
  check('uploadNeighborLevels_wants_two_arguments', throwsA(function () { addon.uploadNeighborLevels({}); }, TypeError, /uploadNeighborLevels\(handle/));
} else {
  const dir = process.argv[3], P = JSON.parse(process.argv[4]);
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32')), n = b0.length / 4;
  const opts = { dt: P.dt, G: P.G, integrator: 'hermite4' };
  const scheme = { radius: P.radius, cap: P.cap, substeps: P.substeps }, levels = { minLevel: P.minLevel, eta: P.eta };
  const L = Math.round(Math.log2(P.substeps));
  const sim = new nb.Simulation(opts);
  sim.init([b0, v0]);
  check('levels_without_the_scheme_are_a_state_error', /^NB_4 /.test(code(function () { sim.setNeighborLevels(levels); })));
  sim.setNeighborScheme(scheme);
  check('stats_off', sim.neighborLevelStats().enabled === false);
  check('min_level_above_L_is_invalid', /^NB_1 .*min_level/.test(code(function () { sim.setNeighborLevels({ minLevel: L + 1 }); })));
  check('download_without_levels_is_a_state_error', /^NB_4 /.test(code(function () { sim.downloadNeighborLevels(); })));
  sim.setNeighborLevels(levels);
  const first = sim.downloadNeighborLevels();
  check('start_levels', first.length === n && first.every(function (l) { return l >= P.minLevel && l <= L; }) && new Set(first).size > 1);
  sim.simulate(P.steps);
  const s = sim.read(), j = sim.readJerk(), st = sim.neighborLevelStats(), lev = sim.downloadNeighborLevels();
  const d = sim.downloadNeighborScheme();
  check('stats', st.enabled === true && st.regularSteps === P.steps && st.ticks === P.steps * P.substeps && st.blockSteps > 0 && st.blockSteps <= st.ticks &&
    st.bodySteps >= P.steps * n * Math.pow(2, P.minLevel) && st.bodySteps < P.steps * n * P.substeps && st.entries > 0 && st.finestLevel <= L, st);
  check('scheme_substeps_keep_counting', sim.neighborSchemeStats().substeps === P.steps * P.substeps);
  for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
  save(path.join(dir, 'jerk.f32'), j);
  save(path.join(dir, 'levels.u8'), lev);
  fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
  // the checkpoint: a second simulation continues bit for bit
  const twin = new nb.Simulation(opts);
  twin.init([s.bodies, s.vel]);
  twin.setNeighborScheme(scheme).setNeighborLevels(levels);
  check('upload_before_the_scheme_is_current_is_a_state_error', /^NB_4 .*not current/.test(code(function () { twin.uploadNeighborLevels(lev); })));
  twin.uploadNeighborScheme(d, null);
  const bad = Uint8Array.from(lev); bad[3] = L + 1;
  check('a_level_out_of_range_is_invalid', /^NB_1 .*levels\[3\]/.test(code(function () { twin.uploadNeighborLevels(bad); })));
  twin.uploadNeighborLevels(lev);
  check('uploaded_levels', same(twin.downloadNeighborLevels(), lev));
  sim.simulate(P.steps); twin.simulate(P.steps);
  const a = sim.read(), b = twin.read(), da = sim.downloadNeighborScheme(), db = twin.downloadNeighborScheme();
  check('restored_state', same(a.bodies, b.bodies) && same(a.vel, b.vel) && same(a.accel, b.accel) && same(sim.readJerk(), twin.readJerk()));
  check('restored_scheme', ['accelIrr', 'jerkIrr', 'accelReg', 'jerkReg', 'list', 'count'].every(function (k) { return same(da[k], db[k]); }));
  check('restored_levels', same(sim.downloadNeighborLevels(), twin.downloadNeighborLevels()));
  sim.setNeighborLevels(null);
  check('switched_off', sim.neighborLevelStats().enabled === false && sim.neighborSchemeStats().enabled === true);
  twin.setNeighborScheme(scheme);
  check('the_scheme_switches_levels_off', twin.neighborLevelStats().enabled === false);
  twin.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
