'use strict';
/* Node-side tests of the neighbour scheme's radii that follow a target count and of its checkpoint (setNeighborAdapt,
 * neighborAdaptStats, downloadNeighborRadii, uploadNeighborScheme), driven by tests/test_ac_adapt_node.py.
 *   node tests/js/node_ac_adapt_tests.js cpu                  -> the surface, no GPU
 *   node tests/js/node_ac_adapt_tests.js gpu <dir> <json>     -> reads <dir>/bodies0.f32 and vel0.f32 and the parameters <json>
 *        ({dt, G, radius, cap, target, substeps, steps}); runs `steps` regular steps through the wrapper, checkpoints into a second
 *        simulation, runs `steps` more on both and compares every array; writes bodies / vel / accel / jerk / next .f32 and
 *        stats.json of the first `steps` into <dir> for the caller to compare with the Python binding
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
const CALLS = ['setNeighborAdapt', 'neighborAdaptStats', 'downloadNeighborRadii', 'uploadNeighborScheme'];

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  for (const k of CALLS) {
    check('addon_exports_' + k, typeof addon[k] === 'function');
    check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
    check(k + '_before_init_throws', throwsA(function () { new nb.Simulation({ integrator: 'hermite4' })[k]({ target: 6 }); }, Error, /call init\(particles\) first/));
  }
  check('setNeighborAdapt_wants_a_handle', throwsA(function () { addon.setNeighborAdapt({}, null); }, Error, /./));
  check('uploadNeighborScheme_wants_eight_arguments', throwsA(function () { addon.uploadNeighborScheme({}); }, TypeError, /uploadNeighborScheme\(handle/));
} else {
  const dir = process.argv[3], P = JSON.parse(process.argv[4]);
  const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32')), n = b0.length / 4;
  const opts = { dt: P.dt, G: P.G, integrator: 'hermite4' };
  const scheme = { radius: P.radius, cap: P.cap, substeps: P.substeps }, adapt = { target: P.target };
  const sim = new nb.Simulation(opts);
  sim.init([b0, v0]);
  check('adapt_without_the_scheme_is_a_state_error', (function () { try { sim.setNeighborAdapt(adapt); } catch (e) { return e.code === 'NB_4'; } return false; })());
  sim.setNeighborScheme({ radius: P.radius, cap: n - 1, substeps: P.substeps });      // (rows that hold whatever the start finds)
  check('stats_off', sim.neighborAdaptStats().enabled === false);
  const fixed = sim.downloadNeighborRadii();
  check('fixed_radii', fixed.built.length === n && same(fixed.built, fixed.next) && fixed.next[n - 1] === Math.fround(P.radius));
  sim.setNeighborScheme(scheme);
  check('target_above_half_the_cap_is_invalid', (function () { try { sim.setNeighborAdapt({ target: P.cap }); } catch (e) { return e.code === 'NB_1' && /target/.test(String(e.message)); } return false; })());
  sim.setNeighborAdapt(adapt);
  sim.simulate(P.steps);
  const s = sim.read(), j = sim.readJerk(), st = Object.assign(sim.neighborSchemeStats(), sim.neighborAdaptStats());
  const d = sim.downloadNeighborScheme(), r = sim.downloadNeighborRadii();
  check('stats', st.enabled === true && st.regularSteps === P.steps && st.builds === P.steps + 1 + st.rebuilds && st.rebuilds >= 1 && st.rowsShrunk >= st.rebuilds && st.overflowed === 0, st);
  for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
  save(path.join(dir, 'jerk.f32'), j);
  save(path.join(dir, 'next.f32'), r.next);
  fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
  // the checkpoint: a second simulation continues bit for bit
  const twin = new nb.Simulation(opts);
  twin.init([s.bodies, s.vel]);
  twin.setNeighborScheme(scheme).setNeighborAdapt(adapt);
  check('upload_without_radii_is_invalid', (function () { try { twin.uploadNeighborScheme(d, null); } catch (e) { return e.code === 'NB_1' && /radii/.test(String(e.message)); } return false; })());
  twin.uploadNeighborScheme(d, r.next);
  check('the_upload_counts_no_build', twin.neighborSchemeStats().builds === 0);
  sim.simulate(P.steps); twin.simulate(P.steps);
  const a = sim.read(), b = twin.read(), da = sim.downloadNeighborScheme(), db = twin.downloadNeighborScheme();
  check('restored_state', same(a.bodies, b.bodies) && same(a.vel, b.vel) && same(a.accel, b.accel) && same(sim.readJerk(), twin.readJerk()));
  check('restored_scheme', ['accelIrr', 'jerkIrr', 'accelReg', 'jerkReg', 'list', 'count'].every(function (k) { return same(da[k], db[k]); }));
  check('restored_radii', same(sim.downloadNeighborRadii().next, twin.downloadNeighborRadii().next) && !same(r.next, sim.downloadNeighborRadii().next));
  sim.setNeighborAdapt(null);
  check('switched_off', sim.neighborAdaptStats().enabled === false && sim.neighborSchemeStats().enabled === true);
  twin.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
