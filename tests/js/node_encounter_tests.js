'use strict';
/* Node-side test of the encounter watch (setEncounterWatch, encounterStats, downloadEncounters, uploadEncounters, resetEncounters),
 * driven by tests/test_encounter_node.py.
 *   node tests/js/node_encounter_tests.js <dir>   -> reads <dir>/bodies0.f32, vel0.f32, levels0.u8 and radii.f32 (the census lattice:
 *                                                    integer sites, v = 0), runs one frozen outer step (dt 2^-4, G 0, eps2 0.25,
 *                                                    maxLevel 3) of an f32 'hermite4' simulation with the watch on through the
 *                                                    wrapper and writes rho2.f32, partner.u32, time.f64, count.u32 and stats.json
 *                                                    into <dir> for the caller to compare with the brute force
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function loadF32(p) { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); }
function save(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function code(fn) { try { fn(); } catch (e) { return e.code || e.name; } return null; }
function same(a, b) { return a.length === b.length && a.every(function (x, i) { return Object.is(x, b[i]); }); }

const dir = process.argv[2];
const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32')), radii = loadF32(path.join(dir, 'radii.f32'));
const lev0 = new Uint8Array(fs.readFileSync(path.join(dir, 'levels0.u8')));
const n = lev0.length;
nb.load();
const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
for (const f of ['setEncounterWatch', 'encounterStats', 'downloadEncounters', 'uploadEncounters', 'resetEncounters']) {
  check('addon_exports_' + f, typeof addon[f] === 'function');
  check('wrapper_has_' + f, typeof nb.Simulation.prototype[f] === 'function');
}
const sim = new nb.Simulation({ dt: 1 / 16, G: 0.0, eps2: 0.25, integrator: 'hermite4' });
sim.init([b0, v0]);
check('needs_block_steps', code(function () { sim.setEncounterWatch({ radius: 4 }); }) === 'NB_4');
check('stats_need_the_watch', code(function () { sim.encounterStats(); }) === 'NB_4');
sim.setBlockSteps({ maxLevel: 3, frozen: true });
check('radius_and_radii_together', code(function () { sim.setEncounterWatch({ radius: 4, radii: radii }); }) === 'TypeError');
check('neither', code(function () { sim.setEncounterWatch({}); }) === 'TypeError');
check('negative_radius', code(function () { sim.setEncounterWatch({ radius: -1 }); }) === 'RangeError');
check('short_radii', code(function () { sim.setEncounterWatch({ radii: radii.slice(1) }); }) === 'RangeError');
check('negative_radii_element_is_invalid', code(function () { const r = radii.slice(); r[3] = -1; sim.setEncounterWatch({ radii: r }); }) === 'NB_1');
sim.setBlockBatch({});
check('refused_with_a_batched_mode', code(function () { sim.setEncounterWatch({ radius: 4 }); }) === 'NB_4');
sim.setBlockBatch(null);
sim.setEncounterWatch({ radii: radii });
check('batch_refused_while_on', code(function () { sim.setBlockBatch({}); }) === 'NB_4');
const fresh = sim.downloadEncounters();
check('records_start_empty', fresh.partner.every(function (p) { return p === 0xffffffff; }) && fresh.rho2.every(function (r) { return r === Infinity; }) &&
  fresh.count.every(function (c) { return c === 0; }));
sim.uploadLevels(lev0);
sim.simulate(1);
const rec = sim.downloadEncounters(), st = sim.encounterStats();
check('stats', st.passes === 8 && st.hits > 0 && st.stopped === false && st.stepsLeft === 0 && st.firstTime > 0 && st.firstTime <= 1, st);
check('hits_are_the_counts', st.hits === rec.count.reduce(function (a, c) { return a + c; }, 0), st);
save(path.join(dir, 'rho2.f32'), rec.rho2);
save(path.join(dir, 'partner.u32'), rec.partner);
save(path.join(dir, 'time.f64'), rec.time);
save(path.join(dir, 'count.u32'), rec.count);
fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
check('reset_true_zeroes_the_counters_only', (function () {
  sim.encounterStats(true); const z = sim.encounterStats(), r = sim.downloadEncounters();
  return z.hits === 0 && z.passes === 0 && z.firstTime === Infinity && same(r.partner, rec.partner) && same(r.count, rec.count);
})());
sim.resetEncounters();
check('reset_clears_the_records', same(sim.downloadEncounters().partner, fresh.partner) && same(sim.downloadEncounters().rho2, fresh.rho2));
sim.uploadEncounters(rec);
const back = sim.downloadEncounters();
check('upload_round_trip', same(back.rho2, rec.rho2) && same(back.partner, rec.partner) && same(back.time, rec.time) && same(back.count, rec.count));
check('short_upload', code(function () { sim.uploadEncounters({ rho2: rec.rho2.slice(1), partner: rec.partner, time: rec.time, count: rec.count }); }) === 'RangeError');
sim.setEncounterWatch({ radius: 4, stop: true });
sim.simulate(3);
const stopped = sim.encounterStats();
check('stop', stopped.stopped === true && stopped.stepsLeft === 2 && sim.blockStats().outerSteps === 2, stopped);
sim.setEncounterWatch(null);
check('switched_off', code(function () { sim.encounterStats(); }) === 'NB_4' && sim.blockStats().enabled === true);
sim.setEncounterWatch({ radius: 4 });
sim.setBlockSteps(null);
check('off_with_the_block_steps', code(function () { sim.downloadEncounters(); }) === 'NB_4');
sim.destroy();
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
