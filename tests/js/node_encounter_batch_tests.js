'use strict';
/* Node-side test of the encounter watch inside batched block steps (setBlockBatchWatch), driven by
 * tests/test_encounter_batch_node.py.
 *   node tests/js/node_encounter_batch_tests.js <dir>  -> reads <dir>/bodies0.f32, vel0.f32, levels0.u8 and radii.f32 (the census
 *                                                         lattice: integer sites, v = 0), runs one frozen outer step (dt 2^-4, G 0,
 *                                                         eps2 0.25, maxLevel 3) of an f32 'hermite4' simulation with the watch and
 *                                                         setBlockBatchWatch({ smallMax: 256 }) on through the wrapper and writes
 *                                                         rho2.f32, partner.u32, time.f64, count.u32, stats.json and batch.json into
 *                                                         <dir> for the caller to compare with the brute force
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

const dir = process.argv[2];
const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32')), radii = loadF32(path.join(dir, 'radii.f32'));
const lev0 = new Uint8Array(fs.readFileSync(path.join(dir, 'levels0.u8')));
nb.load();
const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
check('addon_exports_setBlockBatchWatch', typeof addon.setBlockBatchWatch === 'function');
check('wrapper_has_setBlockBatchWatch', typeof nb.Simulation.prototype.setBlockBatchWatch === 'function');
const sim = new nb.Simulation({ dt: 1 / 16, G: 0.0, eps2: 0.25, integrator: 'hermite4' });
sim.init([b0, v0]);
sim.setBlockSteps({ maxLevel: 3, frozen: true });
check('refused_without_the_watch', code(function () { sim.setBlockBatchWatch({}); }) === 'NB_4');
sim.setEncounterWatch({ radii: radii });
check('unwatched_mode_still_refused', code(function () { sim.setBlockBatch({}); }) === 'NB_4');
check('depth_too_large', code(function () { sim.setBlockBatchWatch({ depth: 1025 }); }) === 'NB_1');
sim.setBlockBatchWatch({ depth: 4, smallMax: 256 });
check('enabled', sim.blockBatchStats().enabled === true);
sim.uploadLevels(lev0);
sim.simulate(1);
const rec = sim.downloadEncounters(), st = sim.encounterStats(), bst = sim.blockBatchStats();
check('stats', st.passes === 8 && st.hits > 0 && st.stopped === false, st);
check('passes_are_the_block_steps', st.passes === sim.blockStats().blockSteps && st.passes === bst.smallSteps + bst.hostSteps, bst);
save(path.join(dir, 'rho2.f32'), rec.rho2);
save(path.join(dir, 'partner.u32'), rec.partner);
save(path.join(dir, 'time.f64'), rec.time);
save(path.join(dir, 'count.u32'), rec.count);
fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
fs.writeFileSync(path.join(dir, 'batch.json'), JSON.stringify(bst));
sim.setBlockBatchWatch(null);
check('mode_off_watch_on', sim.blockBatchStats().enabled === false && code(function () { sim.encounterStats(); }) === null);
sim.setBlockBatchWatch();
sim.setEncounterWatch(null);
check('off_with_the_watch', sim.blockBatchStats().enabled === false && code(function () { sim.encounterStats(); }) === 'NB_4');
sim.destroy();
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
