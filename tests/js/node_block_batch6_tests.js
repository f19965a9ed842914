'use strict';
/* Node-side test of batched block steps on order-6 handles (setBlockBatch6, blockBatchStats), driven by tests/test_block_batch6_node.py.
 *   node tests/js/node_block_batch6_tests.js <dir>   -> reads <dir>/bodies0.f32, vel0.f32 and levels0.u8, runs one frozen outer step
 *                                                       (dt 2^-4, G 1, maxLevel 3, depth 8, smallMax 64) through the wrapper and writes
 *                                                       bodies / vel / accel / jerk / snap / crackle .f32, levels.u8, stats.json and
 *                                                       batch.json into <dir> for the caller to compare with the Python binding
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
function code(fn) { try { fn(); } catch (e) { return e.code; } return null; }

const dir = process.argv[2];
const b0 = loadF32(path.join(dir, 'bodies0.f32')), v0 = loadF32(path.join(dir, 'vel0.f32'));
const lev0 = new Uint8Array(fs.readFileSync(path.join(dir, 'levels0.u8')));
nb.load();
const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
check('addon_exports_setBlockBatch6', typeof addon.setBlockBatch6 === 'function');
check('wrapper_has_setBlockBatch6', typeof nb.Simulation.prototype.setBlockBatch6 === 'function');
const sim = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4' });
sim.init([b0, v0]);
check('order_4_is_a_state_error', code(function () { sim.setBlockBatch6({}); }) === 'NB_4');
sim.setHermiteOrder(6);
check('needs_block_steps6', code(function () { sim.setBlockBatch6({}); }) === 'NB_4');
sim.setBlockSteps6({ maxLevel: 3, frozen: true });
check('the_order_4_setter_stays_refused', code(function () { sim.setBlockBatch({}); }) === 'NB_4');
check('bad_depth_is_invalid', code(function () { sim.setBlockBatch6({ depth: 1025 }); }) === 'NB_1');
check('bad_small_max_is_invalid', code(function () { sim.setBlockBatch6({ smallMax: 1025 }); }) === 'NB_1');
check('off_before', sim.blockBatchStats().enabled === false);
sim.setBlockBatch6({ depth: 8, smallMax: 64 });
sim.uploadLevels(lev0);
sim.simulate(1);
const s = sim.read(), j = sim.readJerk(), sc = sim.readSnap(), lv = sim.readLevels(), st = sim.blockStats(), bs = sim.blockBatchStats();
check('stats_enabled', st.enabled === true && st.outerSteps === 1 && st.blockSteps === 8 && bs.enabled === true, [st, bs]);
check('counters_add_up', bs.smallSteps + bs.hostSteps === st.blockSteps && bs.slots === bs.smallSteps + bs.hostSteps + bs.idleSlots &&
  bs.hostSteps <= bs.hostWaits && bs.hostWaits <= bs.slots && bs.smallSteps > 0, bs);
for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
save(path.join(dir, 'jerk.f32'), j);
save(path.join(dir, 'snap.f32'), sc.snap);
save(path.join(dir, 'crackle.f32'), sc.crackle);
save(path.join(dir, 'levels.u8'), lv);
fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
fs.writeFileSync(path.join(dir, 'batch.json'), JSON.stringify(bs));
check('reset_zeroes', (function () { sim.blockBatchStats(true); const z = sim.blockBatchStats(); return z.slots === 0 && z.hostWaits === 0 && z.smallSteps === 0; })());
sim.setBlockBatch6(null);
check('switched_off', sim.blockBatchStats().enabled === false && sim.blockStats().enabled === true);
sim.setBlockBatch6();
check('on_with_the_defaults', sim.blockBatchStats().enabled === true);
sim.setBlockSteps6(null);
check('off_with_the_block_steps', sim.blockBatchStats().enabled === false && sim.hermiteOrder() === 6);
sim.destroy();
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
