'use strict';
/* Node-side test of batched block steps (setBlockBatch, blockBatchStats), driven by tests/test_block_batch_node.py.
 *   node tests/js/node_block_batch_tests.js <dir>   -> reads <dir>/bodies0.f32 and vel0.f32, runs two outer steps (dt 2^-4, G 1, eta 0.02,
 *                                                      maxLevel 12, depth 8, smallMax 64) through the wrapper and writes bodies / vel /
 *                                                      accel / jerk .f32, levels.u8, stats.json and batch.json into <dir> for the caller
 *                                                      to compare with the Python binding
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
nb.load();
const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
for (const k of ['setBlockBatch', 'blockBatchStats']) {
  check('addon_exports_' + k, typeof addon[k] === 'function');
  check('wrapper_has_' + k, typeof nb.Simulation.prototype[k] === 'function');
}
const sim = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4' });
sim.init([b0, v0]);
check('needs_block_steps', code(function () { sim.setBlockBatch({}); }) === 'NB_4');
sim.setBlockSteps({ eta: 0.02, maxLevel: 12 });
check('bad_depth_is_invalid', code(function () { sim.setBlockBatch({ depth: 1025 }); }) === 'NB_1');
check('bad_small_max_is_invalid', code(function () { sim.setBlockBatch({ smallMax: 1025 }); }) === 'NB_1');
check('off_before', sim.blockBatchStats().enabled === false);
sim.setBlockBatch({ depth: 8, smallMax: 64 });
sim.simulate(2);
const s = sim.read(), j = sim.readJerk(), lv = sim.readLevels(), st = sim.blockStats(), bs = sim.blockBatchStats();
check('stats_enabled', st.enabled === true && st.outerSteps === 2 && bs.enabled === true, [st, bs]);
check('counters_add_up', bs.smallSteps + bs.hostSteps === st.blockSteps && bs.slots === bs.smallSteps + bs.hostSteps + bs.idleSlots &&
  bs.hostSteps <= bs.hostWaits && bs.hostWaits <= bs.slots && bs.smallSteps > 0, bs);
for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f32'), s[k]);
save(path.join(dir, 'jerk.f32'), j);
save(path.join(dir, 'levels.u8'), lv);
fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
fs.writeFileSync(path.join(dir, 'batch.json'), JSON.stringify(bs));
check('reset_zeroes', (function () { sim.blockBatchStats(true); const z = sim.blockBatchStats(); return z.slots === 0 && z.hostWaits === 0 && z.smallSteps === 0; })());
sim.setBlockBatch(null);
check('switched_off', sim.blockBatchStats().enabled === false && sim.blockStats().enabled === true);
sim.setBlockBatch();
sim.setBlockSteps(null);
check('off_with_the_block_steps', sim.blockBatchStats().enabled === false);
sim.destroy();
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
