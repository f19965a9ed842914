'use strict';
/* Node-side test of batched block steps on mixed-precision handles (setBlockBatchMixed, blockBatchStats), driven by
 * tests/test_block_batch_mixed_node.py.
 *   node tests/js/node_block_batch_mixed_tests.js <dir>   -> reads <dir>/bodies0.f64, vel0.f64 and levels0.u8, runs one frozen outer
 *                                                            step (dt 2^-4, G 1, maxLevel 3, depth 8, smallMax 64) of an f64 'hermite4'
 *                                                            simulation with setPassPrecision('mixed') through the wrapper and writes
 *                                                            bodies / vel / accel / jerk .f64, levels.u8, stats.json and batch.json
 *                                                            into <dir> for the caller to compare with the Python binding
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function loadF64(p) { const b = fs.readFileSync(p); return new Float64Array(b.buffer, b.byteOffset, b.length / 8).slice(); }
function save(p, a) { fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
function code(fn) { try { fn(); } catch (e) { return e.code; } return null; }

const dir = process.argv[2];
const b0 = loadF64(path.join(dir, 'bodies0.f64')), v0 = loadF64(path.join(dir, 'vel0.f64'));
const lev0 = new Uint8Array(fs.readFileSync(path.join(dir, 'levels0.u8')));
nb.load();
const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
check('addon_exports_setBlockBatchMixed', typeof addon.setBlockBatchMixed === 'function');
check('wrapper_has_setBlockBatchMixed', typeof nb.Simulation.prototype.setBlockBatchMixed === 'function');
const sim = new nb.Simulation({ dt: 1 / 16, G: 1.0, integrator: 'hermite4', f64: true });
sim.init([b0, v0]);
check('needs_block_steps', code(function () { sim.setBlockBatchMixed({}); }) === 'NB_4');
sim.setBlockSteps({ maxLevel: 3, frozen: true });
check('a_native_handle_is_a_state_error', code(function () { sim.setBlockBatchMixed({}); }) === 'NB_4');
sim.setPassPrecision('mixed');
check('the_native_setter_stays_refused', code(function () { sim.setBlockBatch({}); }) === 'NB_4');
check('bad_depth_is_invalid', code(function () { sim.setBlockBatchMixed({ depth: 1025 }); }) === 'NB_1');
check('bad_small_max_is_invalid', code(function () { sim.setBlockBatchMixed({ smallMax: 1025 }); }) === 'NB_1');
check('off_before', sim.blockBatchStats().enabled === false);
sim.setBlockBatchMixed({ depth: 8, smallMax: 64 });
check('native_is_refused_while_on', code(function () { sim.setPassPrecision('native'); }) === 'NB_4' && sim.passPrecision() === 'mixed');
sim.uploadLevels(lev0);
sim.simulate(1);
const s = sim.read(), j = sim.readJerk(), lv = sim.readLevels(), st = sim.blockStats(), bs = sim.blockBatchStats();
check('stats_enabled', st.enabled === true && st.outerSteps === 1 && st.blockSteps === 8 && bs.enabled === true, [st, bs]);
check('counters_add_up', bs.smallSteps + bs.hostSteps === st.blockSteps && bs.slots === bs.smallSteps + bs.hostSteps + bs.idleSlots &&
  bs.hostSteps <= bs.hostWaits && bs.hostWaits <= bs.slots && bs.smallSteps > 0, bs);
for (const k of ['bodies', 'vel', 'accel']) save(path.join(dir, k + '.f64'), s[k]);
save(path.join(dir, 'jerk.f64'), j);
save(path.join(dir, 'levels.u8'), lv);
fs.writeFileSync(path.join(dir, 'stats.json'), JSON.stringify(st));
fs.writeFileSync(path.join(dir, 'batch.json'), JSON.stringify(bs));
check('reset_zeroes', (function () { sim.blockBatchStats(true); const z = sim.blockBatchStats(); return z.slots === 0 && z.hostWaits === 0 && z.smallSteps === 0; })());
sim.setBlockBatchMixed(null);
check('switched_off', sim.blockBatchStats().enabled === false && sim.blockStats().enabled === true && sim.passPrecision() === 'mixed');
sim.setBlockBatchMixed();
check('on_with_the_defaults', sim.blockBatchStats().enabled === true);
sim.setBlockSteps(null);
check('off_with_the_block_steps', sim.blockBatchStats().enabled === false);
sim.destroy();
console.log(JSON.stringify({ ok: ok, results: results }));
process.exit(ok ? 0 : 1);
