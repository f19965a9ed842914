'use strict';
/* Node-side tests of the neighbour lists (Simulation.prototype.neighborLists / addon.neighborLists), driven by
 * tests/test_neighbor_lists_node.py.
 *   node tests/js/node_neighbor_lists_tests.js cpu   -> the surface, no GPU
 *   node tests/js/node_neighbor_lists_tests.js gpu   -> neighborLists() on an integer lattice against a double loop in JavaScript
 * Prints one JSON object; exit code 0 iff every check passed. */
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throws(fn, re) { try { fn(); } catch (e) { return re.test(String(e.message) + ' ' + String(e.code)); } return false; }

// exact on a lattice: the members in ascending j, the first cap of them, 0xffffffff behind; skip0 >= 0: point k leaves body skip0 + k out
function refLists(b, pts, radii, cap, skip0) {
  const n = b.length / 4, m = pts.length / 4, list = new Uint32Array(m * cap).fill(0xffffffff), count = new Uint32Array(m);
  for (let k = 0; k < m; k++) {
    let c = 0;
    for (let j = 0; j < n; j++) {
      if (skip0 >= 0 && j === skip0 + k) continue;
      const dx = b[4 * j] - pts[4 * k], dy = b[4 * j + 1] - pts[4 * k + 1], dz = b[4 * j + 2] - pts[4 * k + 2];
      if (dx * dx + dy * dy + dz * dz < radii[k] * radii[k]) { if (c < cap) list[k * cap + c] = j; c++; }
    }
    count[k] = c;
  }
  return { list: list, count: count };
}
function equal(got, ref) {
  if (got.list.length !== ref.list.length || got.count.length !== ref.count.length) return false;
  for (let k = 0; k < ref.count.length; k++) if (got.count[k] !== ref.count[k]) return false;
  for (let k = 0; k < ref.list.length; k++) if (got.list[k] !== ref.list[k]) return false;
  return true;
}

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_neighborLists', typeof addon.neighborLists === 'function');
  check('wrapper_has_neighborLists', typeof nb.Simulation.prototype.neighborLists === 'function');
  check('neighborLists_before_init_throws', throws(function () { new nb.Simulation().neighborLists(new Float32Array(4), { radius: 1 }); }, /call init\(particles\) first/));
  check('neighborLists_wants_a_handle', throws(function () { addon.neighborLists({}, null, 0, 1, null, 1, 4, new Uint32Array(4), null); }, /./));
} else {
  const n = 1025;
  let seed = 4321;
  function rnd() { seed = (seed * 1664525 + 1013904223) >>> 0; return seed / 4294967296; }
  const b0 = new Float32Array(4 * n), v0 = new Float32Array(4 * n);
  for (let k = 0; k < n; k++) {
    for (let c = 0; c < 3; c++) b0[4 * k + c] = Math.floor(17 * rnd()) - 8;
    b0[4 * k + 3] = 1 / n;
  }
  for (let k = 0; k < 50; k++) { const d = Math.floor(n * rnd()), s = Math.floor(n * rnd()); for (let c = 0; c < 3; c++) b0[4 * d + c] = b0[4 * s + c]; }
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  sim.init([b0, v0]);
  const r3 = new Float32Array(n).fill(3);
  let most = 0;
  for (const cap of [16, 128]) {
    const own = sim.neighborLists(null, { bodies: [0, n], radius: 3, cap: cap });
    const ref = refLists(b0, b0, r3, cap, 0);
    for (let k = 0; k < n; k++) most = Math.max(most, ref.count[k]);
    check('gpu_lists_cap' + cap + '_vs_double_loop', own.list instanceof Uint32Array && own.count instanceof Uint32Array && own.cap === cap && equal(own, ref));
  }
  check('gpu_lists_cap16_truncates_and_cap128_does_not', most > 16 && most <= 128, most);
  const m = 300, pts = new Float32Array(4 * m), radii = new Float32Array(m);
  for (let k = 0; k < m; k++) {
    for (let c = 0; c < 3; c++) pts[4 * k + c] = k % 10 ? Math.floor(17 * rnd()) - 8 : b0[4 * (k % n) + c];
    radii[k] = 1 + Math.floor(4 * rnd());
  }
  check('gpu_lists_points_vs_double_loop', equal(sim.neighborLists(pts, { radii: radii, cap: 16 }), refLists(b0, pts, radii, 16, -1)));
  const nbr = sim.neighbors(null, { bodies: [0, n], radius: 3 }), lists = sim.neighborLists(null, { bodies: [0, n], radius: 3 });
  check('gpu_lists_count_is_the_neighbors_count', lists.cap === 64 && lists.count.every(function (c, k) { return c === nbr.count[k]; }));
  check('gpu_lists_range_error', throws(function () { sim.neighborLists(null, { bodies: [1000, 26], radius: 3 }); }, /first_body.*NB_1|NB_1/));
  check('gpu_lists_need_a_radius', throws(function () { sim.neighborLists(null, { bodies: [0, n] }); }, /radi/));
  check('gpu_lists_cap_range', throws(function () { sim.neighborLists(null, { bodies: [0, n], radius: 3, cap: 5000 }); }, /cap/));
  sim.destroy();
}
console.log(JSON.stringify({ ok: ok, mode: mode, results: results }));
process.exit(ok ? 0 : 1);
