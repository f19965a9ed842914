'use strict';
/* Node-side tests of the neighbour query (Simulation.prototype.neighbors / closePairs / addon.neighbors), driven by
 * tests/test_neighbors_node.py and tests/test_neighbors_gpu.py.
 *   node tests/js/node_neighbors_tests.js cpu   -> the surface, no GPU
 *   node tests/js/node_neighbors_tests.js gpu   -> neighbors() on an integer lattice against a double loop in JavaScript
 * Prints one JSON object; exit code 0 iff every check passed. */
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));

const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throws(fn, re) { try { fn(); } catch (e) { return re.test(String(e.message) + ' ' + String(e.code)); } return false; }

// exact on a lattice: the smallest j among equal distances; skip0 >= 0: point k leaves body skip0 + k out
function refNeighbors(b, pts, radii, skip0) {
  const n = b.length / 4, m = pts.length / 4, index = new Uint32Array(m), dist2 = new Float64Array(m), count = new Uint32Array(m);
  for (let k = 0; k < m; k++) {
    let best = Infinity, at = 0xffffffff, c = 0;
    for (let j = 0; j < n; j++) {
      if (skip0 >= 0 && j === skip0 + k) continue;
      const dx = b[4 * j] - pts[4 * k], dy = b[4 * j + 1] - pts[4 * k + 1], dz = b[4 * j + 2] - pts[4 * k + 2];
      const d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best) { best = d2; at = j; }
      if (d2 < radii[k] * radii[k]) c++;
    }
    index[k] = at; dist2[k] = best; count[k] = c;
  }
  return { index: index, dist2: dist2, count: count };
}
function equal(got, ref) {
  if (got.index.length !== ref.index.length) return false;
  for (let k = 0; k < ref.index.length; k++)
    if (got.index[k] !== ref.index[k] || got.dist2[k] !== ref.dist2[k] || got.count[k] !== ref.count[k]) return false;
  return true;
}

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_neighbors', typeof addon.neighbors === 'function');
  check('wrapper_has_neighbors', typeof nb.Simulation.prototype.neighbors === 'function');
  check('wrapper_has_closePairs', typeof nb.Simulation.prototype.closePairs === 'function');
  check('neighbors_before_init_throws', throws(function () { new nb.Simulation().neighbors(new Float32Array(4)); }, /call init\(particles\) first/));
  check('closePairs_before_init_throws', throws(function () { new nb.Simulation().closePairs(0.1); }, /call init\(particles\) first/));
  check('neighbors_wants_a_handle', throws(function () { addon.neighbors({}, null, 0, 1, null, 0, null, null, null); }, /./));
  const mp = nb.mutualPairs({ index: Uint32Array.from([1, 0, 3, 4, 3, 0xffffffff, 7, 6]),
    dist2: Float32Array.from([0.25, 0.25, 0.01, 0.04, 0.04, Infinity, 1, 1]) }, 1.0);
  check('mutual_pairs_logic', Array.from(mp.pairs).join() === '0,1,3,4' && mp.dist2.length === 2 && mp.dist2[0] === 0.25, Array.from(mp.pairs));
} else {
  const n = 1000;
  let seed = 4321;
  function rnd() { seed = (seed * 1664525 + 1013904223) >>> 0; return seed / 4294967296; }
  const b0 = new Float32Array(4 * n), v0 = new Float32Array(4 * n);
  for (let k = 0; k < n; k++) {
    for (let c = 0; c < 3; c++) b0[4 * k + c] = Math.floor(129 * rnd()) - 64;
    b0[4 * k + 3] = 1 / n;
  }
  for (let k = 0; k < 50; k++) { const d = Math.floor(n * rnd()), s = Math.floor(n * rnd()); for (let c = 0; c < 3; c++) b0[4 * d + c] = b0[4 * s + c]; }
  const sim = new nb.Simulation({ dt: 1e-3, G: 1.0 });
  sim.init([b0, v0]);
  const own = sim.neighbors(null, { bodies: [0, n], radius: 3 });
  const r3 = new Float32Array(n).fill(3);
  check('gpu_neighbors_bodies_vs_double_loop', own.index instanceof Uint32Array && own.dist2 instanceof Float32Array && own.count instanceof Uint32Array &&
    equal(own, refNeighbors(b0, b0, r3, 0)));
  const m = 300, pts = new Float32Array(4 * m), radii = new Float32Array(m);
  for (let k = 0; k < m; k++) {
    for (let c = 0; c < 3; c++) pts[4 * k + c] = k % 10 ? Math.floor(129 * rnd()) - 64 : b0[4 * (k % n) + c];
    radii[k] = 1 + Math.floor(6 * rnd());
  }
  const got = sim.neighbors(pts, { radii: radii });
  check('gpu_neighbors_points_vs_double_loop', equal(got, refNeighbors(b0, pts, radii, -1)) && got.dist2[0] === 0);
  const bare = sim.neighbors(pts);
  check('gpu_neighbors_without_radius_has_no_count', bare.count === undefined && bare.index.every(function (j, k) { return j === got.index[k]; }));
  const part = sim.neighbors(null, { bodies: [900, 100], radius: 3 });
  check('gpu_neighbors_sub_range_same_bits', part.index.every(function (j, k) { return j === own.index[900 + k] && part.dist2[k] === own.dist2[900 + k] && part.count[k] === own.count[900 + k]; }));
  check('gpu_neighbors_range_error', throws(function () { sim.neighbors(null, { bodies: [900, 101] }); }, /first_body.*NB_1|NB_1/));
  const cp = sim.closePairs(0.5), nn = sim.neighbors(null, { bodies: [0, n] });
  let good = cp.pairs.length % 2 === 0 && cp.pairs.length > 0;       // the duplicates: mutual pairs at d2 = 0 (where no third body shares the spot with a smaller index)
  for (let k = 0; k < cp.pairs.length; k += 2) {
    const i = cp.pairs[k], j = cp.pairs[k + 1];
    if (!(i < j && nn.index[i] === j && nn.index[j] === i && cp.dist2[k / 2] === 0)) good = false;
  }
  check('gpu_close_pairs_are_mutual', good, cp.pairs.length / 2);
  sim.destroy();
}
console.log(JSON.stringify({ ok: ok, mode: mode, results: results }));
process.exit(ok ? 0 : 1);
