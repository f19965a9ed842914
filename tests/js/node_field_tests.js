'use strict';
/* Node-side tests of the field query (Simulation.prototype.field / addon.fieldEval), driven by tests/test_field_node.py and
 * tests/test_field_gpu.py.
 *   node tests/js/node_field_tests.js cpu   -> the surface, no GPU
 *   node tests/js/node_field_tests.js gpu   -> field() against a double loop in JavaScript
 * Prints one JSON object; exit code 0 iff every check passed. */
const fs = require('fs');
const path = require('path');
const ROOT = path.join(__dirname, '..', '..');
const JS = path.join(ROOT, 'nbody3d-webgpu_amd', 'js');
const nb = require(path.join(JS, 'nbody3d_hip.js'));
const GOLD = path.join(ROOT, 'tests', 'golden');

function loadF32(name) { const b = fs.readFileSync(path.join(GOLD, name + '.f32')); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); }
const results = {}; let ok = true;
function check(name, cond, info) { results[name] = { pass: !!cond, info: info }; if (!cond) ok = false; }
function throws(fn, re) { try { fn(); } catch (e) { return re.test(String(e.message) + ' ' + String(e.code)); } return false; }

// fp64 direct sum in JavaScript; skip0 >= 0: point k leaves body skip0 + k out
function refField(b, pts, G, eps2, skip0) {
  const n = b.length / 4, m = pts.length / 4, acc = new Float64Array(4 * m), phi = new Float64Array(m);
  for (let k = 0; k < m; k++) {
    let ax = 0, ay = 0, az = 0, p = 0;
    for (let j = 0; j < n; j++) {
      if (skip0 >= 0 && j === skip0 + k) continue;
      const dx = b[4 * j] - pts[4 * k], dy = b[4 * j + 1] - pts[4 * k + 1], dz = b[4 * j + 2] - pts[4 * k + 2];
      const y = 1 / Math.sqrt(dx * dx + dy * dy + dz * dz + eps2), s = b[4 * j + 3] * y, s3 = s * y * y;
      ax += s3 * dx; ay += s3 * dy; az += s3 * dz; p += s;
    }
    acc[4 * k] = G * ax; acc[4 * k + 1] = G * ay; acc[4 * k + 2] = G * az; phi[k] = -G * p;
  }
  return { accel: acc, phi: phi };
}
function worst(got, ref) {
  let ea = 0, ef = 0;
  for (let k = 0; k < ref.phi.length; k++) {
    let d = 0, s = 0;
    for (let c = 0; c < 3; c++) { d = Math.max(d, Math.abs(got.accel[4 * k + c] - ref.accel[4 * k + c])); s = Math.max(s, Math.abs(ref.accel[4 * k + c])); }
    ea = Math.max(ea, d / s);
    ef = Math.max(ef, Math.abs(got.phi[k] - ref.phi[k]) / Math.abs(ref.phi[k]));
  }
  return { accel: ea, phi: ef };
}

const mode = process.argv[2] || 'cpu';
if (mode === 'cpu') {
  check('addon_loads', nb.load() === 2);
  const addon = require(path.join(JS, 'addon', 'nb_napi.node'));
  check('addon_exports_fieldEval', typeof addon.fieldEval === 'function');
  check('wrapper_has_field', typeof nb.Simulation.prototype.field === 'function');
  check('field_before_init_throws', throws(function () { new nb.Simulation().field(new Float32Array(4)); }, /call init\(particles\) first/));
  check('field_eval_wants_a_handle', throws(function () { addon.fieldEval({}, null, 0, 1, null, null); }, /./));
} else {
  const b0 = loadF32('plummer1024_bodies0'), v0 = loadF32('plummer1024_vel0'), n = 1024, G = 0.5, eps2 = 1e-4;
  const sim = new nb.Simulation({ dt: 1e-3, G: G });
  sim.init([b0, v0]);
  // pseudo-random points in the bodies' bounding box
  let seed = 12345;
  function rnd() { seed = (seed * 1664525 + 1013904223) >>> 0; return seed / 4294967296; }
  const m = 300, pts = new Float32Array(4 * m);
  for (let k = 0; k < m; k++) for (let c = 0; c < 3; c++) pts[4 * k + c] = 4 * rnd() - 2;
  const got = sim.field(pts);
  const e1 = worst(got, refField(b0, pts, G, eps2, -1));
  check('gpu_field_points_vs_double_loop', got.accel instanceof Float32Array && got.accel.length === 4 * m && got.phi.length === m && e1.accel <= 2e-5 && e1.phi <= 2e-5, e1);
  const own = sim.field(null, { bodies: [0, n] });
  const e2 = worst(own, refField(b0, b0, G, eps2, 0));
  check('gpu_field_bodies_vs_double_loop', own.accel.length === 4 * n && own.phi.length === n && e2.accel <= 2e-5 && e2.phi <= 2e-5, e2);
  const part = sim.field(null, { bodies: [1000, 24], accel: false });
  const e3 = worst({ accel: refField(b0, b0.subarray(4000, 4096), G, eps2, 1000).accel, phi: part.phi }, refField(b0, b0.subarray(4000, 4096), G, eps2, 1000));
  check('gpu_field_sub_range_phi_only', part.accel === null && part.phi.length === 24 && e3.phi <= 2e-5, e3);
  check('gpu_field_range_error', throws(function () { sim.field(null, { bodies: [1000, 25] }); }, /first_body.*NB_1|NB_1/));
  // the state is untouched: stepping with queries in between equals stepping without
  const a = new nb.Simulation({ dt: 1e-3, G: G }), c = new nb.Simulation({ dt: 1e-3, G: G });
  a.init([b0, v0]); c.init([b0, v0]);
  for (let k = 0; k < 5; k++) { a.step(); a.field(pts); c.step(); }
  const ra = a.read(), rc = c.read();
  let same = true;
  for (let i = 0; i < ra.bodies.length; i++) if (ra.bodies[i] !== rc.bodies[i] || ra.vel[i] !== rc.vel[i]) same = false;
  check('gpu_field_leaves_the_state_alone', same);
  a.destroy(); c.destroy(); sim.destroy();
}
console.log(JSON.stringify({ ok: ok, mode: mode, results: results }));
process.exit(ok ? 0 : 1);
