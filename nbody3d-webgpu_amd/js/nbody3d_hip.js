'use strict';
/*
 * nbody3d_hip.js -- Node.js host side of the MI355X direct N-body engine.
 *
 * Keeps the JavaScript surface of the reference's force+integrate path.  The
 * reference (huj31415/nbody3d-webgpu) has no exported functions: the path is a
 * region of one browser script.  The names below are the ones BASELINE.json's
 * north_star uses, mapped onto that region (file:line in /root/reference):
 *
 *   init(particles)        nbody3d.js:177-199  generate -> 3x createBuffer ->
 *                                              2x writeBuffer (accel left zero)
 *   step(dt)               nbody3d.js:470 (uniform upload) + :474-480 (compute
 *                          pass, gated by dt > 0) + :489-490 (submit)
 *   simulate(nSteps, dt)   nSteps frames of step() without the render pass
 *   read()                 util.js:163-178     the three readBuffer() copies
 *   restore(state)         util.js:230-244     importSimulation's buffer writes
 *   G / dt / pause()       nbody3d.js:6-7, util.js:36-64 (dt and G are mutable
 *                          between frames; pause saves dt and sets it to 0)
 *   readJerk()             (no reference analogue) the jerk of a {integrator: 'hermite4'} simulation
 *   setHermiteOrder(6 | 4), hermiteOrder(), readSnap(), uploadDerivs6(accel, jerk, snap, crackle)
 *                          (no reference analogue) the 6th-order scheme of a 'hermite4' simulation on force, jerk and snap
 *   setBlockBatch() / setBlockBatch6() / setBlockBatchMixed() / setBlockBatchWatch() / blockBatchStats()
 *   setBlockSteps() / setBlockSteps6() / blockStats() / readLevels() / uploadLevels()
 *   setEncounterWatch() / encounterStats() / downloadEncounters() / uploadEncounters() / resetEncounters()
 *                          (no reference analogue) block individual time steps of a 'hermite4' simulation
 *   requestFrame()/frame() nbody3d.js:408-415,482-487 what the render pass reads each frame
 *                          (bodies + speed), delivered asynchronously to a host-side viewer
 *
 * Data convention is the reference's: Float32Array packed [x,y,z,m, ...] and
 * [vx,vy,vz,0, ...] (nbody3d.js:49,132).  Node >= 12 syntax only.
 *
 * All compute happens in csrc/libnbody3d_hip.so through addon/nb_napi.node;
 * there is no JavaScript fallback -- a missing library or GPU throws.
 */
const path = require('path');

const DEFAULT_LIB = path.join(__dirname, '..', 'csrc', 'libnbody3d_hip.so');
const TILE_SIZE = 256;      // nbody3d.js:4
const DEFAULT_G = 0.0001;   // nbody3d.js:6
const DEFAULT_DT = 1e-4;    // nbody3d.js:7
const EPS2 = 1e-4;          // nbody3d.js:234
const INTEGRATORS = { leapfrog: 0, hermite4: 1 };   // nb_integrator

let addon = null;
let abi = 0;

function load(libPath) {
  if (!addon) addon = require('./addon/nb_napi.node');
  abi = addon.load(libPath || process.env.NBODY3D_HIP_LIB || DEFAULT_LIB);
  return abi;
}

function deviceCount() {
  load();
  return addon.deviceCount();
}

/** The launch plan the engine would build for {n, f64, variant, jsplit, flags, layerBudgetMiB, shardBegin, shardCount}
 *  (nb_plan_query): kernel form, j-partitions, and the symmetric pass's padded rows / partial-sum layers / bytes.  With nCU and
 *  clockHz given (an MI355X: 256, 2.4e9) it needs no GPU -- capacity planning; otherwise the current device's figures are used. */
function planQuery(options) {
  load();
  return addon.planQuery(options || {});
}

function asParticles(particles) {
  // generateGalaxy returns [pos, vel] (nbody3d.js:132); objects are accepted too
  let bodies, vel, accel = null;
  if (Array.isArray(particles)) {
    bodies = particles[0]; vel = particles[1]; accel = particles[2] || null;
  } else if (particles && typeof particles === 'object') {
    bodies = particles.bodies; vel = particles.vel; accel = particles.accel || null;
  }
  if (!bodies || !vel) throw new TypeError('init(particles): expected [bodies, vel] or {bodies, vel[, accel]}');
  return { bodies: bodies, vel: vel, accel: accel };
}

class Simulation {
  /** options: {G, dt, f64, eps2, device, shards, collective, shardBegin, shardCount, variant, jsplit, flags, layerBudgetMiB, integrator}
   *  integrator: 'leapfrog' (default: the reference's lagged scheme, nbody3d.js:274-290) or 'hermite4' (no reference analogue:
   *  4th-order Hermite predictor-corrector; bodies and vel belong to ONE instant, accel and the jerk are derived from them;
   *  whole system on one device).  Anything else throws RangeError here, before the engine is touched.
   *  layerBudgetMiB: nb_config.layer_budget_mib (device memory the symmetric pass may take for its partial sums; 0 = default).
   *  shards > 1: single-process multi-device (i-shards round-robin over the visible GPUs; all-gather
   *  of positions after every step through collective: 'peer' -- event-ordered device-to-device
   *  copies, the default -- or 'rccl' -- ncclCommInitAll + grouped in-place ncclAllGather;
   *  no reference analogue). */
  constructor(options) {
    const o = options || {};
    this.options = o;
    this.G = o.G !== undefined ? o.G : DEFAULT_G;
    this.dt = o.dt !== undefined ? o.dt : DEFAULT_DT;
    this.f64 = !!o.f64;
    this.integrator = o.integrator !== undefined ? o.integrator : 'leapfrog';
    if (!Object.prototype.hasOwnProperty.call(INTEGRATORS, this.integrator)) {
      throw new RangeError("integrator: expected 'leapfrog' or 'hermite4', got " + String(o.integrator));
    }
    this._oldDt = null;     // util.js:35
    this._h = null;
    this.nBodies = 0;       // nbody3d.js:14
  }

  get ArrayType() { return this.f64 ? Float64Array : Float32Array; }

  _coerce(a, name) {
    const T = this.ArrayType;
    if (!(a instanceof T)) {
      if (a && typeof a.length === 'number') a = T.from(a);   // plain arrays as in importSimulation (util.js:231)
      else throw new TypeError(name + ': expected ' + T.name);
    }
    if (a.length !== 4 * this.nBodies) throw new RangeError(name + ': expected ' + (4 * this.nBodies) + ' elements, got ' + a.length);
    return a;
  }

  /** nbody3d.js:177-199.  Re-initialising replaces the buffers (util.js:69-75 "Regenerate"). */
  init(particles) {
    load();
    const p = asParticles(particles);
    if (p.bodies.length % 4 !== 0 || p.bodies.length === 0) throw new RangeError('bodies must hold 4*n elements');
    const n = p.bodies.length / 4;
    if (this._h && n !== this.nBodies) this.destroy();
    this.nBodies = n;
    if (!this._h) {
      const o = this.options;
      this._h = addon.create({
        n: n, f64: this.f64 ? 1 : 0, eps2: o.eps2 !== undefined ? o.eps2 : EPS2,
        device: o.device !== undefined ? o.device : -1, shardBegin: o.shardBegin || 0, shardCount: o.shardCount || 0,
        variant: o.variant || 0, jsplit: o.jsplit || 0, tile: o.tile || 0, shards: o.shards || 0,
        flags: o.flags || 0, layerBudgetMiB: o.layerBudgetMiB || 0, collective: o.collective === 'rccl' ? 1 : 0,
        integrator: INTEGRATORS[this.integrator],
      });
      this._frame = null;
    }
    addon.upload(this._h, this._coerce(p.bodies, 'bodies'), this._coerce(p.vel, 'vel'),
      p.accel ? this._coerce(p.accel, 'accel') : null);
    return this;
  }

  _need() { if (!this._h) throw new Error('simulation not initialised: call init(particles) first'); }

  /** One frame's compute pass.  dt <= 0 (paused) dispatches nothing (nbody3d.js:474). */
  step(dt) {
    this._need();
    if (dt !== undefined) this.dt = dt;
    addon.setParams(this._h, this.dt, this.G);   // nbody3d.js:470: uniforms cross every frame
    addon.step(this._h, 1);
    return this;
  }

  simulate(nSteps, dt) {
    this._need();
    if (dt !== undefined) this.dt = dt;
    addon.setParams(this._h, this.dt, this.G);
    addon.step(this._h, nSteps >>> 0);
    return this;
  }

  /** util.js:56-64 toggleSim: pause saves dt and zeroes it; a second call restores it. */
  togglePause() {
    if (this._oldDt) { this.dt = this._oldDt; this._oldDt = null; }
    else { this._oldDt = this.dt; this.dt = 0; }
    return this.dt;
  }

  /** util.js:37-46: moving the dt slider while paused changes the saved value only. */
  setDt(newDt) {
    if (this._oldDt) this._oldDt = newDt; else this.dt = newDt;
  }

  sync() { this._need(); addon.sync(this._h); return this; }

  /** util.js:163-178: fresh copies {bodies, vel, accel}. */
  read() {
    this._need();
    if (this.integrator !== 'leapfrog') addon.setParams(this._h, this.dt, this.G);   // accel is derived on demand: needs G
    const T = this.ArrayType, len = 4 * this.nBodies;
    const out = { bodies: new T(len), vel: new T(len), accel: new T(len) };
    addon.download(this._h, out.bodies, out.vel, out.accel);
    return out;
  }

  readBodies() {
    this._need();
    const b = new this.ArrayType(4 * this.nBodies);
    addon.download(this._h, b, null, null);
    return b;
  }

  /** The jerk (jx, jy, jz, 0 per body) of a 'hermite4' simulation at the state as it stands (nb_download_jerk; no reference
   *  analogue).  {...read(), jerk: readJerk()} is the whole checkpoint restore() continues bit-identically from. */
  readJerk() {
    this._need();
    addon.setParams(this._h, this.dt, this.G);
    const j = new this.ArrayType(4 * this.nBodies);
    addon.downloadJerk(this._h, j);
    return j;
  }

  /** The order of a 'hermite4' simulation (nb_set_hermite_order; no reference analogue): 6 switches to the 6th-order
   *  predictor-corrector on force, jerk and snap, 4 back (snap and crackle are freed, accel and jerk stay current). */
  setHermiteOrder(order) {
    this._need();
    addon.setHermiteOrder(this._h, order >>> 0);
    return this;
  }

  /** 4 or 6 (nb_hermite_order). */
  hermiteOrder() {
    this._need();
    return addon.hermiteOrder(this._h);
  }

  /** {snap, crackle} (4 elements per body, .w = 0) of an order-6 simulation at the state as it stands (nb_download_snap).  With
   *  read() and readJerk() this is the whole checkpoint uploadDerivs6() continues bit-identically from. */
  readSnap() {
    this._need();
    addon.setParams(this._h, this.dt, this.G);
    const snap = new this.ArrayType(4 * this.nBodies), crackle = new this.ArrayType(4 * this.nBodies);
    addon.downloadSnap(this._h, snap, crackle);
    return { snap: snap, crackle: crackle };
  }

  /** After restore({bodies, vel}) and setHermiteOrder(6): hands a checkpoint's four derivative arrays back (nb_upload_derivs6). */
  uploadDerivs6(accel, jerk, snap, crackle) {
    this._need();
    addon.uploadDerivs6(this._h, this._coerce(accel, 'accel'), this._coerce(jerk, 'jerk'), this._coerce(snap, 'snap'), this._coerce(crackle, 'crackle'));
    return this;
  }

  /** How the engine makes the starts of an order-6 simulation itself (nb_set_start6; no reference analogue): 0 -- snap from the
   *  pass, crackle 0, block levels from (eta / 2)|a|/|j|; 1 -- the crackle is the direct sum on (x, v, a, j) and dynamic block
   *  levels come from the two-rule start.  A start or levels the engine made that no step has consumed are made again; uploaded
   *  ones and a running state are kept. */
  setStart6(mode) {
    this._need();
    addon.setStart6(this._h, mode >>> 0);
    return this;
  }

  /** 0 or 1 (nb_start6). */
  get start6() {
    this._need();
    return addon.start6(this._h);
  }

  /** The precision of the force+jerk pass of an f64 'hermite4' simulation of order 4 (nb_set_pass_precision; no reference analogue):
   *  'native' (0) -- the simulation's own; 'mixed' (1) -- binary32 pair arithmetic on double-single position differences, fp64 sums
   *  across the j-chunks into the unchanged fp64 state.  Touches no state, derivatives or levels; holds from the next pass on. */
  setPassPrecision(mode) {
    if (typeof mode === 'string') {
      if (mode !== 'native' && mode !== 'mixed') throw new RangeError(`setPassPrecision(): mode must be 'native', 'mixed', 0 or 1, not '${mode}'`);
      mode = mode === 'mixed' ? 1 : 0;
    }
    this._need();
    addon.setPassPrecision(this._h, mode >>> 0);
    return this;
  }

  /** 'native' or 'mixed' (nb_pass_precision). */
  passPrecision() {
    this._need();
    return addon.passPrecision(this._h) === 1 ? 'mixed' : 'native';
  }

  /** The guard radius of the mixed pass (nb_set_pass_guard; no reference analogue; 0: off): the terms of pairs closer than rNear are
   *  summed apart from the binary32 registers, compensated, so that a hard pair's members and its barycentre keep the field of the
   *  rest of the system.  Valid while the pass precision is 'mixed'; touches no state, derivatives or levels. */
  setPassGuard(rNear) {
    if (typeof rNear !== 'number') throw new TypeError(`setPassGuard(): rNear must be a number, not ${typeof rNear}`);
    this._need();
    addon.setPassGuard(this._h, rNear);
    return this;
  }

  /** The guard radius, 0 where the guard is off (nb_pass_guard). */
  passGuard() {
    this._need();
    return addon.passGuard(this._h);
  }

  /** Block individual time steps of a 'hermite4' simulation (nb_set_block_steps; no reference analogue): every body steps by
   *  dt / 2^level, minLevel <= level <= maxLevel, chosen from its own derivatives with the accuracy parameter eta; step() and
   *  simulate() still advance by whole dt.  {eta, maxLevel, minLevel, frozen}: missing eta / maxLevel take the library's defaults
   *  (0.02, 20); frozen keeps the levels as initialised or uploaded.  setBlockSteps(null) switches back to one shared step. */
  setBlockSteps(options) {
    this._need();
    if (options === null || options === undefined) { addon.setBlockSteps(this._h, null); return this; }
    addon.setBlockSteps(this._h, options.eta || 0, (options.maxLevel || 0) >>> 0, (options.minLevel || 0) >>> 0, !!options.frozen);
    return this;
  }

  /** Block individual time steps of an order-6 simulation (nb_set_block_steps6; after setHermiteOrder(6)): setBlockSteps' options.
   *  Dynamic levels need precision 'f64'; an 'f32' simulation takes {frozen: true} (levels fixed or uploaded).  blockStats(),
   *  readLevels() and uploadLevels() work as with setBlockSteps().  setBlockSteps6(null) switches back to the shared order-6 step.
   *  Checkpoint restore: restore({bodies, vel}), setHermiteOrder(6), uploadDerivs6(...), setBlockSteps6(...), uploadLevels(levels). */
  setBlockSteps6(options) {
    this._need();
    if (options === null || options === undefined) { addon.setBlockSteps6(this._h, null); return this; }
    addon.setBlockSteps6(this._h, options.eta || 0, (options.maxLevel || 0) >>> 0, (options.minLevel || 0) >>> 0, !!options.frozen);
    return this;
  }

  /** {enabled, outerSteps, blockSteps, bodySteps, clamped, finestLevel} since the last reset (nb_block_stats). */
  blockStats(reset) { this._need(); return addon.blockStats(this._h, !!reset); }

  /** Batched block steps (nb_set_block_batch; after setBlockSteps() on a 'hermite4' simulation of order 4 with the native pass):
   *  block steps with at most smallMax active bodies (default 256; 0: none; at most 1024) run from the device's own header, up to
   *  depth (default 32; at most 1024) of them per host wait.  No stored bit depends on depth.  setBlockBatch(null) switches the
   *  mode off (so does setBlockSteps(null)); setBlockBatch() / setBlockBatch({}) take the defaults. */
  setBlockBatch(options) {
    this._need();
    if (options === null) { addon.setBlockBatch(this._h, null); return this; }
    const o = options || {};
    addon.setBlockBatch(this._h, (o.depth || 0) >>> 0, (o.smallMax === undefined || o.smallMax === null) ? -1 : Number(o.smallMax));
    return this;
  }

  /** setBlockBatch()'s mode on a simulation of order 6 with setBlockSteps6() on (nb_set_block_batch6): the same options, defaults and
   *  refusals; blockBatchStats() serves both.  setBlockBatch6(null) switches the mode off (so do setBlockBatch(null),
   *  setBlockSteps6(null) and setBlockSteps(null)). */
  setBlockBatch6(options) {
    this._need();
    if (options === null) { addon.setBlockBatch6(this._h, null); return this; }
    const o = options || {};
    addon.setBlockBatch6(this._h, (o.depth || 0) >>> 0, (o.smallMax === undefined || o.smallMax === null) ? -1 : Number(o.smallMax));
    return this;
  }

  /** setBlockBatch()'s mode on an f64 simulation of order 4 with setBlockSteps() on, setPassPrecision('mixed') and no guard
   *  (nb_set_block_batch_mixed): the small steps run the double-single pass.  The same options, defaults and refusals;
   *  blockBatchStats() serves all three.  setBlockBatchMixed(null) switches the mode off (so do setBlockBatch(null),
   *  setBlockBatch6(null) and setBlockSteps(null)). */
  setBlockBatchMixed(options) {
    this._need();
    if (options === null) { addon.setBlockBatchMixed(this._h, null); return this; }
    const o = options || {};
    addon.setBlockBatchMixed(this._h, (o.depth || 0) >>> 0, (o.smallMax === undefined || o.smallMax === null) ? -1 : Number(o.smallMax));
    return this;
  }

  /** setBlockBatch()'s mode on a simulation with the encounter watch on (nb_set_block_batch_watch; call setBlockSteps(),
   *  setEncounterWatch(), then this): the small steps watch too, and the records depend on depth as little as the state does.
   *  The same options, defaults and refusals; blockBatchStats() serves all four.  setBlockBatchWatch(null) switches the mode off
   *  and keeps the watch; setEncounterWatch(null) switches off both. */
  setBlockBatchWatch(options) {
    this._need();
    if (options === null) { addon.setBlockBatchWatch(this._h, null); return this; }
    const o = options || {};
    addon.setBlockBatchWatch(this._h, (o.depth || 0) >>> 0, (o.smallMax === undefined || o.smallMax === null) ? -1 : Number(o.smallMax));
    return this;
  }

  /** {enabled, hostWaits, slots, smallSteps, hostSteps, idleSlots} since the last reset (nb_block_batch_stats). */
  blockBatchStats(reset) { this._need(); return addon.blockBatchStats(this._h, !!reset); }

  /** The encounter watch (nb_set_encounter_watch; after setBlockSteps() on a 'hermite4' simulation of order 4 with the native pass,
   *  no batched mode): every body with a watch radius > 0 -- {radius} for all or {radii} one per body (copied; 0: not watched) --
   *  records the closest body it meets below that radius at its OWN block steps: downloadEncounters().  {stop: true} makes step()
   *  return after the first outer step that had a hit (encounterStats().stopped, .stepsLeft).  Changes no bit of the state.
   *  setEncounterWatch(null) switches the watch off (so does setBlockSteps(null)). */
  setEncounterWatch(options) {
    this._need();
    if (options === null || options === undefined) { addon.setEncounterWatch(this._h, null); return this; }
    const T = this.ArrayType, r = options.radii, one = options.radius;
    if ((one === undefined || one === null) === (r === undefined || r === null)) throw new TypeError('setEncounterWatch(): give exactly one of radius and radii');
    const radii = r === null || r === undefined ? null : (r instanceof T ? r : T.from(r));
    if (radii && radii.length !== this.nBodies) throw new RangeError('radii: expected ' + this.nBodies + ' elements, got ' + radii.length);
    if (!radii && !(+one >= 0 && Number.isFinite(+one))) throw new RangeError('setEncounterWatch(): radius must be finite and >= 0');
    addon.setEncounterWatch(this._h, radii ? 0 : +one, radii, !!options.stop);
    return this;
  }

  /** {passes, hits, firstTime, stopped, stepsLeft} (nb_encounter_stats); reset zeroes the counters, not the records. */
  encounterStats(reset) { this._need(); return addon.encounterStats(this._h, !!reset); }

  /** The records (nb_download_encounters): {rho2 (the simulation's precision; Infinity: none), partner (Uint32Array; 0xffffffff:
   *  none), time (Float64Array, in outer steps), count (Uint32Array)}, N elements each. */
  downloadEncounters() {
    this._need();
    const n = this.nBodies;
    const out = { rho2: new this.ArrayType(n), partner: new Uint32Array(n), time: new Float64Array(n), count: new Uint32Array(n) };
    addon.downloadEncounters(this._h, out.rho2, out.partner, out.time, out.count);
    return out;
  }

  /** The records of a checkpoint back (nb_upload_encounters; what downloadEncounters() gave), behind setEncounterWatch(). */
  uploadEncounters(rec) {
    this._need();
    const T = this.ArrayType, n = this.nBodies;
    const as = (a, A, name) => {
      const t = a instanceof A ? a : A.from(a);
      if (t.length !== n) throw new RangeError(name + ': expected ' + n + ' elements, got ' + t.length);
      return t;
    };
    addon.uploadEncounters(this._h, as(rec.rho2, T, 'rho2'), as(rec.partner, Uint32Array, 'partner'), as(rec.time, Float64Array, 'time'),
      as(rec.count, Uint32Array, 'count'));
    return this;
  }

  /** The records to their start values and the counters to 0 (nb_reset_encounters). */
  resetEncounters() { this._need(); addon.resetEncounters(this._h); return this; }

  /** The level of every body (Uint8Array of N; nb_download_levels), initialised first if not current. */
  readLevels() {
    this._need();
    addon.setParams(this._h, this.dt, this.G);
    const l = new Uint8Array(this.nBodies);
    addon.downloadLevels(this._h, l);
    return l;
  }

  /** The last call of a block-step checkpoint restore: restore({bodies, vel, accel, jerk}), setBlockSteps(...), uploadLevels(levels). */
  uploadLevels(levels) {
    this._need();
    const l = levels instanceof Uint8Array ? levels : Uint8Array.from(levels);
    if (l.length !== this.nBodies) throw new RangeError('levels: expected ' + this.nBodies + ' elements, got ' + l.length);
    addon.uploadLevels(this._h, l);
    return this;
  }

  /** The Ahmad-Cohen neighbour scheme of a 'hermite4' simulation (nb_set_neighbor_scheme; no reference analogue): a body's force is
   *  split at its neighbour radius; the sums over its neighbour list run every dt / substeps, the rest once per dt.  {radius | radii,
   *  substeps, cap}: one radius for all or one per body (copied), substeps a power of two (default 8), cap the entries of a list row
   *  (default 128).  A list that does not fit its row makes step() throw NB_4 until the scheme is set again.
   *  setNeighborScheme(null) switches back to plain Hermite steps. */
  setNeighborScheme(options) {
    this._need();
    if (options === null || options === undefined) { addon.setNeighborScheme(this._h, null); this._acCap = 0; return this; }
    const T = this.ArrayType, r = options.radii;
    const radii = r === null || r === undefined ? null : (r instanceof T ? r : T.from(r));
    addon.setParams(this._h, this.dt, this.G);
    addon.setNeighborScheme(this._h, options.radius === undefined || options.radius === null ? 0 : +options.radius, radii,
      (options.substeps || 0) >>> 0, (options.cap || 0) >>> 0);
    this._acCap = (options.cap || 0) >>> 0 || 128;
    return this;
  }

  /** {enabled, regularSteps, substeps, entries, builds, maxCount, overflowed} (nb_neighbor_scheme_stats): entries is the sum of
   *  min(count, cap) over the list builds, the start included; maxCount and overflowed belong to the last build. */
  neighborSchemeStats(reset) { this._need(); return addon.neighborSchemeStats(this._h, !!reset); }

  /** The scheme's own arrays at the simulation's instant (nb_download_neighbor_scheme; runs the scheme's start first if they are
   *  not current): {accelIrr, jerkIrr, accelReg, jerkReg (4*N each), list (Uint32Array N * cap), count (Uint32Array N), cap}. */
  downloadNeighborScheme() {
    this._need();
    if (!this._acCap) throw new Error('downloadNeighborScheme(): the neighbour scheme is not switched on (setNeighborScheme)');
    const T = this.ArrayType, n = this.nBodies;
    const out = { accelIrr: new T(4 * n), jerkIrr: new T(4 * n), accelReg: new T(4 * n), jerkReg: new T(4 * n),
      list: new Uint32Array(n * this._acCap), count: new Uint32Array(n), cap: this._acCap };
    addon.setParams(this._h, this.dt, this.G);
    addon.downloadNeighborScheme(this._h, out.accelIrr, out.jerkIrr, out.accelReg, out.jerkReg, out.list, out.count);
    return out;
  }

  /** Radii that follow a target count (nb_set_neighbor_adapt; needs setNeighborScheme first): after every list build each radius moves
   *  towards the one that would hold `target` members, by at most growMax per build (default cbrt(2)); a build with rows over cap
   *  shrinks those rows and runs again, up to maxRebuilds times (default 4).  {target, growMax, maxRebuilds, radiusMin, radiusMax};
   *  2 * target <= cap.  setNeighborAdapt(null) goes back to the scheme's fixed radii. */
  setNeighborAdapt(options) {
    this._need();
    if (options === null || options === undefined) { addon.setNeighborAdapt(this._h, null); return this; }
    addon.setNeighborAdapt(this._h, (options.target || 0) >>> 0, +(options.growMax || 0), (options.maxRebuilds || 0) >>> 0,
      +(options.radiusMin || 0), +(options.radiusMax || 0));
    return this;
  }

  /** {enabled, rebuilds, rowsShrunk, lastRebuilds} (nb_neighbor_adapt_stats); lastRebuilds belongs to the last build. */
  neighborAdaptStats(reset) { this._need(); return addon.neighborAdaptStats(this._h, !!reset); }

  /** {built, next} (nb_download_neighbor_radii; N each): the radii the current list was cut by and those the next build will use;
   *  with adaptation off both are the scheme's fixed radii. */
  downloadNeighborRadii() {
    this._need();
    const T = this.ArrayType, out = { built: new T(this.nBodies), next: new T(this.nBodies) };
    addon.setParams(this._h, this.dt, this.G);
    addon.downloadNeighborRadii(this._h, out.built, out.next);
    return out;
  }

  /** The last call of a restore that continues bit for bit (nb_upload_neighbor_scheme): restore({bodies, vel}), setNeighborScheme(...),
   *  setNeighborAdapt(...) if used, then uploadNeighborScheme(downloadNeighborScheme()'s object, downloadNeighborRadii().next | null). */
  uploadNeighborScheme(scheme, radii) {
    this._need();
    const T = this.ArrayType, as = (a, A) => (a === null || a === undefined ? null : (a instanceof A ? a : A.from(a)));
    addon.setParams(this._h, this.dt, this.G);
    addon.uploadNeighborScheme(this._h, as(scheme.accelIrr, T), as(scheme.jerkIrr, T), as(scheme.accelReg, T), as(scheme.jerkReg, T),
      as(scheme.list, Uint32Array), as(scheme.count, Uint32Array), as(radii, T));
    return this;
  }

  /** Block individual irregular steps inside the neighbour scheme (nb_set_neighbor_levels; needs setNeighborScheme first): every body
   *  re-evaluates its list force at dt / 2^l of its own, l in [minLevel, log2(substeps)], chosen by the step criterion (eta, default
   *  0.02).  {minLevel, eta, frozen}; minLevel is the accuracy floor of a run; frozen keeps every body at minLevel, or at what
   *  uploadNeighborLevels gave.  setNeighborLevels(null): the shared substeps again (and so does every setNeighborScheme). */
  setNeighborLevels(options) {
    this._need();
    if (options === null || options === undefined) { addon.setNeighborLevels(this._h, null); return this; }
    addon.setNeighborLevels(this._h, (options.minLevel || 0) >>> 0, +(options.eta || 0), !!options.frozen);
    return this;
  }

  /** {enabled, regularSteps, ticks, blockSteps, bodySteps, entries, clamped, finestLevel} (nb_neighbor_level_stats). */
  neighborLevelStats(reset) { this._need(); return addon.neighborLevelStats(this._h, !!reset); }

  /** Uint8Array(N): the levels at the simulation's instant (nb_download_neighbor_levels; runs the starts first where they are due). */
  downloadNeighborLevels() {
    this._need();
    const out = new Uint8Array(this.nBodies);
    addon.setParams(this._h, this.dt, this.G);
    addon.downloadNeighborLevels(this._h, out);
    return out;
  }

  /** After uploadNeighborScheme: the levels are these and the start rule does not run (nb_upload_neighbor_levels). */
  uploadNeighborLevels(levels) {
    this._need();
    addon.setParams(this._h, this.dt, this.G);
    addon.uploadNeighborLevels(this._h, levels instanceof Uint8Array ? levels : Uint8Array.from(levels));
    return this;
  }

  /** util.js:230-244: write the three arrays into the EXISTING buffers (N must match).  A 'hermite4' simulation ignores accel on its
   *  own (a derived array); with BOTH state.accel and state.jerk it takes them as its derivatives (nb_upload_derivs). */
  restore(state) {
    this._need();
    addon.upload(this._h, this._coerce(state.bodies, 'bodies'), this._coerce(state.vel, 'vel'),
      state.accel ? this._coerce(state.accel, 'accel') : null);
    if (state.accel && state.jerk) addon.uploadDerivs(this._h, this._coerce(state.accel, 'accel'), this._coerce(state.jerk, 'jerk'));
    return this;
  }

  /** util.js:186-201 schema: {bodies, vel, accel, camera, G: log10(G).toFixed(2)}.  dt and N are not saved upstream either.
   *  The engine has no camera (rendering is out of scope): the `camera` object of the checkpoint this state was imported
   *  from -- or one handed in -- is passed through untouched, so a browser -> engine -> browser round trip keeps the view
   *  (util.js:190-199 writes it, :246-256 restores it and tolerates its absence). */
  exportJSON(camera) {
    const s = this.read();
    const out = { bodies: Array.from(s.bodies), vel: Array.from(s.vel), accel: Array.from(s.accel) };
    const cam = camera !== undefined ? camera : this.camera;
    if (cam !== undefined && cam !== null) out.camera = cam;
    out.G = (Math.log(this.G) / Math.LN10).toFixed(2);
    return JSON.stringify(out);
  }

  /** util.js:217-263.  Unlike the reference, G takes effect on the next step (the
   *  reference forgets uni.GValue.set, SURVEY.md §5.4), and a different N re-creates. */
  importJSON(text) {
    const json = typeof text === 'string' ? JSON.parse(text) : text;
    const T = this.ArrayType;
    const state = { bodies: T.from(json.bodies), vel: T.from(json.vel), accel: json.accel ? T.from(json.accel) : null };
    if (!this._h || state.bodies.length !== 4 * this.nBodies) this.init(state); else this.restore(state);
    if (json.G !== undefined && json.G !== null) this.G = Math.pow(10, parseFloat(json.G));
    this.camera = json.camera !== undefined ? json.camera : null;       // kept for exportJSON, never read by the engine
    return this;
  }

  /** Viewer frame feed.  The reference's render pass reads bodyBuffer and velBuffer in place
   *  every frame (nbody3d.js:408-415,482-487; colour from length(vel.xyz), :380).  requestFrame()
   *  enqueues a snapshot behind the steps issued so far and returns at once: the copy to the host
   *  runs on a second stream and does not stall later step() calls. */
  requestFrame() { this._need(); addon.requestFrame(this._h); return this; }

  /** Newest snapshot that has landed: {bodies: Float32Array(4n) x,y,z,m; speed: Float32Array(n)
   *  |v|; step} -- the same two arrays refreshed on every call -- or null (wait === false and no
   *  frame has landed yet). */
  frame(wait) {
    this._need();
    if (!this._frame) this._frame = { bodies: new Float32Array(4 * this.nBodies), speed: new Float32Array(this.nBodies), step: 0 };
    const step = addon.frame(this._h, wait !== false, this._frame.bodies, this._frame.speed);
    if (step < 0) return null;
    this._frame.step = step;
    return this._frame;
  }

  enableTiming(on) { this._need(); addon.enableTiming(this._h, on !== false); return this; }
  stepTimes() { this._need(); return addon.stepTimes(this._h); }
  collectiveInfo() { this._need(); return addon.collectiveInfo(this._h); }
  kernelTimes() { this._need(); return addon.kernelTimes(this._h); }
  variant() { this._need(); return addon.variant(this._h); }
  /** Whether the next force pass runs the equal-mass kernels (nb_eqm_info; flags: 1024 = NB_FLAG_NO_EQM keeps the general ones). */
  eqm() { this._need(); return addon.eqm(this._h); }
  /** The form of the force kernels the next force pass runs (nb_eqm_form): 0 general, 1 equal masses, 2 equal masses with unit mass product
   *  (G*m a power of two; flags: 2048 = NB_FLAG_NO_EQM_POW2 keeps form 1). */
  eqmForm() { this._need(); return addon.eqmForm(this._h); }
  diagnostics() { this._need(); addon.setParams(this._h, this.dt, this.G); return addon.diagnostics(this._h); }

  /** Field query (nb_field_eval; no reference analogue): acceleration and potential of the system at `points` -- a typed or
   *  plain array of 4*m elements x, y, z, (ignored) -- or, with options.bodies = [first, count] (and points null), at the
   *  current positions of those bodies, each leaving itself out of its sums.  Returns {accel: 4*m elements ax, ay, az, 0;
   *  phi: m elements} in the handle's precision (Float32Array, Float64Array for f64 handles); options.accel === false /
   *  options.phi === false leave that output out (null).  The positions are those behind every step issued so far; the
   *  simulation state is not touched. */
  field(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    let pts = null, first = 0, m;
    if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    if (points !== null && points !== undefined) {
      if (points instanceof T) pts = points;
      else if (typeof points.length === 'number') pts = T.from(points);
      else throw new TypeError('points: expected ' + T.name);
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('field(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (!o.bodies) throw new TypeError('field(): points, or options.bodies = [first, count], required');
    const out = { accel: o.accel === false ? null : new T(4 * m), phi: o.phi === false ? null : new T(m) };
    addon.setParams(this._h, this.dt, this.G);
    addon.fieldEval(this._h, pts, first, m, out.accel, out.phi);
    return out;
  }

  /** Neighbour query (nb_neighbors; no reference analogue): for each of `points` -- a typed or plain array of 4*m elements x, y, z,
   *  (ignored) -- or, with options.bodies = [first, count] (and points null), for each of those bodies, itself left out by index,
   *  the nearest body, its squared distance (plain, unsoftened) and, with options.radius (one for all) or options.radii (one per
   *  point), the number of bodies strictly closer than that.  Returns {index: Uint32Array, dist2: Float32Array | Float64Array,
   *  count?: Uint32Array}; index is 0xffffffff and dist2 Infinity where there is no candidate; of equal distances the smallest
   *  index wins.  The positions are those behind every step issued so far; the simulation state is not touched. */
  neighbors(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    let pts = null, first = 0, m;
    if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    if (points !== null && points !== undefined) {
      if (points instanceof T) pts = points;
      else if (typeof points.length === 'number') pts = T.from(points);
      else throw new TypeError('points: expected ' + T.name);
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('neighbors(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (!o.bodies) throw new TypeError('neighbors(): points, or options.bodies = [first, count], required');
    let radii = null;
    if (o.radii !== null && o.radii !== undefined) {
      radii = o.radii instanceof T ? o.radii : T.from(o.radii);
      if (radii.length !== m) throw new RangeError('options.radii must hold one radius per point');
    }
    const radius = o.radius === undefined || o.radius === null ? 0 : +o.radius;
    const out = { index: new Uint32Array(m), dist2: new T(m) };
    if (radii || (o.radius !== undefined && o.radius !== null)) out.count = new Uint32Array(m);
    addon.neighbors(this._h, pts, first, m, radii, radius, out.index, out.dist2, out.count || null);
    return out;
  }

  /** Neighbour lists (nb_neighbor_lists; no reference analogue): WHICH bodies lie strictly inside options.radius (one for all) or
   *  options.radii (one per point) of each of `points` -- 4*m elements x, y, z, (ignored) -- or, with options.bodies = [first, count]
   *  (and points null), of each of those bodies, itself left out by index.  Returns {list: Uint32Array of m * cap elements, count:
   *  Uint32Array of m elements, cap}: row k = list.subarray(k * cap, (k + 1) * cap) holds the members in ascending order, padded
   *  with 0xffffffff; count[k] is the true number of members, and where it exceeds cap (options.cap, default 64, at most 4096) the
   *  row holds the cap smallest indices.  The simulation state is not touched. */
  neighborLists(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    let pts = null, first = 0, m;
    if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    if (points !== null && points !== undefined) {
      if (points instanceof T) pts = points;
      else if (typeof points.length === 'number') pts = T.from(points);
      else throw new TypeError('points: expected ' + T.name);
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('neighborLists(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (!o.bodies) throw new TypeError('neighborLists(): points, or options.bodies = [first, count], required');
    let radii = null;
    if (o.radii !== null && o.radii !== undefined) {
      radii = o.radii instanceof T ? o.radii : T.from(o.radii);
      if (radii.length !== m) throw new RangeError('options.radii must hold one radius per point');
    }
    const radius = o.radius === undefined || o.radius === null ? 0 : +o.radius;
    const cap = o.cap === undefined || o.cap === null ? 64 : +o.cap;
    if (!(Number.isInteger(cap) && cap >= 1 && cap <= 4096)) throw new RangeError('options.cap must be an integer in 1 .. 4096');
    const out = { list: new Uint32Array(m * cap), count: new Uint32Array(m), cap: cap };
    addon.neighborLists(this._h, pts, first, m, radii, radius, cap, out.list, out.count);
    return out;
  }

  /** The k nearest bodies (nb_knn; no reference analogue) of each of `points` -- 4*m elements x, y, z, (ignored) -- or, with
   *  options.bodies = [first, count] (and points null), of each of those bodies, itself left out by index.  options.k: 1 .. 64,
   *  default 6.  Returns {index: Uint32Array, dist2: Float32Array | Float64Array, k}, m * k elements each: row r =
   *  index.subarray(r * k, (r + 1) * k) holds the k smallest candidates in the order (dist2 ascending, then index ascending), padded
   *  with 0xffffffff / Infinity where there are fewer than k.  options.dist2 === false leaves dist2 out.  Column 0 is what
   *  neighbors() returns.  The simulation state is not touched. */
  knn(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    let pts = null, first = 0, m;
    if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    if (points !== null && points !== undefined) {
      if (points instanceof T) pts = points;
      else if (typeof points.length === 'number') pts = T.from(points);
      else throw new TypeError('points: expected ' + T.name);
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('knn(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (!o.bodies) throw new TypeError('knn(): points, or options.bodies = [first, count], required');
    const k = o.k === undefined || o.k === null ? 6 : +o.k;
    if (!(Number.isInteger(k) && k >= 1 && k <= 64)) throw new RangeError('options.k must be an integer in 1 .. 64');
    const out = { index: new Uint32Array(m * k), dist2: o.dist2 === false ? null : new T(m * k), k: k };
    addon.knn(this._h, pts, first, m, k, out.index, out.dist2);
    return out;
  }

  /** Acceleration, jerk and potential summed over the entries of neighbour rows (nb_list_force; no reference analogue): `lists` is a
   *  Uint32Array of m * options.cap entries -- the rows neighborLists() or knn() return, or any other --, row k belonging to
   *  options.points[k] (4*m elements x, y, z, ignored) or, with options.bodies = [first, m], to body first + k, an entry equal to
   *  that index skipped.  An entry >= nBodies (the padding 0xffffffff, wherever it stands) adds nothing.  options.count
   *  (Uint32Array, m): only the first min(count, cap) entries of a row are read.  options.accel (default true), options.jerk
   *  (default false: needs a 'hermite4' simulation and, at points, options.pointVel), options.phi (default false) choose the
   *  outputs.  Returns {accel, jerk, phi}: 4*m, 4*m, m elements, null for what was not asked for.  A row's outputs depend on its
   *  entries, its point and the bodies only, bit for bit.  The simulation state is not touched. */
  listForce(lists, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    if (!(lists instanceof Uint32Array)) throw new TypeError('lists: expected Uint32Array');
    const cap = o.cap === undefined || o.cap === null ? NaN : +o.cap;
    if (!(Number.isInteger(cap) && cap >= 1 && cap <= 4096)) throw new RangeError('options.cap must be an integer in 1 .. 4096');
    if (lists.length === 0 || lists.length % cap !== 0) throw new RangeError('lists must hold m * cap entries, m >= 1');
    const m = lists.length / cap;
    const real = function (a, name) {
      if (a === null || a === undefined) return null;
      if (a instanceof T) return a;
      if (typeof a.length === 'number') return T.from(a);
      throw new TypeError(name + ': expected ' + T.name);
    };
    const pts = real(o.points, 'points'), pv = real(o.pointVel, 'pointVel');
    let first = 0;
    if (o.bodies) {
      if (pts) throw new RangeError('listForce(): give either options.points or options.bodies, not both');
      first = o.bodies[0] >>> 0;
      if ((o.bodies[1] >>> 0) !== m) throw new RangeError('options.bodies = [first, count]: count must be the number of rows');
    } else if (!pts) throw new TypeError('listForce(): options.points, or options.bodies = [first, count], required');
    let count = null;
    if (o.count !== null && o.count !== undefined) count = o.count instanceof Uint32Array ? o.count : Uint32Array.from(o.count);
    const out = { accel: o.accel === false ? null : new T(4 * m), jerk: o.jerk ? new T(4 * m) : null, phi: o.phi ? new T(m) : null };
    addon.setParams(this._h, this.dt, this.G);   // the sums carry G
    addon.listForce(this._h, lists, cap, pts, pv, first, count, out.accel, out.jerk, out.phi);
    return out;
  }

  /** The regular and the irregular force+jerk of every point in ONE pass (nb_split_force; no reference analogue): at `points` (4*m
   *  elements x, y, z, ignored) -- or, with options.bodies = [first, m], at those bodies -- the acceleration of ALL bodies, every
   *  pair's term added to exactly one of two sums: *Irr over the bodies with d2 < h^2 (options.radius, or one of options.radii per
   *  point; the strict rule of neighbors()), *Reg over every other row.  Nothing is subtracted.  options.jerk (default: true on a
   *  'hermite4' simulation, which it needs) adds the two jerk sums and wants, at points, options.pointVel.  Returns {accelIrr,
   *  accelReg, jerkIrr, jerkReg}: 4*m elements each, the jerks null when not asked for.  The simulation state is not touched. */
  splitForce(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    const real = function (a, name) {
      if (a === null || a === undefined) return null;
      if (a instanceof T) return a;
      if (typeof a.length === 'number') return T.from(a);
      throw new TypeError(name + ': expected ' + T.name);
    };
    const pts = real(points, 'points'), pv = real(o.pointVel, 'pointVel'), radii = real(o.radii, 'radii');
    let first = 0, m = 0;
    if (pts) {
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('splitForce(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    else throw new TypeError('splitForce(): points, or options.bodies = [first, count], required');
    const jerk = o.jerk === undefined || o.jerk === null ? this.integrator !== 'leapfrog' : !!o.jerk;
    const radius = o.radius === undefined || o.radius === null ? 0 : +o.radius;
    const out = { accelIrr: new T(4 * m), accelReg: new T(4 * m), jerkIrr: jerk ? new T(4 * m) : null, jerkReg: jerk ? new T(4 * m) : null };
    addon.setParams(this._h, this.dt, this.G);   // the sums carry G
    addon.splitForce(this._h, pts, pv, first, m, radii, radius, out.accelIrr, out.accelReg, out.jerkIrr, out.jerkReg);
    return out;
  }

  /** splitForce()'s sums AND neighborLists()' rows from ONE pass over the pairs, cut by one comparison (nb_split_lists; no reference
   *  analogue).  The arguments of splitForce() and options.cap (entries per row, 1 .. 4096, default 64).  Returns splitForce()'s
   *  object with two more members: list (Uint32Array, m * cap: a row's members in ascending order, padded with 0xffffffff, the cap
   *  smallest where there are more) and count (Uint32Array, m: the true number of members) -- what neighborLists() returns; with
   *  options.bodies a body leaves itself out of its row by index.  The simulation state is not touched. */
  splitLists(points, options) {
    this._need();
    const o = options || {}, T = this.ArrayType;
    const real = function (a, name) {
      if (a === null || a === undefined) return null;
      if (a instanceof T) return a;
      if (typeof a.length === 'number') return T.from(a);
      throw new TypeError(name + ': expected ' + T.name);
    };
    const pts = real(points, 'points'), pv = real(o.pointVel, 'pointVel'), radii = real(o.radii, 'radii');
    let first = 0, m = 0;
    if (pts) {
      if (pts.length % 4 !== 0) throw new RangeError('points must hold 4*m elements (x, y, z, ignored)');
      if (o.bodies) throw new RangeError('splitLists(): give either points or options.bodies, not both');
      m = pts.length / 4;
    } else if (o.bodies) { first = o.bodies[0] >>> 0; m = o.bodies[1] >>> 0; }
    else throw new TypeError('splitLists(): points, or options.bodies = [first, count], required');
    const cap = o.cap === undefined || o.cap === null ? 64 : +o.cap;
    if (!(Number.isInteger(cap) && cap >= 1 && cap <= 4096)) throw new RangeError('splitLists(): options.cap must be an integer in 1 .. 4096');
    const jerk = o.jerk === undefined || o.jerk === null ? this.integrator !== 'leapfrog' : !!o.jerk;
    const radius = o.radius === undefined || o.radius === null ? 0 : +o.radius;
    const out = { accelIrr: new T(4 * m), accelReg: new T(4 * m), jerkIrr: jerk ? new T(4 * m) : null, jerkReg: jerk ? new T(4 * m) : null,
      list: new Uint32Array(m * cap), count: new Uint32Array(m), cap: cap };
    addon.setParams(this._h, this.dt, this.G);   // the sums carry G
    addon.splitLists(this._h, pts, pv, first, m, radii, radius, out.accelIrr, out.accelReg, out.jerkIrr, out.jerkReg, cap, out.list, out.count);
    return out;
  }

  /** Whether the next list build of the neighbour scheme is ONE nb_split_lists call (nb_neighbor_scheme_fused): false with
   *  flags: 4096 (NB_FLAG_AC_TWO_CALLS), where the launch shapes differ, and without the scheme.  Both routes leave the same bytes. */
  neighborSchemeFused() {
    this._need();
    return addon.neighborSchemeFused(this._h);
  }

  /** The Casertano-Hut local density at every body, a Float64Array of nBodies elements: one knn() call over all bodies, then per
   *  body the masses of its first k - 1 neighbours over the volume of the sphere that reaches the k-th (k >= 2, default 6); NaN
   *  where a body has fewer than k neighbours. */
  localDensity(k) {
    this._need();
    k = k === undefined || k === null ? 6 : +k;
    if (!(Number.isInteger(k) && k >= 2 && k <= 64)) throw new RangeError('localDensity(k): k must be an integer in 2 .. 64');
    const n = this.nBodies, nn = this.knn(null, { bodies: [0, n], k: k }), b = this.readBodies();
    const rho = new Float64Array(n);
    for (let i = 0; i < n; i++) {
      const row = i * k;
      if (nn.index[row + k - 1] === 0xffffffff) { rho[i] = NaN; continue; }
      let msum = 0;
      for (let t = 0; t < k - 1; t++) msum += b[4 * nn.index[row + t] + 3];
      rho[i] = msum / (4 * Math.PI / 3 * Math.pow(nn.dist2[row + k - 1], 1.5));
    }
    return rho;
  }

  /** The close pairs of the system: the MUTUAL nearest neighbours (i < j, each the other's nearest body) closer than `radius`, as
   *  {pairs: Uint32Array of 2*k elements i0, j0, i1, j1, ... sorted by i, dist2: k elements} -- one neighbors() call over all
   *  bodies and host code on its result. */
  closePairs(radius) {
    this._need();
    return mutualPairs(this.neighbors(null, { bodies: [0, this.nBodies] }), radius);
  }

  destroy() {
    if (this._h) { addon.destroy(this._h); this._h = null; this._frame = null; }
  }
}

/* The mutual nearest-neighbour pairs closer than `radius` of a neighbors() result over all bodies (closePairs: pure host code). */
function mutualPairs(nn, radius) {
  const n = nn.index.length, T = nn.dist2.constructor, h = new T([radius]), h2 = new T([h[0] * h[0]])[0];
  const ij = [], d2 = [];
  for (let i = 0; i < n; i++) {
    const j = nn.index[i];
    if (j < n && i < j && nn.index[j] === i && nn.dist2[i] < h2) { ij.push(i, j); d2.push(nn.dist2[i]); }
  }
  return { pairs: Uint32Array.from(ij), dist2: T.from(d2) };
}

/* Module-level instance: the reference keeps its state in module globals
 * (nbody3d.js:2-34), so `init(p); step(dt)` works without constructing anything. */
let current = null;
function init(particles, options) {
  if (current) current.destroy();
  current = new Simulation(options);
  return current.init(particles);
}
function need() { if (!current) throw new Error('call init(particles) first'); return current; }
function step(dt) { return need().step(dt); }
function simulate(nSteps, dt) { return need().simulate(nSteps, dt); }
function read() { return need().read(); }

module.exports = {
  Simulation: Simulation, init: init, step: step, simulate: simulate, read: read,
  load: load, deviceCount: deviceCount, planQuery: planQuery, mutualPairs: mutualPairs, TILE_SIZE: TILE_SIZE, EPS2: EPS2, DEFAULT_G: DEFAULT_G, DEFAULT_DT: DEFAULT_DT,
  get current() { return current; }, get abiVersion() { return abi; },
};
