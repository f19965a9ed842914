/*
 * nbody3d_hip.h -- C ABI of the MI355X direct N-body engine (libnbody3d_hip.so)
 *
 * This is the drop-in boundary for the ONE hot path of huj31415/nbody3d-webgpu:
 * the tiled O(N^2) force accumulation + leapfrog update that the reference runs
 * as a single WGSL compute pass.  The reference has no FFI/plugin interface for
 * it: the path sits behind the WebGPU object protocol inside nbody3d.js.  Each
 * entry point below names the piece of that protocol it replaces (file:line
 * relative to /root/reference).  INTEGRATION.md shows the N-API / ctypes binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every call returns an nb_status (0 = ok).  Nothing throws or aborts across
 *     the boundary; nb_last_error() gives the message for the last failure.
 *   - Host arrays use the reference's packed layout (nbody3d.js:49,132):
 *       bodies[4*i..] = x, y, z, mass     vel[4*i..] = vx, vy, vz, 0
 *       accel [4*i..] = ax, ay, az, 0     (acceleration of the previous step)
 *     element type float for NB_F32 sims, double for NB_F64 sims.
 *   - The engine never keeps a host pointer past the call (the reference's
 *     writeBuffer copies, nbody3d.js:186,193); it owns all device memory unless
 *     nb_config.ext_bodies is given.  nb_download fills caller-owned arrays
 *     (util.js:163-178 returns a fresh copy).
 *   - One host thread per handle at a time; distinct handles are independent.
 *   - nb_step enqueues on the engine's HIP stream and returns (the reference's
 *     queue.submit is asynchronous, nbody3d.js:490); nb_download / nb_sync block.
 */
#ifndef NBODY3D_HIP_H
#define NBODY3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built -fvisibility=hidden */
#endif

#define NB_ABI_VERSION 2u /* major: a client and a library must agree on it (nb_abi_version) */
#define NB_ABI_MINOR 4u   /* additions within major 2; a client needs nb_abi_minor() >= the minor it was written against:
                             2.1 (round 3)  nb_force_pass, nb_frame_request / nb_frame_acquire, nb_shape_info, NB_FLAG_SYM_SHARD
                             2.2 (round 4)  nb_step_times2, nb_plan_query, NB_FLAG_WHOLE_SWEEPS, nb_config.layer_budget_mib
                             2.3 (round 5)  nb_abi_minor, NB_MULTI_PEER_OVERLAP; nb_plan_info / nb_plan_query moved to nbody3d_hip_plan.h; force_variant 7 II LL 3 takes LL up to 64;
                                            nb_plan_query's table holds four words per wave instead of the W + 1 starts
                             2.4 (round 6)  nb_field_eval, nb_multi_field_eval, nb_field_request, NB_FIELD_*; NB_FLAG_SINGLE_SWEEPS (an older
                                            library ignores the bit: it runs every sweep on its own anyway)
                             2.4 (round 7)  additions WITHIN 2.4, the minor stays 4: nb_config.integrator (in the place of reserved[0]; an older
                                            library ignores it), NB_INT_*, nb_download_jerk, nb_upload_derivs, NB_JERK.  A client detects them by
                                            the presence of the symbol nb_download_jerk (dlsym), not by the minor
                             2.4 (round 8)  likewise within 2.4: nb_set_block_steps, nb_block_stats, nb_download_levels, nb_upload_levels,
                                            NB_BLOCK_*.  Detected by the presence of the symbol nb_set_block_steps
                             2.4 (round 9)  likewise within 2.4: nb_neighbors, nb_multi_neighbors, nb_neighbors_shape, nb_neighbor_request, NB_NBR_*.
                                            Detected by the presence of the symbol nb_neighbors
                             2.4 (round 10) likewise within 2.4: NB_FLAG_NO_EQM (an older library ignores the bit: it has the general kernels only),
                                            nb_eqm_info.  Detected by the presence of the symbol nb_eqm_info
                             2.4 (round 11) likewise within 2.4: NB_FLAG_NO_EQM_POW2 (an older library ignores the bit: its equal-mass kernels keep
                                            their mass product anyway), nb_eqm_form.  Detected by the presence of the symbol nb_eqm_form
                             2.4 (round 12) likewise within 2.4: nb_neighbor_lists, nb_multi_neighbor_lists, nb_neighbor_lists_shape,
                                            nb_neighbor_list_request.  Detected by the presence of the symbol nb_neighbor_lists
                             2.4 (round 13) likewise within 2.4: nb_knn, nb_multi_knn, nb_knn_shape, nb_knn_request.  Detected by the presence
                                            of the symbol nb_knn
                             2.4 (round 14) likewise within 2.4: nb_list_force, nb_multi_list_force, nb_list_force_shape,
                                            nb_list_force_request.  Detected by the presence of the symbol nb_list_force
                             2.4 (round 15) likewise within 2.4: nb_split_force, nb_multi_split_force, nb_split_force_shape,
                                            nb_split_force_request, NB_SPLIT_*.  Detected by the presence of the symbol nb_split_force
                             2.4 (round 16) likewise within 2.4: nb_set_neighbor_scheme, nb_neighbor_scheme_stats, nb_download_neighbor_scheme,
                                            nb_neighbor_scheme.  Detected by the presence of the symbol nb_set_neighbor_scheme
                             2.4 (round 17) likewise within 2.4: nb_split_lists, nb_multi_split_lists, nb_split_lists_shape,
                                            nb_split_lists_request, nb_neighbor_scheme_fused, NB_FLAG_AC_TWO_CALLS (an older library ignores
                                            the bit: its scheme runs the two calls).  Detected by the presence of the symbol nb_split_lists
                             2.4 (round 18) likewise within 2.4: nb_set_neighbor_adapt, nb_neighbor_adapt_stats, nb_download_neighbor_radii,
                                            nb_upload_neighbor_scheme, nb_neighbor_adapt, nb_neighbor_checkpoint.  Detected by the presence of
                                            the symbol nb_set_neighbor_adapt
                             2.4 (round 19) likewise within 2.4: nb_set_neighbor_levels, nb_neighbor_level_stats, nb_download_neighbor_levels,
                                            nb_upload_neighbor_levels, nb_neighbor_levels, NB_NLEV_FROZEN.  Detected by the presence of the
                                            symbol nb_set_neighbor_levels
                             2.4 (round 20) likewise within 2.4: nb_set_hermite_order, nb_hermite_order, nb_download_snap, nb_upload_derivs6.
                                            Detected by the presence of the symbol nb_set_hermite_order
                             2.4 (round 21) likewise within 2.4: nb_set_block_steps6.  Detected by the presence of the symbol
                                            nb_set_block_steps6
                             2.4 (round 22) likewise within 2.4: nb_set_start6, nb_start6, NB_START6_*.  Detected by the presence of the
                                            symbol nb_set_start6
                             2.4 (round 23) likewise within 2.4: nb_set_pass_precision, nb_pass_precision, NB_PASS_*.  Detected by the presence
                                            of the symbol nb_set_pass_precision
                             2.4 (round 24) likewise within 2.4: nb_set_pass_guard, nb_pass_guard.  Detected by the presence of the symbol
                                            nb_set_pass_guard
                             2.4 (round 25) likewise within 2.4: nb_set_block_batch, nb_block_batch_stats, nb_block_batch,
                                            NB_BLOCK_BATCH_SMALL_DEFAULT.  Detected by the presence of the symbol nb_set_block_batch
                             2.4 (round 26) likewise within 2.4: nb_set_block_batch6.  Detected by the presence of the symbol
                             2.4 (round 27) likewise within 2.4: nb_set_block_batch_mixed.  Detected by the presence of the symbol
                             2.4 (round 28) likewise within 2.4: nb_set_encounter_watch, nb_encounter_stats, nb_download_encounters,
                                            nb_upload_encounters, nb_reset_encounters, nb_encounter_watch, NB_ENC_STOP.  Detected by
                                            the presence of the symbol nb_set_encounter_watch
                             2.4 (round 29) likewise within 2.4: nb_set_block_batch_watch.  Detected by the presence of the symbol */

typedef struct nb_sim nb_sim; /* opaque */

typedef enum nb_status {
    NB_OK = 0,
    NB_ERR_INVALID = 1,   /* bad argument / bad config                       */
    NB_ERR_NO_DEVICE = 2, /* no usable HIP device (reference: nbody3d.js:151) */
    NB_ERR_HIP = 3,       /* a HIP runtime call failed                       */
    NB_ERR_STATE = 4,     /* call out of order (e.g. step before upload)     */
    NB_ERR_NOMEM = 5,
    NB_ERR_COMM = 6,      /* the exchange hook / collective failed           */
    NB_NOT_READY = 7      /* nb_frame_acquire(wait = 0): no finished frame yet */
} nb_status;

typedef enum nb_precision { NB_F32 = 0, NB_F64 = 1 } nb_precision;

/* nb_config.flags */
#define NB_FLAG_EXT_STREAM 1u /* ext_stream is meaningful even when NULL (the
                                 HIP null stream, e.g. torch's default stream) */
/* 2u was NB_FLAG_XCD_REMAP in ABI 1 (an XCD-aware workgroup mapping, measured useless for this
 * VALU-bound kernel -- profiles/r01/xcd_remap_ab.txt -- and removed); the bit is ignored. */
#define NB_FLAG_LDS_ONLY 4u  /* tuning/A-B: never pick the SGPR-broadcast force kernel */
#define NB_FLAG_NO_FUSE 8u   /* tuning/A-B: never pick the fused one-launch step (force kernel +
                                integrate kernel instead; bit-identical results) */
#define NB_FLAG_POISON 16u   /* validation: the j-packed step (K = 6) overwrites every partial sum with NaN
                                once its i-block is reduced, so a partial that is ever read stale (a missing
                                release / acquire between workgroups) shows as NaN instead of a small error */

#define NB_FLAG_JPK_FENCED 32u /* the j-packed step (K = 6) hands its partial sums between workgroups with a plain store +
                                  agent-scope RELEASE on the ticket (the form the compiler's memory model guarantees on any
                                  part / partition mode) instead of write-through (sc1) stores + a relaxed ticket: the
                                  conservative fallback, 2-8 us per step slower; bit-identical results */

#define NB_FLAG_NO_SYM 64u     /* tuning/A-B: never pick the symmetric force pass (K = 7: each unordered pair once, both
                                  accelerations), i.e. keep the ordered-pair kernels of ABI 2 at every size */

#define NB_FLAG_SYM_SHARD 128u  /* a SHARD handle (shard_count != 0) may take the rank form of the symmetric force pass: the rank
                                  sweeps the pair lists of its own rows only -- every unordered pair of the system is evaluated
                                  by exactly one rank -- and the ranks reduce-scatter their partial accelerations before the
                                  integrate kernel.  The reduce-scatter is the engine's own (nb_rccl_attach: in-place
                                  ncclReduceScatter; nb_multi sets this flag itself): nb_step fails with NB_ERR_STATE on such a
                                  handle until a communicator is attached.  Needs shard rows that are whole super-blocks
                                  (shard_begin, shard_count and n multiples of 1,024, or of 512); ignored otherwise */

#define NB_FLAG_WHOLE_SWEEPS 256u /* tuning/A-B: the symmetric pass cuts its wave ranges at whole chunk-sweeps (64 rotation steps), as in
                                   ABI 2.0; by default systems with few sweeps per wave cut them in quarter sweeps (variant suffix
                                   "_u4"), which evens out the SIMDs' work (N = 16,384: the longest SIMD runs 4.25 sweeps instead of 5) */

#define NB_FLAG_SINGLE_SWEEPS 512u /* tuning/A-B: the wave-granular symmetric pass (f32, one traveler per lane) runs every chunk-sweep on its
                                    own, as before ABI 2.4's paired sweeps (two whole sweeps rotate together: 14 instead of 20 lane
                                    moves per two traveler-steps).  Same plan, same layers; sums differ in the order of additions */

#define NB_FLAG_NO_EQM 1024u /* tuning/A-B: never run the equal-mass kernels of the symmetric pass.  A whole-system f32 handle of the
                                wave-granular form whose plan has no padding rows runs them while every bodies.w holds the same bits and
                                every vel.w and accel.w is zero (nb_upload decides; after nb_device_ptr the next step looks again): one
                                G*m product per pair instead of two, no mass lane rotated.  Bit-identical results (nb_eqm_info) */

#define NB_FLAG_NO_EQM_POW2 2048u /* tuning/A-B: the equal-mass kernels keep their G*m product per pair (form 1) even where the system's
                                     one G*m is a power of two.  By default such a system -- N-body units with N = 2^k bodies: m = 2^-k --
                                     runs the equal-mass kernels with UNIT mass product (form 2): the sums are kept unscaled and G*m
                                     multiplies each row once, where it is stored; a product by a power of two commutes with every
                                     rounding, so the results are bit-identical (nb_eqm_form) */

#define NB_FLAG_AC_TWO_CALLS 4096u /* tuning/A-B: a list build of the Ahmad-Cohen neighbour scheme (nb_set_neighbor_scheme) always runs
                                      nb_split_force and then nb_neighbor_lists.  By default it runs nb_split_lists -- the sums and the
                                      rows from one pass over the pairs -- wherever that call's launch shape is nb_split_force's.
                                      Bit-identical results (nb_neighbor_scheme_fused) */

/* nb_array: selector for nb_device_ptr */
typedef enum nb_array { NB_BODIES = 0, NB_VEL = 1, NB_ACCEL = 2, NB_JERK = 3 /* Hermite handles only */ } nb_array;

/* nb_config.integrator (no reference analogue: the reference has the one lagged leapfrog, nbody3d.js:274-290) */
typedef enum nb_integrator { NB_INT_LEAPFROG = 0, NB_INT_HERMITE4 = 1 } nb_integrator;

/*
 * Engine configuration.  Replaces: buffer creation (nbody3d.js:179-204), the
 * constants TILE_SIZE (:4) and the hard-coded softening 1e-4 (:234).
 * Zero-initialise, set struct_size = sizeof(nb_config), then fill what you need;
 * zero fields take the defaults noted.
 */
typedef struct nb_config {
    uint32_t struct_size;  /* sizeof(nb_config), for ABI evolution             */
    uint32_t n;            /* total bodies N (any 1 <= N <= 2^30; reference is only
                              defined for N % 256 == 0)        */
    uint32_t precision;    /* nb_precision; default NB_F32                     */
    uint32_t tile;         /* j-tile staged in LDS; 0 -> 256 (nbody3d.js:4)    */
    double eps2;           /* Plummer softening; 0 -> 1e-4 (nbody3d.js:234).
                              Must be > 0 (the self term relies on it)         */
    int32_t device;        /* HIP device ordinal; -1 -> current device         */
    /* i-shard owned by this handle.  The handle integrates
     * bodies [shard_begin, shard_begin+shard_count) against ALL n bodies and
     * keeps vel/accel only for its shard.  shard_count == 0 -> whole system.   */
    uint32_t shard_begin;
    uint32_t shard_count;
    /* Optional: run on a caller-owned hipStream_t (e.g. torch's current
     * stream) instead of a private one.  Used when non-NULL or when
     * NB_FLAG_EXT_STREAM is set.                                               */
    void *ext_stream;
    /* Optional: caller-owned DEVICE buffer of 4*n elements used as the
     * replicated bodies array (so a host framework can run its collective
     * directly on it).  NULL -> engine allocates.                              */
    void *ext_bodies;
    /* Force-kernel launch shape overrides for tuning; 0 -> engine heuristics.  */
    uint32_t force_variant; /* 6 decimal digits K II LL X: K = 1 scalar loop, 2 packed f32 with
                               the j-tile in LDS, 3 packed f32 with j broadcast from SGPRs,
                               4 fused one-launch step (packed, LDS tile), 5 the same with the
                               j-bodies in registers (N <= 1,024 * X; II = 02, LL = 64); II = bodies per
                               lane (01..08); LL = lanes sharing a body (01..64); X = tile
                               units (256 bodies) per LDS stage (K = 2, 4: 1, 4 or 8) or waves splitting j
                               (K = 3: 1 or 4; 5 = 4 waves with 64-bit pair loads).  E.g. 402644.
                               K = 6: fused step with two j-bodies per packed instruction streamed
                               from a pair-transposed copy of the positions (II = 01, LL = 01;
                               X = waves per workgroup splitting j: 4, 8, or 6 for 16); jsplit > 1
                               splits j over workgroups too (reduced in the same launch).
                               K = 7: the symmetric force pass (whole-system f32 handles): every unordered pair is
                               evaluated once and both accelerations accumulated; II = resident bodies per lane (08
                               or 16), LL = 01 (02 / 04 / 08: wave ranges cut in half / quarter / eighth sweeps whatever the size),
                               X = 3 / 1: wave-granular form with 1 / 2 traveling bodies per lane
                               (jsplit = waves per SIMD), X = 4: workgroup form (II = 08; jsplit = segments per
                               super-block).  E.g. 716013.
                               See nb_variant_name().                              */
    uint32_t jsplit;        /* number of j-partitions (grid.y)                  */
    uint32_t flags;         /* NB_FLAG_*                                        */
    uint32_t layer_budget_mib; /* most device memory (MiB) the symmetric pass may take for its partial-sum layers
                               (~ 6 N^2 / S bytes, S = 512 or 1,024 rows: 6.4 GB at N = 1,048,576); a system whose
                               layers would not fit runs the ordered-pair kernels instead.  0 -> a third of the
                               device's memory, at most 96 GiB (N up to ~4 M on an MI355X).  nb_create also checks
                               the memory that is FREE: a whole-system handle whose layers would not fit it falls back
                               the same way (a rank-form shard fails instead: its peers expect the reduce-scatter) */
    uint32_t integrator;    /* nb_integrator; 0 -> NB_INT_LEAPFROG, the reference's scheme.  NB_INT_HERMITE4: see "Hermite handles"
                               below (no reference analogue).  Takes the place of reserved[0]: sizeof(nb_config) is unchanged, and a
                               struct_size that ends in front of this field reads it as 0 */
    uint32_t reserved[3];
} nb_config;

/* Library / ABI version; callable with no device. */
uint32_t nb_abi_version(void);
uint32_t nb_abi_minor(void);   /* NB_ABI_MINOR of the library */

/* Number of visible HIP devices (0 when there is none; never fails). */
int nb_device_count(void);

/* create: nbody3d.js:179-204 (three 16*N-byte buffers + uniform block) and
 * :296-311 (pipeline + bind group).  *out is NULL on failure; the message is
 * then available from nb_last_error(NULL). */
int nb_create(const nb_config *cfg, nb_sim **out);

/* destroy: the reference never frees (util.js:72-73 commented out). */
void nb_destroy(nb_sim *s);

/* upload: queue.writeBuffer of bodyData / velData (nbody3d.js:186,193) and the
 * checkpoint restore (util.js:230-244).  bodies and vel hold 4*n elements
 * (whole system, every rank passes the same arrays); accel may be NULL -> zeros
 * (WebGPU zero-initialises accelBuffer, nbody3d.js:195-199). */
int nb_upload(nb_sim *s, const void *bodies, const void *vel, const void *accel);

/* set_params: uni.dtValue / uni.GValue + per-frame queue.writeBuffer of the
 * uniform block (nbody3d.js:470,516-517; util.js:45,53). */
int nb_set_params(nb_sim *s, double dt, double G);

/* step: `if (dt > 0)` compute pass + submit (nbody3d.js:474-480,489-490),
 * nsteps times back to back.  dt <= 0 -> no-op, state untouched (:474). */
int nb_step(nb_sim *s, uint32_t nsteps);

/* download: exportSimulation's three readBuffer() copies (util.js:163-178).
 * Blocks until all enqueued steps are done.  Any pointer may be NULL (skipped).
 * bodies receives all 4*n elements; vel/accel receive the 4*n-element arrays
 * with only this handle's shard rows filled (others untouched). */
int nb_download(nb_sim *s, void *bodies, void *vel, void *accel);

/* sync: await device idle (the mapAsync await of util.js:174). */
int nb_sync(nb_sim *s);

/* Message for the last failed call on s (s == NULL: last failed nb_create on
 * this thread).  Never NULL; valid until the next call on the same handle. */
const char *nb_last_error(nb_sim *s);

/* ---- multi-GPU support (no reference analogue) ----------- */

/* Device address of a state array (bodies: 4*n elements, replicated;
 * vel/accel: 4*shard_count elements).  Valid until the next nb_step: a fused handle
 * ping-pongs between two position buffers, a jsplit = 1 handle swaps accel buffers. */
int nb_device_ptr(nb_sim *s, int which /* nb_array */, void **out);

/* Exchange hook: called on the calling thread once per step, after the
 * integrate kernel has been ENQUEUED for this handle's shard, with the stream
 * the work was enqueued on.  The hook must make bodies[shard rows of every
 * other rank] current on that stream (an all-gather of position rows) before
 * returning control, and return 0 on success.  NULL -> no exchange (single
 * shard).  The reference has no collective; this is where RCCL plugs in. */
typedef int (*nb_exchange_fn)(void *user, void *bodies_dev, size_t elem_size,
                              uint32_t n, uint32_t shard_begin,
                              uint32_t shard_count, void *hip_stream);
int nb_set_exchange(nb_sim *s, nb_exchange_fn fn, void *user);

/* Overlapped (two-phase) exchange.  begin() is called where the one-phase hook
 * would be (after the integrate kernel is enqueued) and must START the
 * all-gather without making the engine stream wait for it; wait() is called
 * before the engine enqueues work that reads other ranks' rows and must make
 * `hip_stream` wait for the gather begin() started.  Between the two the engine
 * enqueues the next step's force work on the j-range of its OWN rows (which the
 * gather does not touch), hiding the collective behind 1/world of the force
 * pass.  Falls back to calling wait() right after begin() when the j-splits do
 * not line up with the shard boundaries.  Replaces any one-phase hook. */
typedef int (*nb_exchange_wait_fn)(void *user, void *hip_stream);
int nb_set_exchange_overlapped(nb_sim *s, nb_exchange_fn begin, nb_exchange_wait_fn wait, void *user);

/* ---- native RCCL collective, one process per GPU (SURVEY.md §8(e) "Collective") -----------
 * Instead of an exchange hook the engine itself issues the per-step all-gather of position
 * rows: ncclAllGather, in place (send pointer = bodies + rank * rows), on the engine's stream
 * right after the integrate kernel -- no host code between the kernels of a step.  The host
 * only transports the 128-byte ncclUniqueId from rank 0 to the other ranks (any channel).
 * Every rank owns the same number of rows: n == nranks * shard_count and
 * shard_begin == rank * shard_count (pad with zero-mass rows).  librccl is loaded on first
 * use (dlopen; a copy already loaded into the process -- e.g. PyTorch's -- is reused). */
#define NB_RCCL_ID_BYTES 128
#define NB_RCCL_OVERLAP 1u /* all-gather on its own stream, hidden behind the next step's force
                              work on the rank's OWN j-range (see nb_set_exchange_overlapped) */
int nb_rccl_unique_id(void *id_out /* NB_RCCL_ID_BYTES */);
int nb_rccl_attach(nb_sim *s, const void *id, int nranks, int rank, uint32_t flags);
int nb_rccl_detach(nb_sim *s);
/* Communicator facts for reports: ncclCommCount / ncclCommUserRank and RCCL's version code
 * (0 when no communicator is attached). */
int nb_rccl_info(nb_sim *s, int *nranks, int *rank, int *rccl_version);

/* ---- single-process multi-device (for hosts that cannot run one process per
 *      GPU, e.g. Node; no reference analogue) --------------------------------
 * nb_multi_* wraps n_shards shard handles: shard k owns a contiguous block of
 * rows (256-aligned; the system is padded with zero-mass rows at the origin,
 * which exert and feel exactly nothing) on device devices[k].  After every
 * step each shard pulls the other shards' new rows straight into its
 * replicated bodies array (one pull kernel per shard over peer-mapped memory,
 * ordered with HIP events; g*(g-1) device-to-device copies when peer access is
 * missing): on the fully connected xGMI fabric of an 8-GPU node every transfer
 * has its own link, which is the all-gather the topology wants.  f32 / f64
 * systems with >= 2,048 rows per shard divide the PAIRS instead of the rows (rank
 * form of the symmetric force pass, see NB_FLAG_SYM_SHARD) and reduce-scatter
 * their partial accelerations the same way before the integrate kernel.  devices == NULL
 * -> round-robin over the visible devices; several shards may share a device
 * ("virtual shards": the way the partition logic is tested on one GPU).
 * Host arrays hold the UNPADDED n rows, exactly as for a single handle. */
typedef struct nb_multi nb_multi; /* opaque */
int nb_multi_create(const nb_config *cfg, uint32_t n_shards, const int32_t *devices, nb_multi **out);
void nb_multi_destroy(nb_multi *m);
int nb_multi_upload(nb_multi *m, const void *bodies, const void *vel, const void *accel);
int nb_multi_set_params(nb_multi *m, double dt, double G);
int nb_multi_step(nb_multi *m, uint32_t nsteps);
int nb_multi_download(nb_multi *m, void *bodies, void *vel, void *accel);
int nb_multi_sync(nb_multi *m);
const char *nb_multi_last_error(nb_multi *m);
/* Energy / momentum of the whole system: sum of the shards' nb_diagnostics (same out[5]). */
int nb_multi_diagnostics(nb_multi *m, double out[5]);
/* Name of shard 0's force-kernel variant (all shards resolve to the same shape). */
const char *nb_multi_variant_name(nb_multi *m);
/* How the shards exchange their new rows after a step:
 *   NB_MULTI_PEER  g*(g-1) hipMemcpyAsync device-to-device copies ordered by HIP events (default);
 *   NB_MULTI_RCCL  ncclCommInitAll over the shards' devices once, then per step
 *                  ncclGroupStart / in-place ncclAllGather on every shard's stream / ncclGroupEnd
 *                  (SURVEY.md §8(e)).  Needs every shard on its own device.
 *   NB_MULTI_PEER_OVERLAP  (ABI 2.3; rank form of the symmetric pass with pull kernels) the all-gather pull of step n runs on a
 *                  second stream per shard while step n + 1 sweeps the pairs whose travelers are the shard's own rows; the shard's
 *                  stream waits for its pull only in front of the sweeps that read the other shards' rows -- what NB_RCCL_OVERLAP
 *                  does across processes, here with real rows in flight between g shards (also g virtual shards on ONE device:
 *                  the multi-rank check of the overlapped protocol a one-GPU box can run).  Falls back to NB_MULTI_PEER's order
 *                  when the handle is not in the rank form or G != 1.
 * Results are bit-identical; the choice is a measured A/B. */
typedef enum nb_multi_collective { NB_MULTI_PEER = 0, NB_MULTI_RCCL = 1, NB_MULTI_PEER_OVERLAP = 2 } nb_multi_collective;
int nb_multi_set_collective(nb_multi *m, int mode /* nb_multi_collective */);
/* mode in use, communicator size (0 for NB_MULTI_PEER), RCCL version code. */
int nb_multi_collective_info(nb_multi *m, int *mode, int *nranks, int *rccl_version);

/* ---- measurement (role of TimingHelper, util.js:297-423) ------------------- */

/* When enabled, each nb_step records HIP events around every force-kernel and
 * integrate-kernel launch on the engine stream.  nb_kernel_times then blocks
 * for them and returns the averages since the last call (milliseconds) and the
 * number of launches averaged; it resets the accumulators. */
int nb_enable_timing(nb_sim *s, int on);
int nb_kernel_times(nb_sim *s, double *force_ms, double *integrate_ms,
                    uint32_t *launches);
/* Same, plus the average time of the native RCCL collectives of a step (the position all-gather and, for the
 * rank form of the symmetric pass, the reduce-scatter of the partial accelerations before it; 0 when none ran).
 * A fused one-launch step reports its whole kernel as force_ms and 0 for integrate_ms. */
int nb_step_times(nb_sim *s, double *force_ms, double *integrate_ms, double *exchange_ms,
                  uint32_t *launches);
/* The full breakdown of a step, part by part as the engine stream runs them (averages over the recorded steps,
 * milliseconds): force pass [rank form: nb_sym_reduce, ncclReduceScatter] integrate [ncclAllGather].  span_ms is
 * the time from the first event of a step to its last one, so force + sym_reduce + reduce_scatter + integrate +
 * allgather = span - (idle gaps between the kernels).  An overlapped all-gather (NB_RCCL_OVERLAP) runs on its own
 * stream and is not timed: allgathers = 0.  Set struct_size = sizeof(nb_step_timing) before the call.
 * (No reference analogue: TimingHelper times one pass, util.js:297-423; the reference is single-device.) */
typedef struct nb_step_timing {
    uint32_t struct_size;
    uint32_t launches;              /* steps averaged */
    double force_ms;                /* the force kernel (both launches of an overlapped step) */
    double sym_reduce_ms;           /* rank form: this rank's sums for every row (nb_sym_reduce) */
    double reduce_scatter_ms;       /* rank form: in-place ncclReduceScatter of those sums */
    double integrate_ms;
    double allgather_ms;            /* in-place ncclAllGather of the new positions on the engine stream */
    double span_ms;
    uint32_t reduce_scatters;       /* steps whose reduce-scatter was timed */
    uint32_t allgathers;            /* steps whose all-gather was timed */
} nb_step_timing;
int nb_step_times2(nb_sim *s, nb_step_timing *out);
/* Runs ONLY the integrate kernel `reps` times back to back on the state as it stands (the
 * force sums are whatever the last force pass left; first zeroed if none ran) and returns
 * the average launch time: the memory-bound kernel measured on its own at sizes where a
 * full O(N^2) step would take minutes (N >= 4M: state no longer cache-resident).  The
 * particle state is garbage afterwards -- measurement only; not available on a fused handle.
 * A rank-form handle (NB_FLAG_SYM_SHARD shard, or a whole system whose ring distances go in passes) runs what its step runs:
 * the plain integrate kernel on its rows of the reduced sums. */
int nb_integrate_pass(nb_sim *s, uint32_t reps, double *avg_ms);
/* Runs ONLY the force pass `reps` times back to back on the positions as they stand and returns the average time per pass
 * (a rank-form handle: both phases of the force kernel + nb_sym_reduce).  The state is left untouched (the pass writes partial
 * sums only).  Measurement: what ONE rank of an N-rank partition spends in its force pass can be timed on a single GPU
 * without a communicator -- create the shard handle (shard_begin / shard_count, NB_FLAG_SYM_SHARD), upload, call this. */
int nb_force_pass(nb_sim *s, uint32_t reps, double *avg_ms);

/* Name of the force-kernel variant a handle resolved to (for reports), e.g.
 * "f32pk_fused_lds1024_ipl2_ls64" or "f32pk_sgpr_ipl8_ws4_js8".  Valid until nb_destroy. */
const char *nb_variant_name(nb_sim *s);

/* Launch-shape facts of a handle (for reports and tests): the number of j-partitions the force pass runs
 * (grid.y), the bodies per partition, and which partitions lie ENTIRELY inside the handle's own rows -- the
 * part of the next force pass that the overlapped exchange (NB_RCCL_OVERLAP / nb_set_exchange_overlapped)
 * issues before it waits for the other ranks' rows.  own_splits == 0 means the overlapped forms degenerate to
 * begin-then-wait on this handle.  Any out pointer may be NULL. */
int nb_shape_info(nb_sim *s, uint32_t *jsplit, uint32_t *j_per_split, uint32_t *own_split0,
                  uint32_t *own_splits);

/* Whether the next force pass of the handle runs the equal-mass kernels (NB_FLAG_NO_EQM): *eqm = 1 or 0.  Decides it first if a
 * pointer was handed out since it was last known (one small launch and a wait on the handle's stream).  0 before nb_upload. */
int nb_eqm_info(nb_sim *s, int *eqm);

/* Which form of the force kernels the next force pass of the handle runs: *form = 0 the general kernels, 1 the equal-mass kernels, 2 the
 * equal-mass kernels with unit mass product.  Form 2 runs where nb_eqm_info answers 1 and the scalar the kernels stream as G*m -- row 0's
 * mass when G = 1, else (float)G * mass -- is a positive normal power of two with an exponent in [-32, 32] (NB_FLAG_NO_EQM_POW2 keeps
 * form 1); it follows the G of the last nb_set_params.  Decides the equal-mass state first, as nb_eqm_info does.  0 before nb_upload. */
int nb_eqm_form(nb_sim *s, int *form);

/* Planner introspection (the launch plan nb_create WOULD build for a configuration, with the symmetric pass's kernel-internal
 * plan words and tables: for reports, sizing runs and the host-side planner tests) lives in nbody3d_hip_plan.h -- nothing a host
 * that replaces nbody3d.js:179-204,470-490 needs. */

/* ---- Hermite handles (nb_config.integrator = NB_INT_HERMITE4; no reference analogue) --------------------
 * The 4th-order Hermite predictor-corrector of Makino & Aarseth (1992) with one shared step dt, on the force and its time
 * derivative, the jerk:
 *     a_i = sum_j G m_j dr / rho^3          j_i = sum_j G m_j [ dv / rho^3 - 3 (dr.dv) dr / rho^5 ]
 *     dr = x_j - x_i,  dv = v_j - v_i,  rho^2 = |dr|^2 + eps2
 *   - State: bodies = (x, y, z, m) and vel = v, BOTH AT THE SAME INSTANT t (no lag: nb_diagnostics and nb_field_eval describe one
 *     instant).  accel = a(t) and jerk = j(t) are DERIVED quantities.
 *   - The derived arrays go stale with: nb_upload (its accel argument is ignored on a Hermite handle), nb_device_ptr(NB_BODIES) or
 *     nb_device_ptr(NB_VEL) (the caller may write through them), a change of G since they were evaluated.  They are refreshed by
 *     the next nb_step, nb_download with accel != NULL, nb_download_jerk, nb_device_ptr(NB_ACCEL / NB_JERK): each first evaluates
 *     them on the state as it stands with one force+jerk pass on the handle's stream (needs nb_set_params: G).
 *   - One step, h = dt:
 *         xp = x + h v + h^2/2 a + h^3/6 j          vp = v + h a + h^2/2 j
 *         (a1, j1) = FJ(xp, vp)                     -- the only O(N^2) pass of the step
 *         v1 = v + h/2 (a + a1) + h^2/12 (j - j1)
 *         x1 = x + h/2 (v + v1) + h^2/12 (a - a1)
 *         state <- (x1, v1, a1, j1)
 *     The mass lane and vel.w are carried unchanged; accel.w = jerk.w = 0.  Note that the (a, j) a step leaves behind were
 *     evaluated at the PREDICTED state: a restore that recomputes them from (x, v) continues within the scheme's accuracy but not
 *     bit-identically -- nb_upload_derivs is the bit-exact checkpoint path.
 *   - dt <= 0 is a no-op, as for leapfrog; dt may change between steps; G may change (the derivatives are then re-evaluated).
 *   - Deterministic: fixed summation order, no atomics; the same state and dt give the same bits; nb_step(k) is bit-identical to
 *     k x nb_step(1) (plain launches; Hermite steps are not graph-captured).
 *   - Restrictions, each NB_ERR_INVALID from nb_create before any device call, the message naming the field: an unknown integrator
 *     value; integrator = 1 with shard_count != 0, with ext_bodies, with force_variant != 0 or with jsplit != 0.  nb_multi_create
 *     and nb_plan_query with integrator != 0: NB_ERR_INVALID.  nb_set_exchange, nb_set_exchange_overlapped, nb_rccl_attach and
 *     nb_integrate_pass on a Hermite handle: NB_ERR_STATE.  The tuning flags are ignored; ext_stream works.
 *   - nb_diagnostics, nb_field_eval, nb_frame_request / nb_frame_acquire work unchanged (they read bodies and vel only).
 *     nb_force_pass runs the force+jerk pass (kernel + reduce) into scratch: state and derivatives untouched.  nb_enable_timing /
 *     nb_step_times2: force_ms = the force+jerk kernel and its reduce, integrate_ms = predictor + corrector.  nb_variant_name starts
 *     with "hermite4_"; nb_shape_info reports the j-chunks of the force+jerk pass and the bodies per chunk.
 *   - Leapfrog handles: nb_download_jerk, nb_upload_derivs and nb_device_ptr(NB_JERK) return NB_ERR_STATE. */

/* download_jerk (no reference analogue): fills 4*n elements (jx, jy, jz, 0), element type of the handle's precision; blocks. */
int nb_download_jerk(nb_sim *s, void *jerk);

/* upload_derivs (no reference analogue): the checkpoint restore of a Hermite handle.  Both pointers are required, 4*n elements
 * each; valid after nb_upload.  Marks the handle's derivatives as current (for the G in force, or the G of the next nb_set_params
 * when none was made yet), so the next step continues bit-identically from a (bodies, vel, accel, jerk) read with nb_download +
 * nb_download_jerk. */
int nb_upload_derivs(nb_sim *s, const void *accel, const void *jerk);

/* ---- block individual time steps on a Hermite handle (no reference analogue) ----------------------------
 * With one shared step a single tight pair puts the whole system on the pair's step.  nb_set_block_steps gives every body a step
 * of its own, dt / 2^l_i with a LEVEL l_i in [min_level, max_level] (Makino & Aarseth 1992; NBODY4/6, phi-GPU): at every block
 * time only the bodies due there get a new force+jerk, against the predicted positions of all the others.
 *   - nb_step(s, k) still advances the system by exactly k x dt (dt of nb_set_params): k OUTER steps, after each of which all bodies
 *     are at the same instant.  nb_download, nb_download_jerk, nb_diagnostics, nb_field_eval, nb_frame_request / nb_frame_acquire,
 *     nb_device_ptr and nb_upload_derivs keep their meaning; dt <= 0 is a no-op.  nb_step(k) equals k x nb_step(1) bit for bit, two
 *     handles give the same bits, and (bodies, vel, accel, jerk, levels) uploaded into a fresh handle (nb_upload, nb_upload_derivs,
 *     nb_set_block_steps, nb_upload_levels) continues bit-identically.
 *   - The scheme.  L = max_level, tick = dt / 2^L, body i steps by s_i = 2^(L - l_i) ticks.  level_for(tau) is the smallest l in
 *     [min_level, L] with dt / 2^l <= tau; if there is none it is L and the decision counts as `clamped`.
 *     Start (levels not current): (a, j) are made current, then l_i = level_for((eta / 2) |a_i| / |j_i|); |j_i| = 0 gives min_level.
 *     An outer step sets t_i = 0 for all bodies and repeats until t_next == 2^L:
 *       1. t_next = min_i (t_i + s_i), the active set A = { i : t_i + s_i == t_next };
 *       2. EVERY body is predicted from its own (x, v, a, j) at t_i over (t_next - t_i) ticks (the predictor polynomial of a
 *          shared step, fp64, rounded once) -- always from the stored state, never from an earlier prediction;
 *       3. (a1, j1) of i in A against all n predicted rows (the self term is exactly 0);
 *       4. i in A is corrected over h = s_i ticks with the corrector of a shared step: (x, v, a, j)_i <- (x1, v1, a1, j1);
 *       5. a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2, a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3, a2e = a2 + h a3,
 *          tau = sqrt(eta (|a1| |a2e| + |j1|^2) / (|j1| |a3| + |a2e|^2)), inf when the denominator is 0; a1 and j1 as stored
 *          (rounded to the handle's precision); all of this in fp64;
 *       6. unless NB_BLOCK_FROZEN: want = level_for(tau); want >= l_i is taken (refining by any depth); want < l_i coarsens by ONE
 *          level, and only if t_next is a multiple of 2 s_i; otherwise l_i stays;
 *       7. t_i = t_next.
 *   - The levels go stale with everything that stales the derivatives (nb_upload, nb_device_ptr(NB_BODIES / NB_VEL)), with a change of
 *     dt or G and with nb_set_block_steps; stale levels are re-initialised by the start rule at the next nb_step or
 *     nb_download_levels.  With NB_BLOCK_FROZEN stale levels put every body at min_level.
 *   - HOST SYNCHRONISATION (this first version's design).  nb_step on a block handle synchronises with the device ONCE PER BLOCK STEP:
 *     the host reads a small header (active count, next block time) from pinned memory and sizes the next launches by it; the
 *     clamp count and the finest level stay on the device until nb_block_stats asks.  Such a step cannot be captured into a
 *     caller's graph; ext_stream keeps working otherwise.  nb_set_block_batch (below) lets block steps with a small active set run
 *     from the device's own header, many of them per host wait.
 *   - nb_force_pass still runs the full N x N pass into scratch.  nb_enable_timing / nb_step_times2 report one OUTER step per launch:
 *     force_ms is its whole span, integrate_ms = 0 (as on a fused handle).  nb_variant_name is unchanged.
 *   - binary32 handles store the state, a and j in binary32: below steps of about dt / 2^10 (Plummer units) a3 is rounding noise and
 *     the criterion degrades towards smaller steps -- safe, but slower.  Deep hierarchies belong on NB_F64 handles (whose
 *     pass may run in binary32 on double-single differences: nb_set_pass_precision below).
 *   - Leapfrog handles: all four calls return NB_ERR_STATE.  A NULL handle, a wrong struct_size, max_level > 30, min_level >
 *     max_level, eta <= 0 or NaN, unknown flag bits, an uploaded level outside [min_level, max_level]: NB_ERR_INVALID, with a message
 *     that names the function and the field. */
#define NB_BLOCK_FROZEN 1u  /* levels stay as initialised / uploaded: no step-size decisions */
typedef struct nb_block_steps {
    uint32_t struct_size;   /* sizeof(nb_block_steps) */
    uint32_t max_level;     /* finest step = dt / 2^max_level; 0 -> 20; at most 30 */
    uint32_t min_level;     /* coarsest step = dt / 2^min_level; <= max_level */
    uint32_t flags;         /* NB_BLOCK_* */
    double   eta;           /* accuracy parameter; 0 -> 0.02; must be > 0 */
} nb_block_steps;
/* set_block_steps: switches a Hermite handle to block steps (or re-configures them); NULL: back to one shared step.  The state and
 * the derivatives stay; the levels go stale. */
int nb_set_block_steps(nb_sim *s, const nb_block_steps *cfg /* NULL: back to one shared step */);

/* (a struct TAG without a typedef: the function below carries the same name, and in C a typedef name and a function share one name
 * space, a tag does not.  Write `struct nb_block_stats` in C and in C++.) */
struct nb_block_stats {
    uint32_t struct_size, enabled;
    uint64_t outer_steps, block_steps, body_steps;  /* body_steps = sum of active bodies over the block steps */
    uint64_t clamped;                               /* decisions that wanted a step finer than dt / 2^max_level */
    uint32_t finest_level, reserved;                /* deepest level any body held since the last reset */
};
/* block_stats: the counters since the last reset (set out->struct_size); blocks.  reset != 0 zeroes them after the read.  A Hermite
 * handle without block steps reports enabled = 0 and zeros. */
int nb_block_stats(nb_sim *s, struct nb_block_stats *out, int reset);
/* download_levels / upload_levels: n bytes, one level per body.  Both need block steps switched on and an uploaded state
 * (NB_ERR_STATE otherwise).  upload_levels is the last call of a checkpoint restore. */
int nb_download_levels(nb_sim *s, uint8_t *levels /* n */);       /* blocks; initialises the levels first if they are not current */
int nb_upload_levels(nb_sim *s, const uint8_t *levels /* n */);   /* after nb_upload (+ nb_upload_derivs): marks the levels current */

/* ---- batched block steps (round 25): small block steps sized on the device, many per host wait ----------------------------------
 * An opt-in mode of order-4 block-step handles with the native pass.  The scheme of an outer step is the one above (1-7); only who
 * sizes the launches changes.  A SLOT is the launches of one block step with every grid fixed by (n, small_max, CU count): it
 * schedules, predicts every body and reads the header on the device.
 *   - 0 < |A| <= small_max and t_next != 2^L: the slot runs a SMALL step -- a force+jerk pass and a corrector shaped for a small set
 *     (kernels/block_batch.hip.h); criterion, new levels and due are the block corrector's arithmetic.
 *   - otherwise the slot PARKS: its schedule and prediction stand, every later slot of the batch is idle, and after its wait the
 *     host runs that block step through the existing gathered path (a HOST step).  t_next == 2^L always parks: a batch never
 *     crosses an outer step.
 *   The host enqueues up to `depth` slots and waits ONCE per batch.  How many it enqueues is a function of what it has read so far
 *   (one slot after nb_set_block_batch and after the levels went stale; then up to the next tick expected to park); no stored bit
 *   and no nb_block_stats counter depends on it or on depth.
 *   - With a fixed small_max, state, derivatives, levels and nb_block_stats do not depend on depth or on where batches end: nb_step(k)
 *     equals k x nb_step(1), and a checkpoint (bodies, vel, accel, jerk, levels) restored by nb_upload, nb_upload_derivs,
 *     nb_set_block_steps, nb_set_block_batch (same small_max, any depth), nb_upload_levels continues bit-identically.
 *   - small_max = 0 is legal: no small steps, every block step is a host step, and every bit is that of a handle with the mode off.
 *   - What a small step computes for a body depends on the predicted arrays and on n alone (its j-chunks are a function of n and
 *     the CU count), not on |A|, on the body's place in the active list, on small_max or on depth.
 *   - Which path a block step takes depends on small_max, and the two passes add in different orders: results for DIFFERENT small_max
 *     agree to the pass's accuracy, not bit for bit.
 *   - nb_block_stats keeps its meaning: block_steps and body_steps count small and host steps alike.  The header checks of nb_step
 *     (NB_ERR_HIP with the numbers) apply at every wait.  nb_enable_timing, dt <= 0, stale levels, nb_download_levels /
 *     nb_upload_levels, nb_force_pass and ext_stream are unchanged.
 *   - nb_set_block_batch touches no state, no derivatives and no levels (none goes stale) and takes effect from the next nb_step.
 *     NB_ERR_STATE (the message names the function and the reason): a leapfrog handle, a handle without nb_set_block_steps, an
 *     order-6 handle, a handle with nb_set_pass_precision(NB_PASS_MIXED) (its mode: nb_set_block_batch_mixed below).  While the
 *     mode is on, nb_set_hermite_order(6) and nb_set_pass_precision(NB_PASS_MIXED) return NB_ERR_STATE; nb_set_block_steps(NULL)
 *     switches the mode off too, a non-NULL reconfiguration keeps it.  NB_ERR_INVALID (naming the field): a NULL handle, a wrong
 *     struct_size, depth > 1024, small_max > 1024 other than NB_BLOCK_BATCH_SMALL_DEFAULT, flags != 0. */
#define NB_BLOCK_BATCH_SMALL_DEFAULT 0xffffffffu  /* small_max: the default (256); 0 itself means "no small steps" */
typedef struct nb_block_batch {
    uint32_t struct_size;  /* sizeof(nb_block_batch) */
    uint32_t depth;        /* most block-step slots enqueued per host wait; 0 -> 32; at most 1,024 */
    uint32_t small_max;    /* a block step with |A| <= small_max (and t_next != 2^L) runs as a small step; at most 1,024; 0: no small
                              steps; NB_BLOCK_BATCH_SMALL_DEFAULT: 256 */
    uint32_t flags;        /* must be 0 */
} nb_block_batch;
int nb_set_block_batch(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);

/* nb_set_block_batch6 (round 26): the same mode on order-6 handles with nb_set_block_steps6 on -- NB_F64 handles with dynamic or
 * frozen levels, NB_F32 handles with NB_BLOCK_FROZEN.  A separate entry point, as nb_set_block_steps6 is beside nb_set_block_steps:
 * nb_set_block_batch(non-NULL) on an order-6 handle stays NB_ERR_STATE.  The struct, the defaults, the slot protocol, the host's
 * policy and nb_block_batch_stats (enabled = 1 while either mode is on) are the ones above; inside a slot the scheme is
 * nb_set_block_steps6's (steps 1-7): the order-6 predictor, a small force+jerk+snap pass (kernels/block_batch6.hip.h) and the order-6
 * block corrector with its crackle and its a4 / a5 criterion.
 *   - The contract above holds word for word: with a fixed small_max no stored bit and no nb_block_stats counter depends on depth
 *     or on where batches end; nb_step(k) equals k x nb_step(1); two handles give the same bits; small_max = 0 is the mode off, bit
 *     for bit; what a small step computes for a body depends on the predicted arrays and on n alone; results for different small_max
 *     agree to the pass's accuracy, not bit for bit; t_next == 2^L always parks.
 *   - Checkpoint: the seven arrays of nb_set_block_steps6 (bodies, vel, accel, jerk, snap, crackle, levels), restored by nb_upload,
 *     nb_set_params, nb_set_hermite_order(6), nb_upload_derivs6, nb_set_block_steps6, nb_set_block_batch6 (same small_max, any
 *     depth), nb_upload_levels: the restored handle continues bit for bit.
 *   - The setter touches no state, no derived array and no levels, and restarts the policy at one slot.  nb_set_block_batch6(s, NULL),
 *     nb_set_block_batch(s, NULL), nb_set_block_steps6(s, NULL) and nb_set_block_steps(s, NULL) switch the mode off; a non-NULL
 *     nb_set_block_steps6 keeps it; nb_set_start6 keeps working; nb_set_hermite_order(4) and nb_set_neighbor_scheme(non-NULL) stay
 *     NB_ERR_STATE, as on any handle with block steps of order 6.
 *   - NB_ERR_STATE (the message names the function and the reason): a leapfrog handle, an order-4 handle (the message names
 *     nb_set_hermite_order), an order-6 handle without nb_set_block_steps6.  NB_ERR_INVALID (naming nb_set_block_batch6 and the
 *     field): a NULL handle, a wrong struct_size, depth > 1024, small_max > 1024 other than NB_BLOCK_BATCH_SMALL_DEFAULT, flags != 0.
 *   - Not built: the mode on guarded handles (mixed handles: nb_set_block_batch_mixed below), with the neighbour scheme or on
 *     nb_multi. */
int nb_set_block_batch6(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);

/* nb_set_block_batch_mixed (round 27): the same mode on mixed-precision handles -- an NB_F64 Hermite handle of order 4 with
 * nb_set_block_steps on (dynamic or frozen levels), nb_set_pass_precision(NB_PASS_MIXED) and guard radius 0.  A separate entry
 * point, as nb_set_block_batch6 is: nb_set_block_batch(non-NULL) on a mixed handle stays NB_ERR_STATE.  The struct, the defaults,
 * the slot protocol, the scheduler, the host's policy, the header checks at every wait and nb_block_batch_stats (enabled = 1 while
 * any of the three modes is on) are the ones above; inside a slot the predictor writes the mixed pass's three binary32 streams
 * (xh, mf), xl, vf, a small pass runs the mixed pass's pair arithmetic on them (dr = (xh_j - xh_i) + (xl_j - xl_i), dv = vf_j - vf_i,
 * nothing re-associated; kernels/block_batch_mixed.hip.h) and leaves binary32 chunk rows, and the corrector adds them in fp64 across
 * the chunks into the fp64 state.  A parked slot's host step is the mixed handle's gathered pass and block corrector.
 *   - The contract above holds word for word: with a fixed small_max no stored bit and no nb_block_stats counter depends on depth
 *     or on where batches end; nb_step(k) equals k x nb_step(1); two handles give the same bits; read-only calls between steps
 *     change nothing; small_max = 0 is a mixed handle with the mode off, bit for bit; t_next == 2^L always parks.
 *   - What a small step computes for a body depends on the three predicted streams and on n alone (its j-chunks are a function of n
 *     and the CU count), not on |A|, on the body's place in the active list, on small_max or on depth.  Results for DIFFERENT
 *     small_max agree to the pass's accuracy only.
 *   - Checkpoint: the five arrays bodies, vel, accel, jerk and levels, all fp64.  A handle restored by nb_upload, nb_upload_derivs,
 *     nb_set_pass_precision(NB_PASS_MIXED) (anywhere before the batch setter), nb_set_block_steps, nb_set_block_batch_mixed (same
 *     small_max, any depth), nb_upload_levels continues bit for bit.
 *   - nb_force_pass, nb_enable_timing, dt <= 0, stale levels, nb_download_levels / nb_upload_levels and ext_stream are unchanged.
 *   - The setter touches no state, no derivative and no level, and restarts the policy at one slot.  nb_set_block_batch_mixed(s, NULL),
 *     nb_set_block_batch(s, NULL), nb_set_block_batch6(s, NULL) and nb_set_block_steps(s, NULL) switch the mode off; a non-NULL
 *     nb_set_block_steps keeps it.  While the mode is on, nb_set_pass_precision with a mode that would change the precision,
 *     nb_set_pass_guard(r > 0), nb_set_hermite_order(6) and nb_set_neighbor_scheme(non-NULL) are NB_ERR_STATE; calls that change
 *     nothing (NB_PASS_MIXED again, nb_set_pass_guard(0)) stay NB_OK.
 *   - NB_ERR_STATE (the message names the function and the setter to call): a leapfrog handle, an NB_F32 handle, an order-6 handle,
 *     a handle without nb_set_block_steps, a native-precision handle (nb_set_pass_precision, or nb_set_block_batch), a handle with
 *     nb_set_pass_guard > 0.  NB_ERR_INVALID (naming nb_set_block_batch_mixed and the field): a NULL handle, a wrong struct_size,
 *     depth > 1024, small_max > 1024 other than NB_BLOCK_BATCH_SMALL_DEFAULT, flags != 0.
 *   - Not built: the mode on guarded handles, at order 6 with a mixed pass, with the neighbour scheme or on nb_multi; the encounter
 *     watch in mixed and order-6 slots (native order-4 slots: nb_set_block_batch_watch below). */
int nb_set_block_batch_mixed(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);

/* nb_set_block_batch_watch (round 29): nb_set_block_batch's mode on a handle with the encounter watch on (nb_set_encounter_watch,
 * below) -- a Hermite handle of order 4, NB_F32 or NB_F64, with nb_set_block_steps on (dynamic or frozen levels), the native pass,
 * the watch on and no other batched mode on.  Order of the setters: nb_set_block_steps, nb_set_encounter_watch,
 * nb_set_block_batch_watch.  A separate entry point, as nb_set_block_batch6 and nb_set_block_batch_mixed are: with the watch on,
 * nb_set_block_batch, nb_set_block_batch6 and nb_set_block_batch_mixed (non-NULL) stay NB_ERR_STATE, and with one of those modes on
 * nb_set_encounter_watch stays NB_ERR_STATE.  The struct, the defaults, the limits, the slot protocol, the scheduler, the predictor,
 * the host's policy, the header checks at every wait and nb_block_batch_stats (enabled = 1) are nb_set_block_batch's.  Inside a slot
 * the small pass keeps, beside its sums, the slot's closest candidate of each j-chunk, and the small corrector folds the chunks'
 * answers into the body's record before it corrects (kernels/encounter_batch.hip.h): no launch is added to a slot.  A parked slot's
 * host step is the watched handle's gathered pass, fold and block corrector.
 *   - State, derivatives and levels carry nb_set_block_batch's contract word for word: with a fixed small_max nothing depends on
 *     depth or on where batches end; nb_step(k) equals k x nb_step(1); two handles give the same bits; small_max = 0 is the mode
 *     off, bit for bit; t_next == 2^L always parks.
 *   - No stored bit of the state, the derivatives or the levels and no nb_block_stats or nb_block_batch_stats counter depends on the
 *     watch: a handle with nb_set_block_batch (same depth and small_max) and no watch holds the same bits after the same steps.
 *   - The records follow nb_set_encounter_watch's rules unchanged (candidates, the smallest rho^2 and the smallest index on a tie,
 *     strictly smaller replaces, count per own step with an answer, time = outer steps run + t_next / 2^max_level, rho^2 the value
 *     the pass that ran the step holds) and carry the state's contract: with a fixed small_max no record and no counter (passes,
 *     hits, first_time) depends on depth or on where batches end; with small_max = 0 they are those of the watch without the mode,
 *     bit for bit.  What a small step records for a body depends on the predicted arrays, the body's threshold and n alone, not on
 *     |A|, on the body's place in the list or on depth.  passes counts small and host steps alike: it equals
 *     nb_block_stats.block_steps over the same interval.
 *   - NB_ENC_STOP keeps its meaning: one extra host wait per outer step, after the outer step's last (host) block step, whose fold
 *     publishes the running hits, those of the small slots included.
 *   - nb_set_block_batch_watch(s, NULL), nb_set_block_batch(s, NULL), nb_set_block_batch6(s, NULL), nb_set_block_batch_mixed(s, NULL)
 *     and nb_set_block_steps(s, NULL) switch the mode off; the watch stays on with the first four.  nb_set_encounter_watch(s, NULL)
 *     switches the watch off and the mode with it.  nb_set_encounter_watch(non-NULL) while this mode is on replaces radii and flags
 *     and keeps records and counters; nb_set_block_batch_watch(non-NULL) while it is on sets depth and small_max anew.  A non-NULL
 *     nb_set_block_steps keeps both.  nb_set_hermite_order(6), nb_set_pass_precision(NB_PASS_MIXED),
 *     nb_set_neighbor_scheme(non-NULL) and the three other batch setters (non-NULL) stay NB_ERR_STATE, as on any watched handle.
 *   - Checkpoint: the state's five arrays and the four record arrays.  A handle restored by nb_upload, nb_upload_derivs,
 *     nb_set_block_steps, nb_set_encounter_watch, nb_set_block_batch_watch (same small_max, any depth), nb_upload_levels,
 *     nb_upload_encounters continues bit for bit, records included.
 *   - NB_ERR_STATE (the message names nb_set_block_batch_watch and the setter to call): a leapfrog handle, an order-6 handle, a
 *     handle without nb_set_block_steps, a mixed or guarded pass, the watch off (nb_set_encounter_watch; nb_set_block_batch for the
 *     mode without a watch), another batched mode on.  NB_ERR_INVALID (naming the field): a NULL handle, a wrong struct_size,
 *     depth > 1024, small_max > 1024 other than NB_BLOCK_BATCH_SMALL_DEFAULT, flags != 0.
 *   - Not built: the watch in mixed, guarded and order-6 slots, with the neighbour scheme, on nb_multi. */
int nb_set_block_batch_watch(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);

/* (a struct TAG without a typedef, as nb_block_stats) */
struct nb_block_batch_stats {
    uint32_t struct_size, enabled;
    uint64_t host_waits;            /* hipStreamSynchronize calls of nb_step on this handle */
    uint64_t slots;                 /* block-step slots enqueued */
    uint64_t small_steps;           /* block steps done by a slot, no host in between */
    uint64_t host_steps;            /* block steps sized by the host (the existing gathered path) */
    uint64_t idle_slots;            /* slots that found nothing to do */
};
/* block_batch_stats: the counters since the last reset (set out->struct_size); reset != 0 zeroes them after the read.
 * slots == small_steps + host_steps + idle_slots, host_steps <= host_waits <= slots. */
int nb_block_batch_stats(nb_sim *s, struct nb_block_batch_stats *out, int reset);

/* nb_set_encounter_watch (round 28): the closest approach every watched body sees INSIDE block steps.  Between nb_step calls every
 * body stands at a multiple of dt; a hard pair runs through hundreds of orbits inside one outer step, and nb_neighbors at the boundary
 * sees whatever phase it happens to be in.  The gathered pass of a block step already forms rho^2 = |dr|^2 + eps2 for every (active
 * body, body) pair at the active body's own time: with the watch on it keeps the smallest one below the body's threshold, as the
 * force libraries of the GRAPE family return the nearest neighbour with the force.  The primitive under collision and merger
 * detection, close-encounter stopping conditions and the search for pairs to regularise.
 *   - Opt-in, on a Hermite handle of order 4 with nb_set_block_steps on (dynamic or frozen levels), the native pass, NB_F32 or
 *     NB_F64, no batched mode (the watch inside batched slots: nb_set_block_batch_watch above, called with the watch on).  No stored bit of the state, the derivatives or the levels and no nb_block_stats counter depends on
 *     the watch: the pass's sums are the same instructions on the same values.
 *   - Body i has a watch radius h_i >= 0: `radius` for all bodies, or radii[i] (n elements of the handle's precision, host memory,
 *     copied by the call); 0: the body is not watched.  The threshold is w_i = h_i^2 + eps2, evaluated in fp64 and rounded once to
 *     the handle's precision.
 *   - When: at every gathered pass of a block step, for every active body i with h_i > 0 -- the full-set step that ends an outer
 *     step included; the start's pass and read-only calls (nb_force_pass, the queries) not.
 *   - Candidates: bodies j != i BY INDEX, j < n, whose rho^2_ij is strictly below w_i; rho^2_ij is the value the pass holds (the same
 *     fma order on the same predicted rows).  A distinct body at the same position is a candidate with rho^2 = eps2.  The pass's
 *     answer for i is the candidate of smallest rho^2, equal rho^2 to the smallest index (nb_neighbors' rule).
 *   - The record of a body lives until reset: rho2 (the smallest answer so far, the handle's precision; +inf at the start), partner
 *     (uint32; 0xffffffff at the start), time (double, +inf at the start: the number of outer steps the handle had run when that
 *     outer step began + t_next / 2^max_level; exact, independent of dt), count (uint32: own steps that had an answer).  A new answer
 *     replaces (rho2, partner, time) only when strictly smaller -- the earliest time wins a tie --, every step with an answer
 *     increments count.  Only the active body records: a pair is seen from both sides, at each member's own steps.
 *   - Nothing depends on timing: floating-point values are compared, never added; the atomics are integer counts and an integer
 *     minimum for the statistics.
 *   - NB_ENC_STOP: nb_step(k) returns NB_OK after the first outer step at whose end hits (below) is non-zero since the last reset,
 *     with stopped = 1 and steps_left = the outer steps not run.  One extra host wait per outer step, with the flag only.
 *   - nb_upload keeps the configuration and the counters and clears the records.  nb_set_encounter_watch(non-NULL) while the watch
 *     is on replaces radii and flags and keeps records and counters; switched on from off, both start over.
 *     nb_set_encounter_watch(s, NULL) and nb_set_block_steps(s, NULL) switch it off (and nb_set_block_batch_watch's mode with it).  While it is on, nb_set_block_batch,
 *     nb_set_block_batch6, nb_set_block_batch_mixed (non-NULL), nb_set_pass_precision(NB_PASS_MIXED), nb_set_hermite_order(6) and
 *     nb_set_neighbor_scheme(non-NULL) are NB_ERR_STATE.
 *   - Checkpoint: the four record arrays beside the state's (nb_download_encounters / nb_upload_encounters, the last calls of a
 *     restore, behind nb_set_encounter_watch).  The times count the handle's own outer steps.
 *   - Errors.  NB_ERR_INVALID: a NULL handle, unknown flag bits, a radius or radii element negative, NaN or infinite, a NULL out
 *     pointer, a NULL array or a partner that is neither another body's index nor 0xffffffff in nb_upload_encounters.  NB_ERR_STATE
 *     (the message names the function and the reason): a leapfrog handle, block steps off, an order-6 handle, a mixed or guarded
 *     pass, a batched mode on, the neighbour scheme on; the four other calls on a handle without the watch.
 *   - Not built: the watch in the mixed and guarded passes and their batched slots, at order 6, with the neighbour scheme, on
 *     nb_multi; a criterion on r_i + r_j. */
enum { NB_ENC_STOP = 1u };      /* nb_encounter_watch.flags: nb_step returns after the first outer step that had a hit */
typedef struct nb_encounter_watch {
    double radius;          /* h for every body (radii == NULL) */
    const void *radii;      /* n elements of the handle's precision, host memory; NULL: radius */
    uint32_t flags;         /* NB_ENC_* */
} nb_encounter_watch;
int nb_set_encounter_watch(nb_sim *s, const nb_encounter_watch *cfg /* NULL: off */);

/* (a struct TAG without a typedef, as nb_block_stats) */
struct nb_encounter_stats {
    uint64_t passes;        /* gathered passes that ran with the watch on */
    uint64_t hits;          /* body steps that had an answer */
    double first_time;      /* the earliest block time with an answer, as the records' time; +inf: none */
    uint32_t stopped;       /* the last nb_step returned early (NB_ENC_STOP) ... */
    uint32_t steps_left;    /* ... with this many of its outer steps not run */
};
/* encounter_stats: the counters since the last reset; reset != 0 zeroes passes, hits and first_time after the read (the records stay). */
int nb_encounter_stats(nb_sim *s, struct nb_encounter_stats *out, int reset /* counters only */);
/* download_encounters / upload_encounters: the records, n elements each -- rho2 in the handle's precision.  Download: each pointer
 * may be NULL; changes nothing.  Upload: all four are required. */
int nb_download_encounters(nb_sim *s, void *rho2, uint32_t *partner, double *time, uint32_t *count);
int nb_upload_encounters(nb_sim *s, const void *rho2, const uint32_t *partner, const double *time, const uint32_t *count);
/* reset_encounters: the records to their start values, the counters and stopped / steps_left to 0. */
int nb_reset_encounters(nb_sim *s);

/* ---- viewer frame feed ------------------------------------------------
 * The reference's render pass reads bodyBuffer and velBuffer in place every frame
 * (nbody3d.js:408-415,482-487: billboard position + radius from (x,y,z,mass), colour from
 * length(vel.xyz), :380).  A host-side viewer gets the same two arrays without stalling the
 * step stream: nb_frame_request enqueues a small pack kernel behind the steps issued so far
 * (f32 bodies[4n] + speed[n] into a staging buffer) and the copy to pinned host memory runs
 * on a second stream beside the following steps.  nb_frame_acquire returns the newest frame
 * that has landed: pointers into engine-owned pinned memory, valid until the fourth
 * nb_frame_request after the one that produced it (a ring of four slots: the host may run
 * that far ahead of the copies before a request blocks).  On a shard handle speed[]
 * is filled for the handle's own rows only. */
int nb_frame_request(nb_sim *s);
int nb_frame_acquire(nb_sim *s, int wait, const float **bodies, const float **speed,
                     uint64_t *step_index);

/* ---- on-device diagnostics (no reference analogue) ------- */

/* out[0] = kinetic energy of this handle's shard (sum 1/2 m v^2),
 * out[1] = potential energy share of this handle's shard
 *          (-G/2 * sum_i sum_{j != i} m_i m_j / sqrt(r^2 + eps2), i in shard),
 * out[2..4] = momentum of the shard.  Accumulated in fp64 on the device. */
int nb_diagnostics(nb_sim *s, double out[5]);

/* ---- field queries (ABI 2.4; no reference analogue) ------------------------------------------
 * Acceleration and potential of the handle's N bodies at M points, M x N ordered pairs:
 *     a(p)   =   sum_j G m_j (x_j - p) / (|x_j - p|^2 + eps2)^(3/2)
 *     phi(p) = - sum_j G m_j / sqrt(|x_j - p|^2 + eps2)
 * with the handle's eps2 and the G of the last nb_set_params, on the positions AS THEY STAND BEHIND EVERY STEP ENQUEUED SO FAR
 * (a shard handle finishes a pending gather first, as nb_diagnostics does).  Any handle kind: whole system, shard (its bodies
 * array is replicated), fused / ping-pong, symmetric with padded rows (zero-mass rows add exactly nothing).
 *   - Element type of points / accel / phi: the handle's precision.  With NB_FIELD_F64 on an f32 handle the pair arithmetic and
 *     the sums run in fp64 on the stored f32 rows and the two OUTPUTS are double (points stay float): the on-device audit of the
 *     f32 sums.  On an f64 handle NB_FIELD_F64 is accepted and changes nothing.
 *   - Arbitrary points leave nothing out.  A point that coincides with a body gets exactly 0 acceleration from it (eps2 > 0) and
 *     -G m / sqrt(eps2) of potential.  NB_FIELD_AT_BODIES: point k is body first_body + k and leaves ITSELF out of both sums --
 *     inside the loop (that one pair carries a weight of zero), never by subtracting the self term afterwards, so a body of
 *     mass 1e7 gets the small potential of its neighbours to full precision.
 *   - At least one of accel / phi is non-NULL; an output that is not asked for is not computed.
 *   - Errors: NB_ERR_INVALID (NULL handle or request, wrong struct_size, m == 0, both outputs NULL, points given with
 *     NB_FIELD_AT_BODIES or missing without it, first_body + m > n, unknown flag bits), NB_ERR_STATE (nothing uploaded, no
 *     parameters set); nb_last_error names the field.
 *   - The simulation state, the engine's side copies of it, the captured step graphs and the step counter are untouched:
 *     stepping after a call is bit-identical to stepping without it.
 *   - Deterministic: the same request on the same state gives the same bits (fixed summation order, no atomics).  The order
 *     may depend on m, so a sub-range's bits need not equal the same rows of a larger request.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_FIELD_DEVICE: the three pointers are
 *     device memory on the handle's device, the work is enqueued on the handle's stream and the call returns at once.
 *   - Memory: engine-owned staging for a host-pointer request (O(m)) and partial sums of a bounded number of (point, j-chunk)
 *     rows (2^20 rows of 16 or 32 bytes, or two launches' worth of workgroups where that is more); grown on demand, released by
 *     nb_destroy; nothing proportional to m x N.  Large m goes through in batches of at most 262,144 points. */
#define NB_FIELD_AT_BODIES 1u  /* points = current positions of bodies [first_body, first_body + m); each leaves ITSELF out of its sums */
#define NB_FIELD_F64       2u  /* f32 handle: pair arithmetic and sums in fp64 on the stored f32 rows; outputs are double (audit mode) */
#define NB_FIELD_DEVICE    4u  /* points / accel / phi are DEVICE pointers on the handle's device; the work is enqueued on the
                                  handle's stream and the call returns without synchronising */
typedef struct nb_field_request {
    uint32_t struct_size;   /* sizeof(nb_field_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_FIELD_* */
    uint32_t first_body;    /* NB_FIELD_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); must be NULL with NB_FIELD_AT_BODIES */
    void *accel;            /* out, optional: 4*m elements ax, ay, az, 0 */
    void *phi;              /* out, optional: m elements */
} nb_field_request;
int nb_field_eval(nb_sim *s, const nb_field_request *req);
/* The same on a multi-shard system.  The bodies are replicated on every shard after a step, so the request is evaluated on
 * shard 0 (its device, its stream); first_body counts the caller's UNPADDED rows. */
int nb_multi_field_eval(nb_multi *m, const nb_field_request *req);

/* ---- neighbour queries (added within ABI 2.4; no reference analogue) ---------------------------
 * For each of M points: the NEAREST of the handle's N bodies, its squared distance, and the NUMBER of bodies inside a radius --
 * M x N ordered pairs, what the collisional codes return from their O(N^2) pass: the start of close-pair detection, of a
 * neighbour scheme, of a local-density estimate.
 *   - Distance: the plain squared distance, NO softening, in the handle's precision:
 *         dx = x_j - p_x, dy, dz likewise;   d2 = fma(dz, dz, fma(dy, dy, dx * dx))
 *     binary32 on f32 handles, fp64 throughout on f64 handles.  There is no fp64 audit mode on f32 handles (the positions are
 *     binary32 either way); 2u is not a flag here.
 *   - State read: the positions AS THEY STAND BEHIND EVERY STEP ENQUEUED SO FAR, the state nb_field_eval reads (a shard handle
 *     finishes a pending gather first).  Any handle kind: whole system, shard, fused / ping-pong, symmetric, Hermite, block-step.
 *     nb_set_params is not required: G does not enter.
 *   - All n rows of the handle are bodies whatever their mass (tracers count).
 *   - Nearest: index = the j with the smallest d2; among equal d2 the SMALLEST j.  dist2 = that d2.  NB_NBR_AT_BODIES: point k is
 *     body first_body + k and leaves ITSELF out, by index, not by distance: another body at exactly the same position is a
 *     neighbour at d2 = 0.  When there is no candidate (n = 1 with NB_NBR_AT_BODIES): index 0xffffffff, dist2 +inf.
 *   - Count: h = radii[k], or radius when radii is NULL; h2 = h * h in the handle's precision; count = the number of rows, the
 *     own row of an NB_NBR_AT_BODIES point excluded, with d2 < h2, strictly.  The radius enters the count only: the nearest body
 *     is reported however far it is, and without count both radii and radius are ignored (radius must still be >= 0).
 *   - At least one of index / dist2 / count is non-NULL; an output that is not asked for is not written.
 *   - Deterministic, and more than nb_field_eval promises: min and integer sums are exact, so the three outputs of a point depend on
 *     that point and on the bodies ONLY -- not on m, not on the batches a large request is cut into, not on how the engine cuts
 *     j into chunks.  A sub-range request returns the same bits as the same rows of a larger request.
 *   - Points and bodies must be finite; the result for a non-finite one is unspecified (the call does not fault).
 *   - Errors: NB_ERR_INVALID (NULL handle or request -- checked before any device call --, wrong struct_size, m == 0, unknown flag
 *     bits, all three outputs NULL, points given with NB_NBR_AT_BODIES or missing without it, first_body + m > n, count with
 *     neither radii nor radius > 0, radius negative or NaN), NB_ERR_STATE (nothing uploaded); nb_last_error names the function
 *     and the field.
 *   - The simulation state, the engine's side copies of it, the captured step graphs and the step counter are untouched:
 *     stepping after a call is bit-identical to stepping without it.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_NBR_DEVICE: the five pointers are
 *     device memory on the handle's device, the work is enqueued on the handle's stream and the call returns at once.
 *   - Memory: engine-owned staging for a host-pointer request (O(m)) and one 16-byte row per (point of a batch, j-chunk), bounded as
 *     nb_field_eval's partial sums are (the two calls share that buffer); grown on demand, released by nb_destroy.  Large m goes
 *     through in batches of at most 262,144 points (65,536 on f64 handles). */
#define NB_NBR_AT_BODIES 1u  /* point k is body first_body + k and leaves ITSELF out (by index, not by distance) */
#define NB_NBR_DEVICE    4u  /* points / radii / index / dist2 / count are DEVICE pointers on the handle's device; enqueued on the
                                handle's stream, returns at once */
typedef struct nb_neighbor_request {
    uint32_t struct_size;   /* sizeof(nb_neighbor_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_NBR_* (2u is not a flag here: NB_ERR_INVALID) */
    uint32_t first_body;    /* NB_NBR_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_NBR_AT_BODIES */
    const void *radii;      /* optional: m elements, one search radius per point (handle's precision) */
    double radius;          /* used when radii == NULL; 0 = no radius given */
    uint32_t *index;        /* out, optional: m elements, nearest body; 0xffffffff when there is none */
    void *dist2;            /* out, optional: m elements (handle's precision), its squared distance; +inf when there is none */
    uint32_t *count;        /* out, optional: m elements, bodies with d2 < h*h; needs radii or radius > 0 */
} nb_neighbor_request;
int nb_neighbors(nb_sim *s, const nb_neighbor_request *req);
/* The same on a multi-shard system: evaluated on shard 0, which holds every row, against the caller's UNPADDED n rows only -- the
 * zero-mass padding rows at the origin are never returned and never counted; first_body counts the caller's rows. */
int nb_multi_neighbors(nb_multi *m, const nb_neighbor_request *req);
/* The launch shape of an m-point request (no device call): the points of its first batch, the j-chunks each of them is run
 * against, and the bodies of one chunk (whole 256-row tiles).  For tests and tools; the results do not depend on it. */
int nb_neighbors_shape(nb_sim *s, uint32_t m, uint32_t *batch, uint32_t *chunks, uint32_t *j_per_chunk);

/* ---- neighbour lists (added within ABI 2.4; no reference analogue) ----------------------------
 * For each of M points: WHICH of the handle's N bodies lie inside its radius -- the members nb_neighbors only counts --, as one
 * row of `cap` indices per point: the neighbour lists of an Ahmad-Cohen split, friends-of-friends links, all close pairs (the k
 * nearest bodies of a point, whatever their distance, are nb_knn's).
 *   - Membership: body j belongs to the row of point k iff d2(k, j) < h2, strictly, with d2 and h2 computed exactly as
 *     nb_neighbors computes them for its count: the same expression, the handle's precision, no softening, every row of the
 *     handle a body whatever its mass.  An NB_NBR_AT_BODIES point leaves ITSELF out by index; another body at the same position
 *     is a member at d2 = 0.  count[k] therefore equals the count of nb_neighbors bit for bit.
 *   - Order and overflow: row k = list[k * cap .. k * cap + cap) holds the members in ASCENDING j.  With more than cap members it
 *     holds the cap SMALLEST indices, and count[k] > cap says so (count is the true number, never clipped).  The entries
 *     [min(count, cap), cap) of a row hold 0xffffffff: all m * cap elements are defined, in host and in device mode.
 *   - index / dist2: the nearest body and its squared distance, as nb_neighbors returns them (the radius does not enter).
 *   - Deterministic, as nb_neighbors: no atomics; a point's row, count, index and dist2 depend on that point and on the bodies
 *     ONLY -- not on m, not on the batches, not on cap beyond the truncation (the first c entries of a row are the same for every
 *     cap >= c), not on how the engine cuts j into chunks.  A sub-range request returns the bits of the same rows of a larger one.
 *   - State read: that of nb_neighbors -- the positions behind every step enqueued so far, a shard handle finishes a pending
 *     gather first; any handle kind, f32 and f64.  The simulation state, the engine's side copies, the captured step graphs and
 *     the step counter are untouched: stepping after a call is bit-identical to stepping without it.
 *   - Radii and points must be finite; the result for a non-finite one is unspecified (the call does not fault).
 *   - Errors: NB_ERR_INVALID (NULL handle or request -- checked before any device call --, wrong struct_size, m == 0, unknown flag
 *     bits (2u included), list NULL, cap == 0 or cap > 4096, reserved != 0, neither radii nor radius > 0, radius negative or NaN,
 *     points given with NB_NBR_AT_BODIES or missing without it, first_body + m > n), NB_ERR_STATE (nothing uploaded);
 *     nb_last_error names the function and the field.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_NBR_DEVICE: every pointer is device
 *     memory on the handle's device, the work is enqueued on the handle's stream and the call returns at once.
 *   - Memory: the partial rows of nb_neighbors (the same buffer, the same bound) plus 4 bytes per (point of a batch, j-chunk); a
 *     host-pointer request stages `list` one batch at a time.  The batch of nb_neighbors is halved, in whole workgroups' worth of
 *     points, until batch x cap x 4 <= 256 MiB (down to one workgroup's points); nb_neighbor_lists_shape reports it.  Nothing is
 *     proportional to m x N. */
typedef struct nb_neighbor_list_request {
    uint32_t struct_size;   /* sizeof(nb_neighbor_list_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_NBR_AT_BODIES | NB_NBR_DEVICE: the bits and the meaning they have for nb_neighbors */
    uint32_t first_body;    /* NB_NBR_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_NBR_AT_BODIES */
    const void *radii;      /* optional: m elements, one search radius per point (handle's precision) */
    double radius;          /* used when radii == NULL; radii or radius > 0 is REQUIRED here */
    uint32_t cap;           /* entries per point in `list`, 1 <= cap <= 4096 */
    uint32_t reserved;      /* must be 0 */
    uint32_t *list;         /* out, required: m * cap elements, row k = point k */
    uint32_t *count;        /* out, optional: m elements, the TRUE number of bodies with d2 < h*h (may exceed cap) */
    uint32_t *index;        /* out, optional: m elements, nearest body, as nb_neighbors */
    void *dist2;            /* out, optional: m elements (handle's precision), its squared distance, as nb_neighbors */
} nb_neighbor_list_request;
int nb_neighbor_lists(nb_sim *s, const nb_neighbor_list_request *req);
/* The same on a multi-shard system: evaluated on shard 0 against the caller's UNPADDED n rows, as nb_multi_neighbors -- a padding
 * row is never listed and never counted. */
int nb_multi_neighbor_lists(nb_multi *m, const nb_neighbor_list_request *req);
/* The launch shape of an m-point request with rows of cap entries (no device call): as nb_neighbors_shape, the batch cut further
 * as the memory rule above says.  For tests and tools; the results do not depend on it. */
int nb_neighbor_lists_shape(nb_sim *s, uint32_t m, uint32_t cap, uint32_t *batch, uint32_t *chunks, uint32_t *j_per_chunk);

/* ---- k nearest neighbours (added within ABI 2.4; no reference analogue) -----------------------
 * For each of M points: the K NEAREST of the handle's N bodies, nearest first -- what is defined by a number of neighbours and not
 * by a radius: Casertano-Hut densities and the density centre, SPH-style smoothing lengths, k-th-neighbour time-step and
 * softening criteria, Ahmad-Cohen neighbour spheres that hold a fixed number of members.  No radius has to be guessed, no row is
 * longer than k, nothing is sorted on the host.
 *   - Distance: exactly nb_neighbors' expression, d2 = fma(dz, dz, fma(dy, dy, dx * dx)) with dx = x_j - p_x, NO softening, in the
 *     handle's precision; every row of the handle a body whatever its mass.  An NB_NBR_AT_BODIES point leaves ITSELF out by
 *     index; another body at the same position is a neighbour at d2 = 0.
 *   - Order: row r = index[r * k .. r * k + k) / dist2[r * k ..) holds the k smallest candidates under the TOTAL order (d2
 *     ascending, then j ascending), in that order.  index[r * k] and dist2[r * k] are therefore the bytes nb_neighbors returns for
 *     the same point.
 *   - Short rows: with fewer than k candidates (n - 1 < k at the bodies, n < k otherwise) the remaining entries hold 0xffffffff
 *     and +inf; a candidate whose d2 overflows to +inf is no candidate, as in nb_neighbors.  All m * k elements of an output are
 *     defined, in host and in device mode.
 *   - At least one of index / dist2 is non-NULL; an output that is not asked for is not written.
 *   - Deterministic: no atomics; the order is total, so a point's row depends on that point and on the bodies ONLY -- not on m, not
 *     on the batches, not on how the engine cuts j into chunks, not on k beyond its length: the row for k' < k is the first k'
 *     entries of the row for k.  A sub-range request returns the bits of the same rows of a larger one.
 *   - State read: that of nb_neighbors -- the positions behind every step enqueued so far, a shard handle finishes a pending
 *     gather first; any handle kind, f32 and f64; nb_set_params is not required.  The simulation state, the engine's side copies,
 *     the captured step graphs and the step counter are untouched: stepping after a call is bit-identical to stepping without it.
 *   - Points and bodies must be finite; the result for a non-finite one is unspecified (the call does not fault).
 *   - Errors: NB_ERR_INVALID (NULL handle or request -- checked before any device call --, wrong struct_size, m == 0, k == 0 or
 *     k > 64, reserved != 0, unknown flag bits (2u included), both outputs NULL, points given with NB_NBR_AT_BODIES or missing
 *     without it, first_body + m > n), NB_ERR_STATE (nothing uploaded); nb_last_error names the function and the field.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_NBR_DEVICE: every pointer is device
 *     memory on the handle's device, the work is enqueued on the handle's stream and the call returns at once.
 *   - Memory: per (point of a batch, j-chunk) one partial row of k entries (d2, j), kept in an engine-owned working row of 2k
 *     entries (k + 4 below k = 4) of 8 bytes (f32) or 16 bytes (f64); grown on demand, released by nb_destroy.  The shape is
 *     derived ONCE per request: the batch and the j-chunks nb_neighbors would give m points (at most 512 chunks), the batch then
 *     halved, in whole workgroups' worth of points and with the j-chunks kept, until chunks x batch x k x 8 <= 256 MiB (down to one
 *     workgroup's points); every batch of the request, the last and shorter one included, runs against those chunks, and
 *     nb_knn_shape reports them.  The working rows take 2 x that figure on f32 handles and 4 x on f64 handles (up to 1 GiB).  A
 *     host-pointer request stages its outputs one batch at a time.  Nothing is proportional to m x N. */
typedef struct nb_knn_request {
    uint32_t struct_size;   /* sizeof(nb_knn_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_NBR_AT_BODIES | NB_NBR_DEVICE: the bits and the meaning they have for nb_neighbors */
    uint32_t first_body;    /* NB_NBR_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_NBR_AT_BODIES */
    uint32_t k;             /* neighbours per point, 1 <= k <= 64 */
    uint32_t reserved;      /* must be 0 */
    uint32_t *index;        /* out, optional: m * k elements, row r = point r; 0xffffffff past the last candidate */
    void *dist2;            /* out, optional: m * k elements (handle's precision); +inf past the last candidate */
} nb_knn_request;
int nb_knn(nb_sim *s, const nb_knn_request *req);
/* The same on a multi-shard system: evaluated on shard 0 against the caller's UNPADDED n rows, as nb_multi_neighbors -- a padding
 * row is never returned. */
int nb_multi_knn(nb_multi *m, const nb_knn_request *req);
/* The launch shape of an m-point request for k neighbours (no device call): the points of EVERY batch but the last (which takes
 * what is left), the j-chunks and the bodies of one chunk, as the memory rule above says.  For tests and tools; the results do not
 * depend on it. */
int nb_knn_shape(nb_sim *s, uint32_t m, uint32_t k, uint32_t *batch, uint32_t *chunks, uint32_t *j_per_chunk);

/* ---- forces over neighbour rows (added within ABI 2.4; no reference analogue) -----------------
 * For each of M rows of body indices -- the rows nb_neighbor_lists and nb_knn write, or any a caller builds --: acceleration, jerk
 * and potential summed over THE ENTRIES OF THE ROW ONLY, at the row's point or body.  This is the irregular force of an
 * Ahmad-Cohen split, the sum a collisional code evaluates many times per regular step; its cost is the entries, not M x N.
 *   - The sums, for row k, with p, u the position and velocity of its point (or of body first_body + k):
 *         a    =   sum_j G m_j dr / rho^3
 *         jerk =   sum_j G m_j [ dv / rho^3 - 3 (dr.dv) dr / rho^5 ]
 *         phi  = - sum_j G m_j / rho          dr = x_j - p,  dv = v_j - u,  rho^2 = |dr|^2 + eps2
 *     over the entries j of the row, with the handle's eps2 and the G of the last nb_set_params, read from the positions as they
 *     stand behind every step enqueued so far (the state nb_field_eval reads; a shard handle finishes a pending gather first).
 *     accel.w and jerk.w are 0.  Outputs have the handle's precision; at least one of accel / jerk / phi is non-NULL and an
 *     output that is not asked for is not written.
 *   - Entries: row k is list[k * cap .. k * cap + cap); with count, only its first min(count[k], cap) entries are read.  An entry
 *     >= n adds nothing -- the padding 0xffffffff wherever it stands in the row, or any other value past the rows; the call does
 *     not fault.  With NB_LISTF_AT_BODIES an entry equal to the row's own index first_body + k adds nothing (its dr is 0, but its
 *     m / sqrt(eps2) would count in phi).  A duplicated entry is added twice.  The order of a row does not have to ascend:
 *     nb_knn's index rows are valid input.  A row without a valid entry gives exact +0 in every output.
 *   - Jerk: needs velocities at the positions' instant, so it is available on Hermite handles only (block-step handles included);
 *     jerk != NULL on a leapfrog handle is NB_ERR_STATE, as for nb_download_jerk.  accel and phi work on every handle kind (shard,
 *     fused, symmetric, Hermite).  On nb_multi jerk != NULL is NB_ERR_INVALID; nb_multi_list_force evaluates on shard 0 against
 *     the caller's UNPADDED n rows, as the other nb_multi_* queries (an entry that names a padding row adds nothing).
 *   - Deterministic, and more than nb_field_eval promises: no atomics, and the order of additions is a function of an entry's
 *     POSITION IN ITS ROW alone.  Entry e goes to lane e mod LS of the row's group of LS lanes; a lane adds its entries in ascending
 *     e (in the handle's precision, the per-pair arithmetic of the force+jerk pass); the LS lane sums are combined in fp64 in a
 *     fixed tree; G multiplies the total once, in fp64, and the product is rounded once (nb_field_eval's rule).  LS is one build
 *     constant per precision (nb_list_force_shape reports it).  A row's outputs therefore depend on that row's entries, its point
 *     and the bodies ONLY: not on m, not on the batches, not on cap -- the same entries re-packed at another cap give the same
 *     bits --, and not on whether count was passed, provided the tail it skips is padding.
 *   - State: the simulation state, the engine's side copies, the captured step graphs and the step counter are untouched: stepping
 *     after a call is bit-identical to stepping without it.
 *   - Points, point velocities and bodies must be finite and eps2 > 0; otherwise the result is unspecified (the call does not fault).
 *   - Errors: NB_ERR_INVALID (NULL handle or request -- checked before any device call --, wrong struct_size, m == 0, unknown flag
 *     bits (2u included), list NULL, cap outside 1 .. 4096, reserved != 0, all three outputs NULL, points / point_vel given with
 *     NB_LISTF_AT_BODIES, points missing without it, point_vel missing with a jerk at points or given without one,
 *     first_body + m > n), NB_ERR_STATE (nothing uploaded, nb_set_params not called, jerk on a leapfrog handle); nb_last_error
 *     names the function and the field.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_LISTF_DEVICE: every pointer is device
 *     memory on the handle's device, the arrays are read and written in place, the work is enqueued on the handle's stream and the
 *     call returns at once.
 *   - Memory: a host-pointer request stages list, count, the points and the outputs one batch at a time, the batch halved in
 *     whole workgroups' worth of rows until batch x cap x 4 <= 256 MiB (nb_neighbor_lists' rule and its staging buffer).  Nothing
 *     is proportional to m x N. */
#define NB_LISTF_AT_BODIES 1u   /* row k belongs to body first_body + k; an entry equal to that index is skipped */
#define NB_LISTF_DEVICE    4u   /* every pointer is device memory on the handle's device; enqueued on the handle's stream, returns at once */
typedef struct nb_list_force_request {
    uint32_t struct_size;   /* sizeof(nb_list_force_request) */
    uint32_t m;             /* number of rows, >= 1 */
    uint32_t flags;         /* NB_LISTF_AT_BODIES | NB_LISTF_DEVICE */
    uint32_t first_body;    /* NB_LISTF_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_LISTF_AT_BODIES */
    const void *point_vel;  /* 4*m elements vx, vy, vz, (ignored); required iff jerk != NULL and NB_LISTF_AT_BODIES is not set, else must be NULL */
    const uint32_t *list;   /* required: m * cap entries, row k = list[k*cap .. k*cap+cap) */
    const uint32_t *count;  /* optional: m elements; only the first min(count[k], cap) entries of row k are read */
    uint32_t cap;           /* entries per row, 1 <= cap <= 4096 */
    uint32_t reserved;      /* must be 0 */
    void *accel;            /* out, optional: 4*m elements (ax, ay, az, 0) of the handle's precision */
    void *jerk;             /* out, optional: 4*m elements (jx, jy, jz, 0); Hermite handles only */
    void *phi;              /* out, optional: m elements */
} nb_list_force_request;    /* 80 bytes */
int nb_list_force(nb_sim *s, const nb_list_force_request *req);
/* The same on a multi-shard system: evaluated on shard 0 against the caller's UNPADDED n rows; jerk must be NULL. */
int nb_multi_list_force(nb_multi *m, const nb_list_force_request *req);
/* The shape of an m-row request at `cap` entries per row (no device call): the rows of EVERY batch but the last of a host-pointer
 * request (a device-pointer request is one batch), and LS, the lanes that share a row.  For tests and tools; the results do not
 * depend on the batch. */
int nb_list_force_shape(nb_sim *s, uint32_t m, uint32_t cap, uint32_t *batch, uint32_t *lanes_per_row);

/* ---- regular and irregular force+jerk in one pass (added within ABI 2.4; no reference analogue) ----
 * For each of M points (or bodies): the acceleration and the jerk of ALL N rows of the handle, every pair's term added to exactly
 * one of TWO sums -- the irregular sum over the bodies inside the point's radius, the regular sum over every other row.  This
 * is the regular-force pass of an Ahmad-Cohen scheme: one comparison per pair decides which accumulators take the term.  Nothing
 * is subtracted, so the small sum of a point with a close neighbour does not carry the rounding error of the large one (what
 * "full pass minus nb_list_force" does), and the two sums are cut by the same comparison in the same pass.
 *   - Membership: body j is a MEMBER of point k iff d2 < h2, strictly, with d2 = fma(dz, dz, fma(dy, dy, dx * dx)), dx = x_j - p_x,
 *     and h2 = h * h, h = radii[k] or radius, all in the handle's precision: nb_neighbors' expression and rule, letter for letter
 *     (a body exactly on the sphere is no member).  Every row of the handle is a body whatever its mass.  *_irr sums the members,
 *     *_reg sums every other row.
 *   - Pair arithmetic: the force+jerk pass's terms
 *         a    = sum_j G m_j dr / rho^3
 *         jerk = sum_j G m_j [ dv / rho^3 - 3 (dr.dv) dr / rho^5 ]          dr = x_j - p,  dv = v_j - u
 *     with rho^2 = d2 + eps2 -- one rounding more than the force+jerk pass's fused chain, so *_irr + *_reg is NOT bit-comparable
 *     with what nb_force_pass / nb_step leave in accel and jerk --, then that pass's sequence (reciprocal root, s3 = (m y) y^2, the
 *     jerk as ONE sum of s3 (dv - 3 q dr)).  A pair's term goes to exactly one of the two sums: its weight is s3 in that sum and 0
 *     in the other.  Never a subtraction.
 *   - Own row: with NB_SPLIT_AT_BODIES point k is body first_body + k; its own row needs no mask (dr = dv = 0 and eps2 > 0 give an
 *     exact 0 in whichever sum it lands).  Another body at the same position is a member (d2 = 0): it adds 0 to a and its dv term
 *     to the jerk.
 *   - Empty sides: a point without a member (radii[k] = 0 included) gets exactly 0 (== 0) in both irregular rows; a point whose
 *     radius covers every row gets exactly 0 in both regular rows.  .w of every row is 0.
 *   - Summation: as the force+jerk pass -- on f32 handles binary32 in two levels inside a j-chunk (a register takes at most 1,024
 *     terms), fp64 across the j-chunks in ascending order, G multiplied in once in fp64 and the product rounded once.  No atomics:
 *     the same request on the same state gives the same bits, and a scalar radius and a radii array filled with that value give
 *     the same bits.  Nothing more is promised (the order may depend on m, as for nb_field_eval).
 *   - Handles: accel_irr / accel_reg work on every handle kind (whole, shard after its gather, fused, symmetric, Hermite,
 *     block-step), f32 and f64.  The jerk pair needs velocities at the positions' instant: Hermite handles only (block-step
 *     included); on a leapfrog handle it is NB_ERR_STATE, as for nb_list_force.  There is no fp64 audit mode: 2u is an unknown flag.
 *     On nb_multi a jerk pointer is NB_ERR_INVALID; nb_multi_split_force evaluates on shard 0 against the caller's UNPADDED n rows
 *     (the zero-mass padding rows add exactly nothing to either sum).
 *   - Positions read: as they stand behind every step enqueued so far (the state nb_field_eval reads).  The simulation state,
 *     the side copies, the captured graphs and the step counter are untouched: stepping after a call is bit-identical to stepping
 *     without it.  nb_set_params is required (G).
 *   - Points, velocities and bodies must be finite and eps2 > 0; otherwise the result is unspecified (the call does not fault).
 *   - Errors: NB_ERR_INVALID (NULL handle or request -- checked before any device call --, wrong struct_size, m == 0, unknown flag
 *     bits, all four outputs NULL, points / point_vel given with NB_SPLIT_AT_BODIES, points missing without it, point_vel missing
 *     with a jerk at points or given without one, first_body + m > n, neither radii nor radius > 0, radius negative or NaN; on
 *     nb_multi a non-NULL jerk pointer), NB_ERR_STATE (nothing uploaded, nb_set_params not called, a jerk on a leapfrog handle);
 *     nb_last_error names the function and the field.
 *   - Host pointers: the call blocks until the outputs are written; no pointer is kept.  NB_SPLIT_DEVICE: every pointer is device
 *     memory on the handle's device, read and written in place, enqueued on the handle's stream; the call returns at once.
 *   - Memory: up to four partial rows per (point of a batch, j-chunk) in the buffer nb_field_eval and nb_neighbors share, under
 *     its bound (the j-chunks are made longer, then the batch is halved, until it fits); a host-pointer request is staged as
 *     those calls stage theirs.  Nothing is proportional to m x N. */
#define NB_SPLIT_AT_BODIES 1u   /* point k is body first_body + k */
#define NB_SPLIT_DEVICE    4u   /* every pointer is device memory; enqueued on the handle's stream, returns at once */
typedef struct nb_split_force_request {
    uint32_t struct_size;   /* sizeof(nb_split_force_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE */
    uint32_t first_body;    /* NB_SPLIT_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_SPLIT_AT_BODIES */
    const void *point_vel;  /* 4*m elements vx, vy, vz, (ignored); required iff a jerk is asked for at points, else NULL */
    const void *radii;      /* optional: m elements of the handle's precision; an element may be 0 */
    double radius;          /* used when radii == NULL; radii or radius > 0 is required */
    void *accel_irr;        /* out, optional: 4*m elements (ax, ay, az, 0) over the members */
    void *accel_reg;        /* out, optional: 4*m elements over every other row */
    void *jerk_irr;         /* out, optional: 4*m elements (jx, jy, jz, 0); Hermite handles only */
    void *jerk_reg;         /* out, optional: likewise */
} nb_split_force_request;   /* 80 bytes */
int nb_split_force(nb_sim *s, const nb_split_force_request *req);
/* The same on a multi-shard system: evaluated on shard 0 against the caller's UNPADDED n rows; the jerk pointers must be NULL. */
int nb_multi_split_force(nb_multi *m, const nb_split_force_request *req);
/* The shape of an m-point request (no device call): the points of the first batch, its j-chunks, the bodies per chunk and the
 * points one workgroup takes.  For tests and tools. */
int nb_split_force_shape(nb_sim *s, uint32_t m, uint32_t *batch, uint32_t *chunks, uint32_t *j_per_chunk, uint32_t *rows_per_workgroup);

/* ---- the two sums of nb_split_force and the rows of nb_neighbor_lists from one pass (added within ABI 2.4; no reference analogue) ----
 * nb_split_force cuts every pair's term into the irregular or the regular sum by d2 < h2; nb_neighbor_lists derives the same d2,
 * the same h2 and the same comparison twice more (a count pass and a fill pass) only to write down WHICH j were members.  This
 * call does both in one pass over the M x N pairs: the comparison that selects the weights also writes the rows.  It is the start
 * and the regular time of an Ahmad-Cohen scheme, and what a near/far decomposition wants: the two sums and the rows they were cut
 * by, with no chance that the two disagree about a body on the sphere.
 *   - Rows: `list` and `count` are BIT FOR BIT what nb_neighbor_lists returns for the same points, radii or radius, cap and
 *     flags, whatever the launch shape: row k holds its members in ascending j; with more than cap members the cap smallest; the
 *     tail [min(count, cap), cap) holds 0xffffffff (NB_NBR_NONE); all m * cap elements are written, in host and in device mode;
 *     count is the TRUE number of members, never clipped.  With NB_SPLIT_AT_BODIES point k leaves ITSELF out of its row by index
 *     (row first_body + k); another body at the same position is a member.
 *   - Sums: the four sums are BIT FOR BIT what nb_split_force returns for the same request whenever nb_split_lists_shape reports
 *     the (batch, chunks, j_per_chunk) that nb_split_force_shape reports for that m (a point's additions depend on the j-chunks
 *     and the tiles, and on nothing else).  Otherwise they are nb_split_force's sums under another cut: the same membership, the
 *     same terms, its error bounds.  Every rule of nb_split_force's section holds: membership, pair arithmetic, empty sides, the
 *     summation, the handles, the positions read.  In the SUMS the own row and a body at the own position are handled as
 *     nb_split_force handles them (an exact 0, no mask); the exclusion by index applies to the row only.
 *   - Shape: nb_split_force's.  The batch is halved further (the chunks cut again by nb_split_force's rule at every candidate)
 *     only while chunks x batch x cap x 4 bytes exceed 1 GiB: between the 256 MiB one batch of nb_neighbor_lists writes and what
 *     nb_knn's working rows may take, and what N = 262,144 at cap 256 on a Hermite f32 handle needs to keep nb_split_force's shape
 *     (4 chunks x 262,144 points x 256 entries x 4 bytes).  One workgroup's points are the floor of the halving; if very many
 *     short chunks at a large cap still exceed the bound there, the chunks are made longer until they fit.
 *   - State and determinism: the simulation state, the side copies, the captured graphs and the step counter are untouched:
 *     stepping after a call is bit-identical to stepping without it.  No atomics: the same request on the same state gives the
 *     same bits, and a scalar radius and a radii array filled with that value give the same bits.
 *   - Errors: the union of the two calls' rules, each checked before any device call, nb_last_error naming the function and the
 *     field.  NB_ERR_INVALID: NULL handle or request, wrong struct_size, m == 0, unknown flag bits (2u is one: no fp64 audit mode),
 *     all four sums NULL (the message says to use nb_neighbor_lists), points / point_vel given with NB_SPLIT_AT_BODIES, points
 *     missing without it, point_vel missing with a jerk at points or given without one, list NULL, cap outside 1 .. 4096,
 *     reserved != 0, first_body + m > n, neither radii nor radius > 0, radius negative or NaN; on nb_multi a non-NULL jerk pointer.
 *     NB_ERR_STATE: nothing uploaded, nb_set_params not called, a jerk on a leapfrog handle.
 *   - Host pointers: points, point_vel, radii, the sums and count are staged whole (O(m)), `list` batch by batch, as
 *     nb_neighbor_lists stages it; the call blocks until the outputs are written; no pointer is kept.  NB_SPLIT_DEVICE: every
 *     pointer is device memory on the handle's device, read and written in place, enqueued on the handle's stream; the call
 *     returns at once.
 *   - Memory: nb_split_force's partial rows, and an engine-owned buffer, grown on demand and released by nb_destroy, of one
 *     SEGMENT of cap entries per (j-chunk, point of a batch) with the chunk's true count -- a point's offset inside its row is not
 *     known before all of its chunks are done; a second short pass gathers the segments into the rows in ascending chunk order,
 *     pads them and writes the counts.  Bounded as above; nothing is proportional to m x N; the rows are not set beforehand. */
typedef struct nb_split_lists_request {
    uint32_t struct_size;   /* sizeof(nb_split_lists_request) */
    uint32_t m;             /* number of points, >= 1 */
    uint32_t flags;         /* NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE, nb_split_force's meaning */
    uint32_t first_body;    /* NB_SPLIT_AT_BODIES only */
    const void *points;     /* 4*m elements x, y, z, (ignored); NULL with NB_SPLIT_AT_BODIES */
    const void *point_vel;  /* 4*m elements vx, vy, vz, (ignored); required iff a jerk is asked for at points, else NULL */
    const void *radii;      /* optional: m elements of the handle's precision; an element may be 0 */
    double radius;          /* used when radii == NULL; radii or radius > 0 is required */
    void *accel_irr;        /* out, optional (at least one of the four): 4*m elements (ax, ay, az, 0) over the members */
    void *accel_reg;        /* out, optional: 4*m elements over every other row */
    void *jerk_irr;         /* out, optional: 4*m elements (jx, jy, jz, 0); Hermite handles only */
    void *jerk_reg;         /* out, optional: likewise */
    uint32_t cap;           /* entries per row, 1 <= cap <= 4096 */
    uint32_t reserved;      /* must be 0 */
    uint32_t *list;         /* out, required: m * cap indices */
    uint32_t *count;        /* out, optional: m, the TRUE count (may exceed cap) */
} nb_split_lists_request;   /* 104 bytes */
int nb_split_lists(nb_sim *s, const nb_split_lists_request *req);
/* The same on a multi-shard system: evaluated on shard 0 against the caller's UNPADDED n rows; the jerk pointers must be NULL. */
int nb_multi_split_lists(nb_multi *m, const nb_split_lists_request *req);
/* The shape of an m-point request at `cap` entries per row (no device call): the points of the first batch, its j-chunks, the
 * bodies per chunk and the points one workgroup takes (on a Hermite handle: of a request with the jerk pair).  Equal to
 * nb_split_force_shape's answer for the same m wherever the segments fit their bound.  For tests and tools. */
int nb_split_lists_shape(nb_sim *s, uint32_t m, uint32_t cap, uint32_t *batch, uint32_t *chunks, uint32_t *j_per_chunk, uint32_t *rows_per_workgroup);

/* ---- Ahmad-Cohen neighbour scheme with two shared step levels (added within ABI 2.4; no reference analogue) ----
 * A collisional system on a Hermite handle otherwise puts every body on the step its closest encounters need.  With the scheme
 * (Ahmad & Cohen 1973) a body's force is kept as two parts: the IRREGULAR part over the bodies inside its neighbour radius, which
 * changes fast and is re-evaluated every hs = dt / N_sub, and the REGULAR part over every other row, which is evaluated once per dt
 * and extrapolated in between.  Only the list sums -- the entries of the lists, not N x N pairs -- run at the fine step.  Both step
 * levels are shared by all bodies, the radius is fixed (a scalar, or one per body; nb_set_neighbor_adapt below lets it follow a
 * target count), a list that does not fit its row is a reported error.  Hermite handles only.
 *   - Quantities: per body x, v at one instant; the irregular derivatives (ai, ji) over the body's list; the regular derivatives
 *     (ar0, jr0) over every other row, valid at the last regular time t0; the body's row of the list L, of `cap` entries, with its
 *     true count.  Membership is nb_neighbors' rule letter for letter: d2 = fma(dz, dz, fma(dy, dy, dx * dx)) < h * h, strictly, in
 *     the handle's precision, no softening, the own row left out by index.
 *   - Start.  Runs when the scheme's state is not current: after nb_set_neighbor_scheme and after everything that stales a Hermite
 *     handle's derivatives (nb_upload, nb_upload_derivs, nb_device_ptr(NB_BODIES / NB_VEL), a changed G), and after a changed dt
 *     (so that a handle whose dt changes continues exactly as a fresh handle given its (x, v) would), at the next nb_step,
 *     nb_download (accel), nb_download_jerk, nb_device_ptr(NB_ACCEL / NB_JERK) or nb_download_neighbor_scheme.  On (x, v) as they
 *     stand: (ai, ji, ar0, jr0) = the four outputs of nb_split_force at the bodies; L and count = nb_neighbor_lists at the bodies
 *     with the same radius or radii.  Both bit for bit what the public calls return.  (Where nb_neighbor_scheme_fused answers 1 the
 *     start and step 2 + 3 of the regular time are ONE nb_split_lists call: the same bits from one pass over the pairs.)
 *   - Substeps.  One regular step runs s = 0 .. N_sub - 1 with tau = s hs; all polynomial arithmetic is fp64 on the stored values,
 *     each stored value rounded once to the handle's precision, with the expressions of the shared step's predictor and corrector:
 *       1. a = ai + (ar0 + tau jr0), j = ji + jr0;
 *       2. (xp, vp) = the Hermite predictor over hs from (x, v, a, j), for ALL bodies;
 *       3. (ai1, ji1) = the sums of nb_list_force over the body's row of L at the predicted state: points (xp_i, vp_i), entries
 *          gathered from (xp, vp), with its rules (entry e to lane e mod LS, a lane adds in ascending e, the lane sums combined in
 *          the fixed fp64 tree, G multiplied in once, invalid and own entries load row 0 with mass 0);
 *       4. a1 = ai1 + (ar0 + (tau + hs) jr0), j1 = ji1 + jr0;
 *       5. (x, v) <- the Hermite corrector over hs with (a, j, a1, j1);
 *       6. (ai, ji) <- (ai1, ji1).
 *   - Regular time, after the last substep, on the arrived state (x, v):
 *       1. (aio, jio) = the list sums over the OLD list at (x, v);
 *       2. (ai', ji', ar', jr') = nb_split_force at the bodies;
 *       3. L', count' = nb_neighbor_lists at the bodies (the same state as 2: the same membership);
 *       4. aro = (ar' + ai') - aio, jro = (jr' + ji') - jio, in fp64: the regular force with respect to the old list;
 *       5. v += dt/2 (aro - ar0) - dt^2/12 (5 jr0 + jro);
 *       6. x += dt^2/6 (aro - ar0) - dt^3/24 (3 jr0 + jro);
 *       7. (ai, ji, ar0, jr0, L, count) <- the primed values.
 *     5 and 6 are the difference between the Hermite corrector and the Hermite predictor over dt: with every row empty a regular step
 *     is a plain Hermite step of dt in exact arithmetic, with every row holding every other body the substeps are Hermite steps of hs.
 *   - Overflow.  If some count' > cap at a regular time, the state at that time is complete and is kept and steps_done counts the
 *     step, but the next interval would have no consistent list: nb_step returns NB_ERR_STATE (the message names the number of
 *     overflowed rows, the largest count and cap), and so does every later nb_step until nb_set_neighbor_scheme is called again --
 *     a larger cap, a smaller radius or NULL all clear it.  An overflow at the start fails the triggering call with the state
 *     untouched (and every later one, until the scheme is set again or the state changes).
 *   - HOST SYNCHRONISATION.  nb_step with the scheme on synchronises with the device ONCE PER REGULAR STEP: the host reads a small
 *     header (overflowed rows, largest count, entries) from pinned memory.  Such a step cannot be captured into a caller's graph;
 *     ext_stream keeps working otherwise.
 *   - nb_step(k) equals k x nb_step(1) bit for bit, and two handles give the same bits.  dt may change between steps: the first
 *     prediction of a regular step is made at its start, never at the end of the previous one, and the step after a change runs
 *     the start first (the components a regular time leaves were evaluated in front of its correction 5-6; the start's belong to
 *     the corrected state).  dt <= 0 is a no-op.
 *   - nb_download's accel and nb_download_jerk return ai + ar0 and ji + jr0, summed in fp64 and rounded once.  Every query reads the
 *     state at the regular time (nb_field_eval, nb_neighbors, nb_neighbor_lists, nb_knn, nb_list_force, nb_split_force,
 *     nb_diagnostics, frames).  nb_force_pass is unchanged.  nb_enable_timing / nb_step_times2 report one regular step per launch:
 *     force_ms is its span, integrate_ms = 0 (as for block handles).
 *   - Checkpoint: a restore through nb_upload (+ nb_upload_derivs) alone re-runs the start -- the uploaded totals are replaced by
 *     the start's components -- and continues within the scheme's accuracy, NOT bit-identically (the irregular sums a running handle
 *     carries come from the list kernel's order of additions, the start's from nb_split_force's).  nb_upload_neighbor_scheme (below)
 *     hands the running components, rows, counts and radii back and continues bit for bit.
 *   - Switching the scheme off (NULL) leaves a plain Hermite handle whose derivatives are re-evaluated at the next step.
 *   - Errors.  Leapfrog handle: NB_ERR_STATE.  Block steps and the scheme exclude each other: switching either on while the other is
 *     on is NB_ERR_STATE, the message naming both.  NULL handle, wrong struct_size, substeps not a power of two or > 1024,
 *     cap > 4096, flags != 0, radius <= 0 or NaN without radii, a negative or non-finite radii element: NB_ERR_INVALID, checked
 *     before any device call; the message names the function and the field.
 *   - Memory: allocated by nb_set_neighbor_scheme, released by NULL or nb_destroy -- the four component arrays, a second predicted
 *     pair, the list (n x cap x 4 bytes), the counts, a copy of radii, the pinned header.  nb_multi has no counterpart. */
typedef struct nb_neighbor_scheme {
    uint32_t struct_size;  /* sizeof(nb_neighbor_scheme) */
    uint32_t substeps;     /* N_sub: a power of two, 1 .. 1024; 0 -> 8 */
    uint32_t cap;          /* entries per row, 1 .. 4096; 0 -> 128 */
    uint32_t flags;        /* none defined: must be 0 */
    double   radius;       /* used when radii == NULL; must then be > 0 */
    const void *radii;     /* optional: n elements of the handle's precision, >= 0, finite; COPIED by the call */
} nb_neighbor_scheme;      /* 32 bytes */
int nb_set_neighbor_scheme(nb_sim *s, const nb_neighbor_scheme *cfg /* NULL: back to plain Hermite steps */);

/* (a struct TAG without a typedef, as nb_block_stats) */
struct nb_neighbor_scheme_stats {
    uint32_t struct_size, enabled;
    uint64_t regular_steps, substeps, entries;   /* entries = sum of min(count, cap) over the list builds (start included) */
    uint64_t builds;
    uint32_t max_count, overflowed;              /* of the LAST build */
};                                               /* 48 bytes */
/* The counters since the scheme was set or last reset (set out->struct_size).  A Hermite handle without the scheme reports
 * enabled = 0 and zeros. */
int nb_neighbor_scheme_stats(nb_sim *s, struct nb_neighbor_scheme_stats *out, int reset);

/* The scheme's own arrays at the handle's instant (runs the start first if they are not current); any pointer may be NULL.  Blocks.
 * NB_ERR_STATE on a handle without the scheme. */
int nb_download_neighbor_scheme(nb_sim *s, void *accel_irr, void *jerk_irr, void *accel_reg, void *jerk_reg,
                                uint32_t *list /* n * cap */, uint32_t *count /* n */);

/* Which route the next list build of the scheme takes (no device call): *fused = 1 when the start and the regular times call
 * nb_split_lists once -- where its launch shape for (n, cap) is nb_split_force's, so that the four sums stay bit for bit what
 * nb_split_force returns --, 0 when they call nb_split_force and then nb_neighbor_lists (elsewhere, and under
 * NB_FLAG_AC_TWO_CALLS).  Both routes leave the same bits in every array.  0 with NB_OK on a handle without the scheme. */
int nb_neighbor_scheme_fused(nb_sim *s, int *fused);

/* ---- the neighbour scheme on a long run: radii that follow a target count, bit-exact restore (added within ABI 2.4) ----
 * The scheme above cuts every build by the radii it was set with; a system whose density evolves sooner or later puts more than cap
 * members into a row.  With nb_set_neighbor_adapt the engine keeps two per-body arrays in the handle's precision: `built`, the radii the
 * current list was cut by, and `next`, the radii the next build will use.  Both are filled from the scheme's radii (or its scalar
 * radius, rounded once) when adaptation is switched on; the scheme's own copy is never written.  nb_set_neighbor_scheme, with any
 * argument, switches adaptation off; nb_set_neighbor_adapt, with any argument, makes the start run again (and zeroes the counters of
 * nb_neighbor_adapt_stats).  A handle on which these calls are not used runs exactly the code it ran before them.
 *   - A build, at the start and at a regular time, is the pass of the scheme (one nb_split_lists call, or nb_split_force and
 *     nb_neighbor_lists), cut by `next`:
 *       1. the pass; its header (rows with count > cap, largest count, sum of min(count, cap)) is read with the scheme's one host wait;
 *       2. if rows have count > cap and fewer than max_rebuilds rebuilds of THIS build were made: those rows alone get
 *          h <- rnd(h * cbrt((double)n_t / c)), c the row's count, in `next`; back to 1 on the same state (one more host wait);
 *       3. if rows are still over after the last allowed rebuild, the scheme's overflow policy applies to the letter (at the start:
 *          the call fails, the state and `next` are what they were; at a regular time: the state is completed and kept, nb_step
 *          returns NB_ERR_STATE until nb_set_neighbor_scheme is called again);
 *       4. every pass, repeated ones included, counts in nb_neighbor_scheme_stats.builds and adds to .entries.
 *   - After the accepted pass built <- the radii used, and for every row, with c its accepted count, all in fp64:
 *       1. f = cbrt((n_t + 0.5) / (c + 0.5)), clamped to [1.0 / g, g]            (g = grow_max);
 *       2. h' = h * f;
 *       3. h' is clamped to [radius_min, radius_max] where those are > 0;
 *       4. next <- h' rounded once to the handle's precision.
 *     A radius of exactly 0 stays 0: it skips 1-3.  With g = 1 and no clamp next = built, bit for bit.
 *   - Order at a regular time: 1. the old-list sums (step 1 of the scheme's regular time); 2. the build with its rebuilds (steps 2-3);
 *     3. ONE launch that makes the correction (steps 4-7) and applies the rule.  The correction moves x and v, so it runs after the
 *     list is accepted.  aro = (ar' + ai') - aio does not depend on the new radii: any accepted list is consistent with the scheme.
 *   - Checkpoint.  nb_download, nb_download_neighbor_scheme (components, rows, counts) and nb_download_neighbor_radii (`next`) are
 *     the state of a running handle.  Restore, in this order: nb_upload, nb_set_params, nb_set_neighbor_scheme, nb_set_neighbor_adapt
 *     if used, nb_upload_neighbor_scheme LAST.  All six arrays are required; radii is required with adaptation on and becomes `next`
 *     and `built`, with adaptation off it must be NULL.  The call recomputes the totals (ai + ar0, ji + jr0 in fp64, rounded once:
 *     the start's expression) and marks the scheme and the derivatives current for the G and dt in force; it counts no build.  The
 *     next nb_step then equals, bit for bit, the next step of the handle the arrays came from.  Whatever stales the scheme
 *     afterwards (a changed dt or G, nb_upload, ...) runs the start as ever.
 *   - Errors, each before any device call, the message naming function and field.  NB_ERR_INVALID: a NULL handle or request, a wrong
 *     struct_size, flags != 0, target == 0 or 2 target > cap, max_rebuilds > 16, grow_max < 1 (other than 0) or not finite, negative
 *     or non-finite clamps, radius_min > radius_max when both are set; of an upload: a missing array, count[i] > cap, one of the first
 *     count[i] entries of row i >= n or equal to i, a negative or non-finite radius, radii given with adaptation off or missing with
 *     it on.  NB_ERR_STATE: a leapfrog handle, a handle without the scheme, an upload before nb_upload or nb_set_params. */
typedef struct nb_neighbor_adapt {
    uint32_t struct_size;   /* sizeof(nb_neighbor_adapt) */
    uint32_t target;        /* n_t: 1 <= target, 2 * target <= cap of the scheme */
    uint32_t max_rebuilds;  /* per build; 0 -> 4; at most 16 */
    uint32_t flags;         /* none defined: must be 0 */
    double   grow_max;      /* g >= 1: the largest factor per build, the smallest 1 / g; 0 -> cbrt(2.0) */
    double   radius_min, radius_max; /* clamps of a non-zero radius; 0 -> none */
} nb_neighbor_adapt;        /* 40 bytes */
int nb_set_neighbor_adapt(nb_sim *s, const nb_neighbor_adapt *cfg /* NULL: fixed radii again */);

struct nb_neighbor_adapt_stats {
    uint32_t struct_size, enabled;
    uint64_t rebuilds, rows_shrunk;   /* repeated passes, and the rows their shrinks touched, since set or last reset */
    uint32_t last_rebuilds, reserved; /* of the LAST build */
};                                    /* 32 bytes */
int nb_neighbor_adapt_stats(nb_sim *s, struct nb_neighbor_adapt_stats *out, int reset);

/* `built` and `next`, n elements of the handle's precision each (either may be NULL); runs the start first if the scheme is not
 * current.  With adaptation off both hold the scheme's fixed radii.  Blocks. */
int nb_download_neighbor_radii(nb_sim *s, void *built, void *next);

typedef struct nb_neighbor_checkpoint {
    uint32_t struct_size, reserved;                            /* sizeof(nb_neighbor_checkpoint), 0 */
    const void *accel_irr, *jerk_irr, *accel_reg, *jerk_reg;   /* n rows of 4, the handle's precision: nb_download_neighbor_scheme's */
    const uint32_t *list, *count;                              /* n * cap, n */
    const void *radii;                                         /* n: `next`; NULL with adaptation off */
} nb_neighbor_checkpoint;                                      /* 64 bytes */
int nb_upload_neighbor_scheme(nb_sim *s, const nb_neighbor_checkpoint *ck);

/* ---- the neighbour scheme with block individual IRREGULAR steps per body (added within ABI 2.4) ----
 * The scheme above re-evaluates every body's list force at the same fine step dt / N_sub: one tight pair sets N_sub for all n bodies.
 * With nb_set_neighbor_levels every body steps its irregular force at a power-of-two fraction of dt of its own, chosen by the step
 * criterion of the block-step section on the body's TOTAL force.  The regular step, the builds, adaptation, the overflow policy and
 * the regular-time correction stay exactly as they are; only the N_sub shared substeps between two regular times are replaced.
 *   - L = log2(substeps) of the scheme, tick = dt / (double)substeps, T(k) = (double)k * tick.  Body i holds a level l_i in
 *     [min_level, L] and steps by s_i = 2^(L - l_i) ticks.
 *   - Inside one regular step t_i = 0 for all bodies; then, until t_next == 2^L:
 *       1. t_next = min_i (t_i + s_i); the active set is A = { i : t_i + s_i == t_next };
 *       2. EVERY body is predicted to T(t_next) from its own stored (x, v, ai, ji, ar0, jr0) at t_i: a = ai + (ar0 + T(t_i) jr0),
 *          j = ji + jr0, h = (double)(t_next - t_i) * tick, with the predictor expressions of the shared substep, fp64, rounded once
 *          to the handle's precision; always from the stored state, never from an earlier prediction;
 *       3. for i in A: (ai1, ji1) = nb_list_force's sums over i's row at the predicted state (the point (xp_i, vp_i), the entries
 *          gathered from (xp, vp)); every rule of step 3 of the shared substep applies;
 *       4. for i in A: h = (double)s_i * tick, tau0 = T(t_i), tau1 = tau0 + h; a0 = ai + (ar0 + tau0 jr0), j0 = ji + jr0,
 *          a1 = ai1 + (ar0 + tau1 jr0), j1 = ji1 + jr0; the Hermite corrector over h with the shared substep's expressions;
 *          (x, v, ai, ji)_i <- (x1, v1, ai1, ji1), each rounded once;
 *       5. unless NB_NLEV_FROZEN is set, steps 5-6 of the block-step section run with the fp64 totals (a0, j0, a1, j1) of 4 and h:
 *          tau as defined there in fp64, want = level_for(tau) over [min_level, L] (level_for against dt: the smallest l with
 *          dt / 2^l <= tau); want >= l_i is taken; want < l_i coarsens by ONE level, and only if t_next is a multiple of 2 s_i; a
 *          wish finer than L takes L and counts as `clamped`.  The regular part is linear in time and adds nothing to a2 and a3:
 *          a body whose row is empty (min(count, cap) == 0) has tau = infinity and wants min_level;
 *       6. t_i = t_next.
 *     At tick 2^L all bodies stand at the regular time.  Levels persist across regular steps.
 *   - Start of the levels.  Runs when the levels are not current: after the scheme's start has run for any reason, after
 *     nb_upload_neighbor_scheme, and after nb_set_neighbor_levels; at the next nb_step or nb_download_neighbor_levels.
 *     l_i = level_for((eta / 2) |a| / |j|) on a = ai + ar0, j = ji + jr0, summed in fp64 from the stored components; |j| = 0 gives
 *     min_level.  With NB_NLEV_FROZEN every body takes min_level.
 *   - min_level is the accuracy floor: the error of a run is set by the bodies at the coarsest level in use, whatever eta is.  With
 *     min_level = 0 a quiet body's irregular force is stepped with dt itself.
 *   - nb_step(k) equals k x nb_step(1) bit for bit, two handles give the same bits, and every bit is independent of the order in
 *     which the active bodies of a tick are processed.  With every level frozen at L the scheme is the shared scheme at N_sub = 2^L
 *     (bit for bit where dt is a power of two), frozen at 0 it is the shared scheme at N_sub = 1.
 *   - No host wait per tick: the host enqueues one launch for every tick 1 .. 2^L, which leaves at once where no body is due at the
 *     tick or at the one behind it.  The host waits of a regular step stay what they are.  nb_neighbor_scheme_stats.substeps keeps
 *     counting 2^L per step.  The counters of nb_neighbor_level_stats are kept per body on the device and summed when asked for.
 *   - Switching on and off.  nb_set_neighbor_scheme, with any argument, switches levels off, as it switches adaptation off.
 *     nb_set_neighbor_levels leaves the scheme's components and adaptation alone: it makes only the levels stale and zeroes its own
 *     counters.  Levels work with nb_set_neighbor_adapt on or off.  Block steps stay excluded from scheme handles.
 *   - Checkpoint: nb_download_neighbor_levels next to the arrays of the scheme's checkpoint; restore in the scheme's order, then
 *     nb_set_neighbor_levels in front of and nb_upload_neighbor_levels behind nb_upload_neighbor_scheme.  The restored handle
 *     continues bit for bit.
 *   - Errors, each before any device call, the message naming the function and the field.  NB_ERR_STATE: a leapfrog handle, no
 *     scheme set, levels not set (download, upload), an upload before the scheme is current.  NB_ERR_INVALID: a NULL handle, a wrong
 *     struct_size, unknown flag bits, reserved != 0, min_level > log2(substeps), eta < 0 or not finite, an uploaded level outside
 *     [min_level, L]. */
#define NB_NLEV_FROZEN 1u  /* levels never change: min_level everywhere, or what nb_upload_neighbor_levels gave */
typedef struct nb_neighbor_levels {
    uint32_t struct_size;  /* sizeof(nb_neighbor_levels) */
    uint32_t min_level;    /* 0 .. log2(substeps) of the scheme */
    uint32_t flags;        /* NB_NLEV_FROZEN */
    uint32_t reserved;     /* must be 0 */
    double   eta;          /* the accuracy parameter of the step criterion; 0 -> 0.02 */
} nb_neighbor_levels;      /* 24 bytes */
int nb_set_neighbor_levels(nb_sim *s, const nb_neighbor_levels *cfg /* NULL: the shared substeps again */);

struct nb_neighbor_level_stats {
    uint32_t struct_size, enabled;
    uint64_t regular_steps, ticks;    /* ticks = 2^L per regular step */
    uint64_t block_steps;             /* ticks with a due body */
    uint64_t body_steps;              /* correctors */
    uint64_t entries;                 /* sum of min(count, cap) over the body-steps */
    uint64_t clamped;                 /* decisions that wished a level finer than L (the start included) */
    uint32_t finest_level, reserved;  /* the finest level any body held since set or last reset */
};                                    /* 64 bytes */
/* The counters since the levels were set or last reset (set out->struct_size).  Blocks.  A handle without levels: enabled = 0, zeros. */
int nb_neighbor_level_stats(nb_sim *s, struct nb_neighbor_level_stats *out, int reset);
/* n levels at the handle's instant; runs the starts (the scheme's, then the levels') first where they are not current.  Blocks. */
int nb_download_neighbor_levels(nb_sim *s, uint8_t *levels /* n */);
/* After nb_upload_neighbor_scheme (or any call that left the scheme current): the levels are these, the start rule does not run. */
int nb_upload_neighbor_levels(nb_sim *s, const uint8_t *levels /* n */);

/* ---- the 6th-order scheme on a Hermite handle: force, jerk and snap (no reference analogue) ---------------
 * nb_set_hermite_order(s, 6) turns a Hermite handle into the 6th-order predictor-corrector of Nitadori & Makino (2008) with one
 * shared step dt: a higher order at a larger step.  A handle that never calls it runs the 4th-order scheme exactly as before.
 *   - Per pair, with dr = x_j - x_i, dv = v_j - v_i, da = a_j - a_i and rho^2 = |dr|^2 + eps2:
 *         alpha = (dr.dv) / rho^2            beta = (dv.dv + dr.da) / rho^2 + alpha^2
 *         A = m_j dr / rho^3
 *         J = m_j dv / rho^3 - 3 alpha A                      ( = s3 t,  t = dv - 3 alpha dr,  s3 = m_j / rho^3 )
 *         S = m_j da / rho^3 - 6 alpha J - 3 beta A           ( = s3 (da - 6 alpha t - 3 beta dr) )
 *     Each of the nine components is ONE sum s3 (...); no self mask (for j = i all nine terms are exactly 0); G multiplies each row
 *     once in fp64; the chunks of the j-range are added in ascending order in fp64; on f32 handles a chunk is summed in binary32 in
 *     two levels with at most 1,024 terms per register, as the force+jerk pass.
 *   - State: (x, v) at one instant plus the derived a, j, s (snap, d2a/dt2) and c (crackle, d3a/dt3), all in the handle's precision.
 *   - One step, h = dt, the polynomials in fp64 (Horner, fused), each stored value rounded once:
 *         xp = x + h v + h^2/2 a + h^3/6 j + h^4/24 s + h^5/120 c
 *         vp = v + h a + h^2/2 j + h^3/6 s + h^4/24 c
 *         ap = a + h j + h^2/2 s + h^3/6 c
 *         (a1, j1, s1) = FJS(xp, vp, ap)                    -- the only O(N^2) pass of the step
 *         v1 = v + h/2 (a + a1) - h^2/10 (j1 - j) + h^3/120 (s + s1)
 *         x1 = x + h/2 (v + v1) - h^2/10 (a1 - a) + h^3/120 (j + j1)
 *         P = a1 - a - h j - h^2/2 s;   Q = h (j1 - j - h s);   R = h^2 (s1 - s)
 *         c1 = (60 P - 36 Q + 9 R) / h^3                    -- p'''(t1) of the quintic through (a, j, s) at both ends
 *         state <- (x1, v1, a1, j1, s1, c1)
 *     The a1, j1, s1 of the corrector and of c1 are the values as stored; v1 enters x1 before it is rounded.  The mass lane and vel.w
 *     are carried; the .w of a, j, s and c is 0.
 *   - Start.  Runs when the snap is not current: after nb_set_hermite_order(6) and after anything that makes the derivatives of a
 *     Hermite handle stale (see above; a changed G among them).  (a, j) come from the force+jerk pass on (x, v) -- the bits an order-4
 *     handle holds --, s from the force+jerk+snap pass on (x, v, a) (its a and j are discarded), c = 0.  With c = 0 the first step
 *     has a local error of O(h^6), the order of the scheme's global error: no iteration.  dt may change between steps.
 *   - nb_set_hermite_order(s, 4) frees s and c; (a, j) stay current.
 *   - Unchanged on an order-6 handle: nb_download (accel), nb_download_jerk, nb_device_ptr(NB_ACCEL / NB_JERK), every query,
 *     nb_diagnostics, frames (they read bodies and vel), dt <= 0 is a no-op, nb_step(k) equals k x nb_step(1) bit for bit, two handles
 *     give the same bits, plain launches, ext_stream.
 *   - Changed: nb_force_pass first makes the derived arrays current (the start, where it is due: the pass streams the accelerations), then
 *     runs the force+jerk+snap pass and its reduce into scratch: bodies and vel are untouched, and so are current derivatives; nb_step_times2:
 *     force_ms = that kernel and its reduce, integrate_ms = predictor + corrector; nb_variant_name starts with "hermite6_";
 *     nb_shape_info reports the chunks of the force+jerk+snap pass.
 *   - Checkpoint: nb_download (accel), nb_download_jerk, nb_download_snap; restore with nb_upload, nb_set_params,
 *     nb_set_hermite_order(6), nb_upload_derivs6: the next step equals the source handle's bit for bit.
 *   - Errors, each before any device call, the message naming the function and the field.  NB_ERR_INVALID: a NULL handle, an order
 *     other than 4 or 6, a NULL array of nb_upload_derivs6.  NB_ERR_STATE: a leapfrog handle (all four calls); order 6 while block
 *     steps or the neighbour scheme are switched on; nb_set_block_steps or nb_set_neighbor_scheme with a non-NULL argument on an
 *     order-6 handle; nb_upload_derivs on an order-6 handle (see nb_upload_derivs6); nb_download_snap or nb_upload_derivs6 on an
 *     order-4 handle.
 *   - Block steps on an order-6 handle: nb_set_block_steps6 below.  Not built: the neighbour scheme and the 8th order on order-6
 *     handles. */
int nb_set_hermite_order(nb_sim *s, uint32_t order /* 4 or 6 */);
int nb_hermite_order(nb_sim *s, uint32_t *order);
/* 4*n elements each of the handle's precision, either pointer may be NULL; runs the start first if needed.  Blocks. */
int nb_download_snap(nb_sim *s, void *snap, void *crackle);
/* All four arrays are required, 4*n elements each; after nb_upload.  Marks the derivatives current. */
int nb_upload_derivs6(nb_sim *s, const void *accel, const void *jerk, const void *snap, const void *crackle);

/* ---- block individual time steps on an order-6 handle (no reference analogue) -----------------------------
 * nb_set_block_steps6 gives every body of an order-6 Hermite handle a step of its own (Nitadori & Makino 2008, the production setup
 * of phi-GPU): the higher order divides the number of block steps a hierarchy needs.  The scheme is that of "block individual time
 * steps" above with steps 2 - 5 replaced; ticks, levels, level_for, the active set, the coarsen-by-one-when-aligned rule,
 * `clamped`, `finest_level` and the last block step of an outer step restarting the clock are unchanged.  nb_set_block_steps and
 * nb_set_hermite_order keep their behaviour: nb_set_block_steps(non-NULL) on an order-6 handle and nb_set_hermite_order(6) on an
 * order-4 handle with block steps stay NB_ERR_STATE.
 *   - Start (levels not current): the order-6 start makes (a, j, s) current with c = 0, then l_i = level_for((eta / 2) |a_i| / |j_i|);
 *     |j_i| = 0 gives min_level (the order-4 rule).
 *       2. EVERY body is predicted from its own stored (x, v, a, j, s, c) at t_i over (t_next - t_i) ticks with xp, vp, ap of the
 *          shared order-6 step (fp64, Horner, fused, each rounded once) -- always from the stored state;
 *       3. (a1, j1, s1) of i in A against all n predicted rows (xp, vp, ap); all nine self terms are exactly 0;
 *       4. the corrector and c1 = (60 P - 36 Q + 9 R) / h^3 of the shared order-6 step over h = s_i ticks:
 *          (x, v, a, j, s, c)_i <- (x1, v1, a1, j1, s1, c1);
 *       5. (NB_F64, not frozen) from the same P, Q, R, in fp64 on the values as stored:
 *            a4 = (360 P - 192 Q + 36 R) / h^4            -- the quintic's fourth derivative at the end of the step
 *            a5 = (720 P - 360 Q + 60 R) / h^5
 *            tau = cbrt(sqrt(eta^3 (|a1| |s1| + |j1|^2) / (|c1| |a5| + |a4|^2))), inf when the denominator is 0.
 *          This is Nitadori & Makino's dt = eta_NM (A1 / A4)^(1/3) with eta_NM = sqrt(eta): eta keeps Aarseth's scale, its default
 *          0.02 corresponds to eta_NM ~ 0.14.  Step 6 is unchanged.
 *   - Configuration: the nb_block_steps struct, with the defaults and argument checks of nb_set_block_steps.  NULL switches back to
 *     the shared order-6 step; nb_set_block_steps(s, NULL) does the same.
 *   - Precision.  With binary32 storage a4 and a5 are rounding noise (on a 300-body system with a tight pair every body went to the
 *     deepest level and nearly every decision was clamped): an NB_F32 handle without NB_BLOCK_FROZEN is NB_ERR_STATE.  With
 *     NB_BLOCK_FROZEN it works: the levels are fixed, or uploaded by a host that brings its own criterion.
 *   - While it is on: nb_block_stats, nb_download_levels, nb_upload_levels, nb_download, nb_download_jerk, nb_download_snap, the
 *     queries and nb_diagnostics keep their meaning; nb_upload_derivs6 works and marks the derivatives current; nb_step(k) advances
 *     by k x dt, equals k x nb_step(1) bit for bit, and two handles give the same bits; dt <= 0 is a no-op; nb_variant_name keeps its
 *     "hermite6_" prefix; timing reports one outer step per launch (as for order 4); nb_force_pass keeps its order-6 meaning.
 *     nb_set_hermite_order(4) and nb_set_neighbor_scheme(non-NULL) are NB_ERR_STATE.
 *   - Checkpoint: (bodies, vel, accel, jerk, snap, crackle, levels); restore with nb_upload, nb_set_params,
 *     nb_set_hermite_order(6), nb_upload_derivs6, nb_set_block_steps6, nb_upload_levels: the restored handle continues bit for bit.
 *     nb_set_block_steps6 leaves the state and all six derived arrays as they are; only the levels go stale.
 *   - Staleness: the order-4 rules.  Everything that stales the derivatives, a change of dt or G and the setter itself stale the
 *     levels; stale levels are made by the start rule at the next nb_step or nb_download_levels.
 *   - Errors: a NULL handle is NB_ERR_INVALID; an order-4 or leapfrog handle is NB_ERR_STATE with a message that names
 *     nb_set_hermite_order; the argument checks are those of nb_set_block_steps, the message naming nb_set_block_steps6 and the field.
 *   - By default the start rule is order 4's and the first step runs with c = 0: on systems with hard pairs the first outer step
 *     makes most of a run's energy error (profiles/r21/block6.md).  nb_set_start6(s, NB_START6_CRACKLE) below is the start of its own.
 *   - Block steps without the host wait per block step: nb_set_block_batch6 (beside nb_set_block_batch, above).
 *   - Not built: the neighbour scheme on order-6 handles. */
int nb_set_block_steps6(nb_sim *s, const nb_block_steps *cfg /* NULL: back to the shared order-6 step */);

/* ---- the start of an order-6 handle: exact crackle, two-rule levels (no reference analogue) ----------------
 * nb_set_start6 chooses how the engine makes the starts of an order-6 handle ITSELF: after nb_upload, after a changed G, wherever the
 * start of "the 6th-order scheme" above runs.  A handle that never calls it starts as before (NB_START6_ZERO), bit for bit.
 *   - NB_START6_CRACKLE: a, j and s are made as before (the same bits); c is the direct sum of the pair crackles on (x, v, a, j).
 *     Per pair, with dj = j_j - j_i and y^2 = 1 / rho^2 next to the dr, dv, da, s3, alpha, beta, t of the snap:
 *         alpha = (dr.dv) y^2
 *         beta  = (dv.dv + dr.da) y^2 + alpha^2
 *         gamma = (3 dv.da + dr.dj) y^2 + alpha (3 beta - 4 alpha^2)
 *         t = dv - 3 alpha dr
 *         q = da - 6 alpha t - 3 beta dr
 *         w = dj - 9 alpha q - 9 beta t - 3 gamma dr
 *         c_i = G sum_j m_j y^3 w
 *     Each of the three components is ONE sum s3 (...); no self mask (for j = i the term is exactly 0); a row past the range adds
 *     nothing; G multiplies each row once in fp64; chunks and the two-level binary32 sums of f32 handles are the snap pass's.
 *   - The two-rule start of nb_set_block_steps6 (dynamic levels, NB_F64 handles) at NB_START6_CRACKLE, in fp64 on the values as stored:
 *         l_i = max(level_for((eta / 2) |a| / |j|), level_for(sqrt(eta (|a| |s| + |j|^2) / (|j| |c| + |s|^2))))
 *     A rule whose denominator is 0 votes min_level.  A body counts once in `clamped` if either rule found no level.  Frozen handles
 *     and uploaded levels are untouched by the mode.
 *   - A start that arrived through nb_upload_derivs6 is kept as uploaded.  The setter drops a start the engine made itself that no step
 *     has consumed yet (nb_download_snap, the setter, nb_download_snap shows the new c), and levels the engine chose itself that no block
 *     step has consumed; uploaded levels stay.  On a handle that has stepped the setter changes nothing about the running state: the run
 *     continues bit for bit as a twin without the call; the mode governs the next start.
 *   - nb_set_hermite_order(s, 4) returns the mode to NB_START6_ZERO.  f32 and f64 handles both take it.
 *   - Errors: a NULL handle and an unknown mode are NB_ERR_INVALID; a leapfrog handle or an order-4 handle is NB_ERR_STATE.
 *   - Not built: an iterated start; a start rule for order-4 handles; dynamic order-6 levels on f32 handles. */
#define NB_START6_ZERO    0u   /* today's start: snap from the pass, c = 0, block levels from (eta / 2)|a|/|j| */
#define NB_START6_CRACKLE 1u   /* c = the direct sum above; dynamic block levels from the two-rule start */
int nb_set_start6(nb_sim *s, uint32_t mode);
int nb_start6(nb_sim *s, uint32_t *mode);

/* ---- the force+jerk pass of an NB_F64 Hermite handle in mixed precision: double-single differences (no reference analogue) ----
 * nb_set_pass_precision(s, NB_PASS_MIXED) makes every force+jerk pass of an NB_F64 Hermite handle of order 4 run binary32 pair
 * arithmetic on positions carried as a double-single pair of binary32 words (GRAPE-6, Sapporo, phi-GPU).  The STATE is unchanged:
 * fp64 x, v, a, j, levels, every download and every checkpoint.  A handle that never calls the setter runs the native fp64 pass.
 *   - Per body, from the fp64 row the pass reads
 *         xh = (float)x      xl = (float)(x - (double)xh)      vf = (float)v      mf = (float)m
 *   - Per pair, all in binary32, the two differences formed first and then added:
 *         dr = (xh_j - xh_i) + (xl_j - xl_i)        dv = vf_j - vf_i
 *     and from there the f32 handles' sequence: rho^2 = dr.dr + eps2, y = rsq(rho^2), s3 = (mf_j y) y^2, q = (dr.dv) y^2,
 *     a_i += s3 dr, j_i += s3 (dv - 3 q dr) (one sum per component).  No self mask: for j = i the term is exactly 0.
 *   - Sums: binary32 in two levels (at most 1,024 terms per register, then the j-chunk), then fp64 across the j-chunks in ascending
 *     order, times G once, stored as double.  The j-chunks are a function of (n, the device's CU count), and of the active count for
 *     the gathered pass of a block step: the summation order is fixed, two handles give the same bits.
 *   - Accuracy.  dr is good to ~1e-7 OF ITSELF however close the pair is (binary32 positions at |x| ~ 1: 6e-8 / |dr|), so the
 *     accelerations of a hard pair and the block-step criterion's differences of them are those of the fp64 pass to ~1e-6, and
 *     dynamic levels follow the fp64 schedule.  It does NOT give fp64 derivatives: a and j carry binary32 pair-arithmetic and
 *     summation error of about 1e-6 of the row's scale, velocities enter as binary32.  "Of the row's scale" matters for a body
 *     whose sum is dominated by one partner: the other bodies' terms are added to a binary32 register that holds the partner's, and
 *     those below half an ulp of it are lost -- pairs 2e-4 apart at N = 1,025 keep their mutual force to 1e-7 and their row to 1e-5,
 *     but lose most of the external field on their members.  An energy audit to 1e-12 needs the native pass.
 *   - With NB_PASS_MIXED every force+jerk pass the handle runs is the mixed one: the start, the shared step, the gathered pass of
 *     nb_set_block_steps (dynamic and frozen) and nb_force_pass.  The queries (nb_field_eval, nb_list_force, nb_split_*, ...) are untouched.
 *   - The mode takes effect from the next pass on.  The setter touches no state and marks nothing stale, neither the derivatives nor
 *     the levels: the restore order nb_upload, nb_upload_derivs, nb_set_pass_precision, nb_set_block_steps, nb_upload_levels (the setter
 *     anywhere in it) continues bit for bit.  It allocates three binary32 rows per body, released by NB_PASS_NATIVE and nb_destroy.
 *   - nb_variant_name starts with "hermite4_f64mx_"; nb_shape_info reports the mixed pass's j-chunks.
 *   - Errors: a NULL handle, a NULL out pointer and an unknown mode are NB_ERR_INVALID; a leapfrog handle, an NB_F32 handle, an
 *     order-6 handle and a handle with the neighbour scheme on are NB_ERR_STATE.  On a mixed handle nb_set_hermite_order(6) and
 *     nb_set_neighbor_scheme(non-NULL) are NB_ERR_STATE until the mode is NB_PASS_NATIVE again.
 *   - Not built: mixed passes for order 6, for the neighbour scheme and for the queries; double-single velocities (compensated
 *     sums of the near terms: nb_set_pass_guard below);
 *     nb_multi; anything on NB_F32 handles. */
#define NB_PASS_NATIVE 0u   /* the handle's own precision (default) */
#define NB_PASS_MIXED  1u   /* double-single differences, binary32 pair arithmetic, fp64 across chunks */
int nb_set_pass_precision(nb_sim *s, uint32_t mode);
int nb_pass_precision(nb_sim *s, uint32_t *mode);

/* ---- guarded sums of the mixed pass: the external field on hard pairs (no reference analogue) ----
 * nb_set_pass_guard(s, r_near) gives the mixed pass of a handle whose pass precision is NB_PASS_MIXED a GUARD RADIUS: the terms of
 * pairs closer than r_near leave the binary32 registers and are summed apart, compensated.  It is for the quantity that plain
 * NB_PASS_MIXED loses (above): the field of the rest of the system on the members of a hard pair, and with it the acceleration and
 * jerk of the pair's barycentre, where the partner's terms cancel.  r_near = 0 (the default) is plain NB_PASS_MIXED.
 * With a guard, every force+jerk pass of the handle -- the start, the shared step, the gathered pass of nb_set_block_steps and
 * nb_force_pass -- is defined as follows.
 *   - The per-pair arithmetic is exactly NB_PASS_MIXED's, up to and including s3, dr and t = dv - 3 q dr.
 *   - A pair is NEAR iff binary32 d2 < (float)(r_near * r_near): strict, and d2 is the value the pass has, rho^2 with eps2 in it.
 *   - A FAR pair's terms go where they go without a guard: fma into the binary32 two-level sums.
 *   - A NEAR pair's terms p = s3 * dr and p = s3 * t (rounded products) go into a second sum per component, kept as an unevaluated
 *     binary32 pair (hi, lo) by branch-free TwoSum:
 *         s = hi + p;  bb = s - hi;  e = (hi - (s - bb)) + (p - bb);  hi = s;  lo += e
 *     in ascending j.  It is never flushed.
 *   - Per j-chunk the partial row is ((double)far + (double)hi) + (double)lo, formed in the kernel's epilogue and stored as fp64
 *     (the partial rows of a guarded handle are fp64 rows; the setter sizes them as nb_set_pass_precision does).
 *   - Across chunks: fp64, ascending, times G once, as without a guard.
 * Properties:
 *   - A row's bits depend on the state and r_near only, not on which rows share its wave: where some lane of a wave has a near pair
 *     every lane takes the slow sums, in which a lane without a near pair does exactly the fast path's fma, and a lane's near sum
 *     takes p = 0 for far pairs -- TwoSum with 0 changes neither word.
 *   - With r_near^2 <= eps2 no pair is near, and every array is plain NB_PASS_MIXED's bit for bit.
 *   - The self pair is near when r_near^2 > eps2 and contributes exactly 0.
 * Choosing r_near: everything outside r_near still enters binary32 registers, so r_near must cover the partners whose terms exceed the
 * rest of the row by orders of magnitude, and no more: choose it so that a body has O(1) others inside it, for example a quarter of
 * the mean interparticle distance.  When a third body enters the near set accuracy is kept, because the near sum is compensated;
 * when hundreds do, the pass only gets slower.  What it does NOT give: fp64 derivatives.  Pair arithmetic stays binary32 (1e-7 of
 * the pair's term), velocities enter as binary32, and the far sums keep their binary32 summation error relative to the FAR field.
 *   - The setter is valid only while the handle's pass precision is NB_PASS_MIXED; otherwise NB_ERR_STATE, with a message that names
 *     nb_set_pass_precision (a leapfrog handle, an NB_F32 handle, an order-6 handle, a native NB_F64 handle).  r_near negative, NaN
 *     or infinite: NB_ERR_INVALID.  A NULL handle or out pointer: NB_ERR_INVALID.  The getter works on every Hermite handle and
 *     returns 0 where the guard is off.  nb_set_pass_precision(NB_PASS_NATIVE) puts the guard back to 0.
 *   - Like nb_set_pass_precision the setter touches no state and marks nothing stale, neither the derivatives nor the levels; it
 *     holds from the next pass on and may stand anywhere in a restore after nb_set_pass_precision.
 *   - nb_variant_name starts with "hermite4_f64mxg_" while a guard is set; the j-chunks are the mixed pass's.
 *   - Not built: a guard for order 6, the neighbour scheme, the queries or NB_F32 handles; a per-body or adaptive radius. */
int nb_set_pass_guard(nb_sim *s, double r_near);   /* 0 = off (default) */
int nb_pass_guard(nb_sim *s, double *r_near);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* NBODY3D_HIP_H */
