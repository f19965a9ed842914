// nb_internal.h -- state shared by the translation units of libnbody3d_hip.so
// (nb_engine.hip: single handle; nb_comm.hip: RCCL loader, per-process collective,
// nb_multi).  Not part of the ABI.
#pragma once
#include "../../include/nbody3d_hip.h"
#include "nb_plan.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

// Kernel-exact timing: the events are handed to hipExtLaunchKernel, which stamps them at the
// kernel's own begin and end (no marker packets between the kernels of a step).
// e[0]..e[1]: force launch issued before a pending gather is waited for (or the only force
// launch, or the whole fused step); e[3]..e[4]: force launch issued after it; e[6]..e[2]: integrate;
// e[2]..e[5]: position exchange (RCCL all-gather on the engine stream; e[5] is a plain record).
// Rank form of the symmetric pass (plain records on the engine stream): e[0] force pass e[7] nb_sym_reduce e[1]
// ncclReduceScatter e[6] integrate e[2] ncclAllGather e[5]; with the overlapped gather the force pass is two launches,
// e[0]..e[7] (own-row sweeps, issued before the wait) and e[3]..e[4] (the rest), and `rs` says the e[7]/e[1]/e[6] chain is valid.
struct nb_events { hipEvent_t e[8]; bool two, xchg, rs, blk; };   // blk: one outer step of a block-step handle, e[0]..e[1]

struct nb_rccl;   // nb_comm.hip

struct nb_frame_slot {
    float* h_bodies = nullptr;     // pinned host, 4*n floats
    float* h_speed = nullptr;      // pinned host, n floats
    float* d_bodies = nullptr;     // device staging
    float* d_speed = nullptr;
    hipEvent_t packed = nullptr;   // staging written (engine stream)
    hipEvent_t landed = nullptr;   // host copy complete (frame stream)
    uint64_t step = 0;
    bool in_flight = false, valid = false;
};

struct nb_sim {
    uint32_t n = 0, sb = 0, sc = 0;
    bool f64 = false;
    size_t esz = 4;
    int device = 0;
    bool no_device = false;        // nb_plan_query on a host without a GPU: the planner skips its occupancy queries
    double eps2 = 1e-4;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // bodies[cur] is the live position array.  The fused step (force + integrate in ONE launch)
    // reads bodies[cur] and writes bodies[cur ^ 1] (ping-pong: removes the in-place race of the
    // reference, nbody3d.js:283 vs :257); two-kernel steps stay in bodies[cur].
    void* bodies[2] = {nullptr, nullptr};
    int cur = 0;
    bool own_bodies = false;
    // The j-stream of the packed f32 K1 forms (LDS-tile, SGPR, fused, registers-only): rows (x, y, z, G*m), so that a pair
    // multiplies (G*m_j)*inv as the reference does (nbody3d.js:236) at no per-pair cost.  With G == 1 it IS bodies[k]
    // (no copy); otherwise gm[k] goes with bodies[k]: rebuilt by nb_gm_pack when the positions were written from outside the
    // step (upload, exchange, raw pointer) or G changed, and kept current by K2 / the fused epilogues for the rows they write.
    void* gm[2] = {nullptr, nullptr};
    bool gm_ok = false;            // gm[cur] matches bodies[cur] and gm_G
    double gm_G = 0.0;
    void* vel = nullptr;
    void* acc = nullptr;
    void* partial = nullptr;
    size_t partial_bytes = 0;      // what `partial` was allocated with (nb_create checks it against the handle's form)
    double* diag = nullptr;
    void* zero_row = nullptr;      // 64 zero bytes (LDS-DMA source for j past the range)
    uint32_t diag_blocks = 0, diag_chunk = 256;   // nb_diag: workgroups (row blocks x j-chunks), bodies per j-chunk
    double dt = 0.0, G = 0.0;
    bool params_set = false, uploaded = false;
    uint64_t steps_done = 0;
    // launch shape
    int ipl = 1, ls = 1;
    bool packed = false;   // nb_force_pk (f32 only)
    bool sgpr = false;     // nb_force_pk_sgpr: j broadcast from SGPRs instead of the LDS tile
    int ws = 1;            // SGPR kernel: waves of a workgroup that split the j-range (1 or 4)
    int tl = 1;            // LDS kernels: 256-body tiles staged at once (1 or 4)
    bool fused = false;    // nb_step_fused / nb_step_direct: K2 folded into K1's epilogue (jsplit == 1, whole system)
    bool direct = false;   // nb_step_direct: the fused step with each lane's j-bodies in registers (N <= 2,048)
    // nb_step_jpk: the fused step with the j-bodies streamed as SGPR pairs from a pair-transposed copy
    // of the positions (pairs[k] goes with bodies[k]); js > 1 splits j over workgroups that meet at a ticket
    bool jpk = false;
    void* pairs[2] = {nullptr, nullptr};
    bool pairs_ok = false;         // pairs[cur] matches bodies[cur] and pairs_G
    double pairs_G = 0.0;          // G folded into the mass lanes of pairs[cur]
    void* jpartial = nullptr;      // jsplit x 64-row blocks of partial sums (jsplit > 1)
    uint32_t* tickets = nullptr;   // one arrival counter per i-block, zero between launches
    uint32_t junits = 0;           // 4-pair units per wave
    bool poison = false;           // NB_FLAG_POISON
    bool jpk_fenced = false;       // NB_FLAG_JPK_FENCED: release-fenced ticket instead of write-through partial stores
    int acc_parity = 0;    // swap_acc: how often acc/partial have swapped roles (mod 2)
    bool swap_acc = false; // two-kernel step with jsplit == 1: K2 reads the partial as a_new and the
                           // acc/partial buffers swap roles (96 B per body)
    uint32_t jsplit = 1, j_per_split = 0;
    // nb_force_sym: the symmetric force pass (each unordered pair once, both accelerations); whole-system f32 handles.
    // bodies / gm are allocated with sym_np >= n rows (zero-mass padding); `partial` holds sym_layers x sym_np rows.
    bool sym = false;
    uint32_t sym_np = 0, sym_layers = 0;
    uint32_t sym_plan[16] = {0};   // nb::SymPlan / nb::SymWPlan, kept as plain words here (nb_comm.hip does not see the kernels' types)
    bool symw = false;             // wave-granular form (nb_force_symw): sym_plan holds a SymWPlan, sym_tab the per-super-block table
    uint32_t* sym_tab = nullptr;   // device: {first wave, resident layers} per super-block
    std::vector<uint32_t> sym_tab_host;
    void* sym_spill = nullptr;     // ups > 1: one spill row set per wave (traveler sums of the sweep a wave's range starts inside)
    uint32_t sym_spill_rows = 0;
    uint32_t sym_pieces = 0;       // pieces (several sweeps, one resident layer each) in the shared queue of nb_force_symw (nb_plan.cpp::lay_out_symw)
    bool single_sweeps = false;    // NB_FLAG_SINGLE_SWEEPS: nb_force_symw<NG, 1> instead of nb_force_symw_pairs<NG>
    uint32_t* sym_queue = nullptr; // device: the queue's draw counter, zeroed in front of every force launch
    // The equal-mass kernels (nb_force_symw_eqm / nb_force_symw_pairs_eqm): a whole-system f32 handle of the wave-granular form whose plan has
    // no padding rows may run them while every bodies.w is the same bits and every vel.w / acc.w is zero (nb_engine.hip, ensure_eqm).
    bool eqm_capable = false;      // the handle's form and plan allow it (and NB_FLAG_NO_EQM is not set)
    enum { kEqmUnknown = 0, kEqmYes = 1, kEqmNo = 2 };
    int eqm = kEqmUnknown;         // nb_upload decides on the host; a pointer handed out makes it unknown, nb_eqm_check re-decides before the next step
    uint32_t* eqm_flag = nullptr;  // device: what nb_eqm_check writes
    uint32_t eqm_m0 = 0;           // the bits of row 0's mass lane, kept when eqm becomes kEqmYes: with the current G they decide the form (eqm_form)
    bool no_eqm_pow2 = false;      // NB_FLAG_NO_EQM_POW2: the equal-mass kernels keep their mass product (form 1) whatever G*m is
    hipError_t force_err = hipSuccess;   // launch_force: the reset of the queue's draw counter failed (picked up by whoever launched it)
    // rank form (NB_FLAG_SYM_SHARD: a shard handle whose cross-rank reduction the engine's native exchange provides): the
    // handle's own rows are the resident super-blocks [sym_g0, sym_g1); sym_A[np] = this rank's sums for EVERY row, reduce-
    // scattered across the ranks before the integrate kernel reads the rank's own rows of it
    bool sym_rank = false;
    uint32_t sym_g0 = 0, sym_g1 = 0;
    uint32_t sym_rank_plan[16] = {0};   // nb::SymRankPlan: the two phases (own-row travelers first), their wave counts and layer bases
    std::vector<nbp::LaunchPlan::SymPass> sym_passes;   // the passes over the ring distances (one, or several when the layers of one would not fit)
    uint32_t sym_pass = 0;              // the pass launch_force runs
    bool sym_local = false;             // the rank-form pipeline of a WHOLE system on this device: no communicator, no collectives
    void* sym_A = nullptr;
    std::string variant, err;
    nb_exchange_fn xfn = nullptr;
    nb_exchange_wait_fn xwait = nullptr;   // non-null: two-phase (overlapped) exchange
    void* xuser = nullptr;
    bool gather_pending = false;           // begin() called, wait() not yet
    uint32_t own_split0 = 0, own_splits = 0;   // j-splits lying entirely inside this shard's rows
    nb_rccl* rccl = nullptr;               // per-process RCCL communicator (nb_rccl_attach)
    bool timing = false;
    // HIP-graph replay of multi-step calls (launch-bound small N): kGraphChunk steps captured
    // once per (dt, G, buffer parity) and replayed
    struct graph_slot {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        double dt = 0.0, G = 0.0;
        int parity = 0;
        int form = 0;                // the force kernel's form it was captured with (eqm_form)
    } graphs[2];                     // [0]: kGraphChunk steps, [1]: kGraphBig steps (a replay costs the host
                                     // ~10-16 us: amortised over 128 steps it stops showing at N ~ 1,024)
    bool graphs_ok = true;           // cleared if capture ever fails: fall back to plain launches
    std::vector<nb_events> pool;     // recycled events
    std::vector<nb_events> pending;
    size_t pool_next = 0;
    // viewer frame feed
    hipStream_t frame_stream = nullptr;
    static constexpr int kFrameSlots = 4;   // the host may run this many snapshots ahead of the copies
    nb_frame_slot frame[kFrameSlots];
    int frame_next = 0;              // slot the next request writes
    int frame_latest = -1;           // most recently requested slot
    // The queries (nb_field_eval, nb_neighbors, nb_neighbor_lists, nb_knn, nb_list_force, nb_split_force, nb_split_lists): engine-owned
    // buffers by role, grown on demand, released by nb_destroy.  They share them: no two requests overlap on the stream, and within one
    // request no two arrays take the same slot.  q_in / q_out stage a host-pointer request's inputs ([0] points, [1] radii or counts,
    // [2] point velocities, [3] list rows) and its outputs, whole (O(m)) or one batch at a time; q_part holds the partial rows per
    // (j-chunk, point of a batch) and q_off nb_neighbor_lists' uint32 offsets per (j-chunk, point of a batch): a bounded number of
    // rows whatever m and n are; q_work holds nb_knn's working rows, bounded by its memory rule; q_inf is one row at +inf, the LDS-DMA
    // source of the f32 neighbour kernels for j past the range: written once, never used for anything else.  q_out[4], [5] stage the rows
    // and the counts of nb_split_lists (whose four sums take [0] .. [3]); q_seg holds its segments -- cap uint32 per (j-chunk, point of a
    // batch), under its own bound -- and q_segcnt the chunks' true counts.
    int n_cu = 256;
    struct field_buf { void* p = nullptr; size_t cap = 0; } q_in[4], q_out[6], q_part, q_off, q_work, q_inf, q_seg, q_segcnt;
    field_buf knn_stat;       // the calibration build's counters (NB_TUNING with NB_KNN_STATS set): never allocated otherwise
    // NB_INT_HERMITE4: bodies[0] / vel are the state at ONE instant, acc / jerk the derivatives derived from it.  None of the
    // leapfrog launch fields above is used: plain unpadded arrays, no planner, no graphs.
    bool hermite = false;
    void* jerk = nullptr;
    void* hx = nullptr;            // the predicted positions (xp, with the mass lane), then a1: what nb_fj_reduce leaves for the corrector
    void* hv = nullptr;            // the predicted velocities (vp), then j1
    void* fj_part = nullptr;       // 2 x fj_chunks x n rows of partial sums: accelerations, then jerks
    uint32_t fj_chunks = 1, fj_per = 0;   // the force+jerk pass's j-chunks (grid.y) and bodies per chunk (whole 256-row tiles)
    bool derivs_ok = false;        // acc / jerk belong to (bodies, vel) and derivs_G
    bool derivs_any_G = false;     // nb_upload_derivs before the first nb_set_params: the derivatives belong to whatever G comes
    double derivs_G = 0.0;
    // nb_set_hermite_order(6): the 6th-order scheme on force, jerk and snap (kernels/hermite6.hip.h).  Allocated by the call,
    // released by order 4 or nb_destroy.  Off: none of this is read.
    bool h6 = false;
    void* snap = nullptr;          // d2a/dt2 of the state
    void* crackle = nullptr;       // d3a/dt3: 0 after a start, the corrector's c1 afterwards
    void* ha = nullptr;            // the predicted accelerations (ap), then s1 (hx / hv hold xp / vp, then a1 / j1)
    void* h6_part = nullptr;       // 3 x h6_chunks x n rows of partial sums: accelerations, jerks, snaps
    uint32_t h6_chunks = 1, h6_per = 0;   // the force+jerk+snap pass's j-chunks and bodies per chunk
    bool snap_ok = false;          // snap / crackle belong to the current acc / jerk (which derivs_ok and derivs_G speak for); cleared by
                                   // ensure_derivs whenever it re-evaluates acc / jerk, set by the start and by nb_upload_derivs6
    // nb_set_pass_precision(NB_PASS_MIXED) on an NB_F64 handle of order 4 (kernels/mixed.hip.h): every force+jerk pass reads the three
    // binary32 streams below and writes binary32 partial rows into fj_part.  Allocated by the call, released by NB_PASS_NATIVE or
    // nb_destroy.  Off: none of this is read.  The state, the derivatives and the levels are the handle's fp64 arrays either way.
    bool mx = false;
    void* mx_in[3] = {nullptr, nullptr, nullptr};   // (xh, mf), xl, vf: n float4 rows each, rewritten by every predictor / split
    uint32_t mx_chunks = 1, mx_per = 0;   // the mixed pass's j-chunks (kFjRows i-bodies per workgroup) and bodies per chunk
    double mx_guard = 0.0;         // nb_set_pass_guard: r_near; > 0: the guarded kernels (kernels/guard.hip.h) and fp64 partial rows.  0 whenever !mx
    size_t fj_part_bytes = 0;      // what fj_part holds (grown when the mixed shape needs more than the native one)
    uint32_t start6 = 0;           // nb_set_start6: NB_START6_ZERO | NB_START6_CRACKLE, what the engine's own starts (and start levels) are made by
    bool start_own = false;        // snap / crackle came from the engine's start and no step has consumed them (nb_set_start6 may drop them)
    // nb_set_block_steps: block individual time steps (kernels/block.hip.h).  Allocated when first switched on.
    bool blk = false, blk_frozen = false;
    uint32_t blk_L = 20, blk_lmin = 0;
    double blk_eta = 0.02;
    uint8_t* blk_lev = nullptr;      // device: level per body
    uint32_t* blk_due = nullptr;     // device: tick of the body's next corrector
    uint32_t* blk_act = nullptr;     // device: the active list of the block step in flight
    uint32_t* blk_hdr = nullptr;     // device: nb::kBlkWords header words
    uint32_t* blk_hdr_host = nullptr;   // pinned host copy (count, next block time) the step loop reads after its wait
    uint32_t* blk_hdr_pub = nullptr;    // the device's address of blk_hdr_host: nb_blk_sched stores into it
    int levels = 0;                  // 0: stale; 1: blk_lev came from nb_upload_levels, the outer step's clock (blk_due) is not started yet;
                                     // 2: blk_lev / blk_due belong to the state, dt, G and the configuration
    bool levels_own = false;         // levels == 2 by the engine's own start rule, no block step since (nb_set_start6 may drop them)
    uint64_t blk_outer = 0, blk_steps = 0, blk_body_steps = 0;
    // nb_set_block_batch / nb_set_block_batch6: block steps sized on the device, many per host wait (kernels/block_batch.hip.h,
    // kernels/block_batch6.hip.h).  Allocated when first switched on, released by nb_destroy.  Off: none of this is read.
    bool bb = false;
    uint32_t bb_depth = 32, bb_small_max = 256;
    uint32_t bb_chunks = 1, bb_per = 0;   // the small pass's j-chunks: a function of n and the CU count (bb_shape)
    uint32_t* bb_words = nullptr;    // device: nb::kBbWords batch words
    uint32_t* bb_host = nullptr;     // pinned host copy the step loop reads after its wait
    uint32_t* bb_pub = nullptr;      // the device's address of bb_host
    void* bb_part = nullptr;         // the small pass's partial rows: bb_planes planes x bb_chunks x nb::kBbMaxSmall rows
    uint32_t bb_planes = 0;          // the planes bb_part holds (2 | 3: the order it was last switched on for)
    uint32_t bb_seen_small = 0, bb_seen_body = 0;      // the device's running counts as last read (differences per wait)
    // the host's policy (how many slots the next batch has): a function of what was read so far
    bool bb_fresh = true;            // nothing read since the mode was set or the levels went stale: one slot
    uint32_t bb_t = 0, bb_finest = 0, bb_park_ctz = 0;      // the tick reached, the deepest level present, ticks with ctz >= bb_park_ctz are expected to park
    uint64_t bb_waits = 0, bb_slots = 0, bb_small = 0, bb_hoststeps = 0, bb_idle = 0;
    // nb_set_encounter_watch: closest approaches seen inside block steps (kernels/encounter.hip.h).  Allocated when first switched on,
    // released by nb_destroy.  Off: none of this is read.
    bool enc = false;
    uint32_t enc_flags = 0;          // NB_ENC_*
    void* enc_w = nullptr;           // device: n thresholds w_i = h_i^2 + eps2 of the handle's precision (0: not watched)
    void* enc_rho2 = nullptr;        // device: the records, n each -- rho2 (the handle's precision) ...
    uint32_t* enc_partner = nullptr; // ... partner ...
    double* enc_time = nullptr;      // ... time ...
    uint32_t* enc_count = nullptr;   // ... count
    unsigned long long* enc_words = nullptr;   // device: nb::kEncWords words (hits, the bits of first_time, the fold's ticket)
    unsigned long long* enc_host = nullptr;    // pinned host word: hits as nb_enc_fold last published them
    unsigned long long* enc_pub = nullptr;     // the device's address of enc_host
    uint64_t enc_passes = 0;         // gathered passes that ran with the watch on
    uint32_t enc_stopped = 0, enc_steps_left = 0;      // of the last nb_step (NB_ENC_STOP)
    // nb_set_neighbor_scheme: the Ahmad-Cohen neighbour scheme with two shared step levels (kernels/ac_scheme.hip.h).  Allocated
    // by the call, released by NULL or nb_destroy.  While it is on, acc / jerk hold the totals ai + ar0, ji + jr0.
    bool ac = false;
    bool ac_ok = false;              // the scheme's arrays belong to (bodies, vel) and derivs_G (together with derivs_ok)
    bool ac_over = false;            // a build at a regular time overflowed: nb_step fails with ac_msg until the scheme is set again
    std::string ac_msg;
    uint32_t ac_nsub = 8, ac_cap = 128;
    bool ac_two_calls = false;       // NB_FLAG_AC_TWO_CALLS: a list build is nb_split_force + nb_neighbor_lists whatever the shapes are
    double ac_radius = 0.0;
    void* ac_radii = nullptr;        // device copy of the caller's radii (n elements), or null
    void* ac_ai = nullptr;           // the irregular derivatives, over the body's row of ac_list
    void* ac_ji = nullptr;
    void* ac_ar = nullptr;           // the regular derivatives at the last regular time
    void* ac_jr = nullptr;
    void* ac_px = nullptr;           // the second predicted pair (the first is hx / hv)
    void* ac_pv = nullptr;
    uint32_t* ac_list = nullptr;     // n x ac_cap
    uint32_t* ac_count = nullptr;    // n, the true counts
    unsigned long long* ac_hdr = nullptr;        // device: nb::kAcHdrWords words, zeroed in front of every build
    unsigned long long* ac_hdr_host = nullptr;   // pinned host copy the step loop reads after its wait
    uint64_t ac_regular = 0, ac_substeps = 0, ac_entries = 0, ac_builds = 0;
    uint32_t ac_max_count = 0, ac_overflowed = 0;      // of the last build
    // nb_set_neighbor_adapt: radii that follow a target count.  Off: none of this is read and a build is cut by ac_radii / ac_radius.
    bool ad = false;
    uint32_t ad_target = 0, ad_max_rebuilds = 4;
    double ad_gmax = 0.0, ad_rmin = 0.0, ad_rmax = 0.0;
    void* ad_built = nullptr;        // n radii of the handle's precision: what the current list was cut by
    void* ad_next = nullptr;         // what the next build will use
    void* ad_keep = nullptr;         // `next` as a start found it (put back when the start fails)
    uint64_t ad_rebuilds = 0, ad_rows_shrunk = 0;
    uint32_t ad_last_rebuilds = 0;
    // nb_set_neighbor_levels: block individual irregular steps inside the scheme (kernels/ac_levels.hip.h).  Off: none of this is read.
    bool lv = false, lv_frozen = false;
    uint32_t lv_lmin = 0;
    double lv_eta = 0.02;
    int lv_state = 0;                // 0: stale (the start rule runs); 1: lv_lev came from nb_upload_neighbor_levels; 2: current
    uint8_t* lv_lev = nullptr;       // device: level per body
    uint32_t* lv_due = nullptr;      // device: tick of the body's next corrector inside the regular step
    uint32_t* lv_words = nullptr;    // device: nb::lv_words(ac_nsub) words, zeroed in front of every regular step
    unsigned long long* lv_cnt = nullptr;      // device: nb::kLvCntWords counters
    unsigned long long* lv_rec = nullptr;      // device: n records of nb::kLvRecWords counters, each written by its body's own lane
    uint64_t lv_regular = 0, lv_ticks = 0;
};

namespace nbi {

int fail(nb_sim* s, int code, const std::string& msg);
void set_create_error(const std::string& msg);
// nb_neighbors on the first `rows` rows of the handle (nb_multi_neighbors: the caller's unpadded rows of shard 0); `who` names the
// public function in the messages
int neighbors(nb_sim* s, const nb_neighbor_request* req, uint32_t rows, const char* who);
// nb_neighbor_lists likewise (nb_multi_neighbor_lists: the caller's unpadded rows of shard 0)
int neighbor_lists(nb_sim* s, const nb_neighbor_list_request* req, uint32_t rows, const char* who);
// nb_knn likewise (nb_multi_knn: the caller's unpadded rows of shard 0)
int knn(nb_sim* s, const nb_knn_request* req, uint32_t rows, const char* who);
// nb_list_force likewise (nb_multi_list_force: entries >= the caller's unpadded n add nothing)
int list_force(nb_sim* s, const nb_list_force_request* req, uint32_t rows, const char* who);
// nb_split_force likewise (nb_multi_split_force: the caller's unpadded rows of shard 0)
int split_force(nb_sim* s, const nb_split_force_request* req, uint32_t rows, const char* who);
// nb_split_lists likewise (nb_multi_split_lists: the caller's unpadded rows of shard 0)
int split_lists(nb_sim* s, const nb_split_lists_request* req, uint32_t rows, const char* who);
// whether a list build of the neighbour scheme is ONE split_lists call (its shape is split_force's at every batch, and
// NB_FLAG_AC_TWO_CALLS is not set)
bool ac_fused(const nb_sim* s);
const std::string& create_error();

// nb_comm.hip: called by nb_step after the integrate kernel when a communicator is attached.
// begin: enqueue the in-place all-gather of this rank's rows (on the engine stream, or on the
// communicator's own stream when overlapped); wait: make the engine stream wait for it.
int rccl_exchange_begin(nb_sim* s);
// rank form of the symmetric pass: in-place ncclReduceScatter of sym_A on the engine stream (this rank's rows receive the sum)
int rccl_reduce_scatter_A(nb_sim* s);
// the two halves of a rank-form step, for nb_multi (which runs its own reduce-scatter between them)
// force pass [+ a record of the hipEvent_t `after_force`] + nb_sym_reduce.  split_at_gather: the sweeps whose travelers are the rank's
// own rows are launched first, then the engine stream waits for the pending all-gather, then the rest (bit-identical to one launch)
// `stamps` (timed steps, split_at_gather only): the two force launches are stamped at their own begin / end -- e[0]..e[7] and e[3]..e[4],
// stamps->two set -- so the wait for the gather between them is not counted as kernel time
int sym_rank_phase_a(nb_sim* s, void* after_force = nullptr, bool split_at_gather = false, nb_events* stamps = nullptr);
int sym_rank_phase_b(nb_sim* s);     // integrate kernel on the handle's rows of sym_A
int rccl_exchange_wait(nb_sim* s);
bool rccl_overlapped(const nb_sim* s);
void rccl_release(nb_sim* s);

}  // namespace nbi
