// nb_kernels.hip.h -- device code of the MI355X (gfx950) direct N-body engine.
//
// The reference runs ONE WGSL compute pass per frame (/root/reference nbody3d.js:219-292):
// tiled O(N^2) softened-gravity accumulation (:232-237 pair force, :255-272 tile loop)
// followed by the "velocity verlet with frame shift" update (:274-290), writing positions in
// place (:283) while other workgroups still stage them (:257) -- a cross-workgroup race.
// Here a step is well defined in both of its forms:
//
//   two kernels   K1 nb_force*   (reads positions only)  ->  K2 nb_integrate* (after all of K1)
//   one kernel    nb_step_fused  (reads bodies_in, writes bodies_out: ping-pong buffers)
//
//   K1 forms:   nb_force_symw<NG,J>      f32, SYMMETRIC pass (default from N ~ 13,000): every unordered pair once, both
//               nb_force_symw_pairs<NG>  accelerations; residents in registers, travelers rotate through the wave by DPP
//               nb_force_symw64<8>       (_pairs: one traveler per lane and sweep, whole sweeps two at a time -- the default f32 kernel)
//               nb_force_sym<WS,NG,J>    (f64 form; workgroup form with LDS-combined traveler sums: A/B arm)
//               nb_force_pk_sgpr<NG,WS>  f32, packed math, ordered pairs, j broadcast from SGPRs (shards without the native exchange)
//               nb_force_pk<NG,LS,TL>    f32, packed math, j-tile staged in LDS
//               nb_force<T,IPL,LS>       scalar template: f64, and the unpacked f32 shapes
//   fused form: nb_step_fused<NG,LS,TL>  nb_force_pk's loop over ALL j + the integrator in the
//                                        epilogue (no j-split across workgroups: LS lanes of a
//                                        wave share an i-body instead) -- one launch per step,
//                                        no partial sums through memory
//               nb_step_direct<MAXJ>     the same for N <= 2,048 with each lane's j-bodies loaded
//                                        straight into registers (no LDS tile, no barrier)
//               nb_step_jpk<WS>          A/B arm: packed across TWO j-BODIES streamed as SGPR pairs from a
//                                        pair-transposed position copy; j split over the waves of a workgroup
//                                        and over workgroups that meet at a ticket inside the launch
//
// CDNA4 mapping of the force loop (wave = 64 lanes, 4 SIMDs/CU, 160 KiB LDS/CU):
//   * a 256-thread workgroup (4 waves, one per SIMD) stages a j-tile of 256*TL bodies
//     (x, y, z, m) in LDS by LDS-DMA (global_load_lds_dwordx4: no VGPR staging, no ds_write),
//     double buffered, ONE s_barrier per tile; the next tile lands while the current one computes
//     (the scalar template nb_force<T,...> stages (x, y, z, G*m) through registers);
//   * the inner loop reads the tile with ds_read_b128 at a wave-uniform address
//     (LDS broadcast: one read feeds 64*IPL pair evaluations) -- LS == 1 -- or
//     at LS consecutive addresses when LS lanes share one i-body;
//   * each lane keeps IPL i-bodies in VGPRs (register blocking), loaded with coalesced 16-B accesses;
//   * f32: the arithmetic is packed across TWO i-bodies of the lane (v_pk_add/fma/mul_f32):
//     per two pairs 3 v_pk_add, 3 v_pk_fma (r^2 + eps2), 2 v_pk_mul (cube), 2 v_rsq_f32,
//     1 v_pk_mul (m_j), 3 v_pk_fma (accumulate) = 12 packed (4 cycles each) + 2 transcendental
//     (8 cycles each) = 64 issue cycles per 128 pairs, issued stage-major over 4 independent
//     chains so no hazard s_nop is needed;
//   * no branch in the loop: with eps2 > 0 the self term is exactly 0*finite = 0 and bodies
//     past the range are staged as zero-mass;
//   * LS > 1: the LS partial sums of a body are reduced inside the wave (DPP row operations
//     and row broadcasts for f32, wavefront shuffles for f64) before ONE lane stores/integrates;
//   * grid = (i-blocks, jsplit): j may also be partitioned over blockIdx.y (any multiple of 8
//     bodies per split); K2 sums the jsplit partials in ascending order (deterministic, no atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nb_plan.h"

// The device code lives in kernels/*.hip.h, in dependency order:
#include "kernels/common.hip.h"      // row loads, pair(), in-wave sums, leapfrog()
#include "kernels/ordered.hip.h"     // nb_force, nb_force_pk, nb_step_fused, nb_step_direct, nb_force_pk_sgpr
#include "kernels/symmetric.hip.h"   // nb_force_sym*, nb_sym_reduce, nb_peer_*, nb_integrate_sym*
#include "kernels/jpk.hip.h"         // nb_step_jpk, nb_pairs_pack, nb_gm_pack
#include "kernels/integrate.hip.h"   // nb_integrate, nb_integrate_swap, nb_frame_pack, nb_diag
#include "kernels/field.hip.h"       // nb_field_pk, nb_field64, nb_field_reduce (nb_field_eval: the field at arbitrary points)
#include "kernels/neighbors.hip.h"   // nb_nbr_pk, nb_nbr64, nb_nbr_reduce (nb_neighbors: nearest body and bodies inside a radius)
#include "kernels/neighbor_lists.hip.h"   // nb_nbl_offsets, nb_nbl_pk, nb_nbl64 (nb_neighbor_lists: WHICH bodies are inside a radius)
#include "kernels/knn.hip.h"         // nb_knn_pk, nb_knn64, nb_knn_merge (nb_knn: the k nearest bodies of every point)
#include "kernels/list_force.hip.h"  // nb_lf32, nb_lf64 (nb_list_force: acceleration, jerk and potential over neighbour rows)
#include "kernels/hermite.hip.h"     // nb_fj_pk, nb_fj64, nb_fj_reduce, nb_hermite_predict, nb_hermite_correct (NB_INT_HERMITE4)
#include "kernels/split_force.hip.h" // nb_split_pk, nb_split64, nb_split_reduce (nb_split_force: regular and irregular force+jerk in one pass)
#include "kernels/split_lists.hip.h" // nb_spl_pk, nb_spl64, nb_spl_rows (nb_split_lists: the two sums and the neighbour rows from one pass)
#include "kernels/block.hip.h"       // nb_blk_start, nb_blk_sched, nb_blk_predict, nb_blk_fj_pk, nb_blk_fj64, nb_blk_correct (nb_set_block_steps)
#include "kernels/encounter.hip.h"   // nb_enc_fj_pk, nb_enc_fj64, nb_enc_fold (nb_set_encounter_watch: closest approaches seen inside block steps)
#include "kernels/block_batch.hip.h" // nb_blkq_sched, nb_blkq_predict, nb_blkq_fj_pk, nb_blkq_fj64, nb_blkq_correct (nb_set_block_batch: block steps sized on the device)
#include "kernels/mixed.hip.h"       // nb_mx_split, nb_mx_predict, nb_mx_blk_predict, nb_mx_fj, nb_mx_blk_fj (nb_set_pass_precision: double-single force+jerk pass of f64 handles)
#include "kernels/guard.hip.h"       // nb_mxg_fj, nb_mxg_blk_fj, nb_mxg_fold (nb_set_pass_guard: the mixed pass with guarded sums, fp64 partial rows)
#include "kernels/ac_scheme.hip.h"   // nb_ac_sub32, nb_ac_sub64, nb_ac_predict0, nb_ac_regular, nb_ac_start (nb_set_neighbor_scheme: the Ahmad-Cohen neighbour scheme)
#include "kernels/ac_levels.hip.h"   // nb_ac_lv_start, nb_ac_lv_begin, nb_ac_lv_sub32, nb_ac_lv_sub64 (nb_set_neighbor_levels: block individual irregular steps)
#include "kernels/hermite6.hip.h"    // nb_h6_fjs_pk, nb_h6_fjs64, nb_h6_reduce, nb_h6_predict, nb_h6_correct (nb_set_hermite_order(6): force, jerk and snap); nb_h6_crk_pk, nb_h6_crk64, nb_h6_reduce1 (nb_set_start6: the crackle of a start)
#include "kernels/block6.hip.h"      // nb_blk6_start, nb_blk6_predict, nb_blk6_fjs_pk, nb_blk6_fjs64, nb_blk6_correct (nb_set_block_steps6: block steps on order-6 handles)
#include "kernels/block_batch6.hip.h" // nb_blkq6_predict, nb_blkq6_fjs_pk, nb_blkq6_fjs64, nb_blkq6_correct (nb_set_block_batch6: block steps sized on the device, order-6 handles)
#include "kernels/block_batch_mixed.hip.h" // nb_blkqm_predict, nb_blkqm_fj (nb_set_block_batch_mixed: block steps sized on the device, mixed-precision handles)
#include "kernels/encounter_batch.hip.h" // nb_encq_fj_pk, nb_encq_fj64, nb_encq_correct (nb_set_block_batch_watch: the encounter watch inside batched slots)
