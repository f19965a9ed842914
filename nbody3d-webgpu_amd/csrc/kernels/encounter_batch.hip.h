// kernels/encounter_batch.hip.h -- the encounter watch inside the slots of batched block steps (nb_set_block_batch_watch: order-4
// block-step handles with the native pass, nb_set_encounter_watch on).  No reference analogue.  Part of nb_kernels.hip.h (include
// that, not this file).
//
// A slot keeps its launches (kernels/block_batch.hip.h): nb_blkq_sched and nb_blkq_predict as they are, then
//   nb_encq_fj_pk<1>, nb_encq_fj64<T>   the small passes' bodies with WATCH: the same sums, bit for bit, and the slot's answer for the
//                                       chunk in the .w lanes of the two partial rows the kernel stores anyway -- rho^2 in pa.w
//                                       (+inf: none), the index in pj.w (f32 rows: bit-cast; fp64 rows: an exact double; 0xffffffff:
//                                       none), the encoding of nb_enc_fj_pk / nb_enc_fj64.  The four waves of a workgroup hold the
//                                       same slots and sweep different quarters of each tile; their bests are merged in LDS.
//   nb_encq_correct<TP, T>              the small corrector's body with WATCH: nb_enc_fold's work in the same launch (the 16 lanes of
//                                       a slot load its chunk rows whole already), then the corrector, statement for statement.
// The rule is the watch's (kernels/encounter.hip.h): candidates j != i by index, j < n, rho^2 < w_i strict; smaller rho^2 wins, equal
// rho^2 goes to the smaller index -- a total order on (rho^2, index), so what a body records does not depend on |A|, on its place in
// the list, on the waves' quarters or on the chunks' split among lanes.  Floating-point values are compared, never added; the atomics
// are an integer count and an integer minimum.
#pragma once

namespace nb {

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_encq_fj_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const uint32_t* __restrict__ act,
                   const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb, uint32_t small_max, float4* __restrict__ pa,
                   float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row,
                   const float* __restrict__ wth)
{
    static_assert(NG == 1, "one packed pair per lane");
    blkq_fj_pk_body<true>(pos, vel, act, hdr, bb, small_max, pa, pj, n, j_per_chunk, eps2, zero_row, wth);
}

template <typename T>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_encq_fj64(const typename vec4<T>::type* __restrict__ pos, const typename vec4<T>::type* __restrict__ vel,
                  const uint32_t* __restrict__ act, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb,
                  uint32_t small_max, double4* __restrict__ pa, double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk,
                  double eps2, const T* __restrict__ wth)
{
    blkq_fj64_body<T, true>(pos, vel, act, hdr, bb, small_max, pa, pj, n, j_per_chunk, eps2, wth);
}

// tbase: the outer steps the handle had run when this outer step began (a batch never crosses an outer step: 2^L always parks).
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_encq_correct(const typename vec4<TP>::type* __restrict__ pa,
                                                         const typename vec4<TP>::type* __restrict__ pj,
                                                         const uint32_t* __restrict__ act, const uint32_t* __restrict__ bb,
                                                         uint32_t small_max, uint32_t chunks, double G,
                                                         typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                         typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                         uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                         uint32_t* __restrict__ hdr, uint32_t n, uint32_t L, uint32_t lmin,
                                                         int frozen, double eta, double dt, T* __restrict__ rho2,
                                                         uint32_t* __restrict__ partner, double* __restrict__ time,
                                                         uint32_t* __restrict__ count, unsigned long long* __restrict__ words,
                                                         double tbase)
{
    blkq_correct_body<TP, T, true>(pa, pj, act, bb, small_max, chunks, G, x, v, a, j, due, lev, hdr, n, L, lmin, frozen, eta, dt,
                                   rho2, partner, time, count, words, tbase);
}

}  // namespace nb
