// kernels/encounter.hip.h -- the encounter watch of block steps (nb_set_encounter_watch): the closest approach every watched body
// sees at its OWN steps, from the rho^2 the gathered force+jerk pass already forms (the nearest neighbour a GRAPE-style force
// library returns with the force: GRAPE-6, Sapporo, phi-GPU).  No reference analogue.  Part of nb_kernels.hip.h (include that, not
// this file).
//
// Body i has a threshold w_i = h_i^2 + eps2 (fp64 on the host, rounded once; h_i = 0: w_i = 0, the body is not watched).  In a
// gathered pass a body j != i (by index), j < n, with rho^2_ij < w_i (strict) is a candidate; the pass's answer for i is the
// candidate of smallest rho^2, equal rho^2 to the smallest index (nb_neighbors' rule).
//   nb_enc_fj_pk<NG>, nb_enc_fj64<T>   nb_blk_fj_pk's / nb_blk_fj64's bodies (kernels/hermite.hip.h) with WATCH: the same sums, bit
//                                      for bit, and the chunk's answer in the .w lanes of the two partial rows the kernel stores
//                                      anyway -- rho^2 in pa.w (+inf: none), the index in pj.w (f32 rows: bit-cast; fp64 rows: an
//                                      exact double; 0xffffffff: none).  No buffer of its own, no atomics.
//   nb_enc_fold<TP, T>                 one launch behind the pass: for k < |A| the minimum over the chunks' .w pairs under the same
//                                      rule, then the record of act[k].
// The record of a body: rho2 (smallest answer so far, +inf at the start), partner, time (of that answer; the earliest wins a tie:
// a new answer replaces the record only when strictly smaller), count (own steps that had an answer).  Nothing depends on timing:
// floating-point values are compared, never added; the atomics are an integer count, an integer minimum and a ticket.
#pragma once

namespace nb {

// the watch's device words: hits (body steps that had an answer), the bits of first_time (a non-negative double orders as its bits),
// the fold's ticket
enum { kEncHits = 0, kEncFirst = 1, kEncTicket = 2, kEncWords = 3 };
constexpr uint32_t kEncNone = 0xffffffffu;

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_FJ_WAVES, NB_FJ_WAVES)))
void nb_enc_fj_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const uint32_t* __restrict__ act, uint32_t na,
                  float4* __restrict__ pa, float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2,
                  const float4* __restrict__ zero_row, const float* __restrict__ wth)
{
    fj_pk_body<NG, true, true>(pos, vel, act, na, pa, pj, n, j_per_chunk, eps2, zero_row, wth);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nb_enc_fj64(const typename vec4<T>::type* __restrict__ pos,
                                                     const typename vec4<T>::type* __restrict__ vel,
                                                     const uint32_t* __restrict__ act, uint32_t na, double4* __restrict__ pa,
                                                     double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, double eps2,
                                                     const T* __restrict__ wth)
{
    fj64_body<T, true, true>(pos, vel, act, na, pa, pj, n, j_per_chunk, eps2, wth);
}

__device__ __forceinline__ uint32_t enc_index(float w) { return __float_as_uint(w); }
__device__ __forceinline__ uint32_t enc_index(double w) { return (uint32_t)w; }

// Reads the .w lanes only (nb_blk_correct reads x, y, z of the same rows); runs before the next pass reuses them.  t: the block time
// of this pass in outer steps.  lpr lanes share a row (a power of two <= 64, the host's choice from the chunk and row counts: a small active
// set is cut into up to n / 256 chunks, and one lane's chain over them would be that many round trips to memory): each takes the
// chunks lpr apart in ascending order, then the lanes' minima meet in the wave.  The rule -- smaller rho^2, equal rho^2 to the
// smaller index -- is a total order on (rho^2, index), so the minimum is the one a single ascending chain finds.  The last
// workgroup to finish publishes the running count of hits to the host's pinned word.
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_enc_fold(const typename vec4<TP>::type* __restrict__ pa,
                                                     const typename vec4<TP>::type* __restrict__ pj,
                                                     const uint32_t* __restrict__ act, uint32_t na, uint32_t chunks, uint32_t lpr,
                                                     T* __restrict__ rho2, uint32_t* __restrict__ partner, double* __restrict__ time,
                                                     uint32_t* __restrict__ count, unsigned long long* __restrict__ words,
                                                     unsigned long long* __restrict__ host_hits, double t)
{
    const uint32_t k = blockIdx.x * (kBlock / lpr) + threadIdx.x / lpr, sub = threadIdx.x & (lpr - 1u);
    TP br = (TP)__builtin_inf();
    uint32_t bj = kEncNone, i = 0;
    if (k < na) {
        i = act[k];                         // a body is in the list once: its record has one writer
#pragma unroll 4
        for (uint32_t c = sub; c < chunks; c += lpr) {
            const TP r = pa[(size_t)c * na + k].w;
            const uint32_t j = enc_index(pj[(size_t)c * na + k].w);
            if (j != kEncNone && (r < br || (r == br && j < bj))) { br = r; bj = j; }
        }
    }
    for (uint32_t o = lpr >> 1; o > 0; o >>= 1) {      // (the lanes of a row sit in one wave: lpr divides 64)
        const TP r = __shfl_xor(br, (int)o);
        const uint32_t j = (uint32_t)__shfl_xor((int)bj, (int)o);
        if (j != kEncNone && (r < br || (r == br && j < bj))) { br = r; bj = j; }
    }
    const bool hit = k < na && sub == 0 && bj != kEncNone;
    if (hit) {
        count[i] += 1u;
        if ((T)br < rho2[i]) { rho2[i] = (T)br; partner[i] = bj; time[i] = t; }
    }
    // one add of the workgroup's hits and one ticket per workgroup; block times do not decrease, so the minimum is taken by the first
    // pass with a hit only.  (An earlier fold with up to three atomics per wave and eight lanes per row at |A| = N = 65,536 took up to
    // 632 us there; this one takes at most 50 us: profiles/r28/encounters.md.  The two changes were not measured apart.)
    const uint32_t hits = (uint32_t)__syncthreads_count(hit);
    if (threadIdx.x == 0) {
        if (hits) {
            atomicAdd(words + kEncHits, (unsigned long long)hits);
            const unsigned long long tb = (unsigned long long)__double_as_longlong(t);
            if (tb < __hip_atomic_load(words + kEncFirst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(words + kEncFirst, tb);
        }
        __threadfence();
        const unsigned long long ticket = atomicAdd(words + kEncTicket, 1ull);
        if (ticket == (unsigned long long)gridDim.x - 1ull) {
            atomicExch(words + kEncTicket, 0ull);
            *host_hits = atomicAdd(words + kEncHits, 0ull);
        }
    }
}

}  // namespace nb
