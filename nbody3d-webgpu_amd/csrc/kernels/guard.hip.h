// kernels/guard.hip.h -- the guarded sums of the mixed-precision force+jerk pass (nb_set_pass_guard on a handle whose pass precision
// is NB_PASS_MIXED).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// The pass is kernels/mixed.hip.h's fj_mx_body with GUARD: the same three LDS-DMA tile streams, staging, zero-row tail, two-level
// binary32 sums and GATHER form, and per pair the same arithmetic up to s3, dr and t.  A pair with binary32 d2 < near2 (strict; d2
// with eps2 in it; near2 = (float)(r_near * r_near)) is NEAR: its terms leave the binary32 registers and enter a compensated sum of
// their own, so the handful of enormous terms of a hard pair's partner no longer swallow the field of the rest of the system.
//   Per stage: v_cmp_lt_f32 per half of each packed d2 into scalar register pairs, s_or_b64 over the stage's chains, ONE branch.  No
// lane of the wave near: nb_mx_fj's sums, instruction for instruction.  Otherwise the slow sums (fj_mx_body's header): a row's bits
// depend on the state and near2 only, not on which rows share its wave.
//   The near words -- 12 NG packed words per lane, (hi, lo) of six components -- live in LDS beside the tiles (24 KiB + 24 NG KiB):
// nb_mx_fj<2> holds 240 VGPRs at two waves per SIMD, 48 more do not fit, and the words are touched on the slow path only.
//   Partial rows: ((double)far + (double)hi) + (double)lo in the epilogue, stored as fp64 rows; the j-chunks are then added by the
// native pass's nb_fj_reduce<double, double> / nb_blk_correct<double, double> in ascending order, times G once.  With near2 <= eps2
// no pair is near, hi = lo = 0, and every stored row is the plain mixed pass's converted to double: the same bits after the reduce.
//   nb_mxg_fold (below) shortens the block corrector's chain over the fp64 chunk rows of a small gathered pass.
#pragma once

namespace nb {

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_MX_WAVES, NB_MX_WAVES)))
void nb_mxg_fj(const float4* __restrict__ xh, const float4* __restrict__ xl, const float4* __restrict__ vf, double4* __restrict__ pa,
               double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row, float near2)
{
    static_assert(kBlock * 2 * NG == kFjRows, "the engine sizes the grid by kFjRows");
    fj_mx_body<NG, false, true>(xh, xl, vf, nullptr, n, pa, pj, n, j_per_chunk, eps2, zero_row, near2);
}

// The gathered pass of a block step, in nb_mx_blk_fj<2 | 1>'s shapes.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_MX_WAVES, NB_MX_WAVES)))
void nb_mxg_blk_fj(const float4* __restrict__ xh, const float4* __restrict__ xl, const float4* __restrict__ vf,
                   const uint32_t* __restrict__ act, uint32_t na, double4* __restrict__ pa, double4* __restrict__ pj, uint32_t n,
                   uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row, float near2)
{
    fj_mx_body<NG, true, true>(xh, xl, vf, act, na, pa, pj, n, j_per_chunk, eps2, zero_row, near2);
}

// A gathered pass of few rows is cut into up to n / 256 j-chunks, and nb_blk_correct<double, double> adds a row's chunk rows in one
// dependent chain with 8 rows in flight: 256 chunks are 32 round trips to memory.  nb_mxg_fold adds them first -- one workgroup per
// active row: 256 chunk rows per round trip land in LDS, lanes 0 .. 5 add one component each in ascending chunk order, starting
// from +0 as the corrector does -- and leaves the sums in chunk row 0; the corrector then runs with chunks = 1 and adds that row to
// +0, which changes no bit.  The engine calls it where a gathered pass has more than kGuardFoldFrom chunks.
constexpr uint32_t kGuardFoldFrom = 16;

template <int UNUSED = 0>
__global__ __launch_bounds__(kBlock) void nb_mxg_fold(double4* __restrict__ pa, double4* __restrict__ pj, uint32_t na, uint32_t chunks)
{
    __shared__ double part[6][kBlock];                  // [component][chunk of the batch]
    const uint32_t k = blockIdx.x, l = threadIdx.x;     // the grid is na workgroups: k < na
    double s = 0.0;                                     // lanes 0 .. 5: the running sum of component l
    for (uint32_t c0 = 0; c0 < chunks; c0 += kBlock) {
        const uint32_t c = c0 + l;
        if (c < chunks) {
            const double4 a = ld4(pa + (size_t)c * na + k), j = ld4(pj + (size_t)c * na + k);
            part[0][l] = a.x; part[1][l] = a.y; part[2][l] = a.z;
            part[3][l] = j.x; part[4][l] = j.y; part[5][l] = j.z;
        }
        __syncthreads();
        const uint32_t m = chunks - c0 < (uint32_t)kBlock ? chunks - c0 : (uint32_t)kBlock;
        if (l < 6)
            for (uint32_t i = 0; i < m; ++i) s += part[l][i];
        __syncthreads();
    }
    if (l < 6) reinterpret_cast<double*>(l < 3 ? pa + k : pj + k)[l % 3] = s;      // chunk row 0 of row k; its fourth lane stays 0
}

}  // namespace nb
