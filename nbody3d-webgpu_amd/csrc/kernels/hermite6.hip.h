// kernels/hermite6.hip.h -- the 6th-order Hermite predictor-corrector on force, jerk and snap (Nitadori & Makino 2008): the
// force+jerk+snap pass (nb_h6_fjs_pk, nb_h6_fjs64, nb_h6_reduce), the two O(N) kernels around it (nb_h6_predict,
// nb_h6_correct) and, at the end, the crackle pass of a start (nb_h6_crk_pk, nb_h6_crk64, nb_h6_reduce1).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
//   dr = x_j - x_i,  dv = v_j - v_i,  da = a_j - a_i,  rho^2 = |dr|^2 + eps2,  s3 = m_j / rho^3
//   alpha = (dr.dv) / rho^2            beta = (dv.dv + dr.da) / rho^2 + alpha^2
//   A = s3 dr
//   J = s3 t,   t = dv - 3 alpha dr
//   S = s3 (da - 6 alpha t - 3 beta dr)
//
// N x N ORDERED pairs of one (positions, velocities, accelerations) state.  The launch is nb_fj_pk's: grid = (i-blocks) x (j-chunks
// of whole 256-row tiles), workgroup (bx, c) stores one row triple per body into pa[c][i], pj[c][i], ps[c][i]; nb_h6_reduce adds a
// body's chunks in ascending order in fp64 and multiplies by G ONCE.  Fixed order, no atomics.
#pragma once

namespace nb {

#ifndef NB_H6_NG
#define NB_H6_NG 2                                  // packed groups per lane of nb_h6_fjs_pk: 4 bodies per lane (A/B builds: -DNB_H6_NG=1)
#endif
#ifndef NB_H6_WAVES
#define NB_H6_WAVES 2                               // waves per SIMD nb_h6_fjs_pk is compiled for
#endif
constexpr int kH6NG = NB_H6_NG;
constexpr uint32_t kH6Rows = kBlock * 2 * kH6NG;    // i-bodies of one f32 workgroup
constexpr uint32_t kH6Rows64 = kBlock;              // i-bodies of one f64 workgroup
constexpr uint32_t kH6Flush = 4;                    // tiles between two flushes of the first-level sums (1,024 terms per chain)

// f32.  nb_fj_pk's structure with a third tile stream: the i-bodies sit in registers as packed pairs (positions, velocities,
// accelerations), every lane of the wave reads the same three tile rows (LDS broadcast).  Per two pairs:
//   3 + 3 + 3 v_pk_add (dr, dv, da), 3 v_pk_fma (rho^2), 2 v_rsq_f32, 1 v_pk_mul + 2 v_pk_fma (dr.dv), 1 v_pk_mul + 5 v_pk_fma
//   (dv.dv + dr.da), s = m y, y^2 = y y, s3 = s y^2, alpha = (dr.dv) y^2, alpha^2, beta = (dv.dv + dr.da) y^2 + alpha^2,
//   -3 alpha, -6 alpha, -3 beta, 3 v_pk_fma (t), 6 v_pk_fma (u = da - 6 alpha t - 3 beta dr), 9 v_pk_fma (a, j, s += s3 ...)
// = 48 packed + 2 transcendental.
//   Every component is ONE sum s3 (...): the halves of the jerk and of the snap are each far larger than their difference.
//   No self-masking: for j == i dr = dv = da = 0, so t = u = 0 and, with eps2 >= 1e-12, s3 is finite: all nine terms are exactly 0.
// Rows past the range come from zero_row (zero mass: s3 = 0, alpha and beta finite, all nine terms exactly 0).
//   Summation: as nb_fj_pk -- binary32 in two levels (a register takes at most 1,024 terms, then chunk / 1,024), fp64 across the
// chunks.
//   Registers: 9 packed i-values and 2 x 9 packed sums per group, ~14 packed values live per chain, four chains issued
// stage-major.  Two waves per SIMD (256 VGPRs each).  Built: two groups per lane take 240 VGPRs and no scratch, one group 174;
// two groups halve the LDS reads per pair and keep nb_fj_pk's launch shape (profiles/r20/hermite6.md).
//   The body is shared with nb_blk6_fjs_pk (kernels/block6.hip.h), as fj_pk_body is with nb_blk_fj_pk: with GATHER the ni i-rows are
// act[0 .. ni) and the partial rows are compact (row k of chunk c belongs to act[k]); without it ni == n and row k is body k.
// Everything between the prologue's loads and the epilogue's stores is the same code.
template <int NG, bool GATHER>
__device__ __forceinline__ void h6_fjs_pk_body(const float4* __restrict__ pos, const float4* __restrict__ vel,
                                               const float4* __restrict__ acc, const uint32_t* __restrict__ act, uint32_t ni,
                                               float4* __restrict__ pa, float4* __restrict__ pj, float4* __restrict__ ps,
                                               uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4 / NG;            // j-bodies per stage: JB * NG = 4 independent chains
    constexpr uint32_t ROWS = kBlock * 2 * NG;
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][3][TILE];   // [buffer][0 = positions, 1 = velocities, 2 = accelerations][row]
    const int tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * ROWS;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG], ui[NG], vi[NG], wi[NG], fi[NG], gi[NG], hi[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        if constexpr (GATHER) { c0 = act[c0]; c1 = act[c1]; }
        const float4 b0 = ld4(pos + c0), b1 = ld4(pos + c1), v0 = ld4(vel + c0), v1 = ld4(vel + c1);
        const float4 a0 = ld4(acc + c0), a1 = ld4(acc + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        ui[g] = nb_f2{v0.x, v1.x}; vi[g] = nb_f2{v0.y, v1.y}; wi[g] = nb_f2{v0.z, v1.z};
        fi[g] = nb_f2{a0.x, a1.x}; gi[g] = nb_f2{a0.y, a1.y}; hi[g] = nb_f2{a0.z, a1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 sm[NG][9], SM[NG][9];           // first- and second-level sums: a (0..2), j (3..5), s (6..8)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int k = 0; k < 9; ++k) sm[g][k] = SM[g][k] = zero;
    }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const nb_f2 p2 = nb_f2{2.0f, 2.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_fj_pk::stage: whole tiles from a scalar base, the last one per lane with rows past the range
    // taken from zero_row; three tiles per stage (positions, velocities, accelerations)
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst_p = lds_wave + (uint32_t)(buf * 3 * TILE) * 16u, dst_v = dst_p + (uint32_t)TILE * 16u;
        const uint32_t dst_a = dst_v + (uint32_t)TILE * 16u;
        unsigned keep;
        if (jt + TILE <= j1) {
            const float4 *bp = pos + jt, *bv = vel + jt, *ba = acc + jt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bv), "s"(dst_v) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(ba), "s"(dst_a) : "memory");
        } else {
            const uint32_t j = jt + tid;
            const float4* sp = j < j1 ? pos + j : zero_row;
            const float4* sv = j < j1 ? vel + j : zero_row;
            const float4* sa = j < j1 ? acc + j : zero_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sv), "s"(dst_v) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sa), "s"(dst_a) : "memory");
        }
    };

    // one stage: JB tile rows (positions p, velocities q, accelerations r) against the lane's NG packed groups, stage-major over
    // the NC chains
    auto math = [&](const float4* p, const float4* q, const float4* r) {
        nb_f2 bx[JB], by[JB], bz[JB], bu[JB], bv[JB], bw[JB], bf[JB], bg[JB], bh[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u], c = q[u], d = r[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z};
            bf[u] = nb_f2{d.x, d.x}; bg[u] = nb_f2{d.y, d.y}; bh[u] = nb_f2{d.z, d.z};
        }
        nb_f2 dx[NC], dy[NC], dz[NC], du[NC], dv[NC], dw[NC], df[NC], dg[NC], dh[NC], d2[NC], y[NC], s[NC], rv[NC], vv[NC], q6[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) dx[c] = bx[c / NG] - xi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dy[c] = by[c / NG] - yi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dz[c] = bz[c / NG] - zi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dx[c], dx[c], e2);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = nb_f2{nb_rsq(d2[c].x), nb_rsq(d2[c].y)};
        // the differences and the three dot products need nothing of the reciprocal roots: they fill the slots behind them
#pragma unroll
        for (int c = 0; c < NC; ++c) du[c] = bu[c / NG] - ui[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dv[c] = bv[c / NG] - vi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dw[c] = bw[c / NG] - wi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = dx[c] * du[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = __builtin_elementwise_fma(dy[c], dv[c], rv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = __builtin_elementwise_fma(dz[c], dw[c], rv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = bf[c / NG] - fi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = bg[c / NG] - gi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = bh[c / NG] - hi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = du[c] * du[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dv[c], dv[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dw[c], dw[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dx[c], df[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dy[c], dg[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dz[c], dh[c], vv[c]);      // dv.dv + dr.da
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = nb_f2{bm[c / NG], bm[c / NG]} * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * y[c];                 // alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = rv[c] * rv[c];                // alpha^2
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(vv[c], y[c], d2[c]);       // beta
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * m3;                   // -3 alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) q6[c] = rv[c] * p2;                   // -6 alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = vv[c] * m3;                   // -3 beta
#pragma unroll
        for (int c = 0; c < NC; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 alpha dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = __builtin_elementwise_fma(q6[c], du[c], df[c]);      // u = da - 6 alpha t - 3 beta dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = __builtin_elementwise_fma(q6[c], dv[c], dg[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = __builtin_elementwise_fma(q6[c], dw[c], dh[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = __builtin_elementwise_fma(vv[c], dx[c], df[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = __builtin_elementwise_fma(vv[c], dy[c], dg[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = __builtin_elementwise_fma(vv[c], dz[c], dh[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][6] = __builtin_elementwise_fma(s[c], df[c], sm[c % NG][6]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][7] = __builtin_elementwise_fma(s[c], dg[c], sm[c % NG][7]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][8] = __builtin_elementwise_fma(s[c], dh[c], sm[c % NG][8]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][3] = __builtin_elementwise_fma(s[c], du[c], sm[c % NG][3]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][4] = __builtin_elementwise_fma(s[c], dv[c], sm[c % NG][4]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][5] = __builtin_elementwise_fma(s[c], dw[c], sm[c % NG][5]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][0] = __builtin_elementwise_fma(s[c], dx[c], sm[c % NG][0]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][1] = __builtin_elementwise_fma(s[c], dy[c], sm[c % NG][1]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][2] = __builtin_elementwise_fma(s[c], dz[c], sm[c % NG][2]);
    };
    auto flush = [&]() {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll
            for (int k = 0; k < 9; ++k) { SM[g][k] = SM[g][k] + sm[g][k]; sm[g][k] = zero; }
        }
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cur ^ 1);      // lands under this tile's compute
        const uint32_t left = j1 - (j0 + t * TILE);
        const int cnt = left < (uint32_t)TILE ? (int)left : TILE;
        const int chunks = (cnt + U - 1) / U;             // rows past the range are staged zero-mass bodies
        for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
            for (int uu = 0; uu < U / JB; ++uu)
                math(&tile[cur][0][ch * U + uu * JB], &tile[cur][1][ch * U + uu * JB], &tile[cur][2][ch * U + uu * JB]);
        }
        if ((t & (kH6Flush - 1)) == kH6Flush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    float4* oa = pa + (size_t)blockIdx.y * ni;
    float4* oj = pj + (size_t)blockIdx.y * ni;
    float4* os = ps + (size_t)blockIdx.y * ni;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        if (il0 < ni) {
            oa[il0] = float4{SM[g][0].x, SM[g][1].x, SM[g][2].x, 0.0f};
            oj[il0] = float4{SM[g][3].x, SM[g][4].x, SM[g][5].x, 0.0f};
            os[il0] = float4{SM[g][6].x, SM[g][7].x, SM[g][8].x, 0.0f};
        }
        if (il1 < ni) {
            oa[il1] = float4{SM[g][0].y, SM[g][1].y, SM[g][2].y, 0.0f};
            oj[il1] = float4{SM[g][3].y, SM[g][4].y, SM[g][5].y, 0.0f};
            os[il1] = float4{SM[g][6].y, SM[g][7].y, SM[g][8].y, 0.0f};
        }
    }
}

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_H6_WAVES, NB_H6_WAVES)))
void nb_h6_fjs_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ acc,
                  float4* __restrict__ pa, float4* __restrict__ pj, float4* __restrict__ ps, uint32_t n, uint32_t j_per_chunk,
                  float eps2, const float4* __restrict__ zero_row)
{
    static_assert(kBlock * 2 * NG == kH6Rows, "the engine sizes the grid by kH6Rows");
    h6_fjs_pk_body<NG, false>(pos, vel, acc, nullptr, n, pa, pj, ps, n, j_per_chunk, eps2, zero_row);
}

// fp64 handles.  One body per lane, the three j-tiles staged through registers; v_rsq_f64 seed + one correction as in nb_fj64;
// every difference, product and sum is fp64.  (T = double: a template so that every translation unit may include it.)
// h6_fjs64_body<T, GATHER>: shared with nb_blk6_fjs64, as h6_fjs_pk_body above.
template <typename T, bool GATHER>
__device__ __forceinline__ void h6_fjs64_body(const typename vec4<T>::type* __restrict__ pos,
                                              const typename vec4<T>::type* __restrict__ vel,
                                              const typename vec4<T>::type* __restrict__ acc, const uint32_t* __restrict__ act,
                                              uint32_t ni, double4* __restrict__ pa, double4* __restrict__ pj,
                                              double4* __restrict__ ps, uint32_t n, uint32_t j_per_chunk, double eps2)
{
    static_assert(std::is_same<T, double>::value, "the fp64 pass of fp64 handles");
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[kTile];
    __shared__ double4 ta[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kH6Rows64 + tid;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    uint32_t ic = il < ni ? il : ni - 1;
    if constexpr (GATHER) ic = act[ic];
    const double4 bi = ld4(pos + ic), wi = ld4(vel + ic), ci = ld4(acc + ic);
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const double4 b = ld4(pos + j), c = ld4(vel + j), d = ld4(acc + j);
            tp[tid] = b;
            tv[tid] = double4{c.x, c.y, c.z, 0.0};
            ta[tid] = double4{d.x, d.y, d.z, 0.0};
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
            ta[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 2
        for (int jj = 0; jj < cnt; ++jj) {
            const double4 b = tp[jj], c = tv[jj], d = ta[jj];
            const double dx = b.x - bi.x, dy = b.y - bi.y, dz = b.z - bi.z;
            const double du = c.x - wi.x, dv = c.y - wi.y, dw = c.z - wi.z;
            const double df = d.x - ci.x, dg = d.y - ci.y, dh = d.z - ci.z;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double y2 = y * y;
            const double s3 = (b.w * y) * y2;
            const double alpha = nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2;
            const double vr = nb_fma(dz, dh, nb_fma(dy, dg, nb_fma(dx, df, nb_fma(dw, dw, nb_fma(dv, dv, du * du)))));
            const double beta = nb_fma(vr, y2, alpha * alpha);
            const double q3 = -3.0 * alpha, q6 = -6.0 * alpha, b3 = -3.0 * beta;
            const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
            const double ux = nb_fma(b3, dx, nb_fma(q6, tx, df)), uy = nb_fma(b3, dy, nb_fma(q6, ty, dg)),
                         uz = nb_fma(b3, dz, nb_fma(q6, tz, dh));
            sx = nb_fma(s3, ux, sx); sy = nb_fma(s3, uy, sy); sz = nb_fma(s3, uz, sz);
            jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
            ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
        }
    }
    if (il < ni) {
        pa[(size_t)blockIdx.y * ni + il] = double4{ax, ay, az, 0.0};
        pj[(size_t)blockIdx.y * ni + il] = double4{jx, jy, jz, 0.0};
        ps[(size_t)blockIdx.y * ni + il] = double4{sx, sy, sz, 0.0};
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_fjs64(const typename vec4<T>::type* __restrict__ pos,
                                                     const typename vec4<T>::type* __restrict__ vel,
                                                     const typename vec4<T>::type* __restrict__ acc, double4* __restrict__ pa,
                                                     double4* __restrict__ pj, double4* __restrict__ ps, uint32_t n,
                                                     uint32_t j_per_chunk, double eps2)
{
    h6_fjs64_body<T, false>(pos, vel, acc, nullptr, n, pa, pj, ps, n, j_per_chunk, eps2);
}

// Adds a body's chunk rows in ascending chunk order in fp64, multiplies by G once and writes the derivative rows (ax, ay, az, 0),
// (jx, jy, jz, 0), (sx, sy, sz, 0).  acc_out and jerk_out may be null together (the start keeps the force+jerk pass's bits and
// takes the snap only).  T = element type of the partial rows and of the handle.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_reduce(const typename vec4<T>::type* __restrict__ pa,
                                                      const typename vec4<T>::type* __restrict__ pj,
                                                      const typename vec4<T>::type* __restrict__ ps, uint32_t n, uint32_t chunks,
                                                      double G, typename vec4<T>::type* __restrict__ acc_out,
                                                      typename vec4<T>::type* __restrict__ jerk_out,
                                                      typename vec4<T>::type* __restrict__ snap_out)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const auto a = ld4(pa + (size_t)c * n + il);
        const auto j = ld4(pj + (size_t)c * n + il);
        const auto s = ld4(ps + (size_t)c * n + il);
        sx += (double)a.x; sy += (double)a.y; sz += (double)a.z;
        tx += (double)j.x; ty += (double)j.y; tz += (double)j.z;
        ux += (double)s.x; uy += (double)s.y; uz += (double)s.z;
    }
    if (acc_out) {
        acc_out[il] = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
        jerk_out[il] = V4{(T)(G * tx), (T)(G * ty), (T)(G * tz), (T)0};
    }
    snap_out[il] = V4{(T)(G * ux), (T)(G * uy), (T)(G * uz), (T)0};
}

// Predictor, with h = dt:
//   xp = x + h v + h^2/2 a + h^3/6 j + h^4/24 s + h^5/120 c      vp = v + h a + h^2/2 j + h^3/6 s + h^4/24 c
//   ap = a + h j + h^2/2 s + h^3/6 c
// The mass lane and vel.w are carried unchanged, ap.w is 0.  Each polynomial is evaluated in fp64 (Horner, fused) and rounded
// once to the handle's precision.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_predict(const typename vec4<T>::type* __restrict__ x,
                                                       const typename vec4<T>::type* __restrict__ v,
                                                       const typename vec4<T>::type* __restrict__ a,
                                                       const typename vec4<T>::type* __restrict__ j,
                                                       const typename vec4<T>::type* __restrict__ s,
                                                       const typename vec4<T>::type* __restrict__ c,
                                                       typename vec4<T>::type* __restrict__ xp,
                                                       typename vec4<T>::type* __restrict__ vp,
                                                       typename vec4<T>::type* __restrict__ ap, uint32_t n, double h)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il), S = ld4(s + il), K = ld4(c + il);
    const double h2 = h * (1.0 / 2.0), h3 = h * (1.0 / 3.0), h4 = h * (1.0 / 4.0), h5 = h * (1.0 / 5.0);
    auto px = [&](double x0, double v0, double a0, double j0, double s0, double c0) {
        return nb_fma(h, nb_fma(h2, nb_fma(h3, nb_fma(h4, nb_fma(h5, c0, s0), j0), a0), v0), x0);
    };
    auto pv = [&](double v0, double a0, double j0, double s0, double c0) {
        return nb_fma(h, nb_fma(h2, nb_fma(h3, nb_fma(h4, c0, s0), j0), a0), v0);
    };
    auto pa = [&](double a0, double j0, double s0, double c0) { return nb_fma(h, nb_fma(h2, nb_fma(h3, c0, s0), j0), a0); };
    xp[il] = V4{(T)px(X.x, V.x, A.x, J.x, S.x, K.x), (T)px(X.y, V.y, A.y, J.y, S.y, K.y), (T)px(X.z, V.z, A.z, J.z, S.z, K.z), X.w};
    vp[il] = V4{(T)pv(V.x, A.x, J.x, S.x, K.x), (T)pv(V.y, A.y, J.y, S.y, K.y), (T)pv(V.z, A.z, J.z, S.z, K.z), V.w};
    ap[il] = V4{(T)pa(A.x, J.x, S.x, K.x), (T)pa(A.y, J.y, S.y, K.y), (T)pa(A.z, J.z, S.z, K.z), (T)0};
}

// Corrector: (a1, j1, s1) are the derivatives at the predicted state, as stored;
//   v1 = v + h/2 (a + a1) - h^2/10 (j1 - j) + h^3/120 (s + s1)      x1 = x + h/2 (v + v1) - h^2/10 (a1 - a) + h^3/120 (j + j1)
//   P = a1 - a - h j - h^2/2 s,  Q = h (j1 - j - h s),  R = h^2 (s1 - s),  c1 = (60 P - 36 Q + 9 R) / h^3
// in fp64 (v1 enters x1 before it is rounded), each stored value rounded once; the state becomes (x1, v1, a1, j1, s1, c1) in
// place (a lane reads and writes its own rows only).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_correct(typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                       typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                       typename vec4<T>::type* __restrict__ s, typename vec4<T>::type* __restrict__ c,
                                                       const typename vec4<T>::type* __restrict__ a1,
                                                       const typename vec4<T>::type* __restrict__ j1,
                                                       const typename vec4<T>::type* __restrict__ s1, uint32_t n, double h)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il), S = ld4(s + il);
    const auto A1 = ld4(a1 + il), J1 = ld4(j1 + il), S1 = ld4(s1 + il);
    const double hh = 0.5 * h, h10 = -(h * h) * (1.0 / 10.0), h120 = h * h * h * (1.0 / 120.0), ih3 = 1.0 / (h * h * h);
    // y1 = y + h/2 (d0 + d1) - h^2/10 (e1 - e0) + h^3/120 (f0 + f1)
    auto co = [&](double y0, double d0, double d1, double e0, double e1, double f0, double f1) {
        return nb_fma(h120, f0 + f1, nb_fma(h10, e1 - e0, nb_fma(hh, d0 + d1, y0)));
    };
    auto ck = [&](double a0, double an, double j0, double jn, double s0, double sn) {
        const double P = nb_fma(-hh * h, s0, nb_fma(-h, j0, an - a0));
        const double Q = h * nb_fma(-h, s0, jn - j0);
        const double R = (h * h) * (sn - s0);
        return nb_fma(9.0, R, nb_fma(-36.0, Q, 60.0 * P)) * ih3;
    };
    const double vx = co(V.x, A.x, A1.x, J.x, J1.x, S.x, S1.x), vy = co(V.y, A.y, A1.y, J.y, J1.y, S.y, S1.y),
                 vz = co(V.z, A.z, A1.z, J.z, J1.z, S.z, S1.z);
    x[il] = V4{(T)co(X.x, V.x, vx, A.x, A1.x, J.x, J1.x), (T)co(X.y, V.y, vy, A.y, A1.y, J.y, J1.y),
               (T)co(X.z, V.z, vz, A.z, A1.z, J.z, J1.z), X.w};
    v[il] = V4{(T)vx, (T)vy, (T)vz, V.w};
    c[il] = V4{(T)ck(A.x, A1.x, J.x, J1.x, S.x, S1.x), (T)ck(A.y, A1.y, J.y, J1.y, S.y, S1.y),
               (T)ck(A.z, A1.z, J.z, J1.z, S.z, S1.z), (T)0};
    a[il] = V4{A1.x, A1.y, A1.z, (T)0};
    j[il] = V4{J1.x, J1.y, J1.z, (T)0};
    s[il] = V4{S1.x, S1.y, S1.z, (T)0};
}

// ---- the crackle of a start (nb_set_start6(NB_START6_CRACKLE)): nb_h6_crk_pk, nb_h6_crk64, nb_h6_reduce1 -----------------------
//   dj = j_j - j_i, and with dr, dv, da, rho^2, s3, alpha, beta, t of the pass above and q its u:
//   gamma = (3 dv.da + dr.dj) / rho^2 + alpha (3 beta - 4 alpha^2)
//   C = s3 w,   w = dj - 9 alpha q - 9 beta t - 3 gamma dr
// N x N ORDERED pairs of one (positions, velocities, accelerations, jerks) state; launch, j-chunks, partial rows and summation are
// nb_h6_fjs_pk's, with ONE plane of partial rows (a, j and s exist when this runs): pc[c][i].  Runs once per start.
#ifndef NB_H6_CRK_NG
#define NB_H6_CRK_NG 2                              // packed groups per lane of nb_h6_crk_pk (A/B builds: -DNB_H6_CRK_NG=1)
#endif
constexpr int kH6CrkNG = NB_H6_CRK_NG;
constexpr uint32_t kH6CrkRows = kBlock * 2 * kH6CrkNG;      // i-bodies of one f32 workgroup

// f32.  nb_h6_fjs_pk with a fourth tile stream (the jerks) and three sums in place of nine.  Per two pairs:
//   12 v_pk_add (dr, dv, da, dj), 3 (rho^2), 2 v_rsq_f32, 3 (dr.dv), 6 (dv.dv + dr.da), 7 (3 dv.da + dr.dj), 3 (s3), alpha, alpha^2,
//   beta, -3 beta, 4 alpha^2 - 3 beta, alpha (...), gamma, -3 gamma, -3 alpha, -6 alpha, -9 alpha, -9 beta, 3 (t), 6 (q), 9 (w), 3 (sums)
// = 67 packed + 2 transcendental.  Every component is ONE sum s3 (...).  No self-masking: for j == i all four differences are 0,
// so t = q = w = 0 and all three terms are exactly 0; rows past the range come from zero_row (s3 = 0; alpha, beta, gamma finite).
//   Registers: 12 packed i-values and 2 x 3 packed sums per group.  LDS: 2 buffers x 4 tiles x 4 KB = 32 KB.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_H6_WAVES, NB_H6_WAVES)))
void nb_h6_crk_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ acc,
                  const float4* __restrict__ jrk, float4* __restrict__ pc, uint32_t n, uint32_t j_per_chunk, float eps2,
                  const float4* __restrict__ zero_row)
{
    static_assert(kBlock * 2 * NG == kH6CrkRows, "the engine sizes the grid by kH6CrkRows");
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4 / NG;            // j-bodies per stage: JB * NG = 4 independent chains
    constexpr uint32_t ROWS = kBlock * 2 * NG;
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][4][TILE];   // [buffer][0 = positions, 1 = velocities, 2 = accelerations, 3 = jerks][row]
    const int tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * ROWS;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG], ui[NG], vi[NG], wi[NG], fi[NG], gi[NG], hi[NG], ki[NG], li[NG], mi[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const uint32_t c0 = il0 < n ? il0 : n - 1, c1 = il1 < n ? il1 : n - 1;        // clamped, branch-free (never stored)
        const float4 b0 = ld4(pos + c0), b1 = ld4(pos + c1), v0 = ld4(vel + c0), v1 = ld4(vel + c1);
        const float4 a0 = ld4(acc + c0), a1 = ld4(acc + c1), k0 = ld4(jrk + c0), k1 = ld4(jrk + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        ui[g] = nb_f2{v0.x, v1.x}; vi[g] = nb_f2{v0.y, v1.y}; wi[g] = nb_f2{v0.z, v1.z};
        fi[g] = nb_f2{a0.x, a1.x}; gi[g] = nb_f2{a0.y, a1.y}; hi[g] = nb_f2{a0.z, a1.z};
        ki[g] = nb_f2{k0.x, k1.x}; li[g] = nb_f2{k0.y, k1.y}; mi[g] = nb_f2{k0.z, k1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 sm[NG][3], SM[NG][3];           // first- and second-level sums of the crackle
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sm[g][k] = SM[g][k] = zero;
    }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const nb_f2 p2 = nb_f2{2.0f, 2.0f};
    const nb_f2 p3 = nb_f2{3.0f, 3.0f};
    const nb_f2 p4 = nb_f2{4.0f, 4.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_h6_fjs_pk::stage, four tiles per stage
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const float4* src[4] = {pos, vel, acc, jrk};
        unsigned keep;
        if (jt + TILE <= j1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float4* base = src[p] + jt;
                const uint32_t dst = lds_wave + (uint32_t)((buf * 4 + p) * TILE) * 16u;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane_off), "s"(base), "s"(dst) : "memory");
            }
        } else {
            const uint32_t j = jt + tid;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float4* row = j < j1 ? src[p] + j : zero_row;
                const uint32_t dst = lds_wave + (uint32_t)((buf * 4 + p) * TILE) * 16u;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(row), "s"(dst) : "memory");
            }
        }
    };

    // one stage: JB tile rows (positions p, velocities q, accelerations r, jerks k) against the lane's NG packed groups, stage-major
    // over the NC chains
    auto math = [&](const float4* p, const float4* q, const float4* r, const float4* k) {
        nb_f2 bx[JB], by[JB], bz[JB], bu[JB], bv[JB], bw[JB], bf[JB], bg[JB], bh[JB], bk[JB], bl[JB], bn[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u], c = q[u], d = r[u], e = k[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z};
            bf[u] = nb_f2{d.x, d.x}; bg[u] = nb_f2{d.y, d.y}; bh[u] = nb_f2{d.z, d.z};
            bk[u] = nb_f2{e.x, e.x}; bl[u] = nb_f2{e.y, e.y}; bn[u] = nb_f2{e.z, e.z};
        }
        nb_f2 dx[NC], dy[NC], dz[NC], du[NC], dv[NC], dw[NC], df[NC], dg[NC], dh[NC], dk[NC], dl[NC], dn[NC];
        nb_f2 d2[NC], y[NC], s[NC], rv[NC], vv[NC], gg[NC], q6[NC], q9[NC], b9[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) dx[c] = bx[c / NG] - xi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dy[c] = by[c / NG] - yi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dz[c] = bz[c / NG] - zi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dx[c], dx[c], e2);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = nb_f2{nb_rsq(d2[c].x), nb_rsq(d2[c].y)};
        // the differences and the dot products need nothing of the reciprocal roots: they fill the slots behind them
#pragma unroll
        for (int c = 0; c < NC; ++c) du[c] = bu[c / NG] - ui[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dv[c] = bv[c / NG] - vi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dw[c] = bw[c / NG] - wi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = dx[c] * du[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = __builtin_elementwise_fma(dy[c], dv[c], rv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = __builtin_elementwise_fma(dz[c], dw[c], rv[c]);      // dr.dv
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = bf[c / NG] - fi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = bg[c / NG] - gi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = bh[c / NG] - hi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = du[c] * du[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dv[c], dv[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dw[c], dw[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dx[c], df[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dy[c], dg[c], vv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(dz[c], dh[c], vv[c]);      // dv.dv + dr.da
#pragma unroll
        for (int c = 0; c < NC; ++c) dk[c] = bk[c / NG] - ki[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dl[c] = bl[c / NG] - li[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dn[c] = bn[c / NG] - mi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = du[c] * df[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = __builtin_elementwise_fma(dv[c], dg[c], gg[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = __builtin_elementwise_fma(dw[c], dh[c], gg[c]);      // dv.da
#pragma unroll
        for (int c = 0; c < NC; ++c) q6[c] = dx[c] * dk[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) q6[c] = __builtin_elementwise_fma(dy[c], dl[c], q6[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) q6[c] = __builtin_elementwise_fma(dz[c], dn[c], q6[c]);      // dr.dj
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = __builtin_elementwise_fma(gg[c], p3, q6[c]);         // 3 dv.da + dr.dj
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = nb_f2{bm[c / NG], bm[c / NG]} * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * y[c];                 // alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = rv[c] * rv[c];                // alpha^2
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = __builtin_elementwise_fma(vv[c], y[c], d2[c]);       // beta
#pragma unroll
        for (int c = 0; c < NC; ++c) vv[c] = vv[c] * m3;                   // -3 beta
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(d2[c], p4, vv[c]);         // 4 alpha^2 - 3 beta
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = rv[c] * d2[c];                // -alpha (3 beta - 4 alpha^2)
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = __builtin_elementwise_fma(gg[c], y[c], -d2[c]);      // gamma
#pragma unroll
        for (int c = 0; c < NC; ++c) gg[c] = gg[c] * m3;                   // -3 gamma
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * m3;                   // -3 alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) q6[c] = rv[c] * p2;                   // -6 alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) q9[c] = rv[c] * p3;                   // -9 alpha
#pragma unroll
        for (int c = 0; c < NC; ++c) b9[c] = vv[c] * p3;                   // -9 beta
#pragma unroll
        for (int c = 0; c < NC; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 alpha dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = __builtin_elementwise_fma(q6[c], du[c], df[c]);      // q = da - 6 alpha t - 3 beta dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = __builtin_elementwise_fma(q6[c], dv[c], dg[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = __builtin_elementwise_fma(q6[c], dw[c], dh[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) df[c] = __builtin_elementwise_fma(vv[c], dx[c], df[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dg[c] = __builtin_elementwise_fma(vv[c], dy[c], dg[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dh[c] = __builtin_elementwise_fma(vv[c], dz[c], dh[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dk[c] = __builtin_elementwise_fma(q9[c], df[c], dk[c]);      // w = dj - 9 alpha q - 9 beta t - 3 gamma dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dl[c] = __builtin_elementwise_fma(q9[c], dg[c], dl[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dn[c] = __builtin_elementwise_fma(q9[c], dh[c], dn[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dk[c] = __builtin_elementwise_fma(b9[c], du[c], dk[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dl[c] = __builtin_elementwise_fma(b9[c], dv[c], dl[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dn[c] = __builtin_elementwise_fma(b9[c], dw[c], dn[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dk[c] = __builtin_elementwise_fma(gg[c], dx[c], dk[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dl[c] = __builtin_elementwise_fma(gg[c], dy[c], dl[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dn[c] = __builtin_elementwise_fma(gg[c], dz[c], dn[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][0] = __builtin_elementwise_fma(s[c], dk[c], sm[c % NG][0]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][1] = __builtin_elementwise_fma(s[c], dl[c], sm[c % NG][1]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c % NG][2] = __builtin_elementwise_fma(s[c], dn[c], sm[c % NG][2]);
    };
    auto flush = [&]() {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { SM[g][k] = SM[g][k] + sm[g][k]; sm[g][k] = zero; }
        }
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cur ^ 1);      // lands under this tile's compute
        const uint32_t left = j1 - (j0 + t * TILE);
        const int cnt = left < (uint32_t)TILE ? (int)left : TILE;
        const int chunks = (cnt + U - 1) / U;             // rows past the range are staged zero-mass bodies
        for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
            for (int uu = 0; uu < U / JB; ++uu) {
                const int r = ch * U + uu * JB;
                math(&tile[cur][0][r], &tile[cur][1][r], &tile[cur][2][r], &tile[cur][3][r]);
            }
        }
        if ((t & (kH6Flush - 1)) == kH6Flush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    float4* oc = pc + (size_t)blockIdx.y * n;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        if (il0 < n) oc[il0] = float4{SM[g][0].x, SM[g][1].x, SM[g][2].x, 0.0f};
        if (il1 < n) oc[il1] = float4{SM[g][0].y, SM[g][1].y, SM[g][2].y, 0.0f};
    }
}

// fp64 handles.  nb_h6_fjs64 with a fourth tile through registers; every difference, product and sum is fp64.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_crk64(const typename vec4<T>::type* __restrict__ pos,
                                                     const typename vec4<T>::type* __restrict__ vel,
                                                     const typename vec4<T>::type* __restrict__ acc,
                                                     const typename vec4<T>::type* __restrict__ jrk, double4* __restrict__ pc,
                                                     uint32_t n, uint32_t j_per_chunk, double eps2)
{
    static_assert(std::is_same<T, double>::value, "the fp64 pass of fp64 handles");
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[kTile];
    __shared__ double4 ta[kTile];
    __shared__ double4 tj[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kH6Rows64 + tid;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const uint32_t ic = il < n ? il : n - 1;
    const double4 bi = ld4(pos + ic), wi = ld4(vel + ic), ci = ld4(acc + ic), ki = ld4(jrk + ic);
    double cx = 0.0, cy = 0.0, cz = 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const double4 b = ld4(pos + j), c = ld4(vel + j), d = ld4(acc + j), e = ld4(jrk + j);
            tp[tid] = b;
            tv[tid] = double4{c.x, c.y, c.z, 0.0};
            ta[tid] = double4{d.x, d.y, d.z, 0.0};
            tj[tid] = double4{e.x, e.y, e.z, 0.0};
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
            ta[tid] = double4{0.0, 0.0, 0.0, 0.0};
            tj[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 2
        for (int jj = 0; jj < cnt; ++jj) {
            const double4 b = tp[jj], c = tv[jj], d = ta[jj], k = tj[jj];
            const double dx = b.x - bi.x, dy = b.y - bi.y, dz = b.z - bi.z;
            const double du = c.x - wi.x, dv = c.y - wi.y, dw = c.z - wi.z;
            const double df = d.x - ci.x, dg = d.y - ci.y, dh = d.z - ci.z;
            const double dk = k.x - ki.x, dl = k.y - ki.y, dn = k.z - ki.z;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double y2 = y * y;
            const double s3 = (b.w * y) * y2;
            const double alpha = nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2;
            const double vr = nb_fma(dz, dh, nb_fma(dy, dg, nb_fma(dx, df, nb_fma(dw, dw, nb_fma(dv, dv, du * du)))));
            const double a2 = alpha * alpha;
            const double beta = nb_fma(vr, y2, a2);
            const double va = nb_fma(dw, dh, nb_fma(dv, dg, du * df));
            const double rj = nb_fma(dz, dn, nb_fma(dy, dl, dx * dk));
            const double gamma = nb_fma(nb_fma(3.0, va, rj), y2, alpha * nb_fma(-4.0, a2, 3.0 * beta));
            const double q3 = -3.0 * alpha, q6 = -6.0 * alpha, q9 = -9.0 * alpha, b3 = -3.0 * beta, b9 = -9.0 * beta, g3 = -3.0 * gamma;
            const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
            const double ux = nb_fma(b3, dx, nb_fma(q6, tx, df)), uy = nb_fma(b3, dy, nb_fma(q6, ty, dg)),
                         uz = nb_fma(b3, dz, nb_fma(q6, tz, dh));
            const double wx = nb_fma(g3, dx, nb_fma(b9, tx, nb_fma(q9, ux, dk))), wy = nb_fma(g3, dy, nb_fma(b9, ty, nb_fma(q9, uy, dl))),
                         wz = nb_fma(g3, dz, nb_fma(b9, tz, nb_fma(q9, uz, dn)));
            cx = nb_fma(s3, wx, cx); cy = nb_fma(s3, wy, cy); cz = nb_fma(s3, wz, cz);
        }
    }
    if (il < n) pc[(size_t)blockIdx.y * n + il] = double4{cx, cy, cz, 0.0};
}

// nb_h6_reduce for one plane: a body's chunk rows added in ascending chunk order in fp64, G applied once.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_h6_reduce1(const typename vec4<T>::type* __restrict__ pc, uint32_t n, uint32_t chunks,
                                                       double G, typename vec4<T>::type* __restrict__ out)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const auto p = ld4(pc + (size_t)c * n + il);
        sx += (double)p.x; sy += (double)p.y; sz += (double)p.z;
    }
    out[il] = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
}

}  // namespace nb
