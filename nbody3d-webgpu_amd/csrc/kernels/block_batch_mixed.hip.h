// kernels/block_batch_mixed.hip.h -- the batched block steps of kernels/block_batch.hip.h on mixed-precision handles
// (nb_set_block_batch_mixed: order-4 NB_F64 block-step handles with nb_set_pass_precision(NB_PASS_MIXED) and no guard).  No reference
// analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// A slot is round 25's: nb_blkq_sched (the same instantiation), then
//   nb_blkqm_predict   nb_mx_blk_predict behind nb_blkq_predict's idle test: the three binary32 streams (xh, mf), xl, vf
//   nb_blkqm_fj        the small pass in nb_blkq_fj_pk's shape on fj_mx_body's double-single arithmetic (kernels/mixed.hip.h)
//   nb_blkq_correct<float, double>   the binary32 chunk rows summed in fp64 into the fp64 state
// What a small step computes for a body depends on the three predicted streams and on n alone, as there: a list row is one lane's
// chain over the rows of a j-chunk in four fixed quarters, the quarters are added in wave order, the chunks in an order the chunk
// count fixes.  Nothing here may be re-associated: the build has no fast-math.
#pragma once

namespace nb {

// nb_mx_blk_predict for a slot that is not idle.
template <int UNUSED = 0>     // a template only so that the header can be included by several translation units
__global__ __launch_bounds__(kBlock) void nb_blkqm_predict(const double4* __restrict__ x, const double4* __restrict__ v,
                                                          const double4* __restrict__ a, const double4* __restrict__ j,
                                                          const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                          float4* __restrict__ xh, float4* __restrict__ xl,
                                                          float4* __restrict__ vf, uint32_t n, const uint32_t* __restrict__ hdr,
                                                          uint32_t L, double tick, const uint32_t* __restrict__ bb)
{
    if (bb[kBbMode] == kBbModeIdle) return;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const uint32_t t_next = hdr[kBlkNext];
    const double4 X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il);
    const uint32_t t_i = due[il] - (1u << (L - lev[il]));
    const double h = (double)(t_next - t_i) * tick;
    const double h2 = h * (1.0 / 2.0), h3 = h * (1.0 / 3.0);
    auto px = [&](double x0, double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, nb_fma(h3, j0, a0), v0), x0); };
    auto pv = [&](double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, j0, a0), v0); };
    float4 hi, lo, f;
    mx_split_row(px(X.x, V.x, A.x, J.x), px(X.y, V.y, A.y, J.y), px(X.z, V.z, A.z, J.z), X.w,
                 pv(V.x, A.x, J.x), pv(V.y, A.y, J.y), pv(V.z, A.z, J.z), hi, lo, f);
    xh[il] = hi; xl[il] = lo; vf[il] = f;
}

// The small double-single force+jerk pass.  Grid (ceil(small_max / 128), j-chunks).  nb_blkq_fj_pk<1>'s shape: the four waves of a
// workgroup hold the SAME 128 list slots (one packed pair per lane, nine packed i-values), the workgroup stages fj_mx_body's three
// LDS-DMA tile streams, and wave w sweeps rows [64 w, 64 w + 64) of each tile with fj_mx_body's instruction sequence per pair
// (dr = (xh_j - xh_i) + (xl_j - xl_i), dv = vf_j - vf_i, then nb_fj_pk's).  The four waves' binary32 sums meet in LDS and are added
// in wave order; one compact binary32 partial row per (j-chunk, list slot) at pa[c * small_max + k].  Lanes past |A| clamp and
// store nothing; a workgroup whose first slot is past |A| leaves after the header loads.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_blkqm_fj(const float4* __restrict__ xh, const float4* __restrict__ xl, const float4* __restrict__ vf,
                 const uint32_t* __restrict__ act, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb,
                 uint32_t small_max, float4* __restrict__ pa, float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2,
                 const float4* __restrict__ zero_row)
{
    static_assert(NG == 1, "one packed pair per lane");
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4;                 // j-bodies per stage: four independent chains
    __shared__ float4 tile[2][3][TILE];   // [buffer][0 = (xh, mf), 1 = xl, 2 = vf][row]
    __shared__ float red[4][6][kBbRows];  // [wave][ax ay az jx jy jz][slot]
    const uint32_t i0 = blockIdx.x * kBbRows;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t ni = hdr[kBlkCount];
    if (ni == 0 || ni > small_max || ni > n || i0 >= ni) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi, yi, zi, xli, yli, zli, ui, vi, wi;
    {
        const uint32_t il0 = i0 + lane, il1 = il0 + 64;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        c0 = act[c0]; c1 = act[c1];
        c0 = c0 < n ? c0 : n - 1; c1 = c1 < n ? c1 : n - 1;
        const float4 b0 = ld4(xh + c0), b1 = ld4(xh + c1), l0 = ld4(xl + c0), l1 = ld4(xl + c1), v0 = ld4(vf + c0), v1 = ld4(vf + c1);
        xi = nb_f2{b0.x, b1.x}; yi = nb_f2{b0.y, b1.y}; zi = nb_f2{b0.z, b1.z};
        xli = nb_f2{l0.x, l1.x}; yli = nb_f2{l0.y, l1.y}; zli = nb_f2{l0.z, l1.z};
        ui = nb_f2{v0.x, v1.x}; vi = nb_f2{v0.y, v1.y}; wi = nb_f2{v0.z, v1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 ax = zero, ay = zero, az = zero, jx = zero, jy = zero, jz = zero;
    nb_f2 AX = zero, AY = zero, AZ = zero, JX = zero, JY = zero, JZ = zero;
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as fj_mx_body::stage: three tiles per stage
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst = lds_wave + (uint32_t)(buf * 3 * TILE) * 16u;
        const float4* const src[3] = {xh, xl, vf};
        unsigned keep;
        if (jt + TILE <= j1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4* bp = src[k] + jt;
                const uint32_t d = dst + (uint32_t)(k * TILE) * 16u;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane_off), "s"(bp), "s"(d) : "memory");
            }
        } else {
            const uint32_t j = jt + tid;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4* sp = j < j1 ? src[k] + j : zero_row;
                const uint32_t d = dst + (uint32_t)(k * TILE) * 16u;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(sp), "s"(d) : "memory");
            }
        }
    };

    // one stage: JB tile rows (hi words p, lo words l, velocities q) against the lane's packed pair, stage-major over the JB chains
    // (fj_mx_body::math with NG = 1)
    auto math = [&](const float4* p, const float4* l, const float4* q) {
        nb_f2 bx[JB], by[JB], bz[JB], lx[JB], ly[JB], lz[JB], bu[JB], bv[JB], bw[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u], d = l[u], c = q[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            lx[u] = nb_f2{d.x, d.x}; ly[u] = nb_f2{d.y, d.y}; lz[u] = nb_f2{d.z, d.z};
            bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z};
        }
        nb_f2 dx[JB], dy[JB], dz[JB], ex[JB], ey[JB], ez[JB], du[JB], dv[JB], dw[JB], d2[JB], y[JB], s[JB], rv[JB];
        // the double-single difference: hi words, lo words, then their sum
#pragma unroll
        for (int c = 0; c < JB; ++c) dx[c] = bx[c] - xi;
#pragma unroll
        for (int c = 0; c < JB; ++c) ex[c] = lx[c] - xli;
#pragma unroll
        for (int c = 0; c < JB; ++c) dy[c] = by[c] - yi;
#pragma unroll
        for (int c = 0; c < JB; ++c) ey[c] = ly[c] - yli;
#pragma unroll
        for (int c = 0; c < JB; ++c) dz[c] = bz[c] - zi;
#pragma unroll
        for (int c = 0; c < JB; ++c) ez[c] = lz[c] - zli;
#pragma unroll
        for (int c = 0; c < JB; ++c) dx[c] = dx[c] + ex[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) dy[c] = dy[c] + ey[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) dz[c] = dz[c] + ez[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dx[c], dx[c], e2);
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) y[c] = nb_f2{nb_rsq(d2[c].x), nb_rsq(d2[c].y)};
        // the velocity differences and dr.dv need nothing of the reciprocal roots: they fill the slots behind them
#pragma unroll
        for (int c = 0; c < JB; ++c) du[c] = bu[c] - ui;
#pragma unroll
        for (int c = 0; c < JB; ++c) dv[c] = bv[c] - vi;
#pragma unroll
        for (int c = 0; c < JB; ++c) dw[c] = bw[c] - wi;
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = dx[c] * du[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = __builtin_elementwise_fma(dy[c], dv[c], rv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = __builtin_elementwise_fma(dz[c], dw[c], rv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) s[c] = nb_f2{bm[c], bm[c]} * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * y[c];                 // q = (dr.dv) / rho^2
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * m3;                   // -3 q
#pragma unroll
        for (int c = 0; c < JB; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 q dr
#pragma unroll
        for (int c = 0; c < JB; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) jx = __builtin_elementwise_fma(s[c], du[c], jx);
#pragma unroll
        for (int c = 0; c < JB; ++c) jy = __builtin_elementwise_fma(s[c], dv[c], jy);
#pragma unroll
        for (int c = 0; c < JB; ++c) jz = __builtin_elementwise_fma(s[c], dw[c], jz);
#pragma unroll
        for (int c = 0; c < JB; ++c) ax = __builtin_elementwise_fma(s[c], dx[c], ax);
#pragma unroll
        for (int c = 0; c < JB; ++c) ay = __builtin_elementwise_fma(s[c], dy[c], ay);
#pragma unroll
        for (int c = 0; c < JB; ++c) az = __builtin_elementwise_fma(s[c], dz[c], az);
    };
    auto flush = [&]() {
        AX = AX + ax; AY = AY + ay; AZ = AZ + az;
        JX = JX + jx; JY = JY + jy; JZ = JZ + jz;
        ax = ay = az = jx = jy = jz = zero;
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cur ^ 1);      // lands under this tile's compute
        const uint32_t left = j1 - (j0 + t * TILE);
        const int cnt = left < (uint32_t)TILE ? (int)left : TILE;
        const int cntu = (cnt + U - 1) / U * U;           // rows past the range are staged zero-mass bodies
        const int lo = 64 * wave, hi = lo + 64 < cntu ? lo + 64 : cntu;      // the wave's quarter of the tile
        for (int r = lo; r < hi; r += U) {
            math(&tile[cur][0][r], &tile[cur][1][r], &tile[cur][2][r]);
            math(&tile[cur][0][r + JB], &tile[cur][1][r + JB], &tile[cur][2][r + JB]);
        }
        if ((t & 15u) == 15u) flush();                    // 1,024 terms per chain, as nb_blkq_fj_pk
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    red[wave][0][lane] = AX.x; red[wave][0][lane + 64] = AX.y;
    red[wave][1][lane] = AY.x; red[wave][1][lane + 64] = AY.y;
    red[wave][2][lane] = AZ.x; red[wave][2][lane + 64] = AZ.y;
    red[wave][3][lane] = JX.x; red[wave][3][lane + 64] = JX.y;
    red[wave][4][lane] = JY.x; red[wave][4][lane + 64] = JY.y;
    red[wave][5][lane] = JZ.x; red[wave][5][lane + 64] = JZ.y;
    __syncthreads();
    const uint32_t k = i0 + (uint32_t)tid;
    if (tid < (int)kBbRows && k < ni) {
        float r[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) r[c] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
        pa[(size_t)blockIdx.y * small_max + k] = float4{r[0], r[1], r[2], 0.0f};
        pj[(size_t)blockIdx.y * small_max + k] = float4{r[3], r[4], r[5], 0.0f};
    }
}

}  // namespace nb
