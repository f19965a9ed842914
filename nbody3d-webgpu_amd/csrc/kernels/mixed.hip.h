// kernels/mixed.hip.h -- the mixed-precision force+jerk pass of NB_F64 Hermite handles of order 4 (nb_set_pass_precision(NB_PASS_MIXED)):
// the state stays fp64, the O(N^2) pass runs nb_fj_pk's binary32 pair arithmetic on positions carried as a double-single pair of
// binary32 words (as GRAPE-6, Sapporo and phi-GPU do).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// Per body, from the fp64 row:   xh = (float)x    xl = (float)(x - (double)xh)    vf = (float)v    mf = (float)m
// Per pair, all binary32:        dr = (xh_j - xh_i) + (xl_j - xl_i)      (the two differences first, then their sum)
//                                dv = vf_j - vf_i
// and from there nb_fj_pk's sequence unchanged (kernels/hermite.hip.h): rho^2, v_rsq_f32, s3, q, the single-sum jerk s3 (dv - 3 q dr).
// For two bodies closer than a factor two in every coordinate xh_j - xh_i is exact, and so dr is good to ~1e-7 OF ITSELF however
// close the pair is -- where the difference of two binary32 positions at |x| ~ 1 is wrong by 6e-8 / |dr|.  Nothing here may be
// re-associated: the build has no fast-math.
//   Sums: as nb_fj_pk -- binary32 in two levels (a register takes at most 1,024 terms, then the chunk), fp64 across the j-chunks in
// ascending order (nb_fj_reduce<float, double> / nb_blk_correct<float, double>), times G once.  The self term is exactly 0
// (dr = dv = 0, eps2 > 0); rows past the range come from zero_row (zero mass).
//   The kernels: nb_mx_split (the stored state -> the three streams: the start, nb_force_pass), nb_mx_predict / nb_mx_blk_predict
// (the shared and the block predictor, writing the three streams instead of xp / vp: no launch more than a native step),
// nb_mx_fj<NG> / nb_mx_blk_fj<NG> (the pass and its gathered form).
#pragma once

namespace nb {

#ifndef NB_MX_WAVES
#define NB_MX_WAVES 2                               // waves per SIMD nb_mx_fj is compiled for
#endif

// One fp64 (position, velocity) row as the pass's three binary32 rows.
__device__ __forceinline__ void mx_split_row(double x, double y, double z, double m, double u, double v, double w,
                                             float4& xh, float4& xl, float4& vf)
{
    const float hx = (float)x, hy = (float)y, hz = (float)z;
    xh = float4{hx, hy, hz, (float)m};
    xl = float4{(float)(x - (double)hx), (float)(y - (double)hy), (float)(z - (double)hz), 0.0f};
    vf = float4{(float)u, (float)v, (float)w, 0.0f};
}

template <int UNUSED = 0>     // a template only so that the header can be included by several translation units
__global__ __launch_bounds__(kBlock) void nb_mx_split(const double4* __restrict__ x, const double4* __restrict__ v,
                                                     float4* __restrict__ xh, float4* __restrict__ xl, float4* __restrict__ vf,
                                                     uint32_t n)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const double4 X = ld4(x + il), V = ld4(v + il);
    float4 h, l, f;
    mx_split_row(X.x, X.y, X.z, X.w, V.x, V.y, V.z, h, l, f);
    xh[il] = h; xl[il] = l; vf[il] = f;
}

// nb_hermite_predict<double>'s polynomial, rounded once to double as there, then split.
template <int UNUSED = 0>
__global__ __launch_bounds__(kBlock) void nb_mx_predict(const double4* __restrict__ x, const double4* __restrict__ v,
                                                       const double4* __restrict__ a, const double4* __restrict__ j,
                                                       float4* __restrict__ xh, float4* __restrict__ xl, float4* __restrict__ vf,
                                                       uint32_t n, double h)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const double4 X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il);
    const double h2 = h * (1.0 / 2.0), h3 = h * (1.0 / 3.0);
    auto px = [&](double x0, double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, nb_fma(h3, j0, a0), v0), x0); };
    auto pv = [&](double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, j0, a0), v0); };
    float4 hi, lo, f;
    mx_split_row(px(X.x, V.x, A.x, J.x), px(X.y, V.y, A.y, J.y), px(X.z, V.z, A.z, J.z), X.w,
                 pv(V.x, A.x, J.x), pv(V.y, A.y, J.y), pv(V.z, A.z, J.z), hi, lo, f);
    xh[il] = hi; xl[il] = lo; vf[il] = f;
}

// nb_blk_predict<double>'s (every body over its own h_i = (t_next - t_i) ticks, from the stored state), then split.
template <int UNUSED = 0>
__global__ __launch_bounds__(kBlock) void nb_mx_blk_predict(const double4* __restrict__ x, const double4* __restrict__ v,
                                                           const double4* __restrict__ a, const double4* __restrict__ j,
                                                           const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                           float4* __restrict__ xh, float4* __restrict__ xl,
                                                           float4* __restrict__ vf, uint32_t n, const uint32_t* __restrict__ hdr,
                                                           uint32_t L, double tick)
{
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

// fj_pk_body (kernels/hermite.hip.h) with a third LDS-DMA tile stream: (xh, mf), xl, vf.  Staging, double buffering, the zero-row
// tail, the stage-major issue over the chains, the two-level sums and the GATHER form (compact partial rows of the active list) are
// that body's; the i-rows carry three more packed values per group (the lo words) and a pair three more packed additions per
// component pair: 32 packed + 2 transcendental per two pairs = 144 issue cycles by DESIGN §4.1's accounting (nb_fj_pk: 120).
//   GUARD (nb_set_pass_guard, kernels/guard.hip.h): a pair with d2 < near2 is NEAR.  Per stage the compares' lane masks are ORed on
// the scalar unit and one wave-uniform branch chooses between the sums above (no lane of the wave has a near pair among the stage's
// rows) and the slow sums: the weight s3 goes by v_cndmask to exactly one of w_far and w_near, the far fma runs with w_far (a lane
// without a near pair: exactly the fast path's fma), and the rounded products w_near * term enter an unevaluated binary32 pair
// (hi, lo) per component by branch-free TwoSum (a far pair: p = 0, which changes neither word).  The 12 NG packed near words of a
// lane live in LDS, [group][word][lane], touched on the slow path and in the epilogue only; they are never flushed.  The partial row is
// ((double)far + (double)hi) + (double)lo, stored as fp64.  Without GUARD none of this is compiled.
template <bool WIDE> struct mx_part { using type = float; };
template <> struct mx_part<true> { using type = double; };

template <int NG, bool GATHER, bool GUARD = false>
__device__ __forceinline__ void fj_mx_body(const float4* __restrict__ xh, const float4* __restrict__ xl,
                                           const float4* __restrict__ vf, const uint32_t* __restrict__ act, uint32_t ni,
                                           typename vec4<typename mx_part<GUARD>::type>::type* __restrict__ pa,
                                           typename vec4<typename mx_part<GUARD>::type>::type* __restrict__ pj, uint32_t n,
                                           uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row, float near2 = 0.0f)
{
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4 / NG;            // j-bodies per stage: JB * NG = 4 independent chains
    constexpr uint32_t ROWS = kBlock * 2 * NG;
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][3][TILE];   // [buffer][0 = (xh, mf), 1 = xl, 2 = vf][row]
    __shared__ nb_f2 nearw[GUARD ? NG : 1][GUARD ? 12 : 1][GUARD ? kBlock : 1];      // GUARD: [group][2 * component + (0 = hi, 1 = lo)][lane]
    const int tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * ROWS;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG], xli[NG], yli[NG], zli[NG], ui[NG], vi[NG], wi[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        if constexpr (GATHER) { c0 = act[c0]; c1 = act[c1]; }
        const float4 b0 = ld4(xh + c0), b1 = ld4(xh + c1), l0 = ld4(xl + c0), l1 = ld4(xl + c1), v0 = ld4(vf + c0), v1 = ld4(vf + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        xli[g] = nb_f2{l0.x, l1.x}; yli[g] = nb_f2{l0.y, l1.y}; zli[g] = nb_f2{l0.z, l1.z};
        ui[g] = nb_f2{v0.x, v1.x}; vi[g] = nb_f2{v0.y, v1.y}; wi[g] = nb_f2{v0.z, v1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 ax[NG], ay[NG], az[NG], jx[NG], jy[NG], jz[NG], AX[NG], AY[NG], AZ[NG], JX[NG], JY[NG], JZ[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ax[g] = ay[g] = az[g] = jx[g] = jy[g] = jz[g] = zero;
        AX[g] = AY[g] = AZ[g] = JX[g] = JY[g] = JZ[g] = zero;
    }
    if constexpr (GUARD) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int k = 0; k < 12; ++k) nearw[g][k][tid] = zero;         // a lane reads and writes its own words only: no barrier
    }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as fj_pk_body::stage: whole tiles from a scalar base, the last one per lane with rows past the range
    // taken from zero_row; three tiles per stage
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

    // one stage: JB tile rows (hi words p, lo words l, velocities q) against the lane's NG packed groups, stage-major over the NC chains
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
        nb_f2 dx[NC], dy[NC], dz[NC], ex[NC], ey[NC], ez[NC], du[NC], dv[NC], dw[NC], d2[NC], y[NC], s[NC], rv[NC];
        // the double-single difference: hi words, lo words, then their sum
#pragma unroll
        for (int c = 0; c < NC; ++c) dx[c] = bx[c / NG] - xi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) ex[c] = lx[c / NG] - xli[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dy[c] = by[c / NG] - yi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) ey[c] = ly[c / NG] - yli[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dz[c] = bz[c / NG] - zi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) ez[c] = lz[c / NG] - zli[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dx[c] = dx[c] + ex[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) dy[c] = dy[c] + ey[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) dz[c] = dz[c] + ez[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dx[c], dx[c], e2);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = nb_f2{nb_rsq(d2[c].x), nb_rsq(d2[c].y)};
        // the velocity differences and dr.dv need nothing of the reciprocal roots: they fill the slots behind them
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
        for (int c = 0; c < NC; ++c) s[c] = nb_f2{bm[c / NG], bm[c / NG]} * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * y[c];                 // q = (dr.dv) / rho^2
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[c] = rv[c] * m3;                   // -3 q
#pragma unroll
        for (int c = 0; c < NC; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 q dr
#pragma unroll
        for (int c = 0; c < NC; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
        auto fast = [&]() {
#pragma unroll
            for (int c = 0; c < NC; ++c) jx[c % NG] = __builtin_elementwise_fma(s[c], du[c], jx[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jy[c % NG] = __builtin_elementwise_fma(s[c], dv[c], jy[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jz[c % NG] = __builtin_elementwise_fma(s[c], dw[c], jz[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) ax[c % NG] = __builtin_elementwise_fma(s[c], dx[c], ax[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) ay[c % NG] = __builtin_elementwise_fma(s[c], dy[c], ay[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) az[c % NG] = __builtin_elementwise_fma(s[c], dz[c], az[c % NG]);
        };
        if constexpr (!GUARD) fast();
        else {
            bool nr[NC][2];
            bool hit = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                nr[c][0] = d2[c].x < near2; nr[c][1] = d2[c].y < near2;
                hit |= nr[c][0] | nr[c][1];
            }
            if (__builtin_amdgcn_ballot_w64(hit) == 0) fast();      // wave-uniform: no lane has a near pair among these JB rows
            else {
                nb_f2 wn[NC], wf[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    wn[c] = nb_f2{nr[c][0] ? s[c].x : 0.0f, nr[c][1] ? s[c].y : 0.0f};
                    wf[c] = nb_f2{nr[c][0] ? 0.0f : s[c].x, nr[c][1] ? 0.0f : s[c].y};
                }
                // one component: the far fma, then the near TwoSum; c = u * NG + g: a row meets its pairs in ascending j
                auto both = [&](const nb_f2 (&term)[NC], nb_f2 (&far)[NG], int k) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) far[c % NG] = __builtin_elementwise_fma(wf[c], term[c], far[c % NG]);
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        nb_f2 hi = nearw[g][2 * k][tid], lo = nearw[g][2 * k + 1][tid];
#pragma unroll
                        for (int u = 0; u < JB; ++u) {
                            const nb_f2 p = wn[u * NG + g] * term[u * NG + g];
                            const nb_f2 sm = hi + p;
                            const nb_f2 bb = sm - hi;
                            const nb_f2 hs = sm - bb;
                            const nb_f2 e0 = hi - hs;
                            const nb_f2 e1 = p - bb;
                            const nb_f2 e = e0 + e1;
                            hi = sm;
                            lo = lo + e;
                        }
                        nearw[g][2 * k][tid] = hi; nearw[g][2 * k + 1][tid] = lo;
                    }
                };
                both(du, jx, 3); both(dv, jy, 4); both(dw, jz, 5);
                both(dx, ax, 0); both(dy, ay, 1); both(dz, az, 2);
            }
        }
    };
    auto flush = [&]() {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            AX[g] = AX[g] + ax[g]; AY[g] = AY[g] + ay[g]; AZ[g] = AZ[g] + az[g];
            JX[g] = JX[g] + jx[g]; JY[g] = JY[g] + jy[g]; JZ[g] = JZ[g] + jz[g];
            ax[g] = ay[g] = az[g] = jx[g] = jy[g] = jz[g] = zero;
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
        if ((t & (kFjFlush - 1)) == kFjFlush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    if constexpr (GUARD) {
        double4* oa = pa + (size_t)blockIdx.y * ni;
        double4* oj = pj + (size_t)blockIdx.y * ni;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
            const nb_f2 far[6] = {AX[g], AY[g], AZ[g], JX[g], JY[g], JZ[g]};
            double r0[6], r1[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const nb_f2 hi = nearw[g][2 * k][tid], lo = nearw[g][2 * k + 1][tid];
                r0[k] = ((double)far[k].x + (double)hi.x) + (double)lo.x;
                r1[k] = ((double)far[k].y + (double)hi.y) + (double)lo.y;
            }
            if (il0 < ni) { oa[il0] = double4{r0[0], r0[1], r0[2], 0.0}; oj[il0] = double4{r0[3], r0[4], r0[5], 0.0}; }
            if (il1 < ni) { oa[il1] = double4{r1[0], r1[1], r1[2], 0.0}; oj[il1] = double4{r1[3], r1[4], r1[5], 0.0}; }
        }
    } else {
        float4* oa = pa + (size_t)blockIdx.y * ni;
        float4* oj = pj + (size_t)blockIdx.y * ni;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
            if (il0 < ni) { oa[il0] = float4{AX[g].x, AY[g].x, AZ[g].x, 0.0f}; oj[il0] = float4{JX[g].x, JY[g].x, JZ[g].x, 0.0f}; }
            if (il1 < ni) { oa[il1] = float4{AX[g].y, AY[g].y, AZ[g].y, 0.0f}; oj[il1] = float4{JX[g].y, JY[g].y, JZ[g].y, 0.0f}; }
        }
    }
}

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_MX_WAVES, NB_MX_WAVES)))
void nb_mx_fj(const float4* __restrict__ xh, const float4* __restrict__ xl, const float4* __restrict__ vf, float4* __restrict__ pa,
              float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    static_assert(kBlock * 2 * NG == kFjRows, "the engine sizes the grid by kFjRows");
    fj_mx_body<NG, false>(xh, xl, vf, nullptr, n, pa, pj, n, j_per_chunk, eps2, zero_row);
}

// The gathered pass of a block step, as nb_blk_fj_pk<2 | 1> (kernels/block.hip.h): NG = 2: 1,024 rows per workgroup, NG = 1: 512.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_MX_WAVES, NB_MX_WAVES)))
void nb_mx_blk_fj(const float4* __restrict__ xh, const float4* __restrict__ xl, const float4* __restrict__ vf,
                  const uint32_t* __restrict__ act, uint32_t na, float4* __restrict__ pa, float4* __restrict__ pj, uint32_t n,
                  uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    fj_mx_body<NG, true>(xh, xl, vf, act, na, pa, pj, n, j_per_chunk, eps2, zero_row);
}

}  // namespace nb
