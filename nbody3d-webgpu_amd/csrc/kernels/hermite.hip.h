// kernels/hermite.hip.h -- the 4th-order Hermite predictor-corrector (Makino & Aarseth 1992): the force+jerk pass (nb_fj_pk, nb_fj64,
// nb_fj_reduce) and the two O(N) kernels around it (nb_hermite_predict, nb_hermite_correct).  No reference analogue.
// Part of nb_kernels.hip.h (include that, not this file).
//
//   a_i = sum_j G m_j dr / rho^3                              dr = x_j - x_i,  dv = v_j - v_i,  rho^2 = |dr|^2 + eps2
//   j_i = sum_j G m_j [ dv / rho^3 - 3 (dr.dv) dr / rho^5 ]
//
// N x N ORDERED pairs of one (positions, velocities) state.  The launch is nb_field_pk's: grid = (i-blocks) x (j-chunks of whole
// 256-row tiles), workgroup (bx, c) stores one row pair (ax, ay, az, 0), (jx, jy, jz, 0) per body into pa[c][i], pj[c][i];
// nb_fj_reduce adds a body's chunks in ascending order in fp64 and multiplies by G ONCE (both sums are linear in G: the plain
// (x, y, z, m) rows stream through LDS-DMA, the gm / pairs copies are never touched).  Fixed order, no atomics.
#pragma once

namespace nb {

constexpr int kFjNG = 2;                            // packed groups per lane: 4 bodies per lane
constexpr uint32_t kFjRows = kBlock * 2 * kFjNG;    // i-bodies of one f32 workgroup (1,024)
constexpr uint32_t kFjRows64 = kBlock;              // i-bodies of one f64 workgroup
constexpr uint32_t kFjFlush = 4;                    // tiles between two flushes of the first-level sums (1,024 terms per chain)
#ifndef NB_FJ_WAVES
#define NB_FJ_WAVES 2                               // waves per SIMD nb_fj_pk is compiled for (A/B builds: -DNB_FJ_WAVES=k; profiles/r07/hermite.md)
#endif

// f32.  The i-bodies sit in registers as packed pairs (positions and velocities), every lane of the wave reads the same two tile
// rows (position row, velocity row: LDS broadcast).  Per two pairs:
//   3 + 3 v_pk_add (dr, dv), 3 v_pk_fma (rho^2), 2 v_rsq_f32, y^2 = y y, s = m y, s3 = s y^2, 1 v_pk_mul + 2 v_pk_fma (dr.dv),
//   q = (dr.dv) y^2, q3 = -3 q, 3 v_pk_fma (t = dv + q3 dr), 3 v_pk_fma (j += s3 t), 3 v_pk_fma (a += s3 dr)
// = 26 packed + 2 transcendental = 120 issue cycles by DESIGN §4.1's accounting (the ordered-pair force loop: 64).
//   The jerk is accumulated in the form s3 (dv - 3 q dr): ONE sum per component.  Two sums (s3 dv and 3 s3 q dr) subtracted at the
// end would cancel -- in a virialised system each is far larger than their difference.
//   No self-masking: for j == i dr = dv = 0, so t = 0 and, with eps2 >= 1e-12, s3 is finite: both terms are exactly 0.  Rows past the
// range come from zero_row (zero mass: s3 = 0, both terms exactly 0).
//   Summation: as nb_field_pk -- binary32 in two levels (a register takes at most 1,024 terms, then chunk / 1,024), fp64 across
// the chunks.
//   Registers: 12 packed i-values, 2 x 6 packed sums per group, ~20 live per chain.  Four chains (two tile rows x two groups,
// issued stage-major so that no dependent instruction follows its producer) need ~160 VGPRs: the kernel runs two waves per SIMD
// (256 VGPRs each), where the second wave covers the first one's LDS waits and barriers.  profiles/r07/hermite.md.
//   The body is shared with nb_blk_fj_pk (kernels/block.hip.h): with GATHER the ni i-rows are act[0 .. ni) and the partial rows are
// compact (row k of chunk c belongs to act[k]); without it ni == n and row k is body k.  Everything between the prologue's loads
// and the epilogue's stores is the same code.
//   WATCH (nb_set_encounter_watch, kernels/encounter.hip.h; with GATHER only): wth[i] is body i's threshold w_i.  Per stage the
// compares rho^2 < w_i of its chains are ORed on the scalar unit and ONE wave-uniform branch skips the slow path, which tests the
// index (own row, rows past the chunk) and keeps the lane's smallest (rho^2, j), equal rho^2 to the smaller j.  The best pair, the
// own indices live in LDS beside the tiles (touched on the slow path only: nb_blk_fj_pk<2> stands at 228 VGPRs) and leave in the
// .w lanes of the two partial rows.  The sums are the same instructions on the same values: no bit of them moves.  Without WATCH
// none of this is compiled.
template <int NG, bool GATHER, bool WATCH = false>
__device__ __forceinline__ void fj_pk_body(const float4* __restrict__ pos, const float4* __restrict__ vel,
                                           const uint32_t* __restrict__ act, uint32_t ni, float4* __restrict__ pa,
                                           float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2,
                                           const float4* __restrict__ zero_row, const float* __restrict__ wth = nullptr)
{
    static_assert(GATHER || !WATCH, "the watch exists on the gathered pass only");
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4 / NG;            // j-bodies per stage: JB * NG = 4 independent chains
    constexpr uint32_t ROWS = kBlock * 2 * NG;
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][2][TILE];   // [buffer][0 = positions, 1 = velocities][row]
    __shared__ nb_f2 enc_r[WATCH ? NG : 1][WATCH ? kBlock : 1];      // WATCH: the lane's smallest rho^2 so far, per packed half
    __shared__ uint2 enc_j[WATCH ? NG : 1][WATCH ? kBlock : 1];      // ... its index (0xffffffff: none)
    __shared__ uint2 enc_o[WATCH ? NG : 1][WATCH ? kBlock : 1];      // ... and the lane's own bodies
    const int tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * ROWS;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG], ui[NG], vi[NG], wi[NG];
    nb_f2 wq[WATCH ? NG : 1];             // WATCH: the thresholds of the lane's bodies
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        if constexpr (GATHER) { c0 = act[c0]; c1 = act[c1]; }
        if constexpr (WATCH) {            // a clamped lane watches nothing (rho^2 < 0 never holds); a lane reads and writes its own words only: no barrier
            wq[g] = nb_f2{il0 < ni ? wth[c0] : 0.0f, il1 < ni ? wth[c1] : 0.0f};
            enc_r[g][tid] = nb_f2{__builtin_inff(), __builtin_inff()};
            enc_j[g][tid] = uint2{0xffffffffu, 0xffffffffu};
            enc_o[g][tid] = uint2{c0, c1};
        }
        const float4 b0 = ld4(pos + c0), b1 = ld4(pos + c1), v0 = ld4(vel + c0), v1 = ld4(vel + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        ui[g] = nb_f2{v0.x, v1.x}; vi[g] = nb_f2{v0.y, v1.y}; wi[g] = nb_f2{v0.z, v1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 ax[NG], ay[NG], az[NG], jx[NG], jy[NG], jz[NG], AX[NG], AY[NG], AZ[NG], JX[NG], JY[NG], JZ[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ax[g] = ay[g] = az[g] = jx[g] = jy[g] = jz[g] = zero;
        AX[g] = AY[g] = AZ[g] = JX[g] = JY[g] = JZ[g] = zero;
    }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_field_pk::stage: whole tiles from a scalar base, the last one per lane with rows past the range
    // taken from zero_row; two tiles per stage (positions, velocities)
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst_p = lds_wave + (uint32_t)(buf * 2 * TILE) * 16u, dst_v = dst_p + (uint32_t)TILE * 16u;
        unsigned keep;
        if (jt + TILE <= j1) {
            const float4 *bp = pos + jt, *bv = vel + jt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bv), "s"(dst_v) : "memory");
        } else {
            const uint32_t j = jt + tid;
            const float4* sp = j < j1 ? pos + j : zero_row;
            const float4* sv = j < j1 ? vel + j : zero_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sv), "s"(dst_v) : "memory");
        }
    };

    // one stage: JB tile rows (positions p, velocities q) against the lane's NG packed groups, stage-major over the NC chains
    // (jrow: the body index of row p[0], read by the watch only)
    auto math = [&](const float4* p, const float4* q, uint32_t jrow) {
        nb_f2 bx[JB], by[JB], bz[JB], bu[JB], bv[JB], bw[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u], c = q[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z};
        }
        nb_f2 dx[NC], dy[NC], dz[NC], du[NC], dv[NC], dw[NC], d2[NC], y[NC], s[NC], rv[NC];
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
        if constexpr (WATCH) {
            bool lt[NC][2];
            bool hit = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                lt[c][0] = d2[c].x < wq[c % NG].x; lt[c][1] = d2[c].y < wq[c % NG].y;
                hit |= lt[c][0] | lt[c][1];
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {      // wave-uniform: some lane has a pair below its threshold among these JB rows
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    nb_f2 br = enc_r[g][tid];
                    uint2 bj = enc_j[g][tid];
                    const uint2 own = enc_o[g][tid];
#pragma unroll
                    for (int u = 0; u < JB; ++u) {             // c = u * NG + g: a row meets its pairs in ascending j
                        const uint32_t j = jrow + (uint32_t)u;
                        const nb_f2 r = d2[u * NG + g];
                        const bool in = j < j1;                // a row past the chunk is padding (zero_row sits at the origin)
                        // (bitwise, then selects: no branch per lane inside the slow path)
                        const bool t0 = lt[u * NG + g][0] & in & (j != own.x) & ((r.x < br.x) | ((r.x == br.x) & (j < bj.x)));
                        const bool t1 = lt[u * NG + g][1] & in & (j != own.y) & ((r.y < br.y) | ((r.y == br.y) & (j < bj.y)));
                        br.x = t0 ? r.x : br.x; bj.x = t0 ? j : bj.x;
                        br.y = t1 ? r.y : br.y; bj.y = t1 ? j : bj.y;
                    }
                    enc_r[g][tid] = br;
                    enc_j[g][tid] = bj;
                }
            }
        }
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
                math(&tile[cur][0][ch * U + uu * JB], &tile[cur][1][ch * U + uu * JB], j0 + t * TILE + (uint32_t)(ch * U + uu * JB));
        }
        if ((t & (kFjFlush - 1)) == kFjFlush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    float4* oa = pa + (size_t)blockIdx.y * ni;
    float4* oj = pj + (size_t)blockIdx.y * ni;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        float r0 = 0.0f, r1 = 0.0f, k0 = 0.0f, k1 = 0.0f;      // WATCH: the chunk's answer, rho^2 and the index bit-cast
        if constexpr (WATCH) {
            const nb_f2 br = enc_r[g][tid];
            const uint2 bj = enc_j[g][tid];
            r0 = br.x; r1 = br.y; k0 = __uint_as_float(bj.x); k1 = __uint_as_float(bj.y);
        }
        if (il0 < ni) { oa[il0] = float4{AX[g].x, AY[g].x, AZ[g].x, r0}; oj[il0] = float4{JX[g].x, JY[g].x, JZ[g].x, k0}; }
        if (il1 < ni) { oa[il1] = float4{AX[g].y, AY[g].y, AZ[g].y, r1}; oj[il1] = float4{JX[g].y, JY[g].y, JZ[g].y, k1}; }
    }
}

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_FJ_WAVES, NB_FJ_WAVES)))
void nb_fj_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, float4* __restrict__ pa, float4* __restrict__ pj,
              uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    static_assert(kBlock * 2 * NG == kFjRows, "the engine sizes the grid by kFjRows");
    fj_pk_body<NG, false>(pos, vel, nullptr, n, pa, pj, n, j_per_chunk, eps2, zero_row);
}

// fp64 handles (T = double).  One body per lane, the two j-tiles staged through registers; v_rsq_f64 seed + one correction as in
// nb_field64 (y0 (1 + e/2), e = 1 - rho^2 y0^2: relative error ~ 3 e^2 / 8 < 1e-16); every difference, product and sum is fp64.
// fj64_body<T, GATHER>: shared with nb_blk_fj64, as fj_pk_body above.  WATCH: as there, one compare per pair, the lane masks tested
// on the scalar unit; the lane's best pair stays in registers and leaves in the .w lanes (the index as an exact double).  The loop
// ends at the chunk's last row: a zero row of the tile is never met.
template <typename T, bool GATHER, bool WATCH = false>
__device__ __forceinline__ void fj64_body(const typename vec4<T>::type* __restrict__ pos,
                                          const typename vec4<T>::type* __restrict__ vel, const uint32_t* __restrict__ act,
                                          uint32_t ni, double4* __restrict__ pa, double4* __restrict__ pj, uint32_t n,
                                          uint32_t j_per_chunk, double eps2, const T* __restrict__ wth = nullptr)
{
    static_assert(GATHER || !WATCH, "the watch exists on the gathered pass only");
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kFjRows64 + tid;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    uint32_t ic = il < ni ? il : ni - 1;
    if constexpr (GATHER) ic = act[ic];
    const auto bi = ld4(pos + ic);
    const auto wi = ld4(vel + ic);
    const double xi = (double)bi.x, yi = (double)bi.y, zi = (double)bi.z;
    const double ui = (double)wi.x, vi = (double)wi.y, wz = (double)wi.z;
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    double wq = 0.0, br = __builtin_inf();      // WATCH: the lane's threshold (a clamped lane watches nothing), its smallest rho^2 so far ...
    uint32_t bj = 0xffffffffu;                  // ... and that pair's index (0xffffffff: none)
    if constexpr (WATCH) wq = il < ni ? (double)wth[ic] : 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const auto b = ld4(pos + j);
            const auto c = ld4(vel + j);
            tp[tid] = double4{(double)b.x, (double)b.y, (double)b.z, (double)b.w};
            tv[tid] = double4{(double)c.x, (double)c.y, (double)c.z, 0.0};
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 2
        for (int jj = 0; jj < cnt; ++jj) {
            const double4 b = tp[jj];
            const double4 c = tv[jj];
            const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
            const double du = c.x - ui, dv = c.y - vi, dw = c.z - wz;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            if constexpr (WATCH) {
                const bool lt = r2 < wq;
                if (__builtin_amdgcn_ballot_w64(lt) != 0) {      // wave-uniform: some lane has this row below its threshold
                    const uint32_t jb = jt + (uint32_t)jj;
                    if (lt && jb != ic && (r2 < br || (r2 == br && jb < bj))) { br = r2; bj = jb; }
                }
            }
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double y2 = y * y;
            const double s3 = (b.w * y) * y2;
            const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
            const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
            jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
            ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
        }
    }
    if (il < ni) {
        pa[(size_t)blockIdx.y * ni + il] = double4{ax, ay, az, WATCH ? br : 0.0};
        pj[(size_t)blockIdx.y * ni + il] = double4{jx, jy, jz, WATCH ? (double)bj : 0.0};
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nb_fj64(const typename vec4<T>::type* __restrict__ pos,
                                                 const typename vec4<T>::type* __restrict__ vel, double4* __restrict__ pa,
                                                 double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, double eps2)
{
    fj64_body<T, false>(pos, vel, nullptr, n, pa, pj, n, j_per_chunk, eps2);
}

// Adds a body's chunk rows in ascending chunk order in fp64, multiplies by G once and writes the two derivative rows
// (ax, ay, az, 0), (jx, jy, jz, 0).  TP = element type of the partial rows, T = the handle's.
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_fj_reduce(const typename vec4<TP>::type* __restrict__ pa,
                                                      const typename vec4<TP>::type* __restrict__ pj, uint32_t n, uint32_t chunks,
                                                      double G, typename vec4<T>::type* __restrict__ acc,
                                                      typename vec4<T>::type* __restrict__ jerk)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const auto a = ld4(pa + (size_t)c * n + il);
        const auto j = ld4(pj + (size_t)c * n + il);
        sx += (double)a.x; sy += (double)a.y; sz += (double)a.z;
        tx += (double)j.x; ty += (double)j.y; tz += (double)j.z;
    }
    acc[il] = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
    jerk[il] = V4{(T)(G * tx), (T)(G * ty), (T)(G * tz), (T)0};
}

// Predictor: xp = x + h v + h^2/2 a + h^3/6 j, vp = v + h a + h^2/2 j.  The mass lane and vel.w are carried unchanged.  The
// polynomial is evaluated in fp64 (Horner, fused) and rounded once to the handle's precision.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_hermite_predict(const typename vec4<T>::type* __restrict__ x,
                                                            const typename vec4<T>::type* __restrict__ v,
                                                            const typename vec4<T>::type* __restrict__ a,
                                                            const typename vec4<T>::type* __restrict__ j,
                                                            typename vec4<T>::type* __restrict__ xp,
                                                            typename vec4<T>::type* __restrict__ vp, uint32_t n, double h)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il);
    const double h2 = h * (1.0 / 2.0), h3 = h * (1.0 / 3.0);
    auto px = [&](double x0, double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, nb_fma(h3, j0, a0), v0), x0); };
    auto pv = [&](double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, j0, a0), v0); };
    xp[il] = V4{(T)px(X.x, V.x, A.x, J.x), (T)px(X.y, V.y, A.y, J.y), (T)px(X.z, V.z, A.z, J.z), X.w};
    vp[il] = V4{(T)pv(V.x, A.x, J.x), (T)pv(V.y, A.y, J.y), (T)pv(V.z, A.z, J.z), V.w};
}

// Corrector: (a1, j1) are the derivatives at the predicted state;
//   v1 = v + h/2 (a + a1) + h^2/12 (j - j1)        x1 = x + h/2 (v + v1) + h^2/12 (a - a1)
// in fp64, rounded once; the state becomes (x1, v1, a1, j1) in place (a lane reads and writes its own rows only).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_hermite_correct(typename vec4<T>::type* __restrict__ x,
                                                            typename vec4<T>::type* __restrict__ v,
                                                            typename vec4<T>::type* __restrict__ a,
                                                            typename vec4<T>::type* __restrict__ j,
                                                            const typename vec4<T>::type* __restrict__ a1,
                                                            const typename vec4<T>::type* __restrict__ j1, uint32_t n, double h)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il), A1 = ld4(a1 + il), J1 = ld4(j1 + il);
    const double hh = 0.5 * h, h12 = h * h * (1.0 / 12.0);
    auto cv = [&](double v0, double a0, double an, double j0, double jn) { return nb_fma(h12, j0 - jn, nb_fma(hh, a0 + an, v0)); };
    const double vx = cv(V.x, A.x, A1.x, J.x, J1.x), vy = cv(V.y, A.y, A1.y, J.y, J1.y), vz = cv(V.z, A.z, A1.z, J.z, J1.z);
    auto cx = [&](double x0, double v0, double vn, double a0, double an) { return nb_fma(h12, a0 - an, nb_fma(hh, v0 + vn, x0)); };
    x[il] = V4{(T)cx(X.x, V.x, vx, A.x, A1.x), (T)cx(X.y, V.y, vy, A.y, A1.y), (T)cx(X.z, V.z, vz, A.z, A1.z), X.w};
    v[il] = V4{(T)vx, (T)vy, (T)vz, V.w};
    a[il] = V4{A1.x, A1.y, A1.z, (T)0};
    j[il] = V4{J1.x, J1.y, J1.z, (T)0};
}

}  // namespace nb
