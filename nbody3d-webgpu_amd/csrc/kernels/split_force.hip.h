// kernels/split_force.hip.h -- nb_split_force: the force+jerk pass with every pair's term sent to ONE of two sums (nb_split_pk,
// nb_split64, nb_split_reduce).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
//   member(k, j)  <=>  d2 < h_k^2,   d2 = fma(dz, dz, fma(dy, dy, dx dx)),  dx = x_j - p_x ...      (nb_neighbors' expression and rule)
//   a_irr_k = sum_{members} G m_j dr / rho^3          a_reg_k = sum_{all other rows} G m_j dr / rho^3          rho^2 = d2 + eps2
//   j_irr_k, j_reg_k likewise over G m_j [dv / rho^3 - 3 (dr.dv) dr / rho^5]
//
// The regular / irregular split of an Ahmad-Cohen scheme (Nitadori & Aarseth 2012: one comparison per pair in the regular-force
// kernel decides which set of accumulators takes the pair's term).  Nothing is ever subtracted: the weight of a pair is s3 in the
// sum it belongs to and 0 in the other, so the small sum does not inherit the rounding error of the large one.
//   The launch is nb_fj_pk's: grid = (point blocks) x (j-chunks of whole 256-row tiles), positions and velocities arrive by
// LDS-DMA, double buffered, rows past the range come from zero_row (zero mass: both weights 0, exact 0 in whichever sum the row
// lands), lanes past m clamp and store nothing.  Workgroup (bx, c) stores up to four rows per point -- (a_irr, a_reg, j_irr, j_reg)
// [c][k], planes of `m` rows -- and nb_split_reduce adds a point's chunks in ascending order in fp64, multiplies by G ONCE and
// writes the outputs that were asked for.  Fixed order, no atomics.
//   rho^2 = d2 + eps2 is one rounding more than fj_pk_body's fused chain (the comparison needs the plain d2): the two sums of a
// point do not add up to nb_fj_pk's bits.
#pragma once

namespace nb {

#ifndef NB_SPLIT_NG
#define NB_SPLIT_NG 2                                     // packed groups per lane (A/B builds: -DNB_SPLIT_NG=1; profiles/r15/split_force.md §4)
#endif
constexpr int kSplitNG = NB_SPLIT_NG;                     // 4 points per lane
constexpr uint32_t kSplitRows = kBlock * 2 * kSplitNG;    // points of one f32 workgroup (1,024)
constexpr uint32_t kSplitRows64 = kBlock;                 // points of one f64 workgroup
#ifndef NB_SPLIT_WAVES
#define NB_SPLIT_WAVES 2                                  // waves per SIMD nb_split_pk is compiled for (A/B builds: -DNB_SPLIT_WAVES=k)
#endif

// f32.  fj_pk_body's loop with the points as the i-side and, per two pairs, on top of its sequence:
//   d2 = dx dx (v_pk_mul instead of the first v_pk_fma), rho^2 = d2 + eps2 (1 v_pk_add), 2 v_cmp_lt_f32 (gfx950 has no packed
//   compare), 2 + 2 v_cndmask_b32 (w_irr = member ? s3 : 0, w_reg = member ? 0 : s3), and a second set of 3 (+ 3) v_pk_fma.
// The select is a v_cndmask and not a multiply by a 0 / 1 mask: the mask would cost the same compare plus a v_cndmask to make it,
// and then a packed multiply per weight; selecting the weight itself is the shorter sequence and keeps a NaN or inf of the other
// side out of the sum by construction.
//   Registers: NG = 2 (four points per lane, nb_fj_pk's shape: two tile rows per stage against two groups, four chains) holds 14
// packed point values, 2 x 2 x 6 packed sums per group (96 VGPRs with the jerk) and the chains in 221 VGPRs -- no scratch at two
// waves per SIMD.  NG = 1 (234 VGPRs: four tile rows per stage, twice the LDS reads per pair) measured 1.6 % slower; NG = 4 would
// hold 192 VGPRs of sums alone.  profiles/r15/split_force.md has the build's resource report and the A/B.
//   With JERK = false no velocity tile is staged and none of the jerk arithmetic is issued.
template <int NG, bool JERK>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_SPLIT_WAVES, NB_SPLIT_WAVES)))
void nb_split_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ points,
                 const float4* __restrict__ point_vel, const float* __restrict__ radii, float4* __restrict__ part,
                 uint32_t n, uint32_t m, uint32_t j_per_chunk, float eps2, float radius, const float4* __restrict__ zero_row)
{
    static_assert(kBlock * 2 * NG == kSplitRows, "the engine sizes the grid by kSplitRows");
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4 / NG;            // j-bodies per stage: JB * NG = 4 independent chains
    constexpr int NC = JB * NG;
    constexpr int NT = JERK ? 2 : 1;      // tiles per stage: positions (, velocities)
    __shared__ float4 tile[2][NT][TILE];  // [buffer][0 = positions, 1 = velocities][row]
    const int tid = threadIdx.x;
    const uint32_t i0 = blockIdx.x * kSplitRows;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG], ui[NG], vi[NG], wi[NG], h2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const uint32_t c0 = il0 < m ? il0 : m - 1, c1 = il1 < m ? il1 : m - 1;        // clamped, branch-free (never stored)
        const float4 b0 = ld4(points + c0), b1 = ld4(points + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        if constexpr (JERK) {
            const float4 v0 = ld4(point_vel + c0), v1 = ld4(point_vel + c1);
            ui[g] = nb_f2{v0.x, v1.x}; vi[g] = nb_f2{v0.y, v1.y}; wi[g] = nb_f2{v0.z, v1.z};
        }
        const float r0 = radii ? radii[c0] : radius, r1 = radii ? radii[c1] : radius;
        h2[g] = nb_f2{r0 * r0, r1 * r1};
    }
    const nb_f2 zero = nb_f2{0, 0};
    // [0] = irregular (members), [1] = regular (every other row); lower case: first level, upper case: second level
    nb_f2 ax[2][NG], ay[2][NG], az[2][NG], jx[2][NG], jy[2][NG], jz[2][NG];
    nb_f2 AX[2][NG], AY[2][NG], AZ[2][NG], JX[2][NG], JY[2][NG], JZ[2][NG];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            ax[k][g] = ay[k][g] = az[k][g] = jx[k][g] = jy[k][g] = jz[k][g] = zero;
            AX[k][g] = AY[k][g] = AZ[k][g] = JX[k][g] = JY[k][g] = JZ[k][g] = zero;
        }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as fj_pk_body::stage
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst_p = lds_wave + (uint32_t)(buf * NT * TILE) * 16u, dst_v = dst_p + (uint32_t)TILE * 16u;
        unsigned keep;
        if (jt + TILE <= j1) {
            const float4* bp = pos + jt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bp), "s"(dst_p) : "memory");
            if constexpr (JERK) {
                const float4* bv = vel + jt;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(lane_off), "s"(bv), "s"(dst_v) : "memory");
            }
        } else {
            const uint32_t j = jt + tid;
            const float4* sp = j < j1 ? pos + j : zero_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sp), "s"(dst_p) : "memory");
            if constexpr (JERK) {
                const float4* sv = j < j1 ? vel + j : zero_row;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(sv), "s"(dst_v) : "memory");
            }
        }
    };

    // one stage: JB tile rows (positions p, velocities q) against the lane's NG packed groups, stage-major over the NC chains
    auto math = [&](const float4* p, const float4* q) {
        nb_f2 bx[JB], by[JB], bz[JB], bu[JB], bv[JB], bw[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            if constexpr (JERK) { const float4 c = q[u]; bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z}; }
        }
        nb_f2 dx[NC], dy[NC], dz[NC], du[NC], dv[NC], dw[NC], d2[NC], r2[NC], y[NC], s[NC], rv[NC], si[NC], sr[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) dx[c] = bx[c / NG] - xi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dy[c] = by[c / NG] - yi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) dz[c] = bz[c / NG] - zi[c % NG];
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = dx[c] * dx[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) r2[c] = d2[c] + e2;
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = nb_f2{nb_rsq(r2[c].x), nb_rsq(r2[c].y)};
        if constexpr (JERK) {
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
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = nb_f2{bm[c / NG], bm[c / NG]} * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = s[c] * y[c];                   // m / rho^3
        // the one comparison per pair: the weight goes to exactly one of the two sums
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const bool in0 = d2[c].x < h2[c % NG].x, in1 = d2[c].y < h2[c % NG].y;
            si[c] = nb_f2{in0 ? s[c].x : 0.0f, in1 ? s[c].y : 0.0f};
            sr[c] = nb_f2{in0 ? 0.0f : s[c].x, in1 ? 0.0f : s[c].y};
        }
        if constexpr (JERK) {
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
            for (int c = 0; c < NC; ++c) jx[0][c % NG] = __builtin_elementwise_fma(si[c], du[c], jx[0][c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jy[0][c % NG] = __builtin_elementwise_fma(si[c], dv[c], jy[0][c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jz[0][c % NG] = __builtin_elementwise_fma(si[c], dw[c], jz[0][c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jx[1][c % NG] = __builtin_elementwise_fma(sr[c], du[c], jx[1][c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jy[1][c % NG] = __builtin_elementwise_fma(sr[c], dv[c], jy[1][c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) jz[1][c % NG] = __builtin_elementwise_fma(sr[c], dw[c], jz[1][c % NG]);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) ax[0][c % NG] = __builtin_elementwise_fma(si[c], dx[c], ax[0][c % NG]);
#pragma unroll
        for (int c = 0; c < NC; ++c) ay[0][c % NG] = __builtin_elementwise_fma(si[c], dy[c], ay[0][c % NG]);
#pragma unroll
        for (int c = 0; c < NC; ++c) az[0][c % NG] = __builtin_elementwise_fma(si[c], dz[c], az[0][c % NG]);
#pragma unroll
        for (int c = 0; c < NC; ++c) ax[1][c % NG] = __builtin_elementwise_fma(sr[c], dx[c], ax[1][c % NG]);
#pragma unroll
        for (int c = 0; c < NC; ++c) ay[1][c % NG] = __builtin_elementwise_fma(sr[c], dy[c], ay[1][c % NG]);
#pragma unroll
        for (int c = 0; c < NC; ++c) az[1][c % NG] = __builtin_elementwise_fma(sr[c], dz[c], az[1][c % NG]);
    };
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                AX[k][g] = AX[k][g] + ax[k][g]; AY[k][g] = AY[k][g] + ay[k][g]; AZ[k][g] = AZ[k][g] + az[k][g];
                ax[k][g] = ay[k][g] = az[k][g] = zero;
                if constexpr (JERK) {
                    JX[k][g] = JX[k][g] + jx[k][g]; JY[k][g] = JY[k][g] + jy[k][g]; JZ[k][g] = JZ[k][g] + jz[k][g];
                    jx[k][g] = jy[k][g] = jz[k][g] = zero;
                }
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
            for (int uu = 0; uu < U / JB; ++uu) math(&tile[cur][0][ch * U + uu * JB], &tile[cur][NT - 1][ch * U + uu * JB]);
        }
        if ((t & (kFjFlush - 1)) == kFjFlush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    // planes of m rows: [chunk][0 = a_irr, 1 = a_reg, 2 = j_irr, 3 = j_reg][point] (two planes without the jerk)
    constexpr uint32_t NP = JERK ? 4 : 2;
    float4* o = part + (size_t)blockIdx.y * NP * m;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = i0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (il0 < m) {
                o[(size_t)k * m + il0] = float4{AX[k][g].x, AY[k][g].x, AZ[k][g].x, 0.0f};
                if constexpr (JERK) o[(size_t)(2 + k) * m + il0] = float4{JX[k][g].x, JY[k][g].x, JZ[k][g].x, 0.0f};
            }
            if (il1 < m) {
                o[(size_t)k * m + il1] = float4{AX[k][g].y, AY[k][g].y, AZ[k][g].y, 0.0f};
                if constexpr (JERK) o[(size_t)(2 + k) * m + il1] = float4{JX[k][g].y, JY[k][g].y, JZ[k][g].y, 0.0f};
            }
        }
    }
}

// fp64 handles (T = double).  fj64_body's shape with the same split: one point per lane, the j-tiles staged through registers,
// v_rsq_f64 seed + one correction, every difference, product and sum in fp64.  The same plane layout as nb_split_pk.
template <typename T, bool JERK>
__global__ __launch_bounds__(kBlock) void nb_split64(const typename vec4<T>::type* __restrict__ pos,
                                                    const typename vec4<T>::type* __restrict__ vel,
                                                    const typename vec4<T>::type* __restrict__ points,
                                                    const typename vec4<T>::type* __restrict__ point_vel,
                                                    const T* __restrict__ radii, double4* __restrict__ part, uint32_t n, uint32_t m,
                                                    uint32_t j_per_chunk, double eps2, double radius)
{
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[JERK ? kTile : 1];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kSplitRows64 + tid;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const uint32_t ic = il < m ? il : m - 1;
    const auto bi = ld4(points + ic);
    const double xi = (double)bi.x, yi = (double)bi.y, zi = (double)bi.z;
    double ui = 0.0, vi = 0.0, wz = 0.0;
    if constexpr (JERK) { const auto w = ld4(point_vel + ic); ui = (double)w.x; vi = (double)w.y; wz = (double)w.z; }
    const double h = radii ? (double)radii[ic] : radius;
    const double h2 = h * h;
    double ax[2] = {0.0, 0.0}, ay[2] = {0.0, 0.0}, az[2] = {0.0, 0.0}, jx[2] = {0.0, 0.0}, jy[2] = {0.0, 0.0}, jz[2] = {0.0, 0.0};
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const auto b = ld4(pos + j);
            tp[tid] = double4{(double)b.x, (double)b.y, (double)b.z, (double)b.w};
            if constexpr (JERK) { const auto c = ld4(vel + j); tv[tid] = double4{(double)c.x, (double)c.y, (double)c.z, 0.0}; }
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            if constexpr (JERK) tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 2
        for (int jj = 0; jj < cnt; ++jj) {
            const double4 b = tp[jj];
            const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
            const double d2 = nb_fma(dz, dz, nb_fma(dy, dy, dx * dx));
            const double r2 = d2 + eps2;
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double y2 = y * y;
            const double s3 = (b.w * y) * y2;
            const bool in = d2 < h2;
            const double si = in ? s3 : 0.0, sr = in ? 0.0 : s3;
            if constexpr (JERK) {
                const double4 c = tv[jj];
                const double du = c.x - ui, dv = c.y - vi, dw = c.z - wz;
                const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
                const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
                jx[0] = nb_fma(si, tx, jx[0]); jy[0] = nb_fma(si, ty, jy[0]); jz[0] = nb_fma(si, tz, jz[0]);
                jx[1] = nb_fma(sr, tx, jx[1]); jy[1] = nb_fma(sr, ty, jy[1]); jz[1] = nb_fma(sr, tz, jz[1]);
            }
            ax[0] = nb_fma(si, dx, ax[0]); ay[0] = nb_fma(si, dy, ay[0]); az[0] = nb_fma(si, dz, az[0]);
            ax[1] = nb_fma(sr, dx, ax[1]); ay[1] = nb_fma(sr, dy, ay[1]); az[1] = nb_fma(sr, dz, az[1]);
        }
    }
    if (il < m) {
        constexpr uint32_t NP = JERK ? 4 : 2;
        double4* o = part + (size_t)blockIdx.y * NP * m;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            o[(size_t)k * m + il] = double4{ax[k], ay[k], az[k], 0.0};
            if constexpr (JERK) o[(size_t)(2 + k) * m + il] = double4{jx[k], jy[k], jz[k], 0.0};
        }
    }
}

// Adds a point's chunk rows in ascending chunk order in fp64, multiplies by G once and writes the outputs that were asked for
// (out[p] == nullptr: plane p is not wanted; planes >= `planes` do not exist).  TP = element type of the partial rows, T = the handle's.
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_split_reduce(const typename vec4<TP>::type* __restrict__ part, uint32_t m, uint32_t chunks,
                                                         uint32_t planes, double G, typename vec4<T>::type* __restrict__ o0,
                                                         typename vec4<T>::type* __restrict__ o1, typename vec4<T>::type* __restrict__ o2,
                                                         typename vec4<T>::type* __restrict__ o3)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= m) return;
    V4* const out[4] = {o0, o1, o2, o3};
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {
        if (p >= planes || !out[p]) continue;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (uint32_t c = 0; c < chunks; ++c) {
            const auto a = ld4(part + ((size_t)c * planes + p) * m + il);
            sx += (double)a.x; sy += (double)a.y; sz += (double)a.z;
        }
        out[p][il] = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
    }
}

}  // namespace nb
