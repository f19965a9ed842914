// kernels/block_batch6.hip.h -- block steps sized on the device, many per host wait, on order-6 handles (nb_set_block_batch6; handles
// with nb_set_block_steps6).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// The slot of kernels/block_batch.hip.h with the order-6 state (x, v, a, j, s, c) per body: the scheduler nb_blkq_sched, the batch
// words kBb* and the modes are that file's, unchanged and in the same instantiation.
//   nb_blkq_sched      as for order 4: the schedule and the slot's decision
//   nb_blkq6_predict   nb_blk6_predict (small and parked slots)
//   nb_blkq6_fjs_pk/64 force, jerk and snap of the |A| <= small_max listed rows against all n predicted rows (small slots)
//   nb_blkq6_correct   nb_blk6_correct with |A| and t_next from the device header (small slots)
// As there, nothing adds floating-point numbers in an order that depends on timing, and what a small step computes for a body
// depends on the predicted arrays and on n alone: a list row is one lane's chain over the rows of a j-chunk in four fixed quarters,
// the quarters are added in wave order and the chunks in an order the chunk count fixes (the host's bb_shape: n and the CU count).
// A count the kernels read is clamped: above small_max it is a park, never a grid or an index.
#pragma once

namespace nb {

// nb_blk6_predict for a slot that is not idle.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blkq6_predict(const typename vec4<T>::type* __restrict__ x,
                                                          const typename vec4<T>::type* __restrict__ v,
                                                          const typename vec4<T>::type* __restrict__ a,
                                                          const typename vec4<T>::type* __restrict__ j,
                                                          const typename vec4<T>::type* __restrict__ s,
                                                          const typename vec4<T>::type* __restrict__ c,
                                                          const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                          typename vec4<T>::type* __restrict__ xp,
                                                          typename vec4<T>::type* __restrict__ vp,
                                                          typename vec4<T>::type* __restrict__ ap, uint32_t n,
                                                          const uint32_t* __restrict__ hdr, uint32_t L, double tick,
                                                          const uint32_t* __restrict__ bb)
{
    using V4 = typename vec4<T>::type;
    if (bb[kBbMode] == kBbModeIdle) return;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const uint32_t t_next = hdr[kBlkNext];
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il), S = ld4(s + il), K = ld4(c + il);
    const uint32_t t_i = due[il] - (1u << (L - lev[il]));
    const double h = (double)(t_next - t_i) * tick;
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

// f32: the small force+jerk+snap pass.  nb_blkq_fj_pk's shape -- grid (ceil(small_max / 128), j-chunks), the four waves of a
// workgroup hold the SAME 128 list slots (one packed pair per lane), wave w sweeps rows [64 w, 64 w + 64) of each tile -- with
// h6_fjs_pk_body's three LDS-DMA tile streams (predicted positions, velocities, accelerations) and its instruction sequence per
// pair (NG = 1: nine packed sums, flushed into second-level registers every 1,024 terms per chain).  The four waves' binary32 sums
// meet in LDS and are added in wave order; one compact partial row per (j-chunk, list slot) at pa / pj / ps[c * small_max + k].
// Lanes past |A| clamp and store nothing; a workgroup whose first slot is past |A| leaves after the header loads.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_blkq6_fjs_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ acc,
                     const uint32_t* __restrict__ act, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb,
                     uint32_t small_max, float4* __restrict__ pa, float4* __restrict__ pj, float4* __restrict__ ps, uint32_t n,
                     uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    static_assert(NG == 1, "one packed pair per lane");
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4;                 // j-bodies per stage: four independent chains
    __shared__ float4 tile[2][3][TILE];   // [buffer][0 = positions, 1 = velocities, 2 = accelerations][row]
    __shared__ float red[4][9][kBbRows];  // [wave][a (0..2), j (3..5), s (6..8)][slot]
    const uint32_t i0 = blockIdx.x * kBbRows;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t ni = hdr[kBlkCount];
    if (ni == 0 || ni > small_max || ni > n || i0 >= ni) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi, yi, zi, ui, vi, wi, fi, gi, hi;
    {
        const uint32_t il0 = i0 + lane, il1 = il0 + 64;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        c0 = act[c0]; c1 = act[c1];
        c0 = c0 < n ? c0 : n - 1; c1 = c1 < n ? c1 : n - 1;
        const float4 b0 = ld4(pos + c0), b1 = ld4(pos + c1), v0 = ld4(vel + c0), v1 = ld4(vel + c1);
        const float4 a0 = ld4(acc + c0), a1 = ld4(acc + c1);
        xi = nb_f2{b0.x, b1.x}; yi = nb_f2{b0.y, b1.y}; zi = nb_f2{b0.z, b1.z};
        ui = nb_f2{v0.x, v1.x}; vi = nb_f2{v0.y, v1.y}; wi = nb_f2{v0.z, v1.z};
        fi = nb_f2{a0.x, a1.x}; gi = nb_f2{a0.y, a1.y}; hi = nb_f2{a0.z, a1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 sm[9], SM[9];                   // first- and second-level sums: a (0..2), j (3..5), s (6..8)
#pragma unroll
    for (int k = 0; k < 9; ++k) sm[k] = SM[k] = zero;
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const nb_f2 p2 = nb_f2{2.0f, 2.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as h6_fjs_pk_body::stage: three tiles per stage
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

    // one stage: JB tile rows (positions p, velocities q, accelerations r) against the lane's packed pair, stage-major over the JB
    // chains (h6_fjs_pk_body::math with NG = 1)
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
        nb_f2 dx[JB], dy[JB], dz[JB], du[JB], dv[JB], dw[JB], df[JB], dg[JB], dh[JB], d2[JB], y[JB], s[JB], rv[JB], vv[JB], q6[JB];
#pragma unroll
        for (int c = 0; c < JB; ++c) dx[c] = bx[c] - xi;
#pragma unroll
        for (int c = 0; c < JB; ++c) dy[c] = by[c] - yi;
#pragma unroll
        for (int c = 0; c < JB; ++c) dz[c] = bz[c] - zi;
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dx[c], dx[c], e2);
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dy[c], dy[c], d2[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = __builtin_elementwise_fma(dz[c], dz[c], d2[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) y[c] = nb_f2{nb_rsq(d2[c].x), nb_rsq(d2[c].y)};
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
        for (int c = 0; c < JB; ++c) df[c] = bf[c] - fi;
#pragma unroll
        for (int c = 0; c < JB; ++c) dg[c] = bg[c] - gi;
#pragma unroll
        for (int c = 0; c < JB; ++c) dh[c] = bh[c] - hi;
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = du[c] * du[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(dv[c], dv[c], vv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(dw[c], dw[c], vv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(dx[c], df[c], vv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(dy[c], dg[c], vv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(dz[c], dh[c], vv[c]);      // dv.dv + dr.da
#pragma unroll
        for (int c = 0; c < JB; ++c) s[c] = nb_f2{bm[c], bm[c]} * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * y[c];                 // alpha
#pragma unroll
        for (int c = 0; c < JB; ++c) d2[c] = rv[c] * rv[c];                // alpha^2
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = __builtin_elementwise_fma(vv[c], y[c], d2[c]);       // beta
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * m3;                   // -3 alpha
#pragma unroll
        for (int c = 0; c < JB; ++c) q6[c] = rv[c] * p2;                   // -6 alpha
#pragma unroll
        for (int c = 0; c < JB; ++c) vv[c] = vv[c] * m3;                   // -3 beta
#pragma unroll
        for (int c = 0; c < JB; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 alpha dr
#pragma unroll
        for (int c = 0; c < JB; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) df[c] = __builtin_elementwise_fma(q6[c], du[c], df[c]);      // u = da - 6 alpha t - 3 beta dr
#pragma unroll
        for (int c = 0; c < JB; ++c) dg[c] = __builtin_elementwise_fma(q6[c], dv[c], dg[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dh[c] = __builtin_elementwise_fma(q6[c], dw[c], dh[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) df[c] = __builtin_elementwise_fma(vv[c], dx[c], df[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dg[c] = __builtin_elementwise_fma(vv[c], dy[c], dg[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dh[c] = __builtin_elementwise_fma(vv[c], dz[c], dh[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[6] = __builtin_elementwise_fma(s[c], df[c], sm[6]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[7] = __builtin_elementwise_fma(s[c], dg[c], sm[7]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[8] = __builtin_elementwise_fma(s[c], dh[c], sm[8]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[3] = __builtin_elementwise_fma(s[c], du[c], sm[3]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[4] = __builtin_elementwise_fma(s[c], dv[c], sm[4]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[5] = __builtin_elementwise_fma(s[c], dw[c], sm[5]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[0] = __builtin_elementwise_fma(s[c], dx[c], sm[0]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[1] = __builtin_elementwise_fma(s[c], dy[c], sm[1]);
#pragma unroll
        for (int c = 0; c < JB; ++c) sm[2] = __builtin_elementwise_fma(s[c], dz[c], sm[2]);
    };
    auto flush = [&]() {
#pragma unroll
        for (int k = 0; k < 9; ++k) { SM[k] = SM[k] + sm[k]; sm[k] = zero; }
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
        const int lo = 64 * wave, hi_ = lo + 64 < cntu ? lo + 64 : cntu;      // the wave's quarter of the tile
        for (int r = lo; r < hi_; r += U) {
            math(&tile[cur][0][r], &tile[cur][1][r], &tile[cur][2][r]);
            math(&tile[cur][0][r + JB], &tile[cur][1][r + JB], &tile[cur][2][r + JB]);
        }
        if ((t & 15u) == 15u) flush();                    // 1,024 terms per chain: a wave adds 64 rows of a tile
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

#pragma unroll
    for (int c = 0; c < 9; ++c) { red[wave][c][lane] = SM[c].x; red[wave][c][lane + 64] = SM[c].y; }
    __syncthreads();
    const uint32_t k = i0 + (uint32_t)tid;
    if (tid < (int)kBbRows && k < ni) {
        float r[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) r[c] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
        pa[(size_t)blockIdx.y * small_max + k] = float4{r[0], r[1], r[2], 0.0f};
        pj[(size_t)blockIdx.y * small_max + k] = float4{r[3], r[4], r[5], 0.0f};
        ps[(size_t)blockIdx.y * small_max + k] = float4{r[6], r[7], r[8], 0.0f};
    }
}

// f64: the same shape on h6_fjs64_body's arithmetic (v_rsq_f64 seed + one correction, everything in fp64).  Grid
// (ceil(small_max / 64), j-chunks); the four waves hold the same 64 list slots, one body per lane, wave w sweeps rows
// [64 w, 64 w + 64) of each of the three tiles.
template <typename T>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_blkq6_fjs64(const typename vec4<T>::type* __restrict__ pos, const typename vec4<T>::type* __restrict__ vel,
                    const typename vec4<T>::type* __restrict__ acc, const uint32_t* __restrict__ act,
                    const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb, uint32_t small_max,
                    double4* __restrict__ pa, double4* __restrict__ pj, double4* __restrict__ ps, uint32_t n, uint32_t j_per_chunk,
                    double eps2)
{
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[kTile];
    __shared__ double4 ta[kTile];
    __shared__ double red[4][9][kBbRows64];
    const uint32_t i0 = blockIdx.x * kBbRows64;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t ni = hdr[kBlkCount];
    if (ni == 0 || ni > small_max || ni > n || i0 >= ni) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t il = i0 + lane;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    uint32_t ic = il < ni ? il : ni - 1;
    ic = act[ic];
    ic = ic < n ? ic : n - 1;
    const auto bi = ld4(pos + ic);
    const auto wi = ld4(vel + ic);
    const auto ci = ld4(acc + ic);
    const double xi = (double)bi.x, yi = (double)bi.y, zi = (double)bi.z;
    const double ui = (double)wi.x, vi = (double)wi.y, wz = (double)wi.z;
    const double fi = (double)ci.x, gi = (double)ci.y, hi = (double)ci.z;
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const auto b = ld4(pos + j);
            const auto c = ld4(vel + j);
            const auto d = ld4(acc + j);
            tp[tid] = double4{(double)b.x, (double)b.y, (double)b.z, (double)b.w};
            tv[tid] = double4{(double)c.x, (double)c.y, (double)c.z, 0.0};
            ta[tid] = double4{(double)d.x, (double)d.y, (double)d.z, 0.0};
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
            ta[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
        const int lo = 64 * wave, hi_ = lo + 64 < cnt ? lo + 64 : cnt;      // the wave's quarter of the tile
#pragma unroll 2
        for (int jj = lo; jj < hi_; ++jj) {
            const double4 b = tp[jj], c = tv[jj], d = ta[jj];
            const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
            const double du = c.x - ui, dv = c.y - vi, dw = c.z - wz;
            const double df = d.x - fi, dg = d.y - gi, dh = d.z - hi;
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
    red[wave][0][lane] = ax; red[wave][1][lane] = ay; red[wave][2][lane] = az;
    red[wave][3][lane] = jx; red[wave][4][lane] = jy; red[wave][5][lane] = jz;
    red[wave][6][lane] = sx; red[wave][7][lane] = sy; red[wave][8][lane] = sz;
    __syncthreads();
    const uint32_t k = i0 + (uint32_t)tid;
    if (tid < (int)kBbRows64 && k < ni) {
        double r[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) r[c] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
        pa[(size_t)blockIdx.y * small_max + k] = double4{r[0], r[1], r[2], 0.0};
        pj[(size_t)blockIdx.y * small_max + k] = double4{r[3], r[4], r[5], 0.0};
        ps[(size_t)blockIdx.y * small_max + k] = double4{r[6], r[7], r[8], 0.0};
    }
}

// nb_blk6_correct with |A| and t_next from the device header and the small pass's rows (chunk c, slot k at pa[c * small_max + k]).
// nb_blkq_correct's front with nine sums: kBbSumLanes lanes share a slot's chunk rows, lane q adds chunks [q w, (q + 1) w),
// w = ceil(chunks / kBbSumLanes), in ascending order in fp64, and the lanes' sums are added in lane order -- an order fixed by the
// chunk count, i.e. by n and the CU count.  Everything behind the sums (times G, corrector, crackle, criterion, new level, due) is
// nb_blk6_correct's, statement for statement, on the slot's first lane.  Grid ceil(small_max kBbSumLanes / kBlock).
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_blkq6_correct(const typename vec4<TP>::type* __restrict__ pa,
                                                          const typename vec4<TP>::type* __restrict__ pj,
                                                          const typename vec4<TP>::type* __restrict__ ps,
                                                          const uint32_t* __restrict__ act, const uint32_t* __restrict__ bb,
                                                          uint32_t small_max, uint32_t chunks, double G,
                                                          typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                          typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                          typename vec4<T>::type* __restrict__ s, typename vec4<T>::type* __restrict__ c,
                                                          uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                          uint32_t* __restrict__ hdr, uint32_t n, uint32_t L, uint32_t lmin,
                                                          int frozen, double eta, double dt)
{
    using V4 = typename vec4<T>::type;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t na = hdr[kBlkCount], t_next = hdr[kBlkNext];
    if (na > small_max) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, k = t / kBbSumLanes, q = t % kBbSumLanes;
    if (k >= na) return;                                      // (the lanes of a slot leave together)
    const uint32_t il = act[k];
    if (il >= n) return;
    double p[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) p[m] = 0.0;
    const uint32_t w = (chunks + kBbSumLanes - 1) / kBbSumLanes;
    const uint32_t c0 = q * w < chunks ? q * w : chunks, c1 = c0 + w < chunks ? c0 + w : chunks;
#pragma unroll 4
    for (uint32_t cc = c0; cc < c1; ++cc) {
        const auto pa_ = ld4(pa + (size_t)cc * small_max + k);
        const auto pj_ = ld4(pj + (size_t)cc * small_max + k);
        const auto ps_ = ld4(ps + (size_t)cc * small_max + k);
        p[0] += (double)pa_.x; p[1] += (double)pa_.y; p[2] += (double)pa_.z;
        p[3] += (double)pj_.x; p[4] += (double)pj_.y; p[5] += (double)pj_.z;
        p[6] += (double)ps_.x; p[7] += (double)ps_.y; p[8] += (double)ps_.z;
    }
    const int first = (int)((threadIdx.x & 63u) - q);         // the slot's first lane in the wave
    double r[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) {
        r[m] = __shfl(p[m], first);
#pragma unroll
        for (int o = 1; o < (int)kBbSumLanes; ++o) r[m] += __shfl(p[m], first + o);
    }
    if (q != 0) return;
    const V4 A1 = V4{(T)(G * r[0]), (T)(G * r[1]), (T)(G * r[2]), (T)0};
    const V4 J1 = V4{(T)(G * r[3]), (T)(G * r[4]), (T)(G * r[5]), (T)0};
    const V4 S1 = V4{(T)(G * r[6]), (T)(G * r[7]), (T)(G * r[8]), (T)0};
    const uint32_t l = lev[il];
    const double h = __builtin_ldexp(dt, -(int)l);
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il), S = ld4(s + il);
    const double hh = 0.5 * h, h10 = -(h * h) * (1.0 / 10.0), h120 = h * h * h * (1.0 / 120.0), ih3 = 1.0 / (h * h * h);
    auto co = [&](double y0, double d0, double d1, double e0, double e1, double f0, double f1) {
        return nb_fma(h120, f0 + f1, nb_fma(h10, e1 - e0, nb_fma(hh, d0 + d1, y0)));
    };
    struct pqr { double P, Q, R; };
    auto dif = [&](double a0, double an, double j0, double jn, double s0, double sn) {
        return pqr{nb_fma(-hh * h, s0, nb_fma(-h, j0, an - a0)), h * nb_fma(-h, s0, jn - j0), (h * h) * (sn - s0)};
    };
    const pqr dx = dif(A.x, A1.x, J.x, J1.x, S.x, S1.x), dy = dif(A.y, A1.y, J.y, J1.y, S.y, S1.y),
              dz = dif(A.z, A1.z, J.z, J1.z, S.z, S1.z);
    auto ck = [&](const pqr& d) { return nb_fma(9.0, d.R, nb_fma(-36.0, d.Q, 60.0 * d.P)) * ih3; };
    const double vx = co(V.x, A.x, A1.x, J.x, J1.x, S.x, S1.x), vy = co(V.y, A.y, A1.y, J.y, J1.y, S.y, S1.y),
                 vz = co(V.z, A.z, A1.z, J.z, J1.z, S.z, S1.z);
    const V4 C1 = V4{(T)ck(dx), (T)ck(dy), (T)ck(dz), (T)0};
    x[il] = V4{(T)co(X.x, V.x, vx, A.x, A1.x, J.x, J1.x), (T)co(X.y, V.y, vy, A.y, A1.y, J.y, J1.y),
               (T)co(X.z, V.z, vz, A.z, A1.z, J.z, J1.z), X.w};
    v[il] = V4{(T)vx, (T)vy, (T)vz, V.w};
    a[il] = A1;
    j[il] = J1;
    s[il] = S1;
    c[il] = C1;

    uint32_t ln = l;
    if (!frozen) {
        const double ih4 = ih3 / h, ih5 = ih4 / h;
        auto d4 = [&](const pqr& d) { return nb_fma(36.0, d.R, nb_fma(-192.0, d.Q, 360.0 * d.P)) * ih4; };
        auto d5 = [&](const pqr& d) { return nb_fma(60.0, d.R, nb_fma(-360.0, d.Q, 720.0 * d.P)) * ih5; };
        auto nrm = [](double p_, double q_, double r_) { return __builtin_sqrt(p_ * p_ + q_ * q_ + r_ * r_); };
        const double n0 = nrm(A1.x, A1.y, A1.z), n1 = nrm(J1.x, J1.y, J1.z), n2 = nrm(S1.x, S1.y, S1.z), n3 = nrm(C1.x, C1.y, C1.z);
        const double n4 = nrm(d4(dx), d4(dy), d4(dz)), n5 = nrm(d5(dx), d5(dy), d5(dz));
        const double den = n3 * n5 + n4 * n4;
        const double tau = den == 0.0 ? __builtin_inf() : ::cbrt(__builtin_sqrt(eta * eta * eta * (n0 * n2 + n1 * n1) / den));
        const uint32_t want = blk_level_for(tau, dt, lmin, L, hdr + kBlkClamped);
        const uint32_t s_i = 1u << (L - l);
        if (want >= l) ln = want;
        else if ((t_next & (2u * s_i - 1u)) == 0u) ln = l - 1;
        lev[il] = (uint8_t)ln;
        if (ln > l) atomicMax(hdr + kBlkFinest, ln);
    }
    due[il] = (t_next == (1u << L) ? 0u : t_next) + (1u << (L - ln));
}

}  // namespace nb
