// kernels/split_lists.hip.h -- nb_split_lists: nb_split_force's two sums AND nb_neighbor_lists' rows from ONE pass over the pairs
// (nb_spl_pk, nb_spl64, nb_spl_rows).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
//   member(k, j)  <=>  d2 < h_k^2     decides the sum a pair's term goes to (kernels/split_force.hip.h) and, with the own row left
//   out by index, whether j is written into row k (kernels/neighbor_lists.hip.h): one comparison, so the two cannot disagree.
//
// nb_spl_pk / nb_spl64 ARE nb_split_pk / nb_split64 -- the launch, the tile stream, the per-pair sequence, the flush rule and the
// plane layout, restated operation for operation, so that nb_split_reduce over their planes gives nb_split_force's bits -- plus:
//   fast path   the lane masks of a stage's compares (they feed the v_cndmask of the weights anyway) are OR-ed, scalar work, and a
//               wave in which no lane has a member among the stage's rows goes on: nothing is added per pair on the vector ALU;
//   slow path   behind that one scalar branch, per (row, point slot) with a member somewhere in the wave, in ascending j:
//                   if (in && point < m && j < j1 && j != own && cur < cap) seg[...] = j;        cur += in && j < j1 && j != own;
//               The three guards beside the cursor's: lanes past m are clamped copies of point m - 1 (they compare like it and
//               must not store); rows past the range are zero_row, AT THE ORIGIN, which a point near the origin has inside its
//               radius; the sums take the own row as a member (an exact 0), the row of the list leaves it out by index.
// A point's offset inside its row is not known before all of its j-chunks are done, so workgroup (bx, c) writes the members of
// chunk c into the segment seg[c][point][cap] and leaves the chunk's TRUE count in cnt[c][point]; only a chunk's first cap members
// can reach the row.  nb_spl_rows then walks a point's chunks in ascending order, copies min(cnt_c, cap - written) entries, pads
// the rest of the row with 0xffffffff and writes the count: every element of the row is written, nothing is set beforehand, and
// nothing is atomic.  All stores are ordinary vector stores.
#pragma once

namespace nb {

// f32.  nb_split_pk<NG, JERK> with the cursors of the lane's 2 * NG points in registers (4 VGPRs at NG = 2).
template <int NG, bool JERK>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_SPLIT_WAVES, NB_SPLIT_WAVES)))
void nb_spl_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ points,
               const float4* __restrict__ point_vel, const float* __restrict__ radii, float4* __restrict__ part,
               uint32_t n, uint32_t m, uint32_t j_per_chunk, float eps2, float radius, const float4* __restrict__ zero_row,
               uint32_t* __restrict__ seg, uint32_t* __restrict__ cnt, uint32_t cap, uint32_t at_bodies, uint32_t self0)
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
    // slot q = 2 * g + e of the lane is point pt0 + q * kBlock; its write cursor inside the chunk's segment
    const uint32_t pt0 = i0 + (uint32_t)tid;
    uint32_t cur[2 * NG];
#pragma unroll
    for (int q = 0; q < 2 * NG; ++q) cur[q] = 0;
    uint32_t* const segc = seg + (size_t)blockIdx.y * m * cap;
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

    // staging by LDS-DMA, as nb_split_pk::stage
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

    // one stage: JB tile rows (positions p, velocities q; rows jrow .. jrow + JB - 1) against the lane's NG packed groups,
    // stage-major over the NC chains -- nb_split_pk::math, with the members written down at its end
    auto math = [&](const float4* p, const float4* q, const uint32_t jrow) {
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
        // the one comparison per pair: the weight goes to exactly one of the two sums, and its lane mask says who is a member
        bool in[NC][2];
        bool hit = false;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            in[c][0] = d2[c].x < h2[c % NG].x; in[c][1] = d2[c].y < h2[c % NG].y;
            si[c] = nb_f2{in[c][0] ? s[c].x : 0.0f, in[c][1] ? s[c].y : 0.0f};
            sr[c] = nb_f2{in[c][0] ? 0.0f : s[c].x, in[c][1] ? 0.0f : s[c].y};
            hit |= in[c][0] | in[c][1];
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
        // the members.  Written behind the stage's arithmetic: the masks wait in scalar registers and the source keeps the stage's
        // temporaries out of the branch (the compiler is free to move the block up to the compares, and does).
        if (__builtin_amdgcn_ballot_w64(hit) != 0) {              // wave-uniform: some lane has a member among these JB rows
#pragma unroll
            for (int c = 0; c < NC; ++c) {                        // c = u * NG + g: a point meets its rows in ascending j
                const uint32_t j = jrow + (uint32_t)(c / NG);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (__builtin_amdgcn_ballot_w64(in[c][e]) != 0) {
                        const int slot = 2 * (c % NG) + e;
                        const uint32_t point = pt0 + (uint32_t)slot * kBlock;
                        const bool mem = in[c][e] && j < j1 && !(at_bodies && j == self0 + point);
                        if (mem && point < m && cur[slot] < cap) segc[point * cap + cur[slot]] = j;      // (m x cap <= 2^30 entries per chunk)
                        cur[slot] += mem ? 1u : 0u;
                    }
                }
            }
        }
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
        const int cb = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cb ^ 1);       // lands under this tile's compute
        const uint32_t jt = j0 + t * TILE;
        const uint32_t left = j1 - jt;
        const int rows = left < (uint32_t)TILE ? (int)left : TILE;
        const int chunks = (rows + U - 1) / U;            // rows past the range are staged zero-mass bodies (at the origin: j < j1 above)
        for (int ch = 0; ch < chunks; ++ch) {
            // (not unrolled, where nb_split_pk takes two stages at once: the branch ends the scheduler's block in either case, and two
            // stages' worth of temporaries round it cost 256 VGPRs and 52 bytes of scratch; one stage builds in 234 with none.  The order
            // of a point's additions is the same.)
#pragma unroll 1
            for (int uu = 0; uu < U / JB; ++uu)
                math(&tile[cb][0][ch * U + uu * JB], &tile[cb][NT - 1][ch * U + uu * JB], jt + (uint32_t)(ch * U + uu * JB));
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
    // the chunk's true member count of every point (the own row left out)
    uint32_t* const cc = cnt + (size_t)blockIdx.y * m;
#pragma unroll
    for (int q = 0; q < 2 * NG; ++q) {
        const uint32_t point = pt0 + (uint32_t)q * kBlock;
        if (point < m) cc[point] = cur[q];
    }
}

// fp64 handles (T = double).  nb_split64<T, JERK> with one cursor per lane; a stage is one row, its compare's lane mask the branch.
// (The tile loop runs over the chunk's own rows only: j < j1 holds by construction here.)
template <typename T, bool JERK>
__global__ __launch_bounds__(kBlock) void nb_spl64(const typename vec4<T>::type* __restrict__ pos,
                                                  const typename vec4<T>::type* __restrict__ vel,
                                                  const typename vec4<T>::type* __restrict__ points,
                                                  const typename vec4<T>::type* __restrict__ point_vel,
                                                  const T* __restrict__ radii, double4* __restrict__ part, uint32_t n, uint32_t m,
                                                  uint32_t j_per_chunk, double eps2, double radius, uint32_t* __restrict__ seg,
                                                  uint32_t* __restrict__ cnt, uint32_t cap, uint32_t at_bodies, uint32_t self0)
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
    const uint32_t own = at_bodies ? self0 + il : kNbrNone;         // n <= 2^30: never a row
    uint32_t cur = 0;
    uint32_t* const row = seg + ((size_t)blockIdx.y * m + ic) * cap;
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
        const int rows = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 2
        for (int jj = 0; jj < rows; ++jj) {
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
            if (__builtin_amdgcn_ballot_w64(in) != 0) {           // wave-uniform: some lane has this row as a member
                const uint32_t jr = jt + (uint32_t)jj;            // (< j1)
                const bool mem = in && jr != own;
                if (mem && il < m && cur < cap) row[cur] = jr;
                cur += mem ? 1u : 0u;
            }
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
        cnt[(size_t)blockIdx.y * m + il] = cur;
    }
}

// The gather: `lanes` lanes (a power of two, 8 .. 64) share a point and walk its chunks in ascending order: min(cnt_c, cap - written)
// entries of segment c go behind what the chunks before it gave, the rest of the row is padded, the count is the sum of the true
// chunk counts (never clipped).  A row is written front to back by neighbouring lanes.
template <int UNUSED = 0>     // a template only so that the header can be included by several translation units
__global__ __launch_bounds__(kBlock) void nb_spl_rows(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ cnt, uint32_t m,
                                                     uint32_t chunks, uint32_t cap, uint32_t lanes, uint32_t* __restrict__ list,
                                                     uint32_t* __restrict__ count)
{
    const uint32_t p = blockIdx.x * (kBlock / lanes) + threadIdx.x / lanes, l = threadIdx.x % lanes;
    if (p >= m) return;
    uint32_t* const row = list + (size_t)p * cap;
    uint32_t written = 0, total = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t k = cnt[(size_t)c * m + p];
        total += k;
        const uint32_t room = cap - written, take = k < room ? k : room;
        const uint32_t* const src = seg + ((size_t)c * m + p) * cap;
        for (uint32_t e = l; e < take; e += lanes) row[written + e] = src[e];
        written += take;
    }
    for (uint32_t e = written + l; e < cap; e += lanes) row[e] = kNbrNone;
    if (l == 0 && count) count[p] = total;
}

}  // namespace nb
