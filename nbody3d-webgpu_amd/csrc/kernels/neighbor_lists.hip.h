// kernels/neighbor_lists.hip.h -- nb_neighbor_lists: WHICH bodies lie inside a radius, for M points against the N rows of
// bodies[cur] (nb_nbl_offsets, nb_nbl_pk, nb_nbl64).  Part of nb_kernels.hip.h (include that, not this file).
//
//   row(p) = { j : d2(p, j) < h(p)^2 } in ascending j, the first `cap` of them, padded with 0xffffffff
//
// Two passes per batch.  The count pass is nb_neighbors' own (nb_nbr_pk<true> / nb_nbr64, unchanged): it leaves (d2, index,
// count) per (j-chunk, point) in `partial`.  nb_nbl_offsets walks a point's chunks in ascending order as nb_nbr_reduce does,
// writes the outputs that were asked for and stores the EXCLUSIVE PREFIX of the chunk counts into offsets[chunk][point]: where
// in the point's row the members of that chunk start.  The fill pass runs the count pass's grid, tile stream and d2 arithmetic
// once more: workgroup (bx, c) keeps one write cursor per point, started at offsets[c][point]; a point meets the rows of its chunk
// in ascending j, so `if (cursor < cap) list[point * cap + cursor] = j; ++cursor` at every member writes the ascending row with no
// sort and no atomics, and the chunks of a point write disjoint pieces of it.  The row was set to 0xff bytes beforehand.
//   Membership is decided by the very comparison the count pass takes (the same d2 expression, the same h2, the same own-row
// mask), so cursor - offset at the end of a chunk IS that chunk's count and the pieces meet exactly.
#pragma once

namespace nb {

// The count pass's rows of one batch: the outputs of nb_neighbors that were asked for, and per chunk the number of members the
// chunks before it hold.  T = float: rows (d2, index, count, -); double: (d2 lo, d2 hi, index, count).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_nbl_offsets(const uint4* __restrict__ partial, uint32_t m, uint32_t chunks,
                                                        uint32_t* __restrict__ offsets, uint32_t* __restrict__ index,
                                                        T* __restrict__ dist2, uint32_t* __restrict__ count)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= m) return;
    T best = (T)__builtin_huge_val();
    uint32_t idx = kNbrNone, cnt = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint4 q = partial[(size_t)c * m + il];
        T d2; uint32_t j, k;
        if constexpr (std::is_same<T, float>::value) { d2 = __uint_as_float(q.x); j = q.y; k = q.z; }
        else { d2 = __longlong_as_double((long long)(((uint64_t)q.y << 32) | q.x)); j = q.z; k = q.w; }
        const bool l = d2 < best;
        best = l ? d2 : best; idx = l ? j : idx;
        offsets[(size_t)c * m + il] = cnt;
        cnt += k;
    }
    if (index) index[il] = idx;
    if (dist2) dist2[il] = best;
    if (count) count[il] = cnt;
}

// f32 fill pass.  nb_nbr_pk's frame: 4 points per lane as two packed pairs, the tile row broadcast from LDS, 6 packed
// instructions per two pairs for d2.  The hot loop only COMPARES: per group of U = 4 tile rows the 16 lane masks of d2 < h2 are
// OR-ed (scalar work), and only a wave in which some lane has a member in the group goes over its 16 kept d2 once more, in
// ascending j, and does the guarded stores -- each behind a scalar branch of its own.  No nearest-body bookkeeping here.
//   Guards: a lane's point >= m is never stored for (its loads are clamped to point m - 1 as in nb_nbr_pk, its h2 is -1: no d2 is
// below it, so such a lane does not send its wave into the slow path either); a cursor >= cap stores nothing and only counts on.
template <int UNUSED = 0>     // a template only so that the header can be included by several translation units
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4)))
void nb_nbl_pk(const float4* __restrict__ bodies, const float4* __restrict__ points, const float* __restrict__ radii,
               const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list, uint32_t n, uint32_t m, uint32_t j_per_chunk,
               float radius, uint32_t at_bodies, uint32_t self0, uint32_t cap, const float4* __restrict__ inf_row)
{
    constexpr int NG = kNbrNG;
    constexpr int TILE = kTile;
    constexpr int U = 4;                  // tile rows per group: one OR-ed mask, one branch
    constexpr int JB = 2;                 // j-bodies per stage
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][TILE];
    const int tid = threadIdx.x;
    const uint32_t p0 = blockIdx.x * kNbrRows;               // first point of the block
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const float inf = __builtin_huge_valf();

    nb_f2 xi[NG], yi[NG], zi[NG];
    uint32_t own[2 * NG];                 // at_bodies: the row each point leaves out
    uint32_t pt[2 * NG];                  // the point of each slot (>= m: none)
    uint32_t cur[2 * NG];                 // write cursor of each point: entries of its row before the next member
    float h2[2 * NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const uint32_t c0 = il0 < m ? il0 : m - 1, c1 = il1 < m ? il1 : m - 1;      // clamped, branch-free (never stored)
        const float4 b0 = ld4(points + c0);
        const float4 b1 = ld4(points + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        own[2 * g] = self0 + il0; own[2 * g + 1] = self0 + il1;
        pt[2 * g] = il0; pt[2 * g + 1] = il1;
        const float r0 = radii ? radii[c0] : radius, r1 = radii ? radii[c1] : radius;
        h2[2 * g] = il0 < m ? r0 * r0 : -1.0f; h2[2 * g + 1] = il1 < m ? r1 * r1 : -1.0f;
        cur[2 * g] = offsets[(size_t)blockIdx.y * m + c0];
        cur[2 * g + 1] = offsets[(size_t)blockIdx.y * m + c1];
    }
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_nbr_pk: whole tiles from a scalar base, the last one per lane with rows past the range taken
    // from inf_row (d2 = +inf: below no h2)
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst = lds_wave + (uint32_t)(buf * TILE) * 16u;
        unsigned keep;
        if (jt + TILE <= j1) {
            const float4* base = bodies + jt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(base), "s"(dst) : "memory");
        } else {
            const uint32_t j = jt + tid;
            const float4* src = j < j1 ? bodies + j : inf_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        }
    };

    // d2 of one stage: JB tile rows against the lane's NG packed groups (c = u * NG + g) -- nb_nbr_pk's expression, operation for
    // operation
    auto dist = [&](const float4* p, nb_f2 (&d2)[NC]) {
        nb_f2 bx[JB], by[JB], bz[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z};
        }
        nb_f2 dx[NC], dy[NC], dz[NC];
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
    };

    // One group: U rows against the lane's points.  Fast path: the d2 of the group (kept: 2 * U registers), the own row masked
    // where the tile can hold it, and the OR of all compares.  Slow path, only when some lane of the wave has a member: the kept d2
    // in ascending j, and per (row, point slot) again only when some lane has a member THERE (a scalar branch on the compare
    // mask) the guarded store and the cursor.
    auto group = [&](const float4* p, const uint32_t jrow, auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
        nb_f2 d2[U / JB][NC];
        bool hit = false;
#pragma unroll
        for (int uu = 0; uu < U / JB; ++uu) {
            dist(p + uu * JB, d2[uu]);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint32_t j = jrow + (uint32_t)(uu * JB + c / NG);
                const int q0 = 2 * (c % NG), q1 = q0 + 1;
                if constexpr (MASKED) {
                    d2[uu][c].x = j == own[q0] ? inf : d2[uu][c].x;
                    d2[uu][c].y = j == own[q1] ? inf : d2[uu][c].y;
                }
                hit |= d2[uu][c].x < h2[q0];
                hit |= d2[uu][c].y < h2[q1];
            }
        }
        if (__builtin_amdgcn_ballot_w64(hit) != 0) {          // wave-uniform: some lane has a member in these U rows
#pragma unroll
            for (int uu = 0; uu < U / JB; ++uu) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {                // c = u * NG + g: a point meets its rows in ascending j
                    const uint32_t j = jrow + (uint32_t)(uu * JB + c / NG);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int q = 2 * (c % NG) + e;
                        const bool in = (e ? d2[uu][c].y : d2[uu][c].x) < h2[q];
                        if (__builtin_amdgcn_ballot_w64(in) != 0) {
                            if (in && pt[q] < m && cur[q] < cap) list[(size_t)pt[q] * cap + cur[q]] = j;
                            cur[q] += in ? 1u : 0u;
                        }
                    }
                }
            }
        }
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the block's own rows as system indices (at_bodies): [lo, hi)
    const uint32_t own_lo = self0 + p0, own_hi = own_lo + kNbrRows;
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cb = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cb ^ 1);       // lands under this tile's compute
        const uint32_t jt = j0 + t * TILE;
        const uint32_t left = j1 - jt;
        const int rows = left < (uint32_t)TILE ? (int)left : TILE;
        const int groups = (rows + U - 1) / U;            // rows past the range are staged rows at +inf
        if (at_bodies && jt < own_hi && jt + TILE > own_lo) {
            for (int ch = 0; ch < groups; ++ch) group(&tile[cb][ch * U], jt + (uint32_t)(ch * U), std::true_type{});
        } else {
            for (int ch = 0; ch < groups; ++ch) group(&tile[cb][ch * U], jt + (uint32_t)(ch * U), std::false_type{});
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// f64 handles: nb_nbr64's frame -- one point per lane, the j-tile staged through registers, fp64 throughout -- with the rows of the
// last tile past the chunk's end staged at +inf, so that whole groups of U = 4 rows can be probed; the same two paths.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_nbl64(const typename vec4<T>::type* __restrict__ bodies,
                                                  const typename vec4<T>::type* __restrict__ points, const T* __restrict__ radii,
                                                  const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list, uint32_t n,
                                                  uint32_t m, uint32_t j_per_chunk, double radius, uint32_t at_bodies, uint32_t self0,
                                                  uint32_t cap)
{
    constexpr int U = 4;
    __shared__ double4 tile[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kNbrRows64 + tid;
    const uint32_t ic = il < m ? il : m - 1;                         // clamped (never stored)
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const auto pt = ld4(points + ic);
    const double xi = (double)pt.x, yi = (double)pt.y, zi = (double)pt.z;
    const double h = radii ? (double)radii[ic] : radius;
    const double h2 = il < m ? h * h : -1.0;                         // a lane past m has no member
    const uint32_t own = at_bodies ? self0 + il : kNbrNone;         // n <= 2^30: never a row
    const double inf = __builtin_huge_val();
    uint32_t cur = offsets[(size_t)blockIdx.y * m + ic];
    uint32_t* row = list + (size_t)ic * cap;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) { const auto b = ld4(bodies + j); tile[tid] = double4{(double)b.x, (double)b.y, (double)b.z, 0.0}; }
        else tile[tid] = double4{inf, inf, inf, 0.0};
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int rows = left < (uint32_t)kTile ? (int)left : kTile;
        for (int jj = 0; jj < rows; jj += U) {
            double d2[U];
            bool hit = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double4 b = tile[jj + u];
                const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
                const double d = nb_fma(dz, dz, nb_fma(dy, dy, dx * dx));
                d2[u] = jt + (uint32_t)(jj + u) == own ? inf : d;
                hit |= d2[u] < h2;
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {          // some lane of the wave has a member among these U rows
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = d2[u] < h2;
                    if (__builtin_amdgcn_ballot_w64(in) != 0) {
                        if (in && il < m && cur < cap) row[cur] = jt + (uint32_t)(jj + u);
                        cur += in ? 1u : 0u;
                    }
                }
            }
        }
    }
}

}  // namespace nb
