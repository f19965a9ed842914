// kernels/neighbors.hip.h -- nb_neighbors: nearest body and number of bodies inside a radius, for M points against the N rows of
// bodies[cur] (nb_nbr_pk, nb_nbr64, nb_nbr_reduce).  Part of nb_kernels.hip.h (include that, not this file).
//
//   d2(p, j) = fma(dz, dz, fma(dy, dy, dx dx)),  dx = x_j - p_x ...      (no softening, the handle's precision)
//   index(p) = the j with the smallest d2, the SMALLEST such j among equals        count(p) = #{ j : d2(p, j) < h(p)^2 }
//
// The launch shape is nb_field_pk's: grid = (point blocks) x (j-chunks of whole 256-row tiles), workgroup (bx, c) runs its points
// against the bodies of chunk c and stores one 16-byte row (d2, index, count) per point into partial[c][point]; nb_nbr_reduce
// walks a point's chunks in ascending order.  Min and integer sums are exact and every comparison is a strict `<` taken in
// ascending j, so the three outputs of a point depend on that point and on the bodies alone: not on m, not on the batch, not on
// the cut into chunks.  The simulation state is only read.
#pragma once

namespace nb {

constexpr int kNbrNG = 2;                              // packed groups per lane: 4 points per lane
constexpr uint32_t kNbrRows = kBlock * 2 * kNbrNG;     // points of one f32 workgroup (1,024)
constexpr uint32_t kNbrRows64 = kBlock;                // points of one f64 workgroup
constexpr uint32_t kNbrNone = 0xffffffffu;             // "no neighbour"

// f32.  The points are the i-side: 4 per lane in registers as two packed pairs, every lane of the wave reads the same tile row (LDS
// broadcast).  Per two pairs: 3 v_pk_add (differences), 1 v_pk_mul + 2 v_pk_fma (d2) -- 6 packed, no transcendental -- then per
// pair (gfx950 has no packed min or compare) v_cmp_lt + 2 v_cndmask carry (d2, j) of the best so far, and with WANT_COUNT
// v_cmp_lt + v_addc the count.  The rows of a stage are taken in ascending j and `<` is strict: of equal distances the first, the
// smallest j, stays.
//   Rows past the end of the chunk inside its last tile are staged from inf_row, a row at (+inf, +inf, +inf): against a finite
// point d2 = +inf, never NaN, and no strict `<` takes it (a row at the origin, nb_field_pk's zero_row, would be a candidate).
//   at_bodies: point k IS body self0 + k and leaves itself out by INDEX: the tiles that contain rows of the block's own range
// run the masked loop (d2 of the one pair j == own row is replaced by +inf), all others the plain one.  Another body at the same
// position is a neighbour at d2 = 0.
template <bool WANT_COUNT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4)))
void nb_nbr_pk(const float4* __restrict__ bodies, const float4* __restrict__ points, const float* __restrict__ radii, uint4* __restrict__ partial,
               uint32_t n, uint32_t m, uint32_t j_per_chunk, float radius, uint32_t at_bodies, uint32_t self0,
               const float4* __restrict__ inf_row)
{
    constexpr int NG = kNbrNG;
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
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
    float h2[2 * NG];                     // WANT_COUNT: the squared search radius of each point
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const uint32_t c0 = il0 < m ? il0 : m - 1, c1 = il1 < m ? il1 : m - 1;      // clamped, branch-free (never stored)
        const float4 b0 = ld4(points + c0);
        const float4 b1 = ld4(points + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        own[2 * g] = self0 + il0; own[2 * g + 1] = self0 + il1;
        if constexpr (WANT_COUNT) {
            const float r0 = radii ? radii[c0] : radius, r1 = radii ? radii[c1] : radius;
            h2[2 * g] = r0 * r0; h2[2 * g + 1] = r1 * r1;
        } else {
            h2[2 * g] = h2[2 * g + 1] = 0.0f;
        }
    }
    float best[2 * NG];
    uint32_t idx[2 * NG], cnt[2 * NG];
#pragma unroll
    for (int q = 0; q < 2 * NG; ++q) { best[q] = inf; idx[q] = kNbrNone; cnt[q] = 0; }
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_field_pk: whole tiles from a scalar base, the last one per lane with rows past the range taken
    // from inf_row
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

    // one stage: JB tile rows against the lane's NG packed groups; jrow = system index of p[0]
    auto math = [&](const float4* p, const uint32_t jrow, auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
        nb_f2 bx[JB], by[JB], bz[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z};
        }
        nb_f2 dx[NC], dy[NC], dz[NC], d2[NC];
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
        for (int c = 0; c < NC; ++c) {            // c = u * NG + g: a point meets its rows in ascending j
            const uint32_t j = jrow + (uint32_t)(c / NG);
            const int q0 = 2 * (c % NG), q1 = q0 + 1;
            float a = d2[c].x, b = d2[c].y;
            if constexpr (MASKED) {
                a = j == own[q0] ? inf : a;
                b = j == own[q1] ? inf : b;
            }
            const bool la = a < best[q0], lb = b < best[q1];
            best[q0] = la ? a : best[q0]; idx[q0] = la ? j : idx[q0];
            best[q1] = lb ? b : best[q1]; idx[q1] = lb ? j : idx[q1];
            if constexpr (WANT_COUNT) {
                cnt[q0] += a < h2[q0] ? 1u : 0u;
                cnt[q1] += b < h2[q1] ? 1u : 0u;
            }
        }
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the block's own rows as system indices (at_bodies): [lo, hi)
    const uint32_t own_lo = self0 + p0, own_hi = own_lo + kNbrRows;
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cur ^ 1);      // lands under this tile's compute
        const uint32_t jt = j0 + t * TILE;
        const uint32_t left = j1 - jt;
        const int rows = left < (uint32_t)TILE ? (int)left : TILE;
        const int chunks = (rows + U - 1) / U;            // rows past the range are staged rows at +inf
        if (at_bodies && jt < own_hi && jt + TILE > own_lo) {
            for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
                for (int uu = 0; uu < U / JB; ++uu)
                    math(&tile[cur][ch * U + uu * JB], jt + (uint32_t)(ch * U + uu * JB), std::true_type{});
            }
        } else {
            for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
                for (int uu = 0; uu < U / JB; ++uu)
                    math(&tile[cur][ch * U + uu * JB], jt + (uint32_t)(ch * U + uu * JB), std::false_type{});
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    uint4* out = partial + (size_t)blockIdx.y * m;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        if (il0 < m) out[il0] = uint4{__float_as_uint(best[2 * g]), idx[2 * g], cnt[2 * g], 0u};
        if (il1 < m) out[il1] = uint4{__float_as_uint(best[2 * g + 1]), idx[2 * g + 1], cnt[2 * g + 1], 0u};
    }
}

// f64 handles: one point per lane, the j-tile staged through registers as nb_field64 does, fp64 throughout; the loop ends at the
// chunk's last row, so no row past it is ever met.  Partial row: (double d2, index, count).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_nbr64(const typename vec4<T>::type* __restrict__ bodies,
                                                  const typename vec4<T>::type* __restrict__ points, const T* __restrict__ radii,
                                                  uint4* __restrict__ partial, uint32_t n, uint32_t m, uint32_t j_per_chunk,
                                                  double radius, uint32_t at_bodies, uint32_t self0)
{
    __shared__ double4 tile[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kNbrRows64 + tid;
    const uint32_t ic = il < m ? il : m - 1;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const auto pt = ld4(points + ic);
    const double xi = (double)pt.x, yi = (double)pt.y, zi = (double)pt.z;
    const double h = radii ? (double)radii[ic] : radius;
    const double h2 = h * h;
    const uint32_t own = at_bodies ? self0 + il : kNbrNone;         // n <= 2^30: never a row
    double best = __builtin_huge_val();
    uint32_t idx = kNbrNone, cnt = 0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) { const auto b = ld4(bodies + j); tile[tid] = double4{(double)b.x, (double)b.y, (double)b.z, 0.0}; }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int rows = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 4
        for (int jj = 0; jj < rows; ++jj) {
            const double4 b = tile[jj];
            const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
            double d2 = nb_fma(dz, dz, nb_fma(dy, dy, dx * dx));
            const uint32_t jr = jt + (uint32_t)jj;
            d2 = jr == own ? __builtin_huge_val() : d2;
            const bool l = d2 < best;
            best = l ? d2 : best; idx = l ? jr : idx;
            cnt += d2 < h2 ? 1u : 0u;
        }
    }
    if (il < m) {
        const uint64_t bits = (uint64_t)__double_as_longlong(best);
        partial[(size_t)blockIdx.y * m + il] = uint4{(uint32_t)bits, (uint32_t)(bits >> 32), idx, cnt};
    }
}

// Walks a point's chunk rows in ascending chunk order: strict `<` keeps the earlier chunk -- the smaller j -- among equal distances,
// the counts add up.  Writes the outputs that were asked for (T = float: rows (d2, index, count, -); double: (d2 lo, d2 hi, index, count)).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_nbr_reduce(const uint4* __restrict__ partial, uint32_t m, uint32_t chunks,
                                                       uint32_t* __restrict__ index, T* __restrict__ dist2, uint32_t* __restrict__ count)
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
        cnt += k;
    }
    if (index) index[il] = idx;
    if (dist2) dist2[il] = best;
    if (count) count[il] = cnt;
}

}  // namespace nb
