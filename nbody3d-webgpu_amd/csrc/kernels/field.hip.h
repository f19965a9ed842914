// kernels/field.hip.h -- nb_field_eval: acceleration and potential of the system at arbitrary points (nb_field_pk, nb_field64, nb_field_reduce).
// Part of nb_kernels.hip.h (include that, not this file).
//
//   a(p) = sum_j G m_j (x_j - p) / (|x_j - p|^2 + eps2)^(3/2)        phi(p) = - sum_j G m_j / sqrt(|x_j - p|^2 + eps2)
//
// M points against the N rows of bodies[cur]: M x N ORDERED pairs, the simulation state is only read.  Grid = (point blocks) x
// (j-chunks): workgroup (bx, c) accumulates its points against the bodies of chunk c and stores one row (ax, ay, az, sum m/r) per
// point into partial[c][point]; nb_field_reduce adds a point's chunks in ascending order, multiplies by G ONCE (both outputs are
// linear in G: the plain (x, y, z, m) rows stream through LDS-DMA with no register pass, and the gm / pairs copies are never touched)
// and writes the outputs.  Fixed order everywhere, no atomics: the same request on the same state gives the same bits.
#pragma once

namespace nb {

constexpr int kFieldNG = 2;                              // packed groups per lane: 4 points per lane
constexpr uint32_t kFieldRows = kBlock * 2 * kFieldNG;   // points of one f32 workgroup (1,024)
constexpr uint32_t kFieldRows64 = kBlock;                // points of one f64 workgroup
constexpr uint32_t kFieldFlush = 4;                      // tiles between two flushes of the first-level sums (1,024 terms per chain)

// f32.  The points are the i-side: 2*NG per lane in registers as packed pairs, every lane of the wave reads the same tile row
// (LDS broadcast).  Per two pairs: 3 v_pk_add (differences), 3 v_pk_fma (r^2 + eps2), 2 v_rsq_f32 of r^2 -- ONE reciprocal root
// serves both outputs --, y^2 = y y, s = m y, [phi += s], [s3 = s y^2, 3 v_pk_fma into the acceleration]: 13 packed + 2
// transcendental with both outputs, 9 + 2 for the potential alone, 12 + 2 for the acceleration alone.  Every consumer of a
// v_rsq_f32 result is a compiler-emitted instruction (the backend places the wait state gfx950 wants itself).
//   Summation: binary32, two levels inside the kernel.  A lane's running sums take the pairs of kFieldFlush tiles (1,024 terms),
// then are added into a second set and cleared, so no register ever takes more than 1,024 terms (first level) or
// chunk / 1,024 terms (second level) in sequence -- one register summing 2 M terms would be 1e-4 off.  The chunk sums are added
// in fp64 by nb_field_reduce.
//   at_bodies: point k IS body self0 + k and leaves itself out: the tiles that contain rows of the block's own range run the masked
// loop (the mass of the one pair j == own row is replaced by 0 before it is multiplied in), all others the plain one.  Nothing
// is ever subtracted afterwards.
template <bool WANT_ACCEL, bool WANT_PHI>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4)))
void nb_field_pk(const float4* __restrict__ bodies, const float4* __restrict__ points, float4* __restrict__ partial, uint32_t n,
                 uint32_t m, uint32_t j_per_chunk, float eps2, uint32_t at_bodies, uint32_t self0,
                 const float4* __restrict__ zero_row)
{
    constexpr int NG = kFieldNG;
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 2;                 // j-bodies per stage: JB * NG = 4 independent chains, issued stage-major
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][TILE];
    const int tid = threadIdx.x;
    const uint32_t p0 = blockIdx.x * kFieldRows;             // first point of the block
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi[NG], yi[NG], zi[NG];
    uint32_t own[2 * NG];                 // at_bodies: the row each point leaves out
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const float4 b0 = ld4(points + (il0 < m ? il0 : m - 1));      // clamped, branch-free (never stored)
        const float4 b1 = ld4(points + (il1 < m ? il1 : m - 1));
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        own[2 * g] = self0 + il0; own[2 * g + 1] = self0 + il1;
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 ax[NG], ay[NG], az[NG], ph[NG], AX[NG], AY[NG], AZ[NG], PH[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { ax[g] = ay[g] = az[g] = ph[g] = zero; AX[g] = AY[g] = AZ[g] = PH[g] = zero; }
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as PkCore::run (ordered.hip.h): whole tiles from a scalar base, the last one per lane with rows past
    // the range taken from zero_row (a zero-mass body at the origin adds exactly 0 to both sums)
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
            const float4* src = j < j1 ? bodies + j : zero_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        }
    };

    // one stage: JB tile rows against the lane's NG packed groups; jrow = system index of p[0] (masked form only)
    auto math = [&](const float4* p, const uint32_t jrow, auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
        nb_f2 bx[JB], by[JB], bz[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
        }
        nb_f2 dx[NC], dy[NC], dz[NC], d2[NC], y[NC], s[NC];
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
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float mj = bm[c / NG];
            if constexpr (MASKED) {
                const uint32_t j = jrow + (uint32_t)(c / NG);
                s[c] = nb_f2{j == own[2 * (c % NG)] ? 0.0f : mj, j == own[2 * (c % NG) + 1] ? 0.0f : mj} * y[c];
            } else {
                s[c] = nb_f2{mj, mj} * y[c];
            }
        }
        if constexpr (WANT_PHI) {
#pragma unroll
            for (int c = 0; c < NC; ++c) ph[c % NG] = ph[c % NG] + s[c];
        }
        if constexpr (WANT_ACCEL) {
#pragma unroll
            for (int c = 0; c < NC; ++c) y[c] = y[c] * y[c];
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c] = s[c] * y[c];
#pragma unroll
            for (int c = 0; c < NC; ++c) ax[c % NG] = __builtin_elementwise_fma(s[c], dx[c], ax[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) ay[c % NG] = __builtin_elementwise_fma(s[c], dy[c], ay[c % NG]);
#pragma unroll
            for (int c = 0; c < NC; ++c) az[c % NG] = __builtin_elementwise_fma(s[c], dz[c], az[c % NG]);
        }
    };
    auto flush = [&]() {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if constexpr (WANT_ACCEL) {
                AX[g] = AX[g] + ax[g]; AY[g] = AY[g] + ay[g]; AZ[g] = AZ[g] + az[g];
                ax[g] = zero; ay[g] = zero; az[g] = zero;
            }
            if constexpr (WANT_PHI) { PH[g] = PH[g] + ph[g]; ph[g] = zero; }
        }
    };

    if (ntiles) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the block's own rows as system indices (at_bodies): [lo, hi)
    const uint32_t own_lo = self0 + p0, own_hi = own_lo + kFieldRows;
    for (uint32_t t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) stage(t + 1, cur ^ 1);      // lands under this tile's compute
        const uint32_t jt = j0 + t * TILE;
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)TILE ? (int)left : TILE;
        const int chunks = (cnt + U - 1) / U;             // rows past the range are staged zero-mass bodies
        if (at_bodies && jt < own_hi && jt + TILE > own_lo) {
            for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
                for (int uu = 0; uu < U / JB; ++uu)
                    math(&tile[cur][ch * U + uu * JB], jt + (uint32_t)(ch * U + uu * JB), std::true_type{});
            }
        } else {
            for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll 2
                for (int uu = 0; uu < U / JB; ++uu) math(&tile[cur][ch * U + uu * JB], 0u, std::false_type{});
            }
        }
        if ((t & (kFieldFlush - 1)) == kFieldFlush - 1) flush();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    float4* out = partial + (size_t)blockIdx.y * m;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        if (il0 < m) out[il0] = float4{AX[g].x, AY[g].x, AZ[g].x, PH[g].x};
        if (il1 < m) out[il1] = float4{AX[g].y, AY[g].y, AZ[g].y, PH[g].y};
    }
}

// fp64: f64 handles (TB = TP = double) and NB_FIELD_F64 on an f32 handle (TB = TP = float: the stored f32 rows and the f32
// points are converted when they are staged, every difference, product and sum is fp64).  One point per lane, the j-tile staged
// through registers; v_rsq_f64 seed + one correction (y0 (1 + e/2), e = 1 - r^2 y0^2: relative error ~ 3 e^2 / 8 < 1e-16), the
// potential from the corrected root, the acceleration from its cube.  The own row of an at_bodies point gets weight 0 per pair.
// 1e-12 is the bar here, not speed.
template <typename TB>
__global__ __launch_bounds__(kBlock) void nb_field64(const typename vec4<TB>::type* __restrict__ bodies,
                                                    const typename vec4<TB>::type* __restrict__ points,
                                                    double4* __restrict__ partial, uint32_t n, uint32_t m, uint32_t j_per_chunk,
                                                    double eps2, uint32_t at_bodies, uint32_t self0)
{
    __shared__ double4 tile[kTile];
    const int tid = threadIdx.x;
    const uint32_t il = blockIdx.x * kFieldRows64 + tid;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const auto pt = ld4(points + (il < m ? il : m - 1));
    const double xi = (double)pt.x, yi = (double)pt.y, zi = (double)pt.z;
    const uint32_t own = at_bodies ? self0 + il : 0xffffffffu;      // n <= 2^30: never a row
    double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) { const auto b = ld4(bodies + j); tile[tid] = double4{(double)b.x, (double)b.y, (double)b.z, (double)b.w}; }
        else tile[tid] = double4{0.0, 0.0, 0.0, 0.0};             // past the chunk: zero mass
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            const double4 b = tile[jj];
            const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double w = (jt + (uint32_t)jj == own) ? 0.0 : b.w;
            const double s = w * y;
            ph += s;
            const double s3 = s * (y * y);
            ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
        }
    }
    if (il < m) partial[(size_t)blockIdx.y * m + il] = double4{ax, ay, az, ph};
}

// Adds a point's chunk rows in ascending chunk order in fp64, multiplies by G once, writes what was asked for (TO = float or
// double; accel rows (ax, ay, az, 0), phi = -G sum).  TP = element type of the partial rows.
template <typename TP, typename TO>
__global__ __launch_bounds__(kBlock) void nb_field_reduce(const typename vec4<TP>::type* __restrict__ partial, uint32_t m,
                                                         uint32_t chunks, double G, typename vec4<TO>::type* __restrict__ accel,
                                                         TO* __restrict__ phi)
{
    using VO = typename vec4<TO>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= m) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, sp = 0.0;
    uint32_t c = 0;
    for (; c + 3 < chunks; c += 4) {       // four independent loads per trip, added in ascending order
        const auto q0 = ld4(partial + (size_t)c * m + il);
        const auto q1 = ld4(partial + (size_t)(c + 1) * m + il);
        const auto q2 = ld4(partial + (size_t)(c + 2) * m + il);
        const auto q3 = ld4(partial + (size_t)(c + 3) * m + il);
        sx += (double)q0.x; sy += (double)q0.y; sz += (double)q0.z; sp += (double)q0.w;
        sx += (double)q1.x; sy += (double)q1.y; sz += (double)q1.z; sp += (double)q1.w;
        sx += (double)q2.x; sy += (double)q2.y; sz += (double)q2.z; sp += (double)q2.w;
        sx += (double)q3.x; sy += (double)q3.y; sz += (double)q3.z; sp += (double)q3.w;
    }
    for (; c < chunks; ++c) {
        const auto q = ld4(partial + (size_t)c * m + il);
        sx += (double)q.x; sy += (double)q.y; sz += (double)q.z; sp += (double)q.w;
    }
    if (accel) accel[il] = VO{(TO)(G * sx), (TO)(G * sy), (TO)(G * sz), (TO)0};
    if (phi) phi[il] = (TO)(-(G * sp));
}

}  // namespace nb
