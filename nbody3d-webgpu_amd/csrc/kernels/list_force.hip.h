// kernels/list_force.hip.h -- nb_list_force: acceleration, jerk and potential summed over NEIGHBOUR ROWS (nb_lf32, nb_lf64).  No
// reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
//   a_k = sum_e G m_j dr / rho^3      jerk_k = sum_e G m_j [dv / rho^3 - 3 (dr.dv) dr / rho^5]      phi_k = - sum_e G m_j / rho
//   j = list[k * cap + e],  dr = x_j - p_k,  dv = v_j - u_k,  rho^2 = |dr|^2 + eps2
//
// The irregular force of an Ahmad-Cohen split: M rows of at most `cap` indices instead of M x N pairs.  The first pass of this
// engine that is a GATHER and not a tile stream: nothing goes through LDS, every entry is one 16-byte row load (two with the jerk)
// from wherever the index points.
//   Shape: a group of LS = kLfLanes32 / kLfLanes64 consecutive lanes owns one row -- 64 / LS rows per wave, kBlock / LS per workgroup, grid =
// ceil(batch / (kBlock / LS)).  Entry e of a row goes to lane e % LS of its group: the index loads list[row * cap + e] of a group are
// LS consecutive dwords (plain dword loads: row * cap * 4 is not 16-byte aligned for an odd cap).  A lane walks e = lane, lane + LS,
// ... and adds its terms in that order into ONE chain per output component; the trip count is the wave's longest row (min(count,
// cap), or cap without count) rounded up to kLfU * LS entries: wave-uniform, so the loop closes on a scalar branch, and unrolled
// kLfU times so that kLfU index loads, then kLfU (2 kLfU) row gathers are in flight per lane before the first term is formed.
//   An entry that is no body (j >= n: the padding 0xffffffff wherever it stands, or anything else past the rows), the own row of an
// at_bodies point, and every slot past the row's length load ROW 0 with the mass replaced by 0 before it is multiplied in (the
// device of nb_field_pk's masked loop): branch-free, no address outside the arrays is ever formed, and the term is an exact +-0 that
// leaves every chain's bits alone (eps2 > 0 keeps the reciprocal root finite).  A chain starts at +0 and (+0) + (-0) = +0: a row
// without a valid entry gives +0 everywhere.
//   Order of additions: a function of an entry's POSITION in its row alone -- lane e % LS, ascending e inside the lane, then the LS
// lane sums converted to fp64 and combined in the fixed butterfly of group_sum<LS>(double) (every lane ends with the same bits), G
// multiplied in ONCE in fp64 and the product rounded once (nb_field_reduce's rule).  So a row's outputs do not depend on m, on the
// batch, on cap or on whether count was passed (while the tail it skips is padding).
//   Lanes of rows past m clamp their row (they repeat row m - 1) and store nothing; lane 0 of a group stores with vector stores.
// No LDS, no scratch, no atomics.
#pragma once

namespace nb {

// Lanes that share one row: ONE build constant per precision, chosen by measurement (profiles/r14/list_force.md: the libraries
// alternating, N = 65,536 and 262,144, rows of mean count 32 and nb_knn's rows of 6).  A/B builds: -DNB_LF_LANES=8|16|32 sets both.
#ifdef NB_LF_LANES
constexpr int kLfLanes32 = NB_LF_LANES, kLfLanes64 = NB_LF_LANES;
#else
constexpr int kLfLanes32 = 16, kLfLanes64 = 16;
#endif
static_assert(kLfLanes32 == 8 || kLfLanes32 == 16 || kLfLanes32 == 32, "lanes per row: 8, 16 or 32");
static_assert(kLfLanes64 == 8 || kLfLanes64 == 16 || kLfLanes64 == 32, "lanes per row: 8, 16 or 32");
constexpr uint32_t lf_lanes(bool f64) { return (uint32_t)(f64 ? kLfLanes64 : kLfLanes32); }
constexpr uint32_t lf_rows(bool f64) { return kBlock / lf_lanes(f64); }      // rows of one workgroup
constexpr int kLfU = 4;                             // entries a lane has in flight

// whole-row stores through the native vector types, as ld4 loads: ONE global_store_dwordx4 (two for f64)
__device__ __forceinline__ void st4(float4* p, const float4 v) { *reinterpret_cast<nb_v4f*>(p) = nb_v4f{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void st4(double4* p, const double4 v) { *reinterpret_cast<nb_v4d*>(p) = nb_v4d{v.x, v.y, v.z, v.w}; }

// what every lane knows of its row: where its entries are, how many of them there are, who it must leave out
struct LfRow {
    const uint32_t* list;     // the row's first entry
    uint32_t len, own, row;
    bool store;
};
template <int LS>
__device__ __forceinline__ LfRow lf_row(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count, uint32_t m,
                                        uint32_t cap, uint32_t at_bodies, uint32_t self0, uint32_t* trips)
{
    const uint32_t r = blockIdx.x * (kBlock / LS) + threadIdx.x / LS;
    LfRow o;
    o.row = r < m ? r : m - 1;                                    // clamped, branch-free (never stored)
    o.store = r < m && threadIdx.x % LS == 0;
    o.list = list + (size_t)o.row * cap;
    uint32_t len = cap;
    if (count) { const uint32_t c = count[o.row]; len = c < cap ? c : cap; }
    o.len = len;
    o.own = at_bodies ? self0 + o.row : 0xffffffffu;              // n <= 2^30: never a row
    uint32_t longest = len;                                       // the wave's longest row
#pragma unroll
    for (int w = LS; w < 64; w <<= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)longest, w, 64); longest = t > longest ? t : longest; }
    longest = __builtin_amdgcn_readfirstlane(longest);
    *trips = (longest + (uint32_t)(kLfU * LS) - 1) / (uint32_t)(kLfU * LS);
    return o;
}

// f32: the per-pair arithmetic of fj_pk_body / nb_field_pk, one row per lane group, unpacked (one chain per component: the order of
// additions is the contract here, and the pass waits for its gathers, not for the vector ALU).  ONE v_rsq_f32 serves all three
// outputs; the jerk is ONE sum of s3 (dv - 3 q dr).
template <bool WANT_A, bool WANT_J, bool WANT_PHI>
__global__ __launch_bounds__(kBlock)
void nb_lf32(const float4* __restrict__ bodies, const float4* __restrict__ vel, const float4* __restrict__ points,
             const float4* __restrict__ point_vel, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
             uint32_t n, uint32_t m, uint32_t cap, float eps2, double G, uint32_t at_bodies, uint32_t self0,
             float4* __restrict__ accel, float4* __restrict__ jerk, float* __restrict__ phi)
{
    constexpr int LS = kLfLanes32;
    constexpr int U = kLfU;
    uint32_t trips;
    const LfRow r = lf_row<LS>(list, count, m, cap, at_bodies, self0, &trips);
    const uint32_t lane = threadIdx.x % LS;
    const float4 p = ld4(points + r.row);
    float ui = 0.0f, vi = 0.0f, wi = 0.0f;
    if constexpr (WANT_J) { const float4 u = ld4(point_vel + r.row); ui = u.x; vi = u.y; wi = u.z; }
    float ax = 0.0f, ay = 0.0f, az = 0.0f, jx = 0.0f, jy = 0.0f, jz = 0.0f, ph = 0.0f;

    uint32_t e0 = lane;
    for (uint32_t t = 0; t < trips; ++t, e0 += U * LS) {
        uint32_t j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * LS;
            const bool in = e < r.len;
            const uint32_t v = r.list[in ? e : 0u];                 // a slot past the row reads entry 0 and is dropped (cap >= 1)
            ok[u] = in && v < n && v != r.own;
            j[u] = ok[u] ? v : 0u;
        }
        float4 b[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            b[u] = ld4(bodies + j[u]);
            if constexpr (WANT_J) c[u] = ld4(vel + j[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float mj = ok[u] ? b[u].w : 0.0f;
            const float dx = b[u].x - p.x, dy = b[u].y - p.y, dz = b[u].z - p.z;
            const float d2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const float y = nb_rsq(d2);
            const float s = mj * y;
            if constexpr (WANT_PHI) ph = ph + s;
            if constexpr (WANT_A || WANT_J) {
                const float y2 = y * y;
                const float s3 = s * y2;                              // m / rho^3
                if constexpr (WANT_J) {
                    const float du = c[u].x - ui, dv = c[u].y - vi, dw = c[u].z - wi;
                    float rv = dx * du;
                    rv = nb_fma(dy, dv, rv);
                    rv = nb_fma(dz, dw, rv);
                    rv = rv * y2;                                     // q = (dr.dv) / rho^2
                    rv = rv * -3.0f;
                    const float tx = nb_fma(rv, dx, du), ty = nb_fma(rv, dy, dv), tz = nb_fma(rv, dz, dw);      // dv - 3 q dr
                    jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
                }
                if constexpr (WANT_A) { ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az); }
            }
        }
    }

    if constexpr (WANT_A) {
        const double sx = group_sum<LS>((double)ax), sy = group_sum<LS>((double)ay), sz = group_sum<LS>((double)az);
        if (r.store) st4(accel + r.row, float4{(float)(G * sx), (float)(G * sy), (float)(G * sz), 0.0f});
    }
    if constexpr (WANT_J) {
        const double sx = group_sum<LS>((double)jx), sy = group_sum<LS>((double)jy), sz = group_sum<LS>((double)jz);
        if (r.store) st4(jerk + r.row, float4{(float)(G * sx), (float)(G * sy), (float)(G * sz), 0.0f});
    }
    if constexpr (WANT_PHI) {
        const double sp = group_sum<LS>((double)ph);
        if (r.store) phi[r.row] = (float)(0.0 - G * sp);      // (0 - x, not -x: an empty row gives +0)
    }
}

// f64 handles: the per-pair arithmetic of fj64_body / nb_field64 (v_rsq_f64 seed + one correction), everything in fp64.
template <bool WANT_A, bool WANT_J, bool WANT_PHI>
__global__ __launch_bounds__(kBlock)
void nb_lf64(const double4* __restrict__ bodies, const double4* __restrict__ vel, const double4* __restrict__ points,
             const double4* __restrict__ point_vel, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
             uint32_t n, uint32_t m, uint32_t cap, double eps2, double G, uint32_t at_bodies, uint32_t self0,
             double4* __restrict__ accel, double4* __restrict__ jerk, double* __restrict__ phi)
{
    constexpr int LS = kLfLanes64;
    constexpr int U = kLfU;
    uint32_t trips;
    const LfRow r = lf_row<LS>(list, count, m, cap, at_bodies, self0, &trips);
    const uint32_t lane = threadIdx.x % LS;
    const double4 p = ld4(points + r.row);
    double ui = 0.0, vi = 0.0, wi = 0.0;
    if constexpr (WANT_J) { const double4 u = ld4(point_vel + r.row); ui = u.x; vi = u.y; wi = u.z; }
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0, ph = 0.0;

    uint32_t e0 = lane;
    for (uint32_t t = 0; t < trips; ++t, e0 += U * LS) {
        uint32_t j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * LS;
            const bool in = e < r.len;
            const uint32_t v = r.list[in ? e : 0u];
            ok[u] = in && v < n && v != r.own;
            j[u] = ok[u] ? v : 0u;
        }
        double4 b[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            b[u] = ld4(bodies + j[u]);
            if constexpr (WANT_J) c[u] = ld4(vel + j[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double mj = ok[u] ? b[u].w : 0.0;
            const double dx = b[u].x - p.x, dy = b[u].y - p.y, dz = b[u].z - p.z;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double s = mj * y;
            if constexpr (WANT_PHI) ph = ph + s;
            if constexpr (WANT_A || WANT_J) {
                const double y2 = y * y;
                const double s3 = s * y2;
                if constexpr (WANT_J) {
                    const double du = c[u].x - ui, dv = c[u].y - vi, dw = c[u].z - wi;
                    const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
                    const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
                    jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
                }
                if constexpr (WANT_A) { ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az); }
            }
        }
    }

    if constexpr (WANT_A) {
        const double sx = group_sum<LS>(ax), sy = group_sum<LS>(ay), sz = group_sum<LS>(az);
        if (r.store) st4(accel + r.row, double4{G * sx, G * sy, G * sz, 0.0});
    }
    if constexpr (WANT_J) {
        const double sx = group_sum<LS>(jx), sy = group_sum<LS>(jy), sz = group_sum<LS>(jz);
        if (r.store) st4(jerk + r.row, double4{G * sx, G * sy, G * sz, 0.0});
    }
    if constexpr (WANT_PHI) {
        const double sp = group_sum<LS>(ph);
        if (r.store) phi[r.row] = 0.0 - G * sp;
    }
}

}  // namespace nb
