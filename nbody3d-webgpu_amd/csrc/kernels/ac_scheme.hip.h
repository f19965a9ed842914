// kernels/ac_scheme.hip.h -- the Ahmad-Cohen neighbour scheme of a Hermite handle with two shared step levels
// (nb_set_neighbor_scheme): nb_ac_sub32 / nb_ac_sub64 (one launch per irregular substep), nb_ac_predict0, nb_ac_regular,
// nb_ac_start; and, for radii that follow a target count and the checkpoint (nb_set_neighbor_adapt, nb_upload_neighbor_scheme; at
// the end of the file): nb_ac_check, nb_ac_shrink, nb_ac_start_ad, nb_ac_regular_ad, nb_ac_restore.  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// A body's force is kept as two pairs of derivatives: (ai, ji) over the body's row of the neighbour list, re-evaluated every
// hs = dt / N_sub, and (ar0, jr0) over every other row, evaluated at the regular times t0 only and extrapolated in between,
//   a(t0 + tau) = ai + (ar0 + tau jr0)        j = ji + jr0.
// include/nbody3d_hip.h states the scheme; the numbered steps in the comments below are its steps.
//   The substep launch is nb_lf32 / nb_lf64's gather with the corrector and the next predictor in its epilogue: a group of LS lanes
// owns a body, gathers its row from the predicted pair P[s] (lf_row's shape, the loop, the masking and the order of additions of
// kernels/list_force.hip.h, restated here so that the built nb_lf* stay what they are), combines the lane sums with group_sum, and
// ONE lane of the group then corrects the body over hs and, unless this is the last substep, predicts it over the next hs into the
// OTHER predicted pair.  Launch s reads P[s] of every body and writes P[s + 1] of its own: no race inside a launch, no grid
// barrier, and a launch writes its own rows of x, v, ai, ji only.  The body's six own rows are loaded BEHIND the gather loop, by
// that one lane: held across the loop they cost it nb_lf32's occupancy (99 against 62 VGPRs, 4 waves per SIMD against 8), and
// the loop waits for its gathers.
//   All polynomial arithmetic is fp64 on the stored values; every stored value is rounded once to the handle's precision.
// No LDS, no scratch, no atomics in the substep launch; the header words (rows over cap, largest count, entries) are integer
// sums and a maximum -- exact in any order -- and are the only atomics of the scheme.
#pragma once

namespace nb {

constexpr uint32_t kAcHdrWords = 4;      // 64-bit words of the header: rows with count > cap, largest count, sum of min(count, cap), (unused)
enum { kAcOver = 0, kAcMax = 1, kAcEntries = 2 };

template <typename T> struct AcRows { typename vec4<T>::type x, v, ai, ji, ar, jr; };

// the regular derivative extrapolated to t0 + tau, and a Hermite predictor / corrector pair over h: nb_hermite_predict's and
// nb_hermite_correct's expressions
__device__ __forceinline__ double ac_reg(double tau, double ar, double jr) { return nb_fma(tau, jr, ar); }
__device__ __forceinline__ double ac_px(double h, double x0, double v0, double a0, double j0)
{
    return nb_fma(h, nb_fma(h * (1.0 / 2.0), nb_fma(h * (1.0 / 3.0), j0, a0), v0), x0);
}
__device__ __forceinline__ double ac_pv(double h, double v0, double a0, double j0) { return nb_fma(h, nb_fma(h * (1.0 / 2.0), j0, a0), v0); }

// Steps 4-6 of a substep for one body, then steps 1-2 of the next one (pxw != nullptr): s = the G-scaled list sums at the predicted
// state, in fp64.
template <typename T>
__device__ __forceinline__ void ac_finish(uint32_t row, const double (&s)[6], double tau0, double tau1, double hs,
                                          typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                          typename vec4<T>::type* __restrict__ ai, typename vec4<T>::type* __restrict__ ji,
                                          const typename vec4<T>::type* __restrict__ ar0, const typename vec4<T>::type* __restrict__ jr0,
                                          typename vec4<T>::type* __restrict__ pxw, typename vec4<T>::type* __restrict__ pvw)
{
    using V4 = typename vec4<T>::type;
    const AcRows<T> o = {ld4(x + row), ld4(v + row), ld4(ai + row), ld4(ji + row), ld4(ar0 + row), ld4(jr0 + row)};
    const V4 AI1 = V4{(T)s[0], (T)s[1], (T)s[2], (T)0}, JI1 = V4{(T)s[3], (T)s[4], (T)s[5], (T)0};      // what nb_list_force would store
    const double hh = 0.5 * hs, h12 = hs * hs * (1.0 / 12.0);
    double a1[3], j1[3], xs[3], vs[3];
    auto one = [&](int c, double X, double V, double AI, double JI, double AR, double JR, double AN, double JN) {
        const double a0 = AI + ac_reg(tau0, AR, JR), j0 = JI + JR;
        a1[c] = AN + ac_reg(tau1, AR, JR);
        j1[c] = JN + JR;
        const double vn = nb_fma(h12, j0 - j1[c], nb_fma(hh, a0 + a1[c], V));
        const double xn = nb_fma(h12, a0 - a1[c], nb_fma(hh, V + vn, X));
        xs[c] = (double)(T)xn;
        vs[c] = (double)(T)vn;
    };
    one(0, o.x.x, o.v.x, o.ai.x, o.ji.x, o.ar.x, o.jr.x, AI1.x, JI1.x);
    one(1, o.x.y, o.v.y, o.ai.y, o.ji.y, o.ar.y, o.jr.y, AI1.y, JI1.y);
    one(2, o.x.z, o.v.z, o.ai.z, o.ji.z, o.ar.z, o.jr.z, AI1.z, JI1.z);
    st4(x + row, V4{(T)xs[0], (T)xs[1], (T)xs[2], o.x.w});
    st4(v + row, V4{(T)vs[0], (T)vs[1], (T)vs[2], o.v.w});
    st4(ai + row, AI1);
    st4(ji + row, JI1);
    if (pxw) {      // wave-uniform: the next substep's a and j are this one's a1 and j1 (the same expressions on the same stored values)
        st4(pxw + row, V4{(T)ac_px(hs, xs[0], vs[0], a1[0], j1[0]), (T)ac_px(hs, xs[1], vs[1], a1[1], j1[1]),
                          (T)ac_px(hs, xs[2], vs[2], a1[2], j1[2]), o.x.w});
        st4(pvw + row, V4{(T)ac_pv(hs, vs[0], a1[0], j1[0]), (T)ac_pv(hs, vs[1], a1[1], j1[1]), (T)ac_pv(hs, vs[2], a1[2], j1[2]), o.v.w});
    }
}

// f32: nb_lf32<true, true, false>'s loop over the body's row, gathered from the predicted pair (pxr, pvr)
template <int LS>
__global__ __launch_bounds__(kBlock)
void nb_ac_sub32(const float4* __restrict__ pxr, const float4* __restrict__ pvr, const uint32_t* __restrict__ list,
                 const uint32_t* __restrict__ count, uint32_t n, uint32_t cap, float eps2, double G, float4* __restrict__ x,
                 float4* __restrict__ v, float4* __restrict__ ai, float4* __restrict__ ji, const float4* __restrict__ ar0,
                 const float4* __restrict__ jr0, double tau0, double tau1, double hs, float4* __restrict__ pxw, float4* __restrict__ pvw)
{
    static_assert(LS == kLfLanes32, "the engine sizes the grid by lf_rows");
    constexpr int U = kLfU;
    uint32_t trips;
    const LfRow r = lf_row<LS>(list, count, n, cap, 1u, 0u, &trips);
    const uint32_t lane = threadIdx.x % LS;
    const float4 p = ld4(pxr + r.row);
    const float4 uv = ld4(pvr + r.row);
    const float ui = uv.x, vi = uv.y, wi = uv.z;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, jx = 0.0f, jy = 0.0f, jz = 0.0f;

    uint32_t e0 = lane;
    for (uint32_t t = 0; t < trips; ++t, e0 += U * LS) {
        uint32_t j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * LS;
            const bool in = e < r.len;
            const uint32_t w = r.list[in ? e : 0u];                 // a slot past the row reads entry 0 and is dropped (cap >= 1)
            ok[u] = in && w < n && w != r.own;
            j[u] = ok[u] ? w : 0u;
        }
        float4 b[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            b[u] = ld4(pxr + j[u]);
            c[u] = ld4(pvr + j[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float mj = ok[u] ? b[u].w : 0.0f;
            const float dx = b[u].x - p.x, dy = b[u].y - p.y, dz = b[u].z - p.z;
            const float d2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const float y = nb_rsq(d2);
            const float s = mj * y;
            const float y2 = y * y;
            const float s3 = s * y2;                                  // m / rho^3
            const float du = c[u].x - ui, dv = c[u].y - vi, dw = c[u].z - wi;
            float rv = dx * du;
            rv = nb_fma(dy, dv, rv);
            rv = nb_fma(dz, dw, rv);
            rv = rv * y2;                                             // q = (dr.dv) / rho^2
            rv = rv * -3.0f;
            const float tx = nb_fma(rv, dx, du), ty = nb_fma(rv, dy, dv), tz = nb_fma(rv, dz, dw);      // dv - 3 q dr
            jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
            ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
        }
    }

    const double s[6] = {G * group_sum<LS>((double)ax), G * group_sum<LS>((double)ay), G * group_sum<LS>((double)az),
                         G * group_sum<LS>((double)jx), G * group_sum<LS>((double)jy), G * group_sum<LS>((double)jz)};
    if (r.store) ac_finish<float>(r.row, s, tau0, tau1, hs, x, v, ai, ji, ar0, jr0, pxw, pvw);
}

// f64 handles: nb_lf64<true, true, false>'s loop
template <int LS>
__global__ __launch_bounds__(kBlock)
void nb_ac_sub64(const double4* __restrict__ pxr, const double4* __restrict__ pvr, const uint32_t* __restrict__ list,
                 const uint32_t* __restrict__ count, uint32_t n, uint32_t cap, double eps2, double G, double4* __restrict__ x,
                 double4* __restrict__ v, double4* __restrict__ ai, double4* __restrict__ ji, const double4* __restrict__ ar0,
                 const double4* __restrict__ jr0, double tau0, double tau1, double hs, double4* __restrict__ pxw, double4* __restrict__ pvw)
{
    static_assert(LS == kLfLanes64, "the engine sizes the grid by lf_rows");
    constexpr int U = kLfU;
    uint32_t trips;
    const LfRow r = lf_row<LS>(list, count, n, cap, 1u, 0u, &trips);
    const uint32_t lane = threadIdx.x % LS;
    const double4 p = ld4(pxr + r.row);
    const double4 uv = ld4(pvr + r.row);
    const double ui = uv.x, vi = uv.y, wi = uv.z;
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;

    uint32_t e0 = lane;
    for (uint32_t t = 0; t < trips; ++t, e0 += U * LS) {
        uint32_t j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * LS;
            const bool in = e < r.len;
            const uint32_t w = r.list[in ? e : 0u];
            ok[u] = in && w < n && w != r.own;
            j[u] = ok[u] ? w : 0u;
        }
        double4 b[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            b[u] = ld4(pxr + j[u]);
            c[u] = ld4(pvr + j[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double mj = ok[u] ? b[u].w : 0.0;
            const double dx = b[u].x - p.x, dy = b[u].y - p.y, dz = b[u].z - p.z;
            const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
            const double y0 = __builtin_amdgcn_rsq(r2);
            const double e = nb_fma(-(r2 * y0), y0, 1.0);
            const double y = nb_fma(0.5 * y0, e, y0);
            const double sm = mj * y;
            const double y2 = y * y;
            const double s3 = sm * y2;
            const double du = c[u].x - ui, dv = c[u].y - vi, dw = c[u].z - wi;
            const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
            const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
            jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
            ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
        }
    }

    const double s[6] = {G * group_sum<LS>(ax), G * group_sum<LS>(ay), G * group_sum<LS>(az),
                         G * group_sum<LS>(jx), G * group_sum<LS>(jy), G * group_sum<LS>(jz)};
    if (r.store) ac_finish<double>(r.row, s, tau0, tau1, hs, x, v, ai, ji, ar0, jr0, pxw, pvw);
}

// Steps 1-2 of substep 0, for all bodies: P[0] = the predictor over hs from (x, v, ai + ar0, ji + jr0).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_predict0(const typename vec4<T>::type* __restrict__ x,
                                                        const typename vec4<T>::type* __restrict__ v,
                                                        const typename vec4<T>::type* __restrict__ ai,
                                                        const typename vec4<T>::type* __restrict__ ji,
                                                        const typename vec4<T>::type* __restrict__ ar0,
                                                        const typename vec4<T>::type* __restrict__ jr0,
                                                        typename vec4<T>::type* __restrict__ px,
                                                        typename vec4<T>::type* __restrict__ pv, uint32_t n, double hs)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    const double a0 = AI.x + ac_reg(0.0, AR.x, JR.x), a1 = AI.y + ac_reg(0.0, AR.y, JR.y), a2 = AI.z + ac_reg(0.0, AR.z, JR.z);
    const double j0 = (double)JI.x + JR.x, j1 = (double)JI.y + JR.y, j2 = (double)JI.z + JR.z;
    st4(px + il, V4{(T)ac_px(hs, X.x, V.x, a0, j0), (T)ac_px(hs, X.y, V.y, a1, j1), (T)ac_px(hs, X.z, V.z, a2, j2), X.w});
    st4(pv + il, V4{(T)ac_pv(hs, V.x, a0, j0), (T)ac_pv(hs, V.y, a1, j1), (T)ac_pv(hs, V.z, a2, j2), V.w});
}

// The header of a list build: every lane brings its row's count (0 past the rows); one atomic per wave and word.
__device__ __forceinline__ void ac_header(uint32_t c, bool in, uint32_t cap, unsigned long long* __restrict__ hdr)
{
    uint32_t over = in && c > cap ? 1u : 0u, mx = in ? c : 0u, sum = in ? (c < cap ? c : cap) : 0u;      // (cap <= 4096: 64 rows fit a word)
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        over += (uint32_t)__shfl_xor((int)over, w, 64);
        sum += (uint32_t)__shfl_xor((int)sum, w, 64);
        const uint32_t t = (uint32_t)__shfl_xor((int)mx, w, 64);
        mx = t > mx ? t : mx;
    }
    if (threadIdx.x % 64 == 0) {
        if (over) atomicAdd(hdr + kAcOver, (unsigned long long)over);
        if (mx) atomicMax(hdr + kAcMax, (unsigned long long)mx);
        if (sum) atomicAdd(hdr + kAcEntries, (unsigned long long)sum);
    }
}

// The start: the totals nb_download / nb_download_jerk return (ai + ar0, ji + jr0: summed in fp64, rounded once) and the header.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_start(const typename vec4<T>::type* __restrict__ ai,
                                                     const typename vec4<T>::type* __restrict__ ji,
                                                     const typename vec4<T>::type* __restrict__ ar0,
                                                     const typename vec4<T>::type* __restrict__ jr0,
                                                     typename vec4<T>::type* __restrict__ acc,
                                                     typename vec4<T>::type* __restrict__ jerk, const uint32_t* __restrict__ count,
                                                     unsigned long long* __restrict__ hdr, uint32_t n, uint32_t cap)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    const bool in = il < n;
    const uint32_t ic = in ? il : n - 1;
    ac_header(count[ic], in, cap, hdr);
    if (!in) return;
    const auto AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    st4(acc + il, V4{(T)((double)AI.x + AR.x), (T)((double)AI.y + AR.y), (T)((double)AI.z + AR.z), (T)0});
    st4(jerk + il, V4{(T)((double)JI.x + JR.x), (T)((double)JI.y + JR.y), (T)((double)JI.z + JR.z), (T)0});
}

// The regular time, steps 4-7, on the arrived state: (aip, jip, arp, jrp) are nb_split_force's outputs there, (aio, jio) the sums
// over the OLD list there.  aro = (arp + aip) - aio is the regular force with respect to the old list; only its difference from
// ar0 enters, scaled by dt^2: the difference between the Hermite corrector and the Hermite predictor over dt.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_regular(typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                       const typename vec4<T>::type* __restrict__ aip,
                                                       const typename vec4<T>::type* __restrict__ jip,
                                                       const typename vec4<T>::type* __restrict__ arp,
                                                       const typename vec4<T>::type* __restrict__ jrp,
                                                       const typename vec4<T>::type* __restrict__ aio,
                                                       const typename vec4<T>::type* __restrict__ jio,
                                                       typename vec4<T>::type* __restrict__ ar0, typename vec4<T>::type* __restrict__ jr0,
                                                       typename vec4<T>::type* __restrict__ acc, typename vec4<T>::type* __restrict__ jerk,
                                                       const uint32_t* __restrict__ count, unsigned long long* __restrict__ hdr,
                                                       uint32_t n, uint32_t cap, double dt)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    const bool in = il < n;
    const uint32_t ic = in ? il : n - 1;
    ac_header(count[ic], in, cap, hdr);
    if (!in) return;
    const auto X = ld4(x + il), V = ld4(v + il), AIP = ld4(aip + il), JIP = ld4(jip + il), ARP = ld4(arp + il), JRP = ld4(jrp + il);
    const auto AIO = ld4(aio + il), JIO = ld4(jio + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    const double c1 = dt * 0.5, c2 = dt * dt * (1.0 / 12.0), c3 = dt * dt * (1.0 / 6.0), c4 = dt * dt * dt * (1.0 / 24.0);
    double xn[3], vn[3], at[3], jt[3];
    auto one = [&](int c, double X0, double V0, double aip_, double jip_, double arp_, double jrp_, double aio_, double jio_, double ar, double jr) {
        at[c] = arp_ + aip_;
        jt[c] = jrp_ + jip_;
        const double da = (at[c] - aio_) - ar, jro = jt[c] - jio_;
        vn[c] = V0 + (c1 * da - c2 * (5.0 * jr + jro));
        xn[c] = X0 + (c3 * da - c4 * (3.0 * jr + jro));
    };
    one(0, X.x, V.x, AIP.x, JIP.x, ARP.x, JRP.x, AIO.x, JIO.x, AR.x, JR.x);
    one(1, X.y, V.y, AIP.y, JIP.y, ARP.y, JRP.y, AIO.y, JIO.y, AR.y, JR.y);
    one(2, X.z, V.z, AIP.z, JIP.z, ARP.z, JRP.z, AIO.z, JIO.z, AR.z, JR.z);
    st4(x + il, V4{(T)xn[0], (T)xn[1], (T)xn[2], X.w});
    st4(v + il, V4{(T)vn[0], (T)vn[1], (T)vn[2], V.w});
    st4(ar0 + il, V4{ARP.x, ARP.y, ARP.z, (T)0});
    st4(jr0 + il, V4{JRP.x, JRP.y, JRP.z, (T)0});
    st4(acc + il, V4{(T)at[0], (T)at[1], (T)at[2], (T)0});
    st4(jerk + il, V4{(T)jt[0], (T)jt[1], (T)jt[2], (T)0});
}

// ---- radii that follow a target count (nb_set_neighbor_adapt) ----------------------------------------------------------------------
// With adaptation on a build is cut by `next`; its header comes from nb_ac_check, so that the host can have the overflowed rows
// shrunk (nb_ac_shrink) and the pass repeated BEFORE the correction moves x and v.  nb_ac_start_ad / nb_ac_regular_ad are the
// parents without the header, followed by the rule on the accepted counts.  A handle on which adaptation is off launches none of these
// (nb_ac_restore: nb_upload_neighbor_scheme, with adaptation on or off).
struct AcRule { double nt, gmax, rmin, rmax; };      // the target count, the largest factor per build (the smallest: 1 / gmax), the clamps (0: none)

// The rule, steps 1-6 of the header: all fp64, rounded once by the caller; a radius of exactly 0 stays 0.
__device__ __forceinline__ double ac_rule(double h, uint32_t c, const AcRule& r)
{
    if (h == 0.0) return 0.0;
    double f = cbrt((r.nt + 0.5) / ((double)c + 0.5));
    f = fmin(fmax(f, 1.0 / r.gmax), r.gmax);
    double hn = h * f;
    if (r.rmin > 0.0) hn = fmax(hn, r.rmin);
    if (r.rmax > 0.0) hn = fmin(hn, r.rmax);
    return hn;
}

// The header of a build from the counts alone.  (A template as nb_spl_rows<>: the header is part of more than one translation unit.)
template <int B = kBlock>
__global__ __launch_bounds__(B) void nb_ac_check(const uint32_t* __restrict__ count, unsigned long long* __restrict__ hdr, uint32_t n, uint32_t cap)
{
    const uint32_t il = blockIdx.x * B + threadIdx.x;
    const bool in = il < n;
    const uint32_t ic = in ? il : n - 1;
    ac_header(count[ic], in, cap, hdr);
}

// The rows of an overflowed build alone: h <- rnd(h cbrt(n_t / c)), c the row's count (> cap >= 2 n_t: at most cbrt(1/2) h).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_shrink(T* __restrict__ next, const uint32_t* __restrict__ count, uint32_t n, uint32_t cap, double nt)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const uint32_t c = count[il];
    if (c > cap) next[il] = (T)((double)next[il] * cbrt(nt / (double)c));
}

// nb_ac_start's totals, then built <- the radii of the accepted pass and next <- the rule on its counts.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_start_ad(const typename vec4<T>::type* __restrict__ ai,
                                                        const typename vec4<T>::type* __restrict__ ji,
                                                        const typename vec4<T>::type* __restrict__ ar0,
                                                        const typename vec4<T>::type* __restrict__ jr0,
                                                        typename vec4<T>::type* __restrict__ acc,
                                                        typename vec4<T>::type* __restrict__ jerk, const uint32_t* __restrict__ count,
                                                        T* __restrict__ built, T* __restrict__ next, uint32_t n, AcRule rule)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    st4(acc + il, V4{(T)((double)AI.x + AR.x), (T)((double)AI.y + AR.y), (T)((double)AI.z + AR.z), (T)0});
    st4(jerk + il, V4{(T)((double)JI.x + JR.x), (T)((double)JI.y + JR.y), (T)((double)JI.z + JR.z), (T)0});
    const T h = next[il];
    built[il] = h;
    next[il] = (T)ac_rule((double)h, count[il], rule);
}

// nb_upload_neighbor_scheme: the totals of uploaded components (nb_ac_start's expression), nothing else.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_restore(const typename vec4<T>::type* __restrict__ ai,
                                                       const typename vec4<T>::type* __restrict__ ji,
                                                       const typename vec4<T>::type* __restrict__ ar0,
                                                       const typename vec4<T>::type* __restrict__ jr0,
                                                       typename vec4<T>::type* __restrict__ acc,
                                                       typename vec4<T>::type* __restrict__ jerk, uint32_t n)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    st4(acc + il, V4{(T)((double)AI.x + AR.x), (T)((double)AI.y + AR.y), (T)((double)AI.z + AR.z), (T)0});
    st4(jerk + il, V4{(T)((double)JI.x + JR.x), (T)((double)JI.y + JR.y), (T)((double)JI.z + JR.z), (T)0});
}

// nb_ac_regular's steps 4-7, expression for expression, on an ACCEPTED list (its header was read in front of this launch), then the
// rule as in nb_ac_start_ad.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_regular_ad(typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                          const typename vec4<T>::type* __restrict__ aip,
                                                          const typename vec4<T>::type* __restrict__ jip,
                                                          const typename vec4<T>::type* __restrict__ arp,
                                                          const typename vec4<T>::type* __restrict__ jrp,
                                                          const typename vec4<T>::type* __restrict__ aio,
                                                          const typename vec4<T>::type* __restrict__ jio,
                                                          typename vec4<T>::type* __restrict__ ar0, typename vec4<T>::type* __restrict__ jr0,
                                                          typename vec4<T>::type* __restrict__ acc, typename vec4<T>::type* __restrict__ jerk,
                                                          const uint32_t* __restrict__ count, T* __restrict__ built, T* __restrict__ next,
                                                          uint32_t n, double dt, AcRule rule)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const auto X = ld4(x + il), V = ld4(v + il), AIP = ld4(aip + il), JIP = ld4(jip + il), ARP = ld4(arp + il), JRP = ld4(jrp + il);
    const auto AIO = ld4(aio + il), JIO = ld4(jio + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    const double c1 = dt * 0.5, c2 = dt * dt * (1.0 / 12.0), c3 = dt * dt * (1.0 / 6.0), c4 = dt * dt * dt * (1.0 / 24.0);
    double xn[3], vn[3], at[3], jt[3];
    auto one = [&](int c, double X0, double V0, double aip_, double jip_, double arp_, double jrp_, double aio_, double jio_, double ar, double jr) {
        at[c] = arp_ + aip_;
        jt[c] = jrp_ + jip_;
        const double da = (at[c] - aio_) - ar, jro = jt[c] - jio_;
        vn[c] = V0 + (c1 * da - c2 * (5.0 * jr + jro));
        xn[c] = X0 + (c3 * da - c4 * (3.0 * jr + jro));
    };
    one(0, X.x, V.x, AIP.x, JIP.x, ARP.x, JRP.x, AIO.x, JIO.x, AR.x, JR.x);
    one(1, X.y, V.y, AIP.y, JIP.y, ARP.y, JRP.y, AIO.y, JIO.y, AR.y, JR.y);
    one(2, X.z, V.z, AIP.z, JIP.z, ARP.z, JRP.z, AIO.z, JIO.z, AR.z, JR.z);
    st4(x + il, V4{(T)xn[0], (T)xn[1], (T)xn[2], X.w});
    st4(v + il, V4{(T)vn[0], (T)vn[1], (T)vn[2], V.w});
    st4(ar0 + il, V4{ARP.x, ARP.y, ARP.z, (T)0});
    st4(jr0 + il, V4{JRP.x, JRP.y, JRP.z, (T)0});
    st4(acc + il, V4{(T)at[0], (T)at[1], (T)at[2], (T)0});
    st4(jerk + il, V4{(T)jt[0], (T)jt[1], (T)jt[2], (T)0});
    const T h = next[il];
    built[il] = h;
    next[il] = (T)ac_rule((double)h, count[il], rule);
}

}  // namespace nb
