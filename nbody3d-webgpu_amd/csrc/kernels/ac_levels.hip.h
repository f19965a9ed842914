// kernels/ac_levels.hip.h -- block individual IRREGULAR steps of the Ahmad-Cohen neighbour scheme (nb_set_neighbor_levels):
// nb_ac_lv_start, nb_ac_lv_begin, nb_ac_lv_sub32 / nb_ac_lv_sub64.  No reference analogue.  Part of nb_kernels.hip.h (include that,
// not this file).
//
// Time between two regular times is counted in ticks of dt / 2^L, L = log2(N_sub) of the scheme.  Body i holds a level l_i in
// [lmin, L], steps by s_i = 2^(L - l_i) ticks, its stored (x, v, ai, ji) belong to the tick t_i = due_i - s_i; (ar0, jr0) belong to
// tick 0 as ever.  include/nbody3d_hip.h states the steps; the numbers in the comments below are its numbers.
//   The host does not know which ticks have a due body, and must not wait to learn it: it enqueues ONE launch for EVERY tick
// k = 1 .. 2^L, as the shared scheme enqueues one per substep, and launch k leaves at once where neither tick[k] nor tick[k + 1] is
// set.  The words tick[0 .. 2^L + 1] are zeroed by one memset in front of nb_ac_lv_begin, which starts the clock (due_i = s_i,
// tick[s_i] = 1) and predicts every body to T(1) into the predicted pair P[1].
//   nb_ac_lv_sub*(k) is nb_ac_sub*'s launch with the schedule in it: a group of LS lanes owns a body (the grid covers all n).  A body
// with due_i == k is gathered over its row from P[k & 1] with nb_ac_sub*'s loop -- restated here, so that the built nb_ac_sub* and
// nb_lf* stay what they are --, a body that is not due has a row of length 0 (a wave without a due body skips the loop).  ONE lane of
// the group then, for a due body, corrects it over its own h (step 4), decides its next level (step 5), stores (x, v, ai, ji), the
// level and due_i and sets tick[due_i]; and for EVERY body it predicts the body from its stored state (the one it has just stored,
// or the one of t_i) to T(k + 1) into P[(k + 1) & 1] (step 2 of the next tick: always from the stored state, never from an earlier
// prediction).  Launch k reads P[k & 1] of every body and writes P[(k + 1) & 1] and the rows of its own: no race, no grid barrier,
// no active list.  tick[k + 1] is read only where tick[k] == 0, and then this launch writes no tick[]: a body due at k + 1 was
// scheduled either by this launch (tick[k] != 0: it predicts) or by an earlier one (tick[k + 1] was set before this launch began).
//   The counters are kept PER BODY (four 64-bit words a body's one storing lane adds to with plain loads and stores, summed by the
// host when the stats are asked for): a device-wide counter takes one atomic per wave and word on ONE address from n / 4 waves per
// tick, and those serialise -- measured at 0.6 ms per all-due tick at N = 65,536 against 0.03 ms for the whole shared substep launch.
// The only atomic left is one integer add per tick with a due body (block_steps).
//   No LDS, no scratch, no floating-point atomics.
#pragma once

namespace nb {

// the counters of nb_neighbor_level_stats that live on the device (64-bit words): per handle the ticks with a due body, per body
// a record of kLvRecWords words
enum { kLvBlockSteps = 0, kLvCntWords = 2 };
enum { kLvBodySteps = 0, kLvEntries = 1, kLvClamped = 2, kLvFinest = 3, kLvRecWords = 4 };
// the words of one regular step: tick[0 .. 2^L + 1] (tick[k] != 0: a body is due at tick k; tick[2^L + 1] stays 0)
__host__ __device__ constexpr uint32_t lv_words(uint32_t nsub) { return nsub + 2u; }

struct LvCfg { uint32_t L, lmin, frozen, nsub; double eta, dt, tick; };

// blk_level_for without its atomic: the smallest l in [lmin, L] with dt / 2^l <= tau; none: L, *clamped = 1
__device__ __forceinline__ uint32_t lv_level_for(double tau, double dt, uint32_t lmin, uint32_t L, uint32_t* clamped)
{
    for (uint32_t l = lmin; l <= L; ++l)
        if (__builtin_ldexp(dt, -(int)l) <= tau) return l;
    *clamped = 1u;
    return L;
}

// a body's own record, by its one storing lane (sums; the finest level it held)
__device__ __forceinline__ void lv_record(unsigned long long* __restrict__ rec, uint32_t row, uint32_t steps, uint32_t entries,
                                          uint32_t clamped, uint32_t level)
{
    unsigned long long* __restrict__ r = rec + (size_t)row * kLvRecWords;
    const unsigned long long a = r[kLvBodySteps], b = r[kLvEntries], c = r[kLvClamped], d = r[kLvFinest];
    r[kLvBodySteps] = a + steps;
    r[kLvEntries] = b + entries;
    r[kLvClamped] = c + clamped;
    r[kLvFinest] = level > d ? (unsigned long long)level : d;
}

// The start of the levels.  mode 0: l_i = level_for((eta / 2) |a| / |j|) on a = ai + ar0, j = ji + jr0 (fp64 sums of the stored
// components), |j| = 0 -> lmin; mode 1 (frozen): lmin; mode 2: the levels were uploaded and are kept (counted into finest_level).
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_lv_start(const typename vec4<T>::type* __restrict__ ai,
                                                        const typename vec4<T>::type* __restrict__ ji,
                                                        const typename vec4<T>::type* __restrict__ ar0,
                                                        const typename vec4<T>::type* __restrict__ jr0, uint8_t* __restrict__ lev,
                                                        unsigned long long* __restrict__ rec, uint32_t n, int mode, LvCfg c)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    uint32_t l = c.lmin, clamped = 0;
    if (mode == 2) l = lev[il];
    else if (mode == 0) {
        const auto AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
        const double ax = (double)AI.x + AR.x, ay = (double)AI.y + AR.y, az = (double)AI.z + AR.z;
        const double jx = (double)JI.x + JR.x, jy = (double)JI.y + JR.y, jz = (double)JI.z + JR.z;
        const double aa = __builtin_sqrt(ax * ax + ay * ay + az * az), jj = __builtin_sqrt(jx * jx + jy * jy + jz * jz);
        if (jj > 0.0) l = lv_level_for(0.5 * c.eta * aa / jj, c.dt, c.lmin, c.L, &clamped);
    }
    lev[il] = (uint8_t)l;
    lv_record(rec, il, 0u, 0u, clamped, l);
}

// The clock of a regular step: t_i = 0, due_i = s_i, tick[s_i] = 1 (plain stores of the same value: exact in any order; the words
// were zeroed in front of this launch), and step 2 of tick 1 for every body: nb_ac_predict0's expressions over one tick.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_ac_lv_begin(const typename vec4<T>::type* __restrict__ x,
                                                        const typename vec4<T>::type* __restrict__ v,
                                                        const typename vec4<T>::type* __restrict__ ai,
                                                        const typename vec4<T>::type* __restrict__ ji,
                                                        const typename vec4<T>::type* __restrict__ ar0,
                                                        const typename vec4<T>::type* __restrict__ jr0,
                                                        typename vec4<T>::type* __restrict__ px,
                                                        typename vec4<T>::type* __restrict__ pv, const uint8_t* __restrict__ lev,
                                                        uint32_t* __restrict__ due, uint32_t* __restrict__ tick, uint32_t n, LvCfg c)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const uint32_t l = lev[il], s = 1u << (c.L - (l < c.L ? l : c.L));      // (a level is never above L: the clamp keeps the index inside tick[])
    due[il] = s;
    tick[s] = 1u;
    const double h = (double)1u * c.tick;
    const auto X = ld4(x + il), V = ld4(v + il), AI = ld4(ai + il), JI = ld4(ji + il), AR = ld4(ar0 + il), JR = ld4(jr0 + il);
    const double a0 = AI.x + ac_reg(0.0, AR.x, JR.x), a1 = AI.y + ac_reg(0.0, AR.y, JR.y), a2 = AI.z + ac_reg(0.0, AR.z, JR.z);
    const double j0 = (double)JI.x + JR.x, j1 = (double)JI.y + JR.y, j2 = (double)JI.z + JR.z;
    st4(px + il, V4{(T)ac_px(h, X.x, V.x, a0, j0), (T)ac_px(h, X.y, V.y, a1, j1), (T)ac_px(h, X.z, V.z, a2, j2), X.w});
    st4(pv + il, V4{(T)ac_pv(h, V.x, a0, j0), (T)ac_pv(h, V.y, a1, j1), (T)ac_pv(h, V.z, a2, j2), V.w});
}

// lf_row with the schedule: the group's body, its row's length (0 when the body is not due at tick k) and the wave's trip count
template <int LS>
__device__ __forceinline__ LfRow lv_row(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                        const uint32_t* __restrict__ due, bool run, uint32_t k, uint32_t n, uint32_t cap, bool* is_due,
                                        uint32_t* trips)
{
    const uint32_t r = blockIdx.x * (kBlock / LS) + threadIdx.x / LS;
    LfRow o;
    o.row = r < n ? r : n - 1;                                    // clamped, branch-free (never stored)
    o.store = r < n && threadIdx.x % LS == 0;
    o.list = list + (size_t)o.row * cap;
    *is_due = run && due[o.row] == k;
    const uint32_t c = count[o.row];
    o.len = *is_due ? (c < cap ? c : cap) : 0u;
    o.own = o.row;
    uint32_t longest = o.len;
#pragma unroll
    for (int w = LS; w < 64; w <<= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)longest, w, 64); longest = t > longest ? t : longest; }
    longest = __builtin_amdgcn_readfirstlane(longest);
    *trips = (longest + (uint32_t)(kLfU * LS) - 1) / (uint32_t)(kLfU * LS);
    return o;
}

// The one storing lane of a body at tick k.  A due body: steps 4-6 -- s = the G-scaled list sums at the predicted state, in fp64; the
// corrector is ac_finish's, expression for expression; the criterion and the level rule are nb_blk_correct's on the fp64 TOTALS.
// Every body (pxw != nullptr): step 2 of tick k + 1 from the stored state.
template <typename T>
__device__ __forceinline__ void lv_finish(bool is_due, uint32_t row, uint32_t len, const double (&s)[6], uint32_t k, const LvCfg& c,
                                          typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                          typename vec4<T>::type* __restrict__ ai, typename vec4<T>::type* __restrict__ ji,
                                          const typename vec4<T>::type* __restrict__ ar0, const typename vec4<T>::type* __restrict__ jr0,
                                          uint8_t* __restrict__ lev, uint32_t* __restrict__ due, uint32_t* __restrict__ tick,
                                          unsigned long long* __restrict__ rec, typename vec4<T>::type* __restrict__ pxw,
                                          typename vec4<T>::type* __restrict__ pvw)
{
    using V4 = typename vec4<T>::type;
    const AcRows<T> o = {ld4(x + row), ld4(v + row), ld4(ai + row), ld4(ji + row), ld4(ar0 + row), ld4(jr0 + row)};
    const uint32_t l = lev[row], s_i = 1u << (c.L - l);
    // the state the next prediction starts from, and its tick
    double X[3] = {o.x.x, o.x.y, o.x.z}, V[3] = {o.v.x, o.v.y, o.v.z}, AI[3] = {o.ai.x, o.ai.y, o.ai.z}, JI[3] = {o.ji.x, o.ji.y, o.ji.z};
    const double AR[3] = {o.ar.x, o.ar.y, o.ar.z}, JR[3] = {o.jr.x, o.jr.y, o.jr.z};
    uint32_t t_from = due[row] - s_i;
    if (is_due) {
        const double hs = (double)s_i * c.tick, tau0 = (double)(k - s_i) * c.tick, tau1 = tau0 + hs;
        const V4 AI1 = V4{(T)s[0], (T)s[1], (T)s[2], (T)0}, JI1 = V4{(T)s[3], (T)s[4], (T)s[5], (T)0};      // what nb_list_force would store
        const double AN[3] = {AI1.x, AI1.y, AI1.z}, JN[3] = {JI1.x, JI1.y, JI1.z};
        const double hh = 0.5 * hs, h12 = hs * hs * (1.0 / 12.0);
        double a0[3], j0[3], a1[3], j1[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            a0[q] = AI[q] + ac_reg(tau0, AR[q], JR[q]);
            j0[q] = JI[q] + JR[q];
            a1[q] = AN[q] + ac_reg(tau1, AR[q], JR[q]);
            j1[q] = JN[q] + JR[q];
            const double vn = nb_fma(h12, j0[q] - j1[q], nb_fma(hh, a0[q] + a1[q], V[q]));
            const double xn = nb_fma(h12, a0[q] - a1[q], nb_fma(hh, V[q] + vn, X[q]));
            X[q] = (double)(T)xn;
            V[q] = (double)(T)vn;
            AI[q] = AN[q];
            JI[q] = JN[q];
        }
        st4(x + row, V4{(T)X[0], (T)X[1], (T)X[2], o.x.w});
        st4(v + row, V4{(T)V[0], (T)V[1], (T)V[2], o.v.w});
        st4(ai + row, AI1);
        st4(ji + row, JI1);

        uint32_t clamped = 0, ln = l;
        if (!c.frozen) {
            const double h = hs, hq = h * h, hc = hq * h;
            auto d2 = [&](int q) { return (-6.0 * (a0[q] - a1[q]) - h * (4.0 * j0[q] + 2.0 * j1[q])) / hq; };
            auto d3 = [&](int q) { return (12.0 * (a0[q] - a1[q]) + 6.0 * h * (j0[q] + j1[q])) / hc; };
            const double a3x = d3(0), a3y = d3(1), a3z = d3(2);
            const double ex = d2(0) + h * a3x, ey = d2(1) + h * a3y, ez = d2(2) + h * a3z;
            auto nrm = [](double p, double q, double r) { return __builtin_sqrt(p * p + q * q + r * r); };
            const double n1 = nrm(a1[0], a1[1], a1[2]), nj = nrm(j1[0], j1[1], j1[2]), n2 = nrm(ex, ey, ez), n3 = nrm(a3x, a3y, a3z);
            const double den = nj * n3 + n2 * n2;
            // an empty row has no irregular force to resolve: tau = inf, the coarsest level
            const double tau = (len == 0u || den == 0.0) ? __builtin_inf() : __builtin_sqrt(c.eta * (n1 * n2 + nj * nj) / den);
            const uint32_t want = lv_level_for(tau, c.dt, c.lmin, c.L, &clamped);
            if (want >= l) ln = want;
            else if ((k & (2u * s_i - 1u)) == 0u) ln = l - 1;
            lev[row] = (uint8_t)ln;
        }
        if (k < c.nsub) {                      // at tick 2^L every body stands at the regular time: the next nb_ac_lv_begin starts the clock
            const uint32_t d = k + (1u << (c.L - ln));
            due[row] = d;
            if (d <= c.nsub) tick[d] = 1u;      // (always: a step never crosses the regular time; the test keeps the store inside tick[])
        }
        lv_record(rec, row, 1u, len, clamped, ln);
        t_from = k;
    }
    if (pxw) {      // wave-uniform
        const double tau = (double)t_from * c.tick, h = (double)(k + 1u - t_from) * c.tick;
        double a[3], j[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            a[q] = AI[q] + ac_reg(tau, AR[q], JR[q]);
            j[q] = JI[q] + JR[q];
        }
        st4(pxw + row, V4{(T)ac_px(h, X[0], V[0], a[0], j[0]), (T)ac_px(h, X[1], V[1], a[1], j[1]), (T)ac_px(h, X[2], V[2], a[2], j[2]), o.x.w});
        st4(pvw + row, V4{(T)ac_pv(h, V[0], a[0], j[0]), (T)ac_pv(h, V[1], a[1], j[1]), (T)ac_pv(h, V[2], a[2], j[2]), o.v.w});
    }
}

// f32: nb_ac_sub32's loop over the rows of the bodies due at tick k
template <int LS>
__global__ __launch_bounds__(kBlock)
void nb_ac_lv_sub32(const float4* __restrict__ pxr, const float4* __restrict__ pvr, const uint32_t* __restrict__ list,
                    const uint32_t* __restrict__ count, uint32_t* __restrict__ tick, unsigned long long* __restrict__ cnt,
                    unsigned long long* __restrict__ rec, uint32_t n, uint32_t cap, float eps2, double G, float4* __restrict__ x,
                    float4* __restrict__ v, float4* __restrict__ ai, float4* __restrict__ ji, const float4* __restrict__ ar0,
                    const float4* __restrict__ jr0, uint8_t* __restrict__ lev, uint32_t* __restrict__ due, uint32_t k, LvCfg cfg,
                    float4* __restrict__ pxw, float4* __restrict__ pvw)
{
    static_assert(LS == kLfLanes32, "the engine sizes the grid by lf_rows");
    constexpr int U = kLfU;
    const bool run = tick[k] != 0u;
    if (!run && tick[k + 1u] == 0u) return;                         // nobody is due now, and nobody at the next tick (uniform over the launch)
    if (run && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(cnt + kLvBlockSteps, 1ull);
    uint32_t trips;
    bool is_due;
    const LfRow r = lv_row<LS>(list, count, due, run, k, n, cap, &is_due, &trips);
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
    if (r.store) lv_finish<float>(is_due, r.row, r.len, s, k, cfg, x, v, ai, ji, ar0, jr0, lev, due, tick, rec, pxw, pvw);
}

// f64 handles: nb_ac_sub64's loop
template <int LS>
__global__ __launch_bounds__(kBlock)
void nb_ac_lv_sub64(const double4* __restrict__ pxr, const double4* __restrict__ pvr, const uint32_t* __restrict__ list,
                    const uint32_t* __restrict__ count, uint32_t* __restrict__ tick, unsigned long long* __restrict__ cnt,
                    unsigned long long* __restrict__ rec, uint32_t n, uint32_t cap, double eps2, double G, double4* __restrict__ x,
                    double4* __restrict__ v, double4* __restrict__ ai, double4* __restrict__ ji, const double4* __restrict__ ar0,
                    const double4* __restrict__ jr0, uint8_t* __restrict__ lev, uint32_t* __restrict__ due, uint32_t k, LvCfg cfg,
                    double4* __restrict__ pxw, double4* __restrict__ pvw)
{
    static_assert(LS == kLfLanes64, "the engine sizes the grid by lf_rows");
    constexpr int U = kLfU;
    const bool run = tick[k] != 0u;
    if (!run && tick[k + 1u] == 0u) return;
    if (run && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(cnt + kLvBlockSteps, 1ull);
    uint32_t trips;
    bool is_due;
    const LfRow r = lv_row<LS>(list, count, due, run, k, n, cap, &is_due, &trips);
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
    if (r.store) lv_finish<double>(is_due, r.row, r.len, s, k, cfg, x, v, ai, ji, ar0, jr0, lev, due, tick, rec, pxw, pvw);
}

}  // namespace nb
