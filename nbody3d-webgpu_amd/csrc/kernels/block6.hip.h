// kernels/block6.hip.h -- block individual time steps on 6th-order Hermite handles (nb_set_block_steps6; Nitadori & Makino 2008, the
// production setup of phi-GPU).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// The scheme of kernels/block.hip.h -- ticks, levels, due_i, the active list, the header, nb_blk_sched and nb_blk_start are that
// file's, unchanged; nb_blk6_start is the two-rule start of nb_set_start6 -- with the order-6 state (x, v, a, j, s, c) per body.
// One block step, with the launches the host makes of it:
//   nb_blk_sched        as for order 4
//   nb_blk6_predict     every body from its own state over (t_next - t_i) ticks into xp, vp, ap (nb_h6_predict's polynomials)
//   (the host reads the header: |A| sizes the next launches)
//   nb_blk6_fjs_pk/64   |A| x N ordered pairs of force, jerk and snap: the i-rows gathered through the list, compact partial rows
//   nb_blk6_correct     chunk sums in fp64, nb_h6_correct's corrector and crackle over h = s_i ticks, the order-6 step criterion, new
//                       level, due_i
// Nothing here adds floating-point numbers in an order that depends on timing: the chunk rows are added in ascending order, the only
// atomics are the integer count of clamped decisions and the maximum of the levels.
#pragma once

namespace nb {

// nb_blk_start with the two-rule start of nb_set_start6(NB_START6_CRACKLE), on the stored (a, j, s, c) in fp64.  Mode 0:
//   l_i = max(level_for((eta / 2) |a| / |j|), level_for(sqrt(eta (|a| |s| + |j|^2) / (|j| |c| + |s|^2))))
// a rule whose denominator is 0 votes lmin; a body counts ONCE as clamped when either rule found no level.  Modes 1 (frozen) and 2
// (uploaded levels) are nb_blk_start's.  Every mode starts the outer step's clock: due_i = s_i.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk6_start(const typename vec4<T>::type* __restrict__ a,
                                                       const typename vec4<T>::type* __restrict__ j,
                                                       const typename vec4<T>::type* __restrict__ s,
                                                       const typename vec4<T>::type* __restrict__ c, uint8_t* __restrict__ lev,
                                                       uint32_t* __restrict__ due, uint32_t* __restrict__ hdr, uint32_t n, int mode,
                                                       double eta, double dt, uint32_t lmin, uint32_t L)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    uint32_t l = lmin;
    if (mode == 2) l = lev[il];
    else if (mode == 0) {
        const auto A = ld4(a + il), J = ld4(j + il), S = ld4(s + il), C = ld4(c + il);
        auto nrm = [](double p, double q, double r) { return __builtin_sqrt(p * p + q * q + r * r); };
        const double aa = nrm(A.x, A.y, A.z), jj = nrm(J.x, J.y, J.z), ss = nrm(S.x, S.y, S.z), cc = nrm(C.x, C.y, C.z);
        uint32_t clamped = 0, l1 = lmin, l2 = lmin;
        if (jj > 0.0) l1 = lv_level_for(0.5 * eta * aa / jj, dt, lmin, L, &clamped);
        const double den = jj * cc + ss * ss;
        if (den > 0.0) l2 = lv_level_for(__builtin_sqrt(eta * (aa * ss + jj * jj) / den), dt, lmin, L, &clamped);
        l = l1 > l2 ? l1 : l2;
        if (clamped) atomicAdd(hdr + kBlkClamped, 1u);
    }
    lev[il] = (uint8_t)l;
    due[il] = 1u << (L - l);
    atomicMax(hdr + kBlkFinest, l);
}

// nb_h6_predict with a step of the body's own: h_i = (t_next - t_i) ticks, t_i = due_i - s_i.  Always from the stored state, never
// from an earlier prediction.  t_next is read from the device header: the launch follows nb_blk_sched without the host in between.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk6_predict(const typename vec4<T>::type* __restrict__ x,
                                                         const typename vec4<T>::type* __restrict__ v,
                                                         const typename vec4<T>::type* __restrict__ a,
                                                         const typename vec4<T>::type* __restrict__ j,
                                                         const typename vec4<T>::type* __restrict__ s,
                                                         const typename vec4<T>::type* __restrict__ c,
                                                         const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                         typename vec4<T>::type* __restrict__ xp,
                                                         typename vec4<T>::type* __restrict__ vp,
                                                         typename vec4<T>::type* __restrict__ ap, uint32_t n,
                                                         const uint32_t* __restrict__ hdr, uint32_t L, double tick)
{
    using V4 = typename vec4<T>::type;
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

// The force+jerk+snap pass of the na active bodies against all n predicted rows: nb_h6_fjs_pk's / nb_h6_fjs64's body
// (kernels/hermite6.hip.h) with the i-rows gathered through act[] and compact partial rows (row k of chunk c, at pa[c * na + k],
// belongs to act[k]).  An active body's own row is read from the same arrays as the j-rows: all nine self terms are exactly 0.
// Lanes past na clamp to the last active body and store nothing.  NG = 2: 1,024 rows per workgroup, NG = 1: 512.
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_H6_WAVES, NB_H6_WAVES)))
void nb_blk6_fjs_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const float4* __restrict__ acc,
                    const uint32_t* __restrict__ act, uint32_t na, float4* __restrict__ pa, float4* __restrict__ pj,
                    float4* __restrict__ ps, uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    h6_fjs_pk_body<NG, true>(pos, vel, acc, act, na, pa, pj, ps, n, j_per_chunk, eps2, zero_row);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk6_fjs64(const typename vec4<T>::type* __restrict__ pos,
                                                       const typename vec4<T>::type* __restrict__ vel,
                                                       const typename vec4<T>::type* __restrict__ acc,
                                                       const uint32_t* __restrict__ act, uint32_t na, double4* __restrict__ pa,
                                                       double4* __restrict__ pj, double4* __restrict__ ps, uint32_t n,
                                                       uint32_t j_per_chunk, double eps2)
{
    h6_fjs64_body<T, true>(pos, vel, acc, act, na, pa, pj, ps, n, j_per_chunk, eps2);
}

// For k < na, body i = act[k]: (a1, j1, s1) = G x the chunk rows added in ascending order in fp64 (as nb_h6_reduce), rounded to the
// handle's precision; nb_h6_correct's corrector and crackle over h = s_i ticks,
//   P = a1 - a - h j - h^2/2 s,  Q = h (j1 - j - h s),  R = h^2 (s1 - s),  c1 = (60 P - 36 Q + 9 R) / h^3
// then, unless frozen, the step criterion on what was stored, from the same P, Q, R:
//   a4 = (360 P - 192 Q + 36 R) / h^4          a5 = (720 P - 360 Q + 60 R) / h^5          (the quintic's derivatives at the step's end)
//   tau = cbrt(sqrt(eta^3 (|a1| |s1| + |j1|^2) / (|c1| |a5| + |a4|^2)))                   (a zero denominator: inf)
// and the new level by nb_blk_correct's rule: want = level_for(tau); want >= l_i is taken (any depth), want < l_i coarsens by ONE
// level and only where t_next is a multiple of 2 s_i.  TP = element type of the partial rows, T = the handle's.
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_blk6_correct(const typename vec4<TP>::type* __restrict__ pa,
                                                         const typename vec4<TP>::type* __restrict__ pj,
                                                         const typename vec4<TP>::type* __restrict__ ps,
                                                         const uint32_t* __restrict__ act, uint32_t na, uint32_t chunks, double G,
                                                         typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                         typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                         typename vec4<T>::type* __restrict__ s, typename vec4<T>::type* __restrict__ c,
                                                         uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                         uint32_t* __restrict__ hdr, uint32_t t_next, uint32_t L, uint32_t lmin,
                                                         int frozen, double eta, double dt)
{
    using V4 = typename vec4<T>::type;
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= na) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    constexpr int kAhead = sizeof(TP) == 4 ? 8 : 4;           // chunks whose rows are in flight together; the adds stay in ascending order
#pragma unroll kAhead
    for (uint32_t q = 0; q < chunks; ++q) {
        const auto pa_ = ld4(pa + (size_t)q * na + k);
        const auto pj_ = ld4(pj + (size_t)q * na + k);
        const auto ps_ = ld4(ps + (size_t)q * na + k);
        sx += (double)pa_.x; sy += (double)pa_.y; sz += (double)pa_.z;
        tx += (double)pj_.x; ty += (double)pj_.y; tz += (double)pj_.z;
        ux += (double)ps_.x; uy += (double)ps_.y; uz += (double)ps_.z;
    }
    const V4 A1 = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
    const V4 J1 = V4{(T)(G * tx), (T)(G * ty), (T)(G * tz), (T)0};
    const V4 S1 = V4{(T)(G * ux), (T)(G * uy), (T)(G * uz), (T)0};
    const uint32_t il = act[k];
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
        auto nrm = [](double p, double q, double r) { return __builtin_sqrt(p * p + q * q + r * r); };
        const double n0 = nrm(A1.x, A1.y, A1.z), n1 = nrm(J1.x, J1.y, J1.z), n2 = nrm(S1.x, S1.y, S1.z), n3 = nrm(C1.x, C1.y, C1.z);
        const double n4 = nrm(d4(dx), d4(dy), d4(dz)), n5 = nrm(d5(dx), d5(dy), d5(dz));
        const double den = n3 * n5 + n4 * n4;
        const double tau = den == 0.0 ? __builtin_inf() : ::cbrt(__builtin_sqrt(eta * eta * eta * (n0 * n2 + n1 * n1) / den));
        const uint32_t want = blk_level_for(tau, dt, lmin, L, hdr + kBlkClamped);
        const uint32_t s_i = 1u << (L - l);
        if (want >= l) ln = want;
        else if ((t_next & (2u * s_i - 1u)) == 0u) ln = l - 1;
        lev[il] = (uint8_t)ln;
        // a deeper level counts as held from here on: the last block step of a call has no schedule behind it that would see it
        if (ln > l) atomicMax(hdr + kBlkFinest, ln);
    }
    due[il] = (t_next == (1u << L) ? 0u : t_next) + (1u << (L - ln));
}

}  // namespace nb
