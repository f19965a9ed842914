// kernels/block.hip.h -- block individual time steps for the Hermite integrator (nb_set_block_steps; Makino & Aarseth 1992 as in
// NBODY4/6 and phi-GPU).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// Time inside one outer step of dt is counted in ticks of dt / 2^L (L = max_level).  Body i at level l_i steps by s_i = 2^(L - l_i)
// ticks; its state (x, v, a, j) belongs to the tick t_i, and the engine keeps due_i = t_i + s_i, the tick of its next corrector.
// One block step, with the launches the host makes of it:
//   nb_blk_sched     t_next = min due_i, the active list { i : due_i == t_next } in ascending body order, the header
//   nb_blk_predict   every body from its own state over (t_next - t_i) ticks into xp, vp
//   (the host reads the header: |A| sizes the next launches)
//   nb_blk_fj_pk/64  |A| x N ordered pairs: the i-rows gathered through the list, compact partial rows
//   nb_blk_correct   chunk sums in fp64, corrector, step criterion, new level, due_i; the last block step of an outer step (t_next ==
//                    2^L, every body active) starts the next one's clock at 0
// Nothing here adds floating-point numbers in an order that depends on timing: the list is built by a scan, the chunk rows are
// added in ascending order, the only atomics are integer counts and maxima.
#pragma once

namespace nb {

constexpr uint32_t kBlkSched = 1024;       // lanes of nb_blk_sched's one workgroup
// the header nb_blk_sched publishes (device words; count and next also into the host's pinned copy)
enum { kBlkCount = 0, kBlkNext = 1, kBlkClamped = 2, kBlkFinest = 3, kBlkWords = 4 };

// Smallest level l in [lmin, L] with dt / 2^l <= tau; none: L, and the decision is counted as clamped.  tau = inf gives lmin.
__device__ __forceinline__ uint32_t blk_level_for(double tau, double dt, uint32_t lmin, uint32_t L, uint32_t* clamped)
{
    for (uint32_t l = lmin; l <= L; ++l)
        if (__builtin_ldexp(dt, -(int)l) <= tau) return l;
    atomicAdd(clamped, 1u);
    return L;
}

// The start rule (mode 0): l_i = level_for((eta / 2) |a_i| / |j_i|), |j_i| = 0 -> lmin; mode 1 (frozen): every body at lmin; mode 2:
// the levels were uploaded.  Every mode starts the outer step's clock: due_i = s_i.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk_start(const typename vec4<T>::type* __restrict__ a,
                                                      const typename vec4<T>::type* __restrict__ j, uint8_t* __restrict__ lev,
                                                      uint32_t* __restrict__ due, uint32_t* __restrict__ hdr, uint32_t n, int mode,
                                                      double eta, double dt, uint32_t lmin, uint32_t L)
{
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    uint32_t l = lmin;
    if (mode == 2) l = lev[il];
    else if (mode == 0) {
        const auto A = ld4(a + il), J = ld4(j + il);
        const double aa = __builtin_sqrt((double)A.x * A.x + (double)A.y * A.y + (double)A.z * A.z);
        const double jj = __builtin_sqrt((double)J.x * J.x + (double)J.y * J.y + (double)J.z * J.z);
        if (jj > 0.0) l = blk_level_for(0.5 * eta * aa / jj, dt, lmin, L, hdr + kBlkClamped);
    }
    lev[il] = (uint8_t)l;
    due[il] = 1u << (L - l);
    atomicMax(hdr + kBlkFinest, l);
}

// One workgroup; wave w owns a contiguous segment of the bodies (a multiple of 256), a lane four consecutive bodies of every 256-body
// round (one 16-byte load of due, one 4-byte load of lev).  Pass 1: t_next = min due_i and the deepest level present.  Pass 2: the
// active bodies of each segment are counted, and the counts scanned over the waves.  Pass 3: every wave writes its part of the list
// in ascending body order (four ballots per round).  No barrier inside a pass, so the loads of a pass overlap.  The header goes to
// device memory (the kernels that follow read t_next there) and, count and t_next, straight to the host's pinned copy.
// (A template, as every kernel here: the header is part of more than one translation unit.)
template <uint32_t NT>
__global__ __launch_bounds__(NT) void nb_blk_sched(const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev, uint32_t n,
                                                  uint32_t* __restrict__ act, uint32_t* __restrict__ hdr,
                                                  uint32_t* __restrict__ host_hdr)
{
    constexpr uint32_t NW = NT / 64;
    constexpr uint32_t kNever = 0xffffffffu;          // no due_i reaches it (at most 2^31)
    __shared__ uint32_t wmin[NW], wmax[NW], wcnt[NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t seg = ((n + NW - 1) / NW + 255u) & ~255u;
    const uint32_t s0 = wave * seg < n ? wave * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
    // four consecutive due_i from body i on; past the end: kNever
    auto load4 = [&](uint32_t i) {
        if (i + 4 <= n) return *reinterpret_cast<const uint4*>(due + i);
        uint4 d = uint4{kNever, kNever, kNever, kNever};
        if (i < n) d.x = due[i];
        if (i + 1 < n) d.y = due[i + 1];
        if (i + 2 < n) d.z = due[i + 2];
        return d;
    };
    // (the passes are bound by the latency of their loads: unrolled far enough that a lane's loads of a pass are in flight together
    // up to 65,536 bodies)
    uint32_t mn = kNever, mx = 0;
#pragma unroll 16
    for (uint32_t i = s0 + 4 * lane; i < s1; i += 256) {
        const uint4 d = load4(i);
        const uint32_t m01 = d.x < d.y ? d.x : d.y, m23 = d.z < d.w ? d.z : d.w, m = m01 < m23 ? m01 : m23;
        mn = m < mn ? m : mn;
        if (i + 4 <= n) {
            const uint32_t l4 = *reinterpret_cast<const uint32_t*>(lev + i);      // four levels, each below 32
            const uint32_t l01 = (l4 & 0xffu) > ((l4 >> 8) & 0xffu) ? (l4 & 0xffu) : ((l4 >> 8) & 0xffu);
            const uint32_t l23 = ((l4 >> 16) & 0xffu) > (l4 >> 24) ? ((l4 >> 16) & 0xffu) : (l4 >> 24);
            const uint32_t l = l01 > l23 ? l01 : l23;
            mx = l > mx ? l : mx;
        } else {
            for (uint32_t q = 0; i + q < n; ++q) { const uint32_t l = lev[i + q]; mx = l > mx ? l : mx; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t m2 = __shfl_xor(mn, o), x2 = __shfl_xor(mx, o);
        mn = m2 < mn ? m2 : mn;
        mx = x2 > mx ? x2 : mx;
    }
    if (lane == 0) { wmin[wave] = mn; wmax[wave] = mx; }
    __syncthreads();
    for (uint32_t w = 0; w < NW; ++w) {
        mn = wmin[w] < mn ? wmin[w] : mn;
        mx = wmax[w] > mx ? wmax[w] : mx;
    }
    const uint32_t t_next = mn;
    uint32_t cnt = 0;
#pragma unroll 16
    for (uint32_t i = s0 + 4 * lane; i < s1; i += 256) {
        const uint4 d = load4(i);
        cnt += (d.x == t_next) + (d.y == t_next) + (d.z == t_next) + (d.w == t_next);
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (uint32_t w = 0; w < NW; ++w) {
        const uint32_t c = wcnt[w];
        base += w < wave ? c : 0u;
        total += c;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 8
    for (uint32_t r = s0; r < s1; r += 256) {
        const uint32_t i = r + 4 * lane;
        const uint4 d = i < s1 ? load4(i) : uint4{kNever, kNever, kNever, kNever};
        const bool f0 = d.x == t_next, f1 = d.y == t_next, f2 = d.z == t_next, f3 = d.w == t_next;
        const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1), b2 = __ballot(f2), b3 = __ballot(f3);
        uint32_t at = base + (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below));
        if (f0) act[at++] = i;
        if (f1) act[at++] = i + 1;
        if (f2) act[at++] = i + 2;
        if (f3) act[at++] = i + 3;
        base += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
    }
    if (tid == 0) {
        hdr[kBlkCount] = total;
        hdr[kBlkNext] = t_next;
        if (mx > hdr[kBlkFinest]) hdr[kBlkFinest] = mx;
        host_hdr[kBlkCount] = total;
        host_hdr[kBlkNext] = t_next;
    }
}

// The predictor of nb_hermite_predict with a step of the body's own: h_i = (t_next - t_i) ticks, t_i = due_i - s_i.  Always from the
// stored state, never from an earlier prediction.  t_next is read from the device header: the launch follows nb_blk_sched without
// the host in between.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk_predict(const typename vec4<T>::type* __restrict__ x,
                                                        const typename vec4<T>::type* __restrict__ v,
                                                        const typename vec4<T>::type* __restrict__ a,
                                                        const typename vec4<T>::type* __restrict__ j,
                                                        const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                        typename vec4<T>::type* __restrict__ xp,
                                                        typename vec4<T>::type* __restrict__ vp, uint32_t n,
                                                        const uint32_t* __restrict__ hdr, uint32_t L, double tick)
{
    using V4 = typename vec4<T>::type;
    const uint32_t il = blockIdx.x * kBlock + threadIdx.x;
    if (il >= n) return;
    const uint32_t t_next = hdr[kBlkNext];
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il);
    const uint32_t t_i = due[il] - (1u << (L - lev[il]));
    const double h = (double)(t_next - t_i) * tick;
    const double h2 = h * (1.0 / 2.0), h3 = h * (1.0 / 3.0);
    auto px = [&](double x0, double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, nb_fma(h3, j0, a0), v0), x0); };
    auto pv = [&](double v0, double a0, double j0) { return nb_fma(h, nb_fma(h2, j0, a0), v0); };
    xp[il] = V4{(T)px(X.x, V.x, A.x, J.x), (T)px(X.y, V.y, A.y, J.y), (T)px(X.z, V.z, A.z, J.z), X.w};
    vp[il] = V4{(T)pv(V.x, A.x, J.x), (T)pv(V.y, A.y, J.y), (T)pv(V.z, A.z, J.z), V.w};
}

// The force+jerk pass of the na active bodies against all n predicted rows: nb_fj_pk's / nb_fj64's body (kernels/hermite.hip.h) with
// the i-rows gathered through act[] and compact partial rows (row k of chunk c, at pa[c * na + k], belongs to act[k]).  An active
// body's own row is read from the same arrays as the j-rows: the self term is exactly 0.  Lanes past na clamp to the last active
// body and store nothing.  NG = 2: 1,024 rows per workgroup, NG = 1: 512 (a small active set then fills more workgroups).
template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NB_FJ_WAVES, NB_FJ_WAVES)))
void nb_blk_fj_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const uint32_t* __restrict__ act, uint32_t na,
                  float4* __restrict__ pa, float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2,
                  const float4* __restrict__ zero_row)
{
    fj_pk_body<NG, true>(pos, vel, act, na, pa, pj, n, j_per_chunk, eps2, zero_row);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blk_fj64(const typename vec4<T>::type* __restrict__ pos,
                                                     const typename vec4<T>::type* __restrict__ vel,
                                                     const uint32_t* __restrict__ act, uint32_t na, double4* __restrict__ pa,
                                                     double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, double eps2)
{
    fj64_body<T, true>(pos, vel, act, na, pa, pj, n, j_per_chunk, eps2);
}

// For k < na, body i = act[k]: (a1, j1) = G x the chunk rows added in ascending order in fp64 (as nb_fj_reduce), rounded to the
// handle's precision; nb_hermite_correct's corrector over h = s_i ticks; then the step criterion on what was stored
//   a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2      a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3      a2e = a2 + h a3
//   tau = sqrt(eta (|a1| |a2e| + |j1|^2) / (|j1| |a3| + |a2e|^2))                      (a zero denominator: inf)
// and, unless frozen, the new level: want = level_for(tau); want >= l_i is taken (any depth), want < l_i coarsens by ONE level and only
// where t_next is a multiple of 2 s_i.  TP = element type of the partial rows, T = the handle's.
template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_blk_correct(const typename vec4<TP>::type* __restrict__ pa,
                                                        const typename vec4<TP>::type* __restrict__ pj,
                                                        const uint32_t* __restrict__ act, uint32_t na, uint32_t chunks, double G,
                                                        typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                        typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                        uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                        uint32_t* __restrict__ hdr, uint32_t t_next, uint32_t L, uint32_t lmin,
                                                        int frozen, double eta, double dt)
{
    using V4 = typename vec4<T>::type;
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= na) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    constexpr int kAhead = sizeof(TP) == 4 ? 16 : 8;          // chunks whose rows are in flight together; the adds stay in ascending order
#pragma unroll kAhead
    for (uint32_t c = 0; c < chunks; ++c) {
        const auto pa_ = ld4(pa + (size_t)c * na + k);
        const auto pj_ = ld4(pj + (size_t)c * na + k);
        sx += (double)pa_.x; sy += (double)pa_.y; sz += (double)pa_.z;
        tx += (double)pj_.x; ty += (double)pj_.y; tz += (double)pj_.z;
    }
    const V4 A1 = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
    const V4 J1 = V4{(T)(G * tx), (T)(G * ty), (T)(G * tz), (T)0};
    const uint32_t il = act[k];
    const uint32_t l = lev[il];
    const double h = __builtin_ldexp(dt, -(int)l);
    const auto X = ld4(x + il), V = ld4(v + il), A = ld4(a + il), J = ld4(j + il);
    const double hh = 0.5 * h, h12 = h * h * (1.0 / 12.0);
    auto cv = [&](double v0, double a0, double an, double j0, double jn) { return nb_fma(h12, j0 - jn, nb_fma(hh, a0 + an, v0)); };
    const double vx = cv(V.x, A.x, A1.x, J.x, J1.x), vy = cv(V.y, A.y, A1.y, J.y, J1.y), vz = cv(V.z, A.z, A1.z, J.z, J1.z);
    auto cx = [&](double x0, double v0, double vn, double a0, double an) { return nb_fma(h12, a0 - an, nb_fma(hh, v0 + vn, x0)); };
    x[il] = V4{(T)cx(X.x, V.x, vx, A.x, A1.x), (T)cx(X.y, V.y, vy, A.y, A1.y), (T)cx(X.z, V.z, vz, A.z, A1.z), X.w};
    v[il] = V4{(T)vx, (T)vy, (T)vz, V.w};
    a[il] = A1;
    j[il] = J1;

    uint32_t ln = l;
    if (!frozen) {
        const double hq = h * h, hc = hq * h;
        auto d2 = [&](double a0, double an, double j0, double jn) { return (-6.0 * (a0 - an) - h * (4.0 * j0 + 2.0 * jn)) / hq; };
        auto d3 = [&](double a0, double an, double j0, double jn) { return (12.0 * (a0 - an) + 6.0 * h * (j0 + jn)) / hc; };
        const double a3x = d3(A.x, A1.x, J.x, J1.x), a3y = d3(A.y, A1.y, J.y, J1.y), a3z = d3(A.z, A1.z, J.z, J1.z);
        const double ex = d2(A.x, A1.x, J.x, J1.x) + h * a3x, ey = d2(A.y, A1.y, J.y, J1.y) + h * a3y,
                     ez = d2(A.z, A1.z, J.z, J1.z) + h * a3z;
        auto nrm = [](double p, double q, double r) { return __builtin_sqrt(p * p + q * q + r * r); };
        const double n1 = nrm(A1.x, A1.y, A1.z), nj = nrm(J1.x, J1.y, J1.z), n2 = nrm(ex, ey, ez), n3 = nrm(a3x, a3y, a3z);
        const double den = nj * n3 + n2 * n2;
        const double tau = den == 0.0 ? __builtin_inf() : __builtin_sqrt(eta * (n1 * n2 + nj * nj) / den);
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
