// kernels/block_batch.hip.h -- block steps sized on the device, many per host wait (nb_set_block_batch; order-4 block-step handles
// with the native pass).  No reference analogue.  Part of nb_kernels.hip.h (include that, not this file).
//
// A SLOT is the launches of one block step with every grid fixed by (n, small_max, CU count):
//   nb_blkq_sched     nb_blk_sched's schedule, then the decision: 0 < |A| <= small_max and t_next != 2^L -> a SMALL step (mode 0);
//                     otherwise the slot PARKS (mode 1): its schedule and prediction stand, the host runs that block step through
//                     the gathered path.  A slot that finds the batch parked is IDLE (mode 2): every kernel of it leaves at once.
//   nb_blkq_predict   nb_blk_predict (small and parked slots)
//   nb_blkq_fj_pk/64  the force+jerk of the |A| <= small_max listed rows against all n predicted rows (small slots)
//   nb_blkq_correct   nb_blk_correct with |A| and t_next from the device header (small slots)
// The batch words are written by ONE lane (lane 0 of the scheduler's one workgroup): integer adds, then published to the host's
// pinned copy.  As in kernels/block.hip.h nothing adds floating-point numbers in an order that depends on timing, and what a small
// step computes for a body depends on the predicted arrays and on n alone: a list row is one lane's chain over the rows of a j-chunk
// in four fixed quarters, the quarters are added in wave order and the chunks in an order the chunk count fixes, and the chunk rule
// (the host's bb_shape) is a function of n and the CU count.  A count the kernels read is clamped: above small_max it is a park,
// never a grid or an index.
#pragma once

namespace nb {

constexpr uint32_t kBbRows = 128;          // list slots of one nb_blkq_fj_pk workgroup (one packed pair per lane, the same in all four waves)
constexpr uint32_t kBbRows64 = 64;         // ... of one nb_blkq_fj64 workgroup (one body per lane)
constexpr uint32_t kBbMaxSmall = 1024;     // the largest small_max
constexpr uint32_t kBbSumLanes = 16;       // lanes of nb_blkq_correct that share the chunk rows of one list slot
// the batch words (device; a copy in pinned host memory).  kBbSmall / kBbBody count up for the life of the handle (mod 2^32: the host
// takes differences per wait).
enum { kBbMode = 0, kBbSmall = 1, kBbBody = 2, kBbFinest = 3, kBbWords = 4 };
enum { kBbModeSmall = 0, kBbModeParked = 1, kBbModeIdle = 2 };

// nb_blk_sched, statement for statement, between the slot's entry (first == 0: a parked batch makes the slot idle) and its
// decision.  end = 2^L.
template <uint32_t NT>
__global__ __launch_bounds__(NT) void nb_blkq_sched(const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev, uint32_t n,
                                                   uint32_t* __restrict__ act, uint32_t* __restrict__ hdr,
                                                   uint32_t* __restrict__ host_hdr, uint32_t* __restrict__ bb,
                                                   uint32_t* __restrict__ host_bb, uint32_t first, uint32_t small_max, uint32_t end)
{
    constexpr uint32_t NW = NT / 64;
    constexpr uint32_t kNever = 0xffffffffu;          // no due_i reaches it (at most 2^31)
    __shared__ uint32_t wmin[NW], wmax[NW], wcnt[NW];
    __shared__ uint32_t entry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) entry = first ? (uint32_t)kBbModeSmall : bb[kBbMode];
    __syncthreads();
    if (entry != kBbModeSmall) {                      // the batch is parked: idle (the host's copy keeps the parked slot's words)
        if (tid == 0) bb[kBbMode] = kBbModeIdle;
        return;
    }
    const uint32_t seg = ((n + NW - 1) / NW + 255u) & ~255u;
    const uint32_t s0 = wave * seg < n ? wave * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
    auto load4 = [&](uint32_t i) {
        if (i + 4 <= n) return *reinterpret_cast<const uint4*>(due + i);
        uint4 d = uint4{kNever, kNever, kNever, kNever};
        if (i < n) d.x = due[i];
        if (i + 1 < n) d.y = due[i + 1];
        if (i + 2 < n) d.z = due[i + 2];
        return d;
    };
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
        // the slot's decision and the counters of the batch: one lane, integer adds
        const bool small = total > 0u && total <= small_max && t_next != end;
        const uint32_t ns = bb[kBbSmall] + (small ? 1u : 0u), nbs = bb[kBbBody] + (small ? total : 0u);
        const uint32_t mode = small ? (uint32_t)kBbModeSmall : (uint32_t)kBbModeParked;
        bb[kBbMode] = mode; bb[kBbSmall] = ns; bb[kBbBody] = nbs; bb[kBbFinest] = mx;
        host_bb[kBbMode] = mode; host_bb[kBbSmall] = ns; host_bb[kBbBody] = nbs; host_bb[kBbFinest] = mx;
    }
}

// nb_blk_predict for a slot that is not idle.
template <typename T>
__global__ __launch_bounds__(kBlock) void nb_blkq_predict(const typename vec4<T>::type* __restrict__ x,
                                                         const typename vec4<T>::type* __restrict__ v,
                                                         const typename vec4<T>::type* __restrict__ a,
                                                         const typename vec4<T>::type* __restrict__ j,
                                                         const uint32_t* __restrict__ due, const uint8_t* __restrict__ lev,
                                                         typename vec4<T>::type* __restrict__ xp,
                                                         typename vec4<T>::type* __restrict__ vp, uint32_t n,
                                                         const uint32_t* __restrict__ hdr, uint32_t L, double tick,
                                                         const uint32_t* __restrict__ bb)
{
    using V4 = typename vec4<T>::type;
    if (bb[kBbMode] == kBbModeIdle) return;
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

// f32: the small force+jerk pass.  Grid (ceil(small_max / 128), j-chunks).  The four waves of a workgroup hold the SAME 128 list
// slots (one packed pair per lane: fj_pk_body's NG = 1 registers), the workgroup stages fj_pk_body's two LDS-DMA tile streams, and
// wave w sweeps rows [64 w, 64 w + 64) of each tile with fj_pk_body's instruction sequence per pair: a lane's dependent chain is a
// quarter of the chunk.  The four waves' binary32 sums meet in LDS and are added in wave order; one compact partial row per
// (j-chunk, list slot) at pa[c * small_max + k].  Lanes past |A| clamp and store nothing; a workgroup whose first slot is past |A|
// leaves after the header loads.
//   The body is shared with nb_encq_fj_pk (kernels/encounter_batch.hip.h).  WATCH (nb_set_block_batch_watch): wth[i] is body i's
// threshold w_i, as in fj_pk_body.  Per stage the eight compares rho^2 < w of its chains are ORed on the scalar unit and ONE
// wave-uniform branch skips the slow path, which tests the index (the own row, rows past the chunk) and keeps the lane's smallest
// (rho^2, j) per packed half in registers.  The four waves hold the same slots and sweep different quarters of each tile: their
// four bests meet in LDS beside red and are merged under the total order (rho^2, index), and the slot's answer for the chunk leaves
// in the .w lanes of the two rows (rho^2; the index bit-cast, 0xffffffff: none).  The sums are the same instructions on the same
// values; without WATCH none of this is compiled.
template <bool WATCH>
__device__ __forceinline__ void blkq_fj_pk_body(const float4* __restrict__ pos, const float4* __restrict__ vel,
                                                const uint32_t* __restrict__ act, const uint32_t* __restrict__ hdr,
                                                const uint32_t* __restrict__ bb, uint32_t small_max, float4* __restrict__ pa,
                                                float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2,
                                                const float4* __restrict__ zero_row, const float* __restrict__ wth = nullptr)
{
    constexpr int TILE = kTile;
    constexpr int U = 8;                  // tile rows per unrolled chunk
    constexpr int JB = 4;                 // j-bodies per stage: four independent chains
    __shared__ float4 tile[2][2][TILE];   // [buffer][0 = positions, 1 = velocities][row]
    __shared__ float red[4][6][kBbRows];  // [wave][ax ay az jx jy jz][slot]
    __shared__ float enc_r[WATCH ? 4 : 1][WATCH ? kBbRows : 1];         // WATCH: [wave][slot] the wave's smallest rho^2 ...
    __shared__ uint32_t enc_j[WATCH ? 4 : 1][WATCH ? kBbRows : 1];      // ... and its index (0xffffffff: none)
    const uint32_t i0 = blockIdx.x * kBbRows;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t ni = hdr[kBlkCount];
    if (ni == 0 || ni > small_max || ni > n || i0 >= ni) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;

    nb_f2 xi, yi, zi, ui, vi, wi;
    nb_f2 wq = nb_f2{0, 0}, br = nb_f2{__builtin_inff(), __builtin_inff()};      // WATCH: the thresholds of the lane's bodies, the smallest rho^2 so far ...
    uint32_t bj0 = 0xffffffffu, bj1 = 0xffffffffu, own0 = 0, own1 = 0;           // ... its index per half, and the lane's own bodies
    {
        const uint32_t il0 = i0 + lane, il1 = il0 + 64;
        uint32_t c0 = il0 < ni ? il0 : ni - 1, c1 = il1 < ni ? il1 : ni - 1;        // clamped, branch-free (never stored)
        c0 = act[c0]; c1 = act[c1];
        c0 = c0 < n ? c0 : n - 1; c1 = c1 < n ? c1 : n - 1;
        if constexpr (WATCH) {            // a clamped lane watches nothing (rho^2 < 0 never holds)
            wq = nb_f2{il0 < ni ? wth[c0] : 0.0f, il1 < ni ? wth[c1] : 0.0f};
            own0 = c0; own1 = c1;
        }
        const float4 b0 = ld4(pos + c0), b1 = ld4(pos + c1), v0 = ld4(vel + c0), v1 = ld4(vel + c1);
        xi = nb_f2{b0.x, b1.x}; yi = nb_f2{b0.y, b1.y}; zi = nb_f2{b0.z, b1.z};
        ui = nb_f2{v0.x, v1.x}; vi = nb_f2{v0.y, v1.y}; wi = nb_f2{v0.z, v1.z};
    }
    const nb_f2 zero = nb_f2{0, 0};
    nb_f2 ax = zero, ay = zero, az = zero, jx = zero, jy = zero, jz = zero;
    nb_f2 AX = zero, AY = zero, AZ = zero, JX = zero, JY = zero, JZ = zero;
    const nb_f2 e2 = nb_f2{eps2, eps2};
    const nb_f2 m3 = nb_f2{-3.0f, -3.0f};
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as fj_pk_body::stage
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        const uint32_t jt = j0 + t * TILE;                        // wave-uniform
        const uint32_t dst_p = lds_wave + (uint32_t)(buf * 2 * TILE) * 16u, dst_v = dst_p + (uint32_t)TILE * 16u;
        unsigned keep;
        if (jt + TILE <= j1) {
            const float4 *bp = pos + jt, *bv = vel + jt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane_off), "s"(bv), "s"(dst_v) : "memory");
        } else {
            const uint32_t j = jt + tid;
            const float4* sp = j < j1 ? pos + j : zero_row;
            const float4* sv = j < j1 ? vel + j : zero_row;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sp), "s"(dst_p) : "memory");
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(sv), "s"(dst_v) : "memory");
        }
    };

    // one stage: JB tile rows (positions p, velocities q) against the lane's packed pair, stage-major over the JB chains
    // (fj_pk_body::math with NG = 1; jrow: the body index of row p[0], read by the watch only)
    auto math = [&](const float4* p, const float4* q, uint32_t jrow) {
        nb_f2 bx[JB], by[JB], bz[JB], bu[JB], bv[JB], bw[JB];
        float bm[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float4 b = p[u], c = q[u];
            bx[u] = nb_f2{b.x, b.x}; by[u] = nb_f2{b.y, b.y}; bz[u] = nb_f2{b.z, b.z}; bm[u] = b.w;
            bu[u] = nb_f2{c.x, c.x}; bv[u] = nb_f2{c.y, c.y}; bw[u] = nb_f2{c.z, c.z};
        }
        nb_f2 dx[JB], dy[JB], dz[JB], du[JB], dv[JB], dw[JB], d2[JB], y[JB], s[JB], rv[JB];
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
        if constexpr (WATCH) {
            bool lt[JB][2];
            bool hit = false;
#pragma unroll
            for (int c = 0; c < JB; ++c) {
                lt[c][0] = d2[c].x < wq.x; lt[c][1] = d2[c].y < wq.y;
                hit |= lt[c][0] | lt[c][1];
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {      // wave-uniform: some lane has a pair below its threshold among these JB rows
#pragma unroll
                for (int u = 0; u < JB; ++u) {                // a slot meets the rows of its quarter in ascending j
                    const uint32_t j = jrow + (uint32_t)u;
                    const nb_f2 r = d2[u];
                    const bool in = j < j1;                   // a row past the chunk is padding (zero_row sits at the origin)
                    // (bitwise, then selects: no branch per lane inside the slow path)
                    const bool t0 = lt[u][0] & in & (j != own0) & ((r.x < br.x) | ((r.x == br.x) & (j < bj0)));
                    const bool t1 = lt[u][1] & in & (j != own1) & ((r.y < br.y) | ((r.y == br.y) & (j < bj1)));
                    br.x = t0 ? r.x : br.x; bj0 = t0 ? j : bj0;
                    br.y = t1 ? r.y : br.y; bj1 = t1 ? j : bj1;
                }
            }
        }
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
        for (int c = 0; c < JB; ++c) s[c] = nb_f2{bm[c], bm[c]} * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) y[c] = y[c] * y[c];
#pragma unroll
        for (int c = 0; c < JB; ++c) s[c] = s[c] * y[c];                   // m / rho^3
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * y[c];                 // q = (dr.dv) / rho^2
#pragma unroll
        for (int c = 0; c < JB; ++c) rv[c] = rv[c] * m3;                   // -3 q
#pragma unroll
        for (int c = 0; c < JB; ++c) du[c] = __builtin_elementwise_fma(rv[c], dx[c], du[c]);      // t = dv - 3 q dr
#pragma unroll
        for (int c = 0; c < JB; ++c) dv[c] = __builtin_elementwise_fma(rv[c], dy[c], dv[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) dw[c] = __builtin_elementwise_fma(rv[c], dz[c], dw[c]);
#pragma unroll
        for (int c = 0; c < JB; ++c) jx = __builtin_elementwise_fma(s[c], du[c], jx);
#pragma unroll
        for (int c = 0; c < JB; ++c) jy = __builtin_elementwise_fma(s[c], dv[c], jy);
#pragma unroll
        for (int c = 0; c < JB; ++c) jz = __builtin_elementwise_fma(s[c], dw[c], jz);
#pragma unroll
        for (int c = 0; c < JB; ++c) ax = __builtin_elementwise_fma(s[c], dx[c], ax);
#pragma unroll
        for (int c = 0; c < JB; ++c) ay = __builtin_elementwise_fma(s[c], dy[c], ay);
#pragma unroll
        for (int c = 0; c < JB; ++c) az = __builtin_elementwise_fma(s[c], dz[c], az);
    };
    auto flush = [&]() {
        AX = AX + ax; AY = AY + ay; AZ = AZ + az;
        JX = JX + jx; JY = JY + jy; JZ = JZ + jz;
        ax = ay = az = jx = jy = jz = zero;
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
        const int lo = 64 * wave, hi = lo + 64 < cntu ? lo + 64 : cntu;      // the wave's quarter of the tile
        for (int r = lo; r < hi; r += U) {
            math(&tile[cur][0][r], &tile[cur][1][r], j0 + t * TILE + (uint32_t)r);
            math(&tile[cur][0][r + JB], &tile[cur][1][r + JB], j0 + t * TILE + (uint32_t)(r + JB));
        }
        if ((t & 15u) == 15u) flush();                    // 1,024 terms per chain, as nb_fj_pk
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush();

    red[wave][0][lane] = AX.x; red[wave][0][lane + 64] = AX.y;
    red[wave][1][lane] = AY.x; red[wave][1][lane + 64] = AY.y;
    red[wave][2][lane] = AZ.x; red[wave][2][lane + 64] = AZ.y;
    red[wave][3][lane] = JX.x; red[wave][3][lane + 64] = JX.y;
    red[wave][4][lane] = JY.x; red[wave][4][lane + 64] = JY.y;
    red[wave][5][lane] = JZ.x; red[wave][5][lane + 64] = JZ.y;
    if constexpr (WATCH) {
        enc_r[wave][lane] = br.x; enc_r[wave][lane + 64] = br.y;
        enc_j[wave][lane] = bj0; enc_j[wave][lane + 64] = bj1;
    }
    __syncthreads();
    const uint32_t k = i0 + (uint32_t)tid;
    if (tid < (int)kBbRows && k < ni) {
        float r[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) r[c] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
        float er = 0.0f, ej = 0.0f;       // WATCH: the chunk's answer, rho^2 and the index bit-cast
        if constexpr (WATCH) {            // the four quarters' bests under the total order (rho^2, index)
            float mr = enc_r[0][tid];
            uint32_t mj = enc_j[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float wr = enc_r[w][tid];
                const uint32_t wj = enc_j[w][tid];
                const bool t = (wj != 0xffffffffu) & ((wr < mr) | ((wr == mr) & (wj < mj)));
                mr = t ? wr : mr; mj = t ? wj : mj;
            }
            er = mr; ej = __uint_as_float(mj);
        }
        pa[(size_t)blockIdx.y * small_max + k] = float4{r[0], r[1], r[2], er};
        pj[(size_t)blockIdx.y * small_max + k] = float4{r[3], r[4], r[5], ej};
    }
}

template <int NG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_blkq_fj_pk(const float4* __restrict__ pos, const float4* __restrict__ vel, const uint32_t* __restrict__ act,
                   const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb, uint32_t small_max, float4* __restrict__ pa,
                   float4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk, float eps2, const float4* __restrict__ zero_row)
{
    static_assert(NG == 1, "one packed pair per lane");
    blkq_fj_pk_body<false>(pos, vel, act, hdr, bb, small_max, pa, pj, n, j_per_chunk, eps2, zero_row);
}

// f64: the same shape on fj64_body's arithmetic (v_rsq_f64 seed + one correction, everything in fp64).  Grid (ceil(small_max / 64),
// j-chunks); the four waves hold the same 64 list slots, one body per lane, wave w sweeps rows [64 w, 64 w + 64) of each tile.
// WATCH: as blkq_fj_pk_body, one compare per pair and the lane masks tested on the scalar unit; the four waves' bests meet in LDS
// and the index leaves as an exact double.  The loop ends at the chunk's last row: a zero row of the tile is never met.
template <typename T, bool WATCH>
__device__ __forceinline__ void blkq_fj64_body(const typename vec4<T>::type* __restrict__ pos,
                                               const typename vec4<T>::type* __restrict__ vel, const uint32_t* __restrict__ act,
                                               const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb,
                                               uint32_t small_max, double4* __restrict__ pa, double4* __restrict__ pj, uint32_t n,
                                               uint32_t j_per_chunk, double eps2, const T* __restrict__ wth = nullptr)
{
    __shared__ double4 tp[kTile];
    __shared__ double4 tv[kTile];
    __shared__ double red[4][6][kBbRows64];
    __shared__ double enc_r[WATCH ? 4 : 1][WATCH ? kBbRows64 : 1];        // WATCH: [wave][slot] the wave's smallest rho^2 ...
    __shared__ uint32_t enc_j[WATCH ? 4 : 1][WATCH ? kBbRows64 : 1];      // ... and its index (0xffffffff: none)
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
    const double xi = (double)bi.x, yi = (double)bi.y, zi = (double)bi.z;
    const double ui = (double)wi.x, vi = (double)wi.y, wz = (double)wi.z;
    double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
    double wq = 0.0, br = __builtin_inf();      // WATCH: the lane's threshold (a clamped lane watches nothing), its smallest rho^2 so far ...
    uint32_t bj = 0xffffffffu;                  // ... and that pair's index (0xffffffff: none)
    if constexpr (WATCH) wq = il < ni ? (double)wth[ic] : 0.0;
    for (uint32_t jt = j0; jt < j1; jt += kTile) {
        const uint32_t j = jt + tid;
        __syncthreads();                                          // the previous tile has been read
        if (j < j1) {
            const auto b = ld4(pos + j);
            const auto c = ld4(vel + j);
            tp[tid] = double4{(double)b.x, (double)b.y, (double)b.z, (double)b.w};
            tv[tid] = double4{(double)c.x, (double)c.y, (double)c.z, 0.0};
        } else {
            tp[tid] = double4{0.0, 0.0, 0.0, 0.0};                // past the chunk: zero mass
            tv[tid] = double4{0.0, 0.0, 0.0, 0.0};
        }
        __syncthreads();
        const uint32_t left = j1 - jt;
        const int cnt = left < (uint32_t)kTile ? (int)left : kTile;
        const int lo = 64 * wave, hi = lo + 64 < cnt ? lo + 64 : cnt;      // the wave's quarter of the tile
        if constexpr (WATCH) {
            // the loop below, statement for statement, with the watch behind rho^2 -- two rows per trip and an odd last row, written
            // out: the wave-wide test keeps the compiler from unrolling a loop of unknown length with a remainder, as it does below
            auto row = [&](int jj) {
                const double4 b = tp[jj];
                const double4 c = tv[jj];
                const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
                const double du = c.x - ui, dv = c.y - vi, dw = c.z - wz;
                const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
                const bool lt = r2 < wq;
                if (__builtin_amdgcn_ballot_w64(lt) != 0) {      // wave-uniform: some lane has this row below its threshold
                    const uint32_t jb = jt + (uint32_t)jj;
                    if (lt && jb != ic && (r2 < br || (r2 == br && jb < bj))) { br = r2; bj = jb; }
                }
                const double y0 = __builtin_amdgcn_rsq(r2);
                const double e = nb_fma(-(r2 * y0), y0, 1.0);
                const double y = nb_fma(0.5 * y0, e, y0);
                const double y2 = y * y;
                const double s3 = (b.w * y) * y2;
                const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
                const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
                jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
                ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
            };
            int jj = lo;
            for (; jj + 2 <= hi; jj += 2) { row(jj); row(jj + 1); }
            if (jj < hi) row(jj);
        } else {
#pragma unroll 2
            for (int jj = lo; jj < hi; ++jj) {
                const double4 b = tp[jj];
                const double4 c = tv[jj];
                const double dx = b.x - xi, dy = b.y - yi, dz = b.z - zi;
                const double du = c.x - ui, dv = c.y - vi, dw = c.z - wz;
                const double r2 = nb_fma(dz, dz, nb_fma(dy, dy, nb_fma(dx, dx, eps2)));
                const double y0 = __builtin_amdgcn_rsq(r2);
                const double e = nb_fma(-(r2 * y0), y0, 1.0);
                const double y = nb_fma(0.5 * y0, e, y0);
                const double y2 = y * y;
                const double s3 = (b.w * y) * y2;
                const double q3 = -3.0 * (nb_fma(dz, dw, nb_fma(dy, dv, dx * du)) * y2);
                const double tx = nb_fma(q3, dx, du), ty = nb_fma(q3, dy, dv), tz = nb_fma(q3, dz, dw);
                jx = nb_fma(s3, tx, jx); jy = nb_fma(s3, ty, jy); jz = nb_fma(s3, tz, jz);
                ax = nb_fma(s3, dx, ax); ay = nb_fma(s3, dy, ay); az = nb_fma(s3, dz, az);
            }
        }
    }
    red[wave][0][lane] = ax; red[wave][1][lane] = ay; red[wave][2][lane] = az;
    red[wave][3][lane] = jx; red[wave][4][lane] = jy; red[wave][5][lane] = jz;
    if constexpr (WATCH) { enc_r[wave][lane] = br; enc_j[wave][lane] = bj; }
    __syncthreads();
    const uint32_t k = i0 + (uint32_t)tid;
    if (tid < (int)kBbRows64 && k < ni) {
        double r[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) r[c] = ((red[0][c][tid] + red[1][c][tid]) + red[2][c][tid]) + red[3][c][tid];
        double er = 0.0, ej = 0.0;        // WATCH: the chunk's answer, rho^2 and the index as an exact double
        if constexpr (WATCH) {            // the four quarters' bests under the total order (rho^2, index)
            double mr = enc_r[0][tid];
            uint32_t mj = enc_j[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const double wr = enc_r[w][tid];
                const uint32_t wj = enc_j[w][tid];
                const bool t = (wj != 0xffffffffu) & ((wr < mr) | ((wr == mr) & (wj < mj)));
                mr = t ? wr : mr; mj = t ? wj : mj;
            }
            er = mr; ej = (double)mj;
        }
        pa[(size_t)blockIdx.y * small_max + k] = double4{r[0], r[1], r[2], er};
        pj[(size_t)blockIdx.y * small_max + k] = double4{r[3], r[4], r[5], ej};
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
void nb_blkq_fj64(const typename vec4<T>::type* __restrict__ pos, const typename vec4<T>::type* __restrict__ vel,
                  const uint32_t* __restrict__ act, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bb,
                  uint32_t small_max, double4* __restrict__ pa, double4* __restrict__ pj, uint32_t n, uint32_t j_per_chunk,
                  double eps2)
{
    blkq_fj64_body<T, false>(pos, vel, act, hdr, bb, small_max, pa, pj, n, j_per_chunk, eps2);
}

// nb_blk_correct with |A| and t_next from the device header and the small pass's rows (chunk c, slot k at pa[c * small_max + k]).
// kBbSumLanes lanes share a slot's chunk rows: lane q adds chunks [q w, (q + 1) w), w = ceil(chunks / kBbSumLanes), in ascending
// order in fp64, and the lanes' sums are added in lane order -- an order fixed by the chunk count, i.e. by n and the CU count.
// Everything behind the sums (times G, corrector, criterion, new level, due) is nb_blk_correct's, statement for statement, on
// the slot's first lane.  Grid ceil(small_max kBbSumLanes / kBlock).
//   The body is shared with nb_encq_correct (kernels/encounter_batch.hip.h).  WATCH: nb_enc_fold's work inside this launch.  Each
// lane keeps the minimum over its chunks' .w pairs under the rule of the pass (smaller rho^2, equal rho^2 to the smaller index: a
// total order, so the minimum is the one a single ascending chain finds), the lanes' minima meet by shuffles before any lane
// leaves, and the slot's first lane updates the record of its body: count, and (rho2, partner, time) when strictly smaller.  The
// block time is formed here, exactly: t = tbase + t_next 2^-L, tbase the outer steps run when this outer step began.  A wave's hits
// are counted by ballot and added once per wave that has any: an integer add and an integer minimum (the bits of t, read first),
// no floating-point atomics, no workgroup barrier (lanes leave early above).  Without WATCH none of this is compiled.
template <typename TP, typename T, bool WATCH>
__device__ __forceinline__ void blkq_correct_body(const typename vec4<TP>::type* __restrict__ pa,
                                                  const typename vec4<TP>::type* __restrict__ pj,
                                                  const uint32_t* __restrict__ act, const uint32_t* __restrict__ bb,
                                                  uint32_t small_max, uint32_t chunks, double G,
                                                  typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                  typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                  uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                  uint32_t* __restrict__ hdr, uint32_t n, uint32_t L, uint32_t lmin,
                                                  int frozen, double eta, double dt, T* __restrict__ rho2 = nullptr,
                                                  uint32_t* __restrict__ partner = nullptr, double* __restrict__ time = nullptr,
                                                  uint32_t* __restrict__ count = nullptr,
                                                  unsigned long long* __restrict__ words = nullptr, double tbase = 0.0)
{
    using V4 = typename vec4<T>::type;
    if (bb[kBbMode] != kBbModeSmall) return;
    const uint32_t na = hdr[kBlkCount], t_next = hdr[kBlkNext];
    if (na > small_max) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, k = t / kBbSumLanes, q = t % kBbSumLanes;
    if (k >= na) return;                                      // (the lanes of a slot leave together)
    const uint32_t il = act[k];
    if (il >= n) return;
    double px = 0.0, py = 0.0, pz = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
    const uint32_t w = (chunks + kBbSumLanes - 1) / kBbSumLanes;
    const uint32_t c0 = q * w < chunks ? q * w : chunks, c1 = c0 + w < chunks ? c0 + w : chunks;
    TP er = (TP)__builtin_inf();          // WATCH: the smallest (rho^2, index) of the lane's chunks
    uint32_t ej = kEncNone;
#pragma unroll 8
    for (uint32_t c = c0; c < c1; ++c) {
        const auto pa_ = ld4(pa + (size_t)c * small_max + k);
        const auto pj_ = ld4(pj + (size_t)c * small_max + k);
        px += (double)pa_.x; py += (double)pa_.y; pz += (double)pa_.z;
        qx += (double)pj_.x; qy += (double)pj_.y; qz += (double)pj_.z;
        if constexpr (WATCH) {
            const TP r = pa_.w;
            const uint32_t jb = enc_index(pj_.w);
            if (jb != kEncNone && (r < er || (r == er && jb < ej))) { er = r; ej = jb; }
        }
    }
    const int first = (int)((threadIdx.x & 63u) - q);         // the slot's first lane in the wave
    double sx = __shfl(px, first), sy = __shfl(py, first), sz = __shfl(pz, first);
    double tx = __shfl(qx, first), ty = __shfl(qy, first), tz = __shfl(qz, first);
#pragma unroll
    for (int o = 1; o < (int)kBbSumLanes; ++o) {
        sx += __shfl(px, first + o); sy += __shfl(py, first + o); sz += __shfl(pz, first + o);
        tx += __shfl(qx, first + o); ty += __shfl(qy, first + o); tz += __shfl(qz, first + o);
    }
    if constexpr (WATCH) {
#pragma unroll
        for (int o = (int)kBbSumLanes >> 1; o > 0; o >>= 1) {      // (a slot's lanes are kBbSumLanes aligned lanes of one wave, all here)
            const TP r = __shfl_xor(er, o);
            const uint32_t jb = (uint32_t)__shfl_xor((int)ej, o);
            if (jb != kEncNone && (r < er || (r == er && jb < ej))) { er = r; ej = jb; }
        }
        const bool hit = q == 0 && ej != kEncNone;
        const unsigned long long hits = __ballot(hit);             // over the lanes still here
        if (hit) {
            const double t = tbase + __builtin_ldexp((double)t_next, -(int)L);      // exact: t_next <= 2^L <= 2^30
            count[il] += 1u;                                       // a body is in the list once: its record has one writer
            if ((T)er < rho2[il]) { rho2[il] = (T)er; partner[il] = ej; time[il] = t; }
            if ((threadIdx.x & 63u) == (uint32_t)__ffsll(hits) - 1u) {      // once per wave that has any
                atomicAdd(words + kEncHits, (unsigned long long)__popcll(hits));
                const unsigned long long tb = (unsigned long long)__double_as_longlong(t);
                if (tb < __hip_atomic_load(words + kEncFirst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(words + kEncFirst, tb);
            }
        }
    }
    if (q != 0) return;
    const V4 A1 = V4{(T)(G * sx), (T)(G * sy), (T)(G * sz), (T)0};
    const V4 J1 = V4{(T)(G * tx), (T)(G * ty), (T)(G * tz), (T)0};
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
        if (ln > l) atomicMax(hdr + kBlkFinest, ln);
    }
    due[il] = (t_next == (1u << L) ? 0u : t_next) + (1u << (L - ln));
}

template <typename TP, typename T>
__global__ __launch_bounds__(kBlock) void nb_blkq_correct(const typename vec4<TP>::type* __restrict__ pa,
                                                         const typename vec4<TP>::type* __restrict__ pj,
                                                         const uint32_t* __restrict__ act, const uint32_t* __restrict__ bb,
                                                         uint32_t small_max, uint32_t chunks, double G,
                                                         typename vec4<T>::type* __restrict__ x, typename vec4<T>::type* __restrict__ v,
                                                         typename vec4<T>::type* __restrict__ a, typename vec4<T>::type* __restrict__ j,
                                                         uint32_t* __restrict__ due, uint8_t* __restrict__ lev,
                                                         uint32_t* __restrict__ hdr, uint32_t n, uint32_t L, uint32_t lmin,
                                                         int frozen, double eta, double dt)
{
    blkq_correct_body<TP, T, false>(pa, pj, act, bb, small_max, chunks, G, x, v, a, j, due, lev, hdr, n, L, lmin, frozen, eta, dt);
}

}  // namespace nb
