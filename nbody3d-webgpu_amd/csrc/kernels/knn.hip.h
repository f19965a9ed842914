// kernels/knn.hip.h -- nb_knn: the K NEAREST of the N rows of bodies[cur] for each of M points, in the total order (d2 ascending,
// then j ascending) (nb_knn_pk, nb_knn64, nb_knn_merge).  Part of nb_kernels.hip.h (include that, not this file).
//
// The grid, the tile stream and the d2 arithmetic are nb_nbl_pk's / nb_nbl64's.  Workgroup (bx, c) keeps per point a THRESHOLD
// thr = the k-th smallest d2 the chunk has shown it so far (+inf until k candidates exist) and the hot loop only compares
// d2 < thr.  j ascends inside a chunk, so an equal d2 at a larger j loses to the incumbent: strict `<` is exact.
//   The candidates of (chunk c, point p) are appended, unsorted, to the point's WORKING ROW in global memory, knn_cap(k) entries
// of (d2, j).  A row that cannot take another group's worth of candidates is COMPACTED by the whole wave: each lane holds one or
// two of its entries, ranks them by counting the entries below under (d2, j) -- the keys are distinct, the ranks a permutation --
// and the entries of rank < k go back to row[rank]; thr becomes the d2 of rank k - 1.  The end of the chunk compacts every row once
// more and pads it to k entries with (+inf, 0xffffffff).  nb_knn_merge then merges a point's sorted chunk rows.
//   Every row is written and read by ONE wave only, in program order (s_waitcnt vmcnt(0) before a compaction reads what the wave's
// lanes appended): no atomics, no barrier beyond the tile stream's.  A point's final row depends on that point and the bodies only.
#pragma once

namespace nb {

constexpr uint32_t kKnnMaxK = 64;                      // most neighbours per point
constexpr int kKnnU = 4;                               // tile rows per group: what one slow-path visit can append to a row
constexpr uint32_t kKnnMergeLanes = 64;                // points of one nb_knn_merge workgroup

// entries of a working row: 2k, and room for one group's candidates on top of k where k is tiny (never more than 128)
__host__ __device__ constexpr uint32_t knn_cap(uint32_t k) { return k >= (uint32_t)kKnnU ? 2 * k : k + (uint32_t)kKnnU; }

// One entry of a row.  float: (d2 bits, j); double: (d2 lo, d2 hi, j, -).
template <typename T> struct knn_row;
template <> struct knn_row<float> {
    using type = uint2;
    static __device__ __forceinline__ uint2 pack(float d, uint32_t j) { return uint2{__float_as_uint(d), j}; }
    static __device__ __forceinline__ float d2(const uint2 e) { return __uint_as_float(e.x); }
    static __device__ __forceinline__ uint32_t j(const uint2 e) { return e.y; }
};
template <> struct knn_row<double> {
    using type = uint4;
    static __device__ __forceinline__ uint4 pack(double d, uint32_t j)
    {
        const uint64_t b = (uint64_t)__double_as_longlong(d);
        return uint4{(uint32_t)b, (uint32_t)(b >> 32), j, 0u};
    }
    static __device__ __forceinline__ double d2(const uint4 e) { return __longlong_as_double((long long)(((uint64_t)e.y << 32) | e.x)); }
    static __device__ __forceinline__ uint32_t j(const uint4 e) { return e.z; }
};

__device__ __forceinline__ uint32_t knn_lane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint64_t knn_lane(uint64_t v, uint32_t l) { return ((uint64_t)knn_lane((uint32_t)(v >> 32), l) << 32) | knn_lane((uint32_t)v, l); }

// (d, j) before (D, J) in the total order
template <typename T>
__device__ __forceinline__ bool knn_less(T d, uint32_t j, T D, uint32_t J) { return d < D || (d == D && j < J); }

// The sort key of an entry inside a compaction.  float: ONE 64-bit integer, d2's bits above j -- a candidate's d2 is finite and
// >= +0, where the bits of a binary32 order as the values do, so one unsigned compare is the whole order.  double: (d2 bits, j).
template <typename T> struct knn_key;
template <> struct knn_key<float> {
    uint64_t v;
    static __device__ __forceinline__ knn_key none() { return {~0ull}; }
    static __device__ __forceinline__ knn_key of(uint2 e) { return {((uint64_t)e.x << 32) | e.y}; }
    __device__ __forceinline__ uint2 entry() const { return uint2{(uint32_t)(v >> 32), (uint32_t)v}; }
    __device__ __forceinline__ float d2() const { return __uint_as_float((uint32_t)(v >> 32)); }
    __device__ __forceinline__ knn_key at(uint32_t l) const { return {knn_lane(v, l)}; }
    __device__ __forceinline__ bool before(const knn_key o) const { return v < o.v; }
};
template <> struct knn_key<double> {
    uint64_t d; uint32_t j;       // d2 >= +0 and finite: its bits order as the values do
    static __device__ __forceinline__ knn_key none() { return {~0ull, kNbrNone}; }
    static __device__ __forceinline__ knn_key of(uint4 e) { return {((uint64_t)e.y << 32) | e.x, e.z}; }
    __device__ __forceinline__ uint4 entry() const { return uint4{(uint32_t)d, (uint32_t)(d >> 32), j, 0u}; }
    __device__ __forceinline__ double d2() const { return __longlong_as_double((long long)d); }
    __device__ __forceinline__ knn_key at(uint32_t l) const { return {knn_lane(d, l), knn_lane(j, l)}; }
    __device__ __forceinline__ bool before(const knn_key o) const { return d < o.d || (d == o.d && j < o.j); }
};

// The whole wave compacts ONE row (row, cnt: wave-uniform; cnt <= knn_cap(k) <= 128): afterwards its first min(cnt, k) entries
// are its smallest, sorted.  Returns the new threshold: the d2 of rank k - 1, +inf with fewer than k entries.  FINAL also pads the
// row to k entries.
template <typename T, bool FINAL>
__device__ __forceinline__ T knn_compact(typename knn_row<T>::type* __restrict__ row, uint32_t cnt, uint32_t k, uint32_t lane)
{
    using R = knn_row<T>;
    using K = knn_key<T>;
    const T inf = (T)__builtin_huge_val();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // what the lanes of this wave appended has landed
    const bool va = lane < cnt, vb = lane + 64u < cnt;        // the lane's entries: `lane` and `lane + 64`
    K a = K::none(), b = K::none();
    if (va) a = K::of(row[lane]);
    uint32_t ra = 0, rb = 0;                                  // entries before mine
    if (cnt <= 64u) {                                         // (k <= 32, and the short rows of a chunk's end: one entry per lane)
        for (uint32_t i = 0; i < cnt; ++i) ra += a.at(i).before(a) ? 1u : 0u;
    } else {
        if (vb) b = K::of(row[lane + 64u]);
        for (uint32_t i = 0; i < 64u; ++i) {
            const K o = a.at(i);
            ra += o.before(a) ? 1u : 0u;
            rb += o.before(b) ? 1u : 0u;
        }
        for (uint32_t i = 64u; i < cnt; ++i) {
            const K o = b.at(i - 64u);
            ra += o.before(a) ? 1u : 0u;
            rb += o.before(b) ? 1u : 0u;
        }
    }
    // every entry is in registers (the ranks needed them all): the row can be rewritten in place
    if (va && ra < k) row[ra] = a.entry();
    if (vb && rb < k) row[rb] = b.entry();
    if constexpr (FINAL) {
        for (uint32_t e = cnt + lane; e < k; e += 64u) row[e] = R::pack(inf, kNbrNone);
    }
    const uint64_t ma = __builtin_amdgcn_ballot_w64(va && ra == k - 1u), mb = __builtin_amdgcn_ballot_w64(vb && rb == k - 1u);
    // (both reads unconditional: every path out of here has waited for the row's loads, so the compiler keeps no wait for them at
    // the head of the hot loop, where it would also wait for the next tile's LDS-DMA)
    const K ta = a.at(ma ? (uint32_t)__builtin_ctzll(ma) : 0u), tb = b.at(mb ? (uint32_t)__builtin_ctzll(mb) : 0u);
    return ma ? ta.d2() : mb ? tb.d2() : inf;
}

// f32.  nb_nbl_pk's frame: 4 points per lane as two packed pairs, the tile double-buffered by LDS-DMA with rows past the range at
// +inf, 6 packed instructions per two pairs for d2, the own row masked only in the tiles that can hold it; the fast path is that
// kernel's with thr in the place of h2.  Slow path, only in a wave where some lane has a candidate among the U rows: per
// (row, point slot), behind a scalar branch, the guarded 8-byte append; then the rows that are nearly full are compacted.
//   Guards: a lane's point >= m has thr = -1 (no d2 is below it: never appended, never sends its wave into the slow path), its
// loads are clamped to point m - 1; a row never holds more than knn_cap(k) entries (<= cap - U before a group, <= U appended).
//   STATS (the calibration build's counters, tools/knn_bench.py --stats; never launched by the library the bindings load): per
// (chunk, point) the candidates appended and the compactions before the end of the chunk, per wave the groups that left the fast path.
template <bool STATS = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4)))
void nb_knn_pk(const float4* __restrict__ bodies, const float4* __restrict__ points, uint2* __restrict__ work, uint32_t n, uint32_t m,
               uint32_t j_per_chunk, uint32_t k, uint32_t at_bodies, uint32_t self0, const float4* __restrict__ inf_row,
               uint2* __restrict__ stat_rows, uint32_t* __restrict__ stat_waves)
{
    constexpr int NG = kNbrNG;
    constexpr int TILE = kTile;
    constexpr int U = kKnnU;              // tile rows per group: one OR-ed mask, one branch
    constexpr int JB = 2;                 // j-bodies per stage
    constexpr int NC = JB * NG;
    __shared__ float4 tile[2][TILE];
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint32_t p0 = blockIdx.x * kNbrRows;               // first point of the block
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const float inf = __builtin_huge_valf();
    const uint32_t cap = knn_cap(k);
    const size_t row0 = (size_t)blockIdx.y * m;               // the chunk's first working row

    nb_f2 xi[NG], yi[NG], zi[NG];
    uint32_t own[2 * NG];                 // at_bodies: the row each point leaves out
    uint32_t pt[2 * NG];                  // the point of each slot (>= m: none)
    uint32_t cnt[2 * NG];                 // entries of each point's working row
    float thr[2 * NG];                    // the k-th smallest d2 so far (+inf: fewer than k)
    uint32_t ncand[2 * NG] = {}, ncomp[2 * NG] = {}, nslow = 0;      // STATS only
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint32_t il0 = p0 + (2 * g) * kBlock + tid, il1 = il0 + kBlock;
        const uint32_t c0 = il0 < m ? il0 : m - 1, c1 = il1 < m ? il1 : m - 1;      // clamped, branch-free (never stored)
        const float4 b0 = ld4(points + c0);
        const float4 b1 = ld4(points + c1);
        xi[g] = nb_f2{b0.x, b1.x}; yi[g] = nb_f2{b0.y, b1.y}; zi[g] = nb_f2{b0.z, b1.z};
        own[2 * g] = self0 + il0; own[2 * g + 1] = self0 + il1;
        pt[2 * g] = il0; pt[2 * g + 1] = il1;
        thr[2 * g] = il0 < m ? inf : -1.0f; thr[2 * g + 1] = il1 < m ? inf : -1.0f;
        cnt[2 * g] = cnt[2 * g + 1] = 0;
    }
    const uint32_t ntiles = j1 > j0 ? (j1 - j0 + TILE - 1) / TILE : 0;

    // staging by LDS-DMA, as nb_nbr_pk: whole tiles from a scalar base, the last one per lane with rows past the range taken
    // from inf_row (d2 = +inf: below no threshold)
    const uint32_t lds_wave = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4*)&tile[0][tid & ~63]);
    const uint32_t lane_off = (uint32_t)tid * 16u;
    auto stage = [&](uint32_t t, int buf) {
        // wave-uniform, and said so: with the slow path's loops around, the compiler keeps the tile counter in a vector register
        const uint32_t jt = __builtin_amdgcn_readfirstlane(j0 + t * TILE);
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_wave + (uint32_t)(buf * TILE) * 16u);
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
    // where the tile can hold it, and the OR of all compares against the thresholds.
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
                hit |= d2[uu][c].x < thr[q0];
                hit |= d2[uu][c].y < thr[q1];
            }
        }
        if (__builtin_amdgcn_ballot_w64(hit) != 0) {          // wave-uniform: some lane has a candidate in these U rows
            if constexpr (STATS) nslow += 1;
#pragma unroll
            for (int uu = 0; uu < U / JB; ++uu) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {                // c = u * NG + g: a point meets its rows in ascending j
                    const uint32_t j = jrow + (uint32_t)(uu * JB + c / NG);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int q = 2 * (c % NG) + e;
                        const float d = e ? d2[uu][c].y : d2[uu][c].x;
                        const bool in = d < thr[q];
                        if (__builtin_amdgcn_ballot_w64(in) != 0) {
                            if (in && pt[q] < m && cnt[q] < cap) work[(row0 + pt[q]) * cap + cnt[q]] = knn_row<float>::pack(d, j);
                            cnt[q] += in ? 1u : 0u;
                            if constexpr (STATS) ncand[q] += in ? 1u : 0u;
                        }
                    }
                }
            }
            // the rows that could not take another group: the wave compacts them one by one
#pragma unroll
            for (int q = 0; q < 2 * NG; ++q) {
                uint64_t full = __builtin_amdgcn_ballot_w64(cnt[q] + (uint32_t)U > cap);
                while (full) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(full);
                    full &= full - 1;
                    const uint32_t pl = knn_lane(pt[q], l), cl = knn_lane(cnt[q], l);
                    const float t = knn_compact<float, false>(work + (row0 + pl) * cap, cl < cap ? cl : cap, k, lane);
                    thr[q] = lane == l ? t : thr[q];
                    cnt[q] = lane == l ? k : cnt[q];           // (cl > cap - U >= k)
                    if constexpr (STATS) ncomp[q] += lane == l ? 1u : 0u;
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

    // the end of the chunk: every row of a point < m sorted and padded to k entries
#pragma unroll
    for (int q = 0; q < 2 * NG; ++q) {
        uint64_t live = __builtin_amdgcn_ballot_w64(pt[q] < m);
        while (live) {
            const uint32_t l = (uint32_t)__builtin_ctzll(live);
            live &= live - 1;
            const uint32_t pl = knn_lane(pt[q], l), cl = knn_lane(cnt[q], l);
            (void)knn_compact<float, true>(work + (row0 + pl) * cap, cl < cap ? cl : cap, k, lane);
        }
    }
    if constexpr (STATS) {
#pragma unroll
        for (int q = 0; q < 2 * NG; ++q)
            if (pt[q] < m) stat_rows[row0 + pt[q]] = uint2{ncand[q], ncomp[q]};
        if (lane == 0) stat_waves[(blockIdx.y * gridDim.x + blockIdx.x) * (kBlock / 64) + tid / 64] = nslow;
    }
}

// f64 handles: nb_nbl64's frame -- one point per lane, the j-tile staged through registers with the rows past the chunk's end at
// +inf, fp64 throughout -- with the same threshold, the same working rows (16-byte entries) and the same compaction.
template <typename T, bool STATS = false>
__global__ __launch_bounds__(kBlock) void nb_knn64(const typename vec4<T>::type* __restrict__ bodies,
                                                  const typename vec4<T>::type* __restrict__ points, uint4* __restrict__ work,
                                                  uint32_t n, uint32_t m, uint32_t j_per_chunk, uint32_t k, uint32_t at_bodies,
                                                  uint32_t self0, uint2* __restrict__ stat_rows, uint32_t* __restrict__ stat_waves)
{
    constexpr int U = kKnnU;
    __shared__ double4 tile[kTile];
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint32_t il = blockIdx.x * kNbrRows64 + tid;
    const uint32_t ic = il < m ? il : m - 1;                         // clamped (never stored)
    const uint32_t j0 = blockIdx.y * j_per_chunk;
    const uint32_t j1 = j0 + j_per_chunk < n ? j0 + j_per_chunk : n;
    const auto pt = ld4(points + ic);
    const double xi = (double)pt.x, yi = (double)pt.y, zi = (double)pt.z;
    const uint32_t own = at_bodies ? self0 + il : kNbrNone;         // n <= 2^30: never a row
    const double inf = __builtin_huge_val();
    const uint32_t cap = knn_cap(k);
    const size_t row0 = (size_t)blockIdx.y * m;
    double thr = il < m ? inf : -1.0;                                // a lane past m has no candidate
    uint32_t cnt = 0;
    uint32_t ncand = 0, ncomp = 0, nslow = 0;                         // STATS only
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
                hit |= d2[u] < thr;
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {          // some lane of the wave has a candidate among these U rows
                if constexpr (STATS) nslow += 1;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = d2[u] < thr;
                    if (__builtin_amdgcn_ballot_w64(in) != 0) {
                        if (in && il < m && cnt < cap) work[(row0 + il) * cap + cnt] = knn_row<double>::pack(d2[u], jt + (uint32_t)(jj + u));
                        cnt += in ? 1u : 0u;
                        if constexpr (STATS) ncand += in ? 1u : 0u;
                    }
                }
                uint64_t full = __builtin_amdgcn_ballot_w64(cnt + (uint32_t)U > cap);
                while (full) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(full);
                    full &= full - 1;
                    const uint32_t pl = knn_lane(il, l), cl = knn_lane(cnt, l);
                    const double t = knn_compact<double, false>(work + (row0 + pl) * cap, cl < cap ? cl : cap, k, lane);
                    thr = lane == l ? t : thr;
                    cnt = lane == l ? k : cnt;
                    if constexpr (STATS) ncomp += lane == l ? 1u : 0u;
                }
            }
        }
    }
    uint64_t live = __builtin_amdgcn_ballot_w64(il < m);
    while (live) {
        const uint32_t l = (uint32_t)__builtin_ctzll(live);
        live &= live - 1;
        const uint32_t pl = knn_lane(il, l), cl = knn_lane(cnt, l);
        (void)knn_compact<double, true>(work + (row0 + pl) * cap, cl < cap ? cl : cap, k, lane);
    }
    if constexpr (STATS) {
        if (il < m) stat_rows[row0 + il] = uint2{ncand, ncomp};
        if (lane == 0) stat_waves[(blockIdx.y * gridDim.x + blockIdx.x) * (kBlock / 64) + tid / 64] = nslow;
    }
}

// One lane per point: merges the point's sorted chunk rows (k entries each, padded with (+inf, none)) under (d2, j) and writes the
// outputs that were asked for -- nb_nbl_offsets' counterpart.  heads: one byte per (chunk, lane) in dynamic LDS, chunks * 64
// bytes (a register array indexed by the chunk would be scratch); a lane reads and writes its own bytes only.
template <typename T>
__global__ __launch_bounds__(kKnnMergeLanes) void nb_knn_merge(const typename knn_row<T>::type* __restrict__ work, uint32_t m,
                                                              uint32_t chunks, uint32_t k, uint32_t* __restrict__ index,
                                                              T* __restrict__ dist2)
{
    using R = knn_row<T>;
    extern __shared__ uint8_t knn_heads[];
    const uint32_t lane = threadIdx.x;
    const uint32_t il = blockIdx.x * kKnnMergeLanes + lane;
    if (il >= m) return;
    const uint32_t cap = knn_cap(k);
    const T inf = (T)__builtin_huge_val();
    for (uint32_t c = 0; c < chunks; ++c) knn_heads[c * kKnnMergeLanes + lane] = 0;
    for (uint32_t t = 0; t < k; ++t) {
        T best = inf;
        uint32_t bj = kNbrNone, bc = 0;
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t h = knn_heads[c * kKnnMergeLanes + lane];
            if (h < k) {
                const auto e = work[((size_t)c * m + il) * cap + h];
                const T d = R::d2(e);
                const uint32_t j = R::j(e);
                if (knn_less(d, j, best, bj)) { best = d; bj = j; bc = c; }
            }
        }
        if (bj != kNbrNone) knn_heads[bc * kKnnMergeLanes + lane] += 1;
        if (index) index[(size_t)il * k + t] = bj;
        if (dist2) dist2[(size_t)il * k + t] = best;
    }
}

}  // namespace nb
