// nb_engine.hip -- C ABI (include/nbody3d_hip.h) over the HIP particle pool
// and the gfx950 kernels in nb_kernels.hip.h: the single-handle entry points.
// (nb_comm.hip holds the RCCL collective and the single-process multi-device handle.)
//
// Device state per handle (reference layout float4 AoS,
// nbody3d.js:179-199, kept as-is on the device because one 16-B lane access is
// the widest coalesced load and the j-tile is read back as one ds_read_b128):
//   bodies  : 4*n elements, replicated on every shard (x, y, z, mass); a fused handle keeps two
//             (ping-pong: a step reads one and writes the other)
//   vel     : 4*shard_count elements
//   accel   : 4*shard_count elements (acceleration of the previous step)
//   partial : jsplit * 4*shard_count elements (K1 output, summed by K2; none when fused)
#include "nb_internal.h"
#include "nb_kernels.hip.h"
#include "../../include/nbody3d_hip_plan.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

namespace {
thread_local std::string g_create_error = "";
}

namespace nbi {
int fail(nb_sim* s, int code, const std::string& msg)
{
    if (s) s->err = msg; else g_create_error = msg;
    return code;
}
void set_create_error(const std::string& msg) { g_create_error = msg; }
const std::string& create_error() { return g_create_error; }
}  // namespace nbi

namespace {

using nbi::fail;

#define NB_HIP(s, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return fail((s), NB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));              \
    } while (0)

using namespace nbp;     // Kind, Shape, ceil_div, ipb_of, ... (nb_plan.h)

// ---- kernel tables ---------------------------------------------------------------------------
// packed LDS kernels: NG in {1,2,4}, LS in {1,2,4,8,16,32,64}, TL = 1; TL = 4 for LS >= 16
// (a tile of 256 bodies is only 256/LS loop iterations: short loops want 1024 staged at once)
#define NB_LS_CASES(F, NG, TL, ls)                                      \
    switch (ls) {                                                        \
        case 1: return (const void*)&nb::F<NG, 1, TL>;                   \
        case 2: return (const void*)&nb::F<NG, 2, TL>;                   \
        case 4: return (const void*)&nb::F<NG, 4, TL>;                   \
        case 8: return (const void*)&nb::F<NG, 8, TL>;                   \
        case 16: return (const void*)&nb::F<NG, 16, TL>;                 \
        case 32: return (const void*)&nb::F<NG, 32, TL>;                 \
        case 64: return (const void*)&nb::F<NG, 64, TL>;                 \
        default: return nullptr;                                         \
    }
#define NB_LS_CASES_T4(F, NG, ls)                                       \
    switch (ls) {                                                        \
        case 16: return (const void*)&nb::F<NG, 16, 4>;                  \
        case 32: return (const void*)&nb::F<NG, 32, 4>;                  \
        case 64: return (const void*)&nb::F<NG, 64, 4>;                  \
        default: return nullptr;                                         \
    }
#define NB_LS_CASES_T8(F, NG, ls)                                       \
    switch (ls) {                                                        \
        case 32: return (const void*)&nb::F<NG, 32, 8>;                  \
        case 64: return (const void*)&nb::F<NG, 64, 8>;                  \
        default: return nullptr;                                         \
    }
#define NB_PK_TABLE(NAME, F)                                            \
    const void* NAME(int ng, int ls, int tl)                            \
    {                                                                    \
        if (tl == 8) {          /* 2048-body stages: 64 KiB of LDS, <= 2 workgroups per CU */ \
            if (ng == 1) { NB_LS_CASES_T8(F, 1, ls) }                    \
            if (ng == 2) { NB_LS_CASES_T8(F, 2, ls) }                    \
            if (ng == 4) { NB_LS_CASES_T8(F, 4, ls) }                    \
        }                                                                \
        if (tl == 1) {                                                   \
            if (ng == 1) { NB_LS_CASES(F, 1, 1, ls) }                    \
            if (ng == 2) { NB_LS_CASES(F, 2, 1, ls) }                    \
            if (ng == 4) { NB_LS_CASES(F, 4, 1, ls) }                    \
        } else if (tl == 4) {                                            \
            if (ng == 1) { NB_LS_CASES_T4(F, 1, ls) }                    \
            if (ng == 2) { NB_LS_CASES_T4(F, 2, ls) }                    \
            if (ng == 4) { NB_LS_CASES_T4(F, 4, ls) }                    \
        }                                                                \
        return nullptr;                                                  \
    }
NB_PK_TABLE(pk_force_kernel, nb_force_pk)
NB_PK_TABLE(pk_fused_kernel, nb_step_fused)

template <typename T>
const void* scalar_kernel(int ipl, int ls)
{
    if (ls == 1) {
        if (ipl == 1) return (const void*)&nb::nb_force<T, 1, 1>;
        if (ipl == 2) return (const void*)&nb::nb_force<T, 2, 1>;
        if (ipl == 4) return (const void*)&nb::nb_force<T, 4, 1>;
        return nullptr;
    }
    if (ipl != 1) return nullptr;
    if (ls == 4) return (const void*)&nb::nb_force<T, 1, 4>;
    if (ls == 16) return (const void*)&nb::nb_force<T, 1, 16>;
    if (ls == 64) return (const void*)&nb::nb_force<T, 1, 64>;
    return nullptr;
}

const void* sgpr_kernel(int ipl, int ws)
{
    if (ipl == 4 && ws == 5) return (const void*)&nb::nb_force_pk_sgpr<2, 4, true>;     // 64-bit pair loads
    if (ipl == 4) return ws == 4 ? (const void*)&nb::nb_force_pk_sgpr<2, 4> : (const void*)&nb::nb_force_pk_sgpr<2, 1>;
    if (ipl == 8 && ws == 5) return (const void*)&nb::nb_force_pk_sgpr<4, 4, true>;     // A/B arm: 64-bit pair loads
    if (ipl == 8) return ws == 4 ? (const void*)&nb::nb_force_pk_sgpr<4, 4> : (const void*)&nb::nb_force_pk_sgpr<4, 1>;
    return nullptr;
}

// The rank form's force kernel (two phases: nb::SymRankPlan); ipl = residents per lane.
const void* rank_kernel_of(bool f64, int ipl)
{
    if (f64) return ipl == 8 ? (const void*)&nb::nb_force_symw64_rank<8> : nullptr;
    return ipl == 16 ? (const void*)&nb::nb_force_symw_rank<8> : ipl == 8 ? (const void*)&nb::nb_force_symw_rank<4> : nullptr;
}

// The kernel a shape launches (nullptr: no such instantiation).
// single_sweeps (NB_FLAG_SINGLE_SWEEPS): the wave-granular symmetric pass with one traveler per lane runs every sweep on its own.
// form: 0 the general kernels, 1 the equal-mass form of that pass, 2 the equal-mass form with unit mass product (eqm_form below; only the
// shapes eqm_shape names have the two).
bool eqm_shape(bool f64, const Shape& sh) { return !f64 && sh.kind == kSym && sh.ls == 1 && sh.x == 3 && (sh.ipl == 8 || sh.ipl == 16); }
const void* kernel_of(bool f64, const Shape& sh, bool single_sweeps = false, int form = 0)
{
    if (form == 2) {
        if (!eqm_shape(f64, sh)) return nullptr;
        if (sh.ipl == 8) return single_sweeps ? (const void*)&nb::nb_force_symw_unit<4, 1> : (const void*)&nb::nb_force_symw_pairs_unit<4>;
        return single_sweeps ? (const void*)&nb::nb_force_symw_unit<8, 1> : (const void*)&nb::nb_force_symw_pairs_unit<8>;
    }
    if (form == 1) {
        if (!eqm_shape(f64, sh)) return nullptr;
        if (sh.ipl == 8) return single_sweeps ? (const void*)&nb::nb_force_symw_eqm<4, 1> : (const void*)&nb::nb_force_symw_pairs_eqm<4>;
        return single_sweeps ? (const void*)&nb::nb_force_symw_eqm<8, 1> : (const void*)&nb::nb_force_symw_pairs_eqm<8>;
    }
    switch (sh.kind) {
        case kScalar: return f64 ? scalar_kernel<double>(sh.ipl, sh.ls) : scalar_kernel<float>(sh.ipl, sh.ls);
        case kPkLds: return f64 || (sh.ipl & 1) ? nullptr : pk_force_kernel(sh.ipl / 2, sh.ls, sh.x);
        case kFused: return f64 || (sh.ipl & 1) ? nullptr : pk_fused_kernel(sh.ipl / 2, sh.ls, sh.x);
        case kPkSgpr: return f64 || sh.ls != 1 || !(sh.x == 1 || sh.x == 4 || sh.x == 5) ? nullptr : sgpr_kernel(sh.ipl, sh.x);
        case kDirect:
            if (f64 || sh.ipl != 2 || sh.ls != 64) return nullptr;
            return sh.x == 1 ? (const void*)&nb::nb_step_direct<16> : sh.x == 2 ? (const void*)&nb::nb_step_direct<32> : nullptr;
        case kSym:       // ipl = residents per lane (8 or 16); x = 1 / 3: wave-granular form with 2 / 1 travelers per lane,
                         // x = 4: workgroup form (4 waves, 8 residents per lane)
            if (sh.ls != 1) return nullptr;
            if (f64) return sh.ipl == 8 && sh.x == 3 ? (const void*)&nb::nb_force_symw64<8> : nullptr;      // 8 residents, 1 traveler per lane
            if (sh.x == 4) return sh.ipl == 8 ? (const void*)&nb::nb_force_sym<4, 4, 2> : nullptr;
            if (sh.ipl == 4) return sh.x == 3 ? (const void*)&nb::nb_force_symw<2, 1> : nullptr;      // (an arm: whole sweeps round finer with 4 residents)
            if (sh.ipl == 8 && sh.x == 3) return single_sweeps ? (const void*)&nb::nb_force_symw<4, 1> : (const void*)&nb::nb_force_symw_pairs<4>;
            if (sh.ipl == 16 && sh.x == 3) return single_sweeps ? (const void*)&nb::nb_force_symw<8, 1> : (const void*)&nb::nb_force_symw_pairs<8>;
            if (sh.ipl == 8) return sh.x == 1 ? (const void*)&nb::nb_force_symw<4, 2> : nullptr;
            if (sh.ipl == 16) return sh.x == 1 ? (const void*)&nb::nb_force_symw<8, 2> : nullptr;
            return nullptr;
        case kJpk:
            if (f64 || sh.ipl != 1 || sh.ls != 1) return nullptr;
            return sh.x == 4 ? (const void*)&nb::nb_step_jpk<4> : sh.x == 8 ? (const void*)&nb::nb_step_jpk<8>
                   : sh.x == 6 ? (const void*)&nb::nb_step_jpk<16> : nullptr;
        default: return nullptr;
    }
}

// Runs the planner (nb_plan.cpp) for a handle and copies its answer into the handle's launch fields.
void plan_handle(nb_sim* s, const nb_config& cfg, int n_cu, double clock_hz, double device_mem)
{
    PlanInput in;
    if (device_mem > 0) in.device_mem = device_mem;
    in.n = s->n; in.sb = s->sb; in.sc = s->sc; in.f64 = s->f64; in.cfg = cfg; in.n_cu = n_cu; in.clock_hz = clock_hz;
    if (!s->no_device)
        in.occupancy = [f64 = s->f64](const Shape& sh, int block) {
            int occ = 0;
            const void* fn = kernel_of(f64, sh);
            if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, block, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
            return occ;
        };
    LaunchPlan p = plan_launch(in);
    s->ipl = p.ipl; s->ls = p.ls; s->ws = p.ws; s->tl = p.tl;
    s->packed = p.packed; s->sgpr = p.sgpr; s->fused = p.fused; s->direct = p.direct; s->jpk = p.jpk; s->swap_acc = p.swap_acc;
    s->jsplit = p.jsplit; s->j_per_split = p.j_per_split; s->junits = p.junits; s->own_split0 = p.own_split0; s->own_splits = p.own_splits;
    s->sym = p.sym; s->symw = p.symw; s->sym_rank = p.sym_rank;
    s->sym_np = p.sym_np; s->sym_layers = p.sym_layers; s->sym_g0 = p.sym_g0; s->sym_g1 = p.sym_g1;
    static_assert(sizeof(s->sym_plan) == sizeof(p.sym_plan), "nb_sim::sym_plan mirrors LaunchPlan::sym_plan");
    memcpy(s->sym_plan, p.sym_plan, sizeof s->sym_plan);
    static_assert(sizeof(s->sym_rank_plan) == sizeof(p.sym_rank_plan), "nb_sim::sym_rank_plan mirrors LaunchPlan::sym_rank_plan");
    memcpy(s->sym_rank_plan, p.sym_rank_plan, sizeof s->sym_rank_plan);
    s->sym_passes = std::move(p.sym_passes);
    s->sym_local = p.sym_local;
    s->sym_tab_host = std::move(p.sym_tab_host);
    s->sym_spill_rows = p.sym_spill_rows;
    s->sym_pieces = p.sym_pieces;
    s->variant = std::move(p.variant);
}

Shape shape_of(const nb_sim* s)
{
    if (s->sym) return {kSym, s->ipl, 1, s->ws};
    if (s->jpk) return {kJpk, 1, 1, s->ws};
    if (s->direct) return {kDirect, s->ipl, s->ls, s->tl};
    if (s->fused) return {kFused, s->ipl, s->ls, s->tl};
    if (s->sgpr) return {kPkSgpr, s->ipl, 1, s->ws};
    if (s->packed) return {kPkLds, s->ipl, s->ls, s->tl};
    return {kScalar, s->ipl, s->ls, 1};
}

// Rows of one partial-sum layer of a symmetric handle: the padded system, or (rank form: compact layers) the handle's own super-blocks.
size_t sym_layer_rows(const nb_sim* s) { return s->sym_rank ? (size_t)(s->sym_g1 - s->sym_g0) * ipb_of(shape_of(s)) : (size_t)s->sym_np; }

// The packed f32 K1 forms stream their j-bodies as (x, y, z, G*m) rows (nb_internal.h, `gm`).
bool streams_gm(const nb_sim* s) { return !s->f64 && s->packed && !s->jpk; }
bool gm_active(const nb_sim* s) { return streams_gm(s) && (float)s->G != 1.0f; }
const void* jstream(const nb_sim* s, int k) { return gm_active(s) ? s->gm[k] : s->bodies[k]; }

// Makes gm[cur] current (allocates on first use; a no-op for G == 1 and for the kernels that fold G themselves).
int ensure_gm(nb_sim* s)
{
    if (!gm_active(s)) { s->gm_ok = false; return NB_OK; }      // steps taken meanwhile leave any old copy behind
    const size_t bytes = (size_t)16 * (s->sym ? s->sym_np : s->n);
    for (int k = 0; k < (s->fused ? 2 : 1); ++k)
        if (!s->gm[k]) {
            NB_HIP(s, hipMalloc(&s->gm[k], bytes));
            if (s->sym) NB_HIP(s, hipMemsetAsync(s->gm[k], 0, bytes, s->stream));     // zero-mass rows past n
        }
    if (s->gm_ok && s->gm_G == s->G) return NB_OK;
    const float4* b = (const float4*)s->bodies[s->cur];
    float4* g = (float4*)s->gm[s->cur];
    uint32_t n = s->n;
    float G = (float)s->G;
    void* args[] = {&b, &g, &n, &G};
    NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_gm_pack<0>, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    s->gm_ok = true; s->gm_G = s->G;
    return NB_OK;
}

// The equal-mass kernels run while the handle's state is known to be an equal-mass system (nb_sim::eqm) and nothing rewrites its rows
// between steps (an exchange hook or a communicator may); a dt that is not finite would turn the zero w lanes into NaN (0 * inf).
bool eqm_active(const nb_sim* s) { return s->eqm_capable && s->eqm == nb_sim::kEqmYes && !s->xfn && !s->rccl && std::isfinite((float)s->dt); }

// The force kernels' form: 0 general, 1 equal masses, 2 equal masses with unit mass product (kernels/symmetric.hip.h, `UNIT`).  Form 2 asks of
// the scalar the kernel streams -- the w lane of row 0 of the j-stream: m0 when G = 1, else (float)G * m0 as nb_gm_pack forms it -- that it be
// a power of two (zero mantissa, positive, normal) with an exponent in [-32, 32]: gm * inv >= 2^-96 stays normal in the form-1 kernels the
// bytes are held to (inv = rsq(d2^3) >= 2^-64), and the unscaled sums are at most 2^32 times the scaled ones.  The window bounds the
// products only: a SUM that is subnormal when scaled (an acceleration component below about 2^-126, met on its way or at the end) is
// rounded or flushed in form 1 and not in form 2, and there the two forms may differ in that component's last bits -- the identity
// holds while the scaled sums themselves stay normal, which no system of physical interest leaves.  Derived from the current G:
// nb_set_params switches the form without a new check.
int eqm_form(const nb_sim* s)
{
    if (!eqm_active(s)) return 0;
    if (s->no_eqm_pow2) return 1;
    float m0;
    memcpy(&m0, &s->eqm_m0, sizeof m0);
    const float gm = (float)s->G != 1.0f ? (float)s->G * m0 : m0;      // (gm_active, nb_gm_pack)
    uint32_t bits;
    memcpy(&bits, &gm, sizeof bits);
    const int e = (int)(bits >> 23) - 127;        // (sign set: e >= 129)
    return (bits & 0x007fffffu) == 0u && e >= -32 && e <= 32 ? 2 : 1;
}

// Makes nb_sim::eqm known: one small launch and one host wait, once per invalidation (an upload decides on the host instead).
int ensure_eqm(nb_sim* s)
{
    if (!s->eqm_capable || s->eqm != nb_sim::kEqmUnknown) return NB_OK;
    const float4 *b = (const float4*)s->bodies[s->cur], *v = (const float4*)s->vel, *a = (const float4*)s->acc;
    uint32_t n = s->n, found = 1, m0 = 0;
    uint32_t* flag = s->eqm_flag;
    void* args[] = {&b, &v, &a, &n, &flag};
    NB_HIP(s, hipMemsetAsync(flag, 0, sizeof(uint32_t), s->stream));
    NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_eqm_check<0>, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    NB_HIP(s, hipMemcpyAsync(&found, flag, sizeof found, hipMemcpyDeviceToHost, s->stream));
    // row 0's mass lane, in the same wait: with the current G it decides the form (eqm_form); used only if the system is an equal-mass one
    NB_HIP(s, hipMemcpyAsync(&m0, (const char*)s->bodies[s->cur] + 12, sizeof m0, hipMemcpyDeviceToHost, s->stream));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    s->eqm = found ? nb_sim::kEqmNo : nb_sim::kEqmYes;
    if (!found) s->eqm_m0 = m0;
    return NB_OK;
}

// part: 0 = all splits, 1 = only the splits inside this shard's own rows,
//       2 = all the others
// t0/t1 (optional): events stamped at the kernel's begin / end (hipExtLaunchKernel)
void launch_kernel(const void* fn, dim3 grid, dim3 block, void** args, hipStream_t stream, hipEvent_t t0, hipEvent_t t1)
{
    // error picked up by hipGetLastError in nb_step
    if (t0 || t1) (void)hipExtLaunchKernel(fn, grid, block, args, 0, stream, t0, t1, 0);
    else (void)hipLaunchKernel(fn, grid, block, args, 0, stream);
}

template <typename T>
void launch_force(nb_sim* s, int part = 0, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr)
{
    using V4 = typename nb::vec4<T>::type;
    const Shape sh = shape_of(s);
    if (s->sym_rank) {
        // part 0: every wave; 1: phase A (travelers = own rows; nothing of the other ranks is read); 2: phase B
        const nbp::LaunchPlan::SymPass& ps = s->sym_passes[s->sym_pass];
        nb::SymRankPlan rp;
        memcpy(&rp, ps.plan, sizeof rp);
        uint32_t w0 = part == 2 ? rp.WA : 0u, w1 = part == 1 ? rp.WA : rp.WA + rp.WB;
        if (w1 <= w0) return;
        const void* b = jstream(s, s->cur);
        void* p = s->partial;
        const uint32_t* tab = s->sym_tab + ps.tab_off;
        uint32_t n = s->n, k_lo = ps.k_lo, k_hi = ps.k_hi, d0 = ps.d0;
        void* sp = s->sym_spill;
        if (s->f64) {
            double G = s->G, e2 = s->eps2;
            void* args[] = {&b, &p, &tab, &rp, &n, &G, &e2, &w0, &w1, &sp, &k_lo, &k_hi, &d0};
            launch_kernel(rank_kernel_of(true, sh.ipl), dim3(ceil_div(w1 - w0, 4u)), dim3(256), args, s->stream, t0, t1);
        } else {
            float e2 = (float)s->eps2;
            void* args[] = {&b, &p, &tab, &rp, &n, &e2, &w0, &w1, &sp, &k_lo, &k_hi, &d0};
            launch_kernel(rank_kernel_of(false, sh.ipl), dim3(ceil_div(w1 - w0, 4u)), dim3(256), args, s->stream, t0, t1);
        }
        return;
    }
    if (s->symw) {
        nb::SymWPlan pl;
        memcpy(&pl, s->sym_plan, sizeof pl);
        const void* b = jstream(s, s->cur);                // f32: rows (x, y, z, G*m); f64: (x, y, z, m) and G
        void* p = s->partial;
        const uint32_t* tab = s->sym_tab;
        void* sp = s->sym_spill;                           // one row set per wave (wave ranges cut inside sweeps); null with whole sweeps
        // (the order of kernels/symmetric.hip.h SYMW_PLAN_PARAMS: the table pointer and the plan words inside the preloaded 14 dwords)
        uint32_t* queue = s->sym_queue;
        uint32_t npieces = s->sym_pieces, pieces_off = 2u * (pl.np / ipb_of(sh)) + 4u * pl.W;      // the queued sweeps behind the wave records (lay_out_symw)
        // the queue's draw counter.  A reset that fails would leave the last launch's count (>= npieces): every wave would skip the queue
        // and K2 would add the piece layers' stale sums -- so the error is kept for the caller (nb_step, ensure_graph, nb_force_pass)
        if (npieces) { const hipError_t e = hipMemsetAsync(queue, 0, sizeof(uint32_t), s->stream); if (e != hipSuccess) s->force_err = e; }
        if (s->f64) {
            double G = s->G, e2 = s->eps2;
            void* args[] = {&tab, &b, &p, &sp, &pl.W, &pl.ups, &pl.nsb, &pl.zc, &pl.r_layer0, &pl.t_layer0, &G, &e2, &queue, &npieces, &pieces_off};
            launch_kernel(kernel_of(true, sh), dim3(ceil_div(pl.W, 4u)), dim3(256), args, s->stream, t0, t1);
        } else {
            float e2 = (float)s->eps2;
            void* args[] = {&tab, &b, &p, &sp, &pl.W, &pl.ups, &pl.nsb, &pl.zc, &pl.r_layer0, &pl.t_layer0, &e2, &queue, &npieces, &pieces_off};
            launch_kernel(kernel_of(false, sh, s->single_sweeps, eqm_form(s)), dim3(ceil_div(pl.W, 4u)), dim3(256), args, s->stream, t0, t1);
        }
        return;
    }
    if (s->sym) {
        nb::SymPlan pl;
        memcpy(&pl, s->sym_plan, sizeof pl);
        const float4* b = (const float4*)jstream(s, s->cur);
        nb::SymRow* p = (nb::SymRow*)s->partial;       // 12-byte rows
        float e2 = (float)s->eps2;
        uint32_t n = s->n;
        void* args[] = {&b, &p, &pl, &n, &e2};
        launch_kernel(kernel_of(false, sh), dim3(pl.nsb * pl.q), dim3(64 * sh.x), args, s->stream, t0, t1);
        return;
    }
    nb::SplitWindow win{0, 0xffffffffu, 0};
    uint32_t ny = s->jsplit;
    if (part == 1) { win.base = s->own_split0; ny = s->own_splits; }
    else if (part == 2) { win.hole_begin = s->own_split0; win.hole_count = s->own_splits; ny = s->jsplit - s->own_splits; }
    if (ny == 0) return;
    dim3 grid(ceil_div(s->sc, ipb_of(sh)), ny), block(nb::kBlock);
    const V4* b = (const V4*)jstream(s, s->cur);    // packed f32 forms: rows (x, y, z, G*m); scalar template: (x, y, z, m) and G
    V4* p = (V4*)s->partial;
    T G = (T)s->G, e2 = (T)s->eps2;
    uint32_t n = s->n, sb = s->sb, sc = s->sc, jps = s->j_per_split;
    const V4* zr = (const V4*)s->zero_row;          // LDS-DMA source for j past the range (packed LDS-tile kernels)
    void* args[] = {&b, &p, &n, &sb, &sc, &G, &e2, &jps, &win, &zr};   // every K1 form declares exactly these ten parameters
    launch_kernel(kernel_of(s->f64, sh), grid, block, args, s->stream, t0, t1);
}

// The fused one-launch step: reads bodies[cur], writes bodies[cur ^ 1], then the roles flip.
// The pair-transposed copy the j-packed step streams from: rebuilt from bodies[cur] whenever the positions
// were written from outside the step (upload, a raw device pointer handed out) or G changed (it is folded
// into the mass lanes); the step itself keeps it current.
void ensure_pairs(nb_sim* s)
{
    if (!s->jpk || (s->pairs_ok && s->pairs_G == s->G)) return;
    const float4* b = (const float4*)s->bodies[s->cur];
    float4* p = (float4*)s->pairs[s->cur];
    uint32_t n = s->n;
    float G = (float)s->G;
    void* args[] = {&b, &p, &n, &G};
    (void)hipLaunchKernel((const void*)&nb::nb_pairs_pack<0>, dim3(ceil_div(ceil_div(n, 2u), nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream);
    s->pairs_ok = true; s->pairs_G = s->G;
}

void launch_jpk(nb_sim* s, hipEvent_t t0, hipEvent_t t1)
{
    const Shape sh = shape_of(s);
    dim3 grid(ceil_div(s->n, 64u), s->jsplit), block(64 * jpk_ws(sh.x));
    const float4 *bin = (const float4*)s->bodies[s->cur], *pin = (const float4*)s->pairs[s->cur];
    float4 *bout = (float4*)s->bodies[s->cur ^ 1], *pout = (float4*)s->pairs[s->cur ^ 1];
    float4 *v = (float4*)s->vel, *a = (float4*)s->acc, *part = (float4*)s->jpartial;
    uint32_t* tk = s->tickets;
    uint32_t n = s->n, upw = s->junits, poison = (s->poison ? 1u : 0u) | (s->jpk_fenced ? 2u : 0u);
    float G = (float)s->G, e2 = (float)s->eps2, dt = (float)s->dt;
    void* args[] = {&bin, &pin, &bout, &pout, &v, &a, &part, &tk, &n, &upw, &poison, &G, &e2, &dt};
    launch_kernel(kernel_of(false, sh), grid, block, args, s->stream, t0, t1);
    s->cur ^= 1;
}

void launch_fused(nb_sim* s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr)
{
    if (s->jpk) { ensure_pairs(s); launch_jpk(s, t0, t1); return; }
    const Shape sh = shape_of(s);
    dim3 grid(ceil_div(s->n, ipb_of(sh))), block(nb::kBlock);
    const float4 *bin = (const float4*)s->bodies[s->cur], *jin = (const float4*)jstream(s, s->cur);
    float4 *bout = (float4*)s->bodies[s->cur ^ 1], *gout = gm_active(s) ? (float4*)s->gm[s->cur ^ 1] : nullptr;
    float4 *v = (float4*)s->vel, *a = (float4*)s->acc;
    uint32_t n = s->n;
    float G = (float)s->G, e2 = (float)s->eps2, dt = (float)s->dt;
    const float4* zr = (const float4*)s->zero_row;
    void* args[] = {&bin, &jin, &bout, &gout, &v, &a, &n, &G, &e2, &dt, &zr};   // nb_step_fused and nb_step_direct: the same eleven
    launch_kernel(kernel_of(false, sh), grid, block, args, s->stream, t0, t1);
    s->cur ^= 1;
}

template <typename T>
void launch_integrate(nb_sim* s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr)
{
    using V4 = typename nb::vec4<T>::type;
    V4 *b = (V4*)s->bodies[s->cur], *v = (V4*)s->vel;
    uint32_t sb = s->sb, sc = s->sc, js = s->jsplit;
    T dt = (T)s->dt, G = (T)s->G;
    // the j-stream rows of the new positions; a handle whose rows are exchanged rebuilds the whole copy after the gather instead
    V4* gout = gm_active(s) && !(s->xfn || s->rccl) ? (V4*)s->gm[s->cur] : nullptr;
    if (s->sym_rank) {
        // A rank-form handle (a shard, or a whole system whose ring distances go in passes) has no layered integrate: its sums
        // are reduced into sym_A by nb_sym_reduce and the PLAIN integrate kernel reads the handle's rows of it (sym_rank_phase_b_t).
        // lay_out_symw_rank also sets `symw` (its SymWPlan is a summary for the reports): without this branch nb_integrate_symw would
        // walk the rank table as {first wave, layers} pairs and stride compact layers by np -- reads far past `partial`.
        V4* a = (V4*)s->acc;
        const V4* p = (const V4*)s->sym_A + sb;
        uint32_t one = 1;
        V4* none = nullptr;                         // the (x, y, z, G*m) copy is rebuilt whole after the position all-gather
        void* args[] = {&b, &v, &a, &p, &sb, &sc, &one, &dt, &none, &G};
        launch_kernel((const void*)&nb::nb_integrate<T, 1>, dim3(ceil_div(sc, nb::kBlock)), dim3(nb::kBlock), args, s->stream, t0, t1);
        return;
    }
    if (s->symw) {
        nb::SymWPlan pl;
        memcpy(&pl, s->sym_plan, sizeof pl);
        V4* aa = (V4*)s->acc;
        const nb::SymRowT<T>* pp = (const nb::SymRowT<T>*)s->partial;
        const uint32_t* tab = s->sym_tab;
        uint32_t n = s->n, S = ipb_of(shape_of(s)), ch_shift = s->ws == 3 ? 6u : 7u;      // travelers per chunk: X = 3 one per lane (64), X = 1 two (128)
        uint32_t shifts = (uint32_t)__builtin_ctz(S) | ch_shift << 8;                       // (S is a power of two: 64 * residents per lane)
        uint32_t spill_off = pl.ups > 1 ? 2u * (pl.np / S) + 4u * pl.W : 0u;                // the spill lists behind the wave records (lay_out_symw)
        const void* sp = s->sym_spill;
        void* args[] = {&tab, &pp, &b, &v, &aa, &n, &shifts, &pl.np, &spill_off, &sp, &gout, &dt, &G, &pl.t_layer0, &pl.r_layer0, &pl.nsb, &pl.n_hi, &pl.H, &pl.zc};
        launch_kernel((const void*)&nb::nb_integrate_symw<T, 8>, dim3(ceil_div(n * 8u, nb::kBlock)), dim3(nb::kBlock), args, s->stream, t0, t1);
        return;
    }
    if (s->sym) {
        if constexpr (std::is_same<T, float>::value) {
            nb::SymPlan pl;
            memcpy(&pl, s->sym_plan, sizeof pl);
            float4 *bb = (float4*)b, *vv = (float4*)v, *aa = (float4*)s->acc, *gg = (float4*)gout;
            const nb::SymRow* pp = (const nb::SymRow*)s->partial;
            uint32_t n = s->n, S = ipb_of(shape_of(s));
            float fdt = (float)s->dt, fG = (float)s->G;
            void* args[] = {&bb, &vv, &aa, &pp, &n, &pl, &S, &fdt, &gg, &fG};
            launch_kernel((const void*)&nb::nb_integrate_sym<8>, dim3(ceil_div(n * 8u, nb::kBlock)), dim3(nb::kBlock), args, s->stream, t0, t1);
        }
        return;
    }
    if (s->swap_acc) {
        // jsplit == 1: the single partial array IS a_new; K2 reads it beside a_old and the two
        // buffers swap roles (no 16-B store of a per body: 96 B per body in all)
        const V4 *ao = (const V4*)s->acc, *an = (const V4*)s->partial;
        void* args[] = {&b, &v, &ao, &an, &sb, &sc, &dt, &gout, &G};
        launch_kernel((const void*)&nb::nb_integrate_swap<T>, dim3(ceil_div(sc, nb::kBlock)), dim3(nb::kBlock), args, s->stream, t0, t1);
        std::swap(s->acc, s->partial);
        s->acc_parity ^= 1;
        return;
    }
    // lanes per body: enough to keep ~8 partial loads per lane at most
    const int R = js >= 32 ? 8 : js >= 8 ? 4 : 1;
    V4* a = (V4*)s->acc;
    const V4* p = (const V4*)s->partial;
    void* args[] = {&b, &v, &a, &p, &sb, &sc, &js, &dt, &gout, &G};
    const void* fn = R == 8 ? (const void*)&nb::nb_integrate<T, 8> : R == 4 ? (const void*)&nb::nb_integrate<T, 4> : (const void*)&nb::nb_integrate<T, 1>;
    launch_kernel(fn, dim3(ceil_div(sc * (uint32_t)R, nb::kBlock)), dim3(nb::kBlock), args, s->stream, t0, t1);
}

void launch_step(nb_sim* s)
{
    if (s->fused) { launch_fused(s); return; }
    if (s->f64) { launch_force<double>(s); launch_integrate<double>(s); }
    else { launch_force<float>(s); launch_integrate<float>(s); }
}

constexpr uint32_t kGraphChunk = 16;   // even: buffer roles (ping-pong, acc swap) are back where they started
constexpr uint32_t kGraphBig = 128;
constexpr uint32_t kGraphSteps[2] = {kGraphChunk, kGraphBig};

void drop_graph(nb_sim* s)
{
    for (auto& g : s->graphs) {
        if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
        if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; }
    }
}

// buffer-role parity a captured graph is valid for
int role_parity(const nb_sim* s) { return s->cur | (s->acc_parity << 1); }

// Captures kGraphSteps[which] steps on the engine's own stream.  Returns false (and disables graphs
// for the handle) if anything goes wrong; the caller then issues plain launches -- same
// kernels, same results.
bool ensure_graph(nb_sim* s, int which)
{
    auto& slot = s->graphs[which];
    if (slot.exec && slot.dt == s->dt && slot.G == s->G && slot.parity == role_parity(s) && slot.form == eqm_form(s)) return true;
    if (slot.exec) { (void)hipGraphExecDestroy(slot.exec); slot.exec = nullptr; }
    if (slot.graph) { (void)hipGraphDestroy(slot.graph); slot.graph = nullptr; }
    void *acc0 = s->acc, *par0 = s->partial;
    const int cur0 = s->cur, par_bit0 = s->acc_parity;
    ensure_pairs(s);             // not part of the captured steps
    if (ensure_gm(s) != NB_OK) { s->graphs_ok = false; return false; }
    if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { s->graphs_ok = false; return false; }
    for (uint32_t k = 0; k < kGraphSteps[which]; ++k) launch_step(s);
    hipGraph_t g = nullptr;
    const bool ok = hipStreamEndCapture(s->stream, &g) == hipSuccess && g;
    s->acc = acc0; s->partial = par0; s->cur = cur0; s->acc_parity = par_bit0;   // an even number of role flips: explicit for clarity
    if (!ok || s->force_err != hipSuccess) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); s->force_err = hipSuccess; s->graphs_ok = false; return false; }
    hipGraphExec_t ge = nullptr;
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(g); (void)hipGetLastError(); s->graphs_ok = false; return false; }
    slot.graph = g; slot.exec = ge; slot.dt = s->dt; slot.G = s->G; slot.parity = role_parity(s); slot.form = eqm_form(s);
    return true;
}

// Makes the engine stream wait for an all-gather started by the two-phase hook / the
// overlapped native collective.
int finish_gather(nb_sim* s)
{
    if (!s->gather_pending) return NB_OK;
    s->gather_pending = false;
    if (s->rccl) return nbi::rccl_exchange_wait(s);
    if (!s->xwait) return NB_OK;
    const int rc = s->xwait(s->xuser, (void*)s->stream);
    if (rc != 0) return fail(s, NB_ERR_COMM, "exchange wait hook failed with code " + std::to_string(rc));
    return NB_OK;
}

int get_events(nb_sim* s, nb_events* out)
{
    if (s->pool_next == s->pool.size()) {
        if (s->pool.size() >= 4096) return 1;   // stop recording, keep running
        nb_events t;
        t.two = t.xchg = t.rs = t.blk = false;
        for (auto& e : t.e)
            if (hipEventCreate(&e) != hipSuccess) return 1;
        s->pool.push_back(t);
    }
    *out = s->pool[s->pool_next++];
    out->two = out->xchg = out->rs = out->blk = false;
    return 0;
}

// Releases what nb_set_neighbor_adapt allocated, switches adaptation off and zeroes its counters.
void ad_release(nb_sim* s)
{
    for (void** p : {&s->ad_built, &s->ad_next, &s->ad_keep})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    s->ad = false;
    s->ad_rebuilds = s->ad_rows_shrunk = 0;
    s->ad_last_rebuilds = 0;
}

// Releases what nb_set_neighbor_levels allocated, switches the levels off and zeroes their counters.
void lv_release(nb_sim* s)
{
    for (void** p : {(void**)&s->lv_lev, (void**)&s->lv_due, (void**)&s->lv_words, (void**)&s->lv_cnt, (void**)&s->lv_rec})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    s->lv = s->lv_frozen = false;
    s->lv_state = 0;
    s->lv_regular = s->lv_ticks = 0;
}

// Releases what nb_set_neighbor_scheme allocated, switches the scheme (and with it adaptation and the levels) off and zeroes its counters.
void ac_release(nb_sim* s)
{
    lv_release(s);
    for (void** p : {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->ac_px, &s->ac_pv, &s->ac_radii, (void**)&s->ac_list, (void**)&s->ac_count, (void**)&s->ac_hdr})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (s->ac_hdr_host) { (void)hipHostFree(s->ac_hdr_host); s->ac_hdr_host = nullptr; }
    s->ac = s->ac_ok = s->ac_over = false;
    s->ac_msg.clear();
    s->ac_regular = s->ac_substeps = s->ac_entries = s->ac_builds = 0;
    s->ac_max_count = s->ac_overflowed = 0;
    ad_release(s);
}

void free_frames(nb_sim* s)
{
    for (auto& f : s->frame) {
        if (f.landed) (void)hipEventSynchronize(f.landed);
        if (f.h_bodies) (void)hipHostFree(f.h_bodies);     // h_speed / d_speed point into the same allocations
        if (f.d_bodies) (void)hipFree(f.d_bodies);
        if (f.packed) (void)hipEventDestroy(f.packed);
        if (f.landed) (void)hipEventDestroy(f.landed);
        f = nb_frame_slot();
    }
    if (s->frame_stream) { (void)hipStreamDestroy(s->frame_stream); s->frame_stream = nullptr; }
    s->frame_next = 0; s->frame_latest = -1;
}

// ---- NB_INT_HERMITE4 ---------------------------------------------------------------------------
constexpr uint32_t kFjWavesPerSimd = 8;        // workgroups a force+jerk launch is cut into, per SIMD, when N x N gives that many
constexpr uint32_t kFjMinChunk = 2048;         // fewest bodies of a j-chunk once there is more than one (two flushes of the first-level sums)
constexpr uint32_t kFjMaxChunk = 1u << 20;     // most bodies of one j-chunk (bounds the second-level sums of nb_fj_pk)

// The j-chunks of a handle's force+jerk pass: enough workgroups for kFjWavesPerSimd per SIMD, in chunks of whole 256-row tiles and
// at least kFjMinChunk bodies; the partial sums (2 x chunks x n rows) stay below ~ 2 x (workgroups wanted x rows per workgroup + n) rows.
void chunk_shape(uint32_t n, uint32_t rows, int n_cu, uint32_t* chunks, uint32_t* per)      // rows: i-bodies of one workgroup
{
    const uint32_t want = kFjWavesPerSimd * (uint32_t)n_cu;
    uint32_t c = std::min(ceil_div(want, ceil_div(n, rows)), n / kFjMinChunk);
    c = std::max(std::max(c, 1u), ceil_div(n, kFjMaxChunk));
    *per = ceil_div(ceil_div(n, c), (uint32_t)nb::kTile) * nb::kTile;
    *chunks = ceil_div(n, *per);
}

// What the host needs to know about an order, as data: the order-4 scheme works on (a, j), the order-6 one on (a, j, s).  Everything
// below that serves both orders reads the order here and nowhere else.  Arrays of two are indexed by the handle's f64.
struct hermite_order {
    const char* name;                 // the head of nb_variant_name
    uint32_t planes;                  // derivative planes of a pass, and predicted arrays: (a, j) | (a, j, s) and (xp, vp) | (xp, vp, ap)
    uint32_t inputs;                  // arrays a pass reads: (x, v) | (x, v, a); the crackle pass of a start: (x, v, a, j) into one plane
    uint32_t states;                  // arrays the predictor and the corrector take: (x, v, a, j) | (x, v, a, j, s, c)
    uint32_t rows[2];                 // i-bodies of one workgroup of the full pass
    uint32_t gather_rows[2];          // ... and of the gathered pass; f32: the NG = 2 kernel's, the NG = 1 kernel takes half of them
    const void *pass[2], *reduce[2];
    const void *gather[2], *gather_ng1;      // gather[0]: the f32 kernel with NG = 2
    const void *predict[2], *correct[2], *blk_predict[2], *blk_correct[2];
    void* nb_sim::*part;              // the partial sums the order's passes write (planes x chunks x n rows) ...
    uint32_t nb_sim::*chunks, nb_sim::*per;      // ... and the j-chunks of its full pass
    bool mixed;                       // the [1] entries are binary32 kernels on an f64 handle's streams (nb_set_pass_precision): f32 shapes and partial rows
    bool guard = false;               // ... with guarded sums (nb_set_pass_guard): the pass takes near2 last and leaves fp64 partial rows
    // the kernels of a batched slot behind its scheduler (nb_set_block_batch, nb_set_block_batch6, nb_set_block_batch_mixed); null: the
    // order has no batched mode
    const void *bb_predict[2] = {nullptr, nullptr}, *bb_pass[2] = {nullptr, nullptr}, *bb_correct[2] = {nullptr, nullptr};
    // the encounter watch (nb_set_encounter_watch): the gathered pass takes the thresholds last and leaves its answers in the .w lanes;
    // enc_fold reads them behind it
    bool watch = false;
    const void* enc_fold[2] = {nullptr, nullptr};
};

#define NB_BOTH(K) {(const void*)&nb::K<float>, (const void*)&nb::K<double>}
const hermite_order kOrder4 = {
    "hermite4_", 2, 2, 4, {nb::kFjRows, nb::kFjRows64}, {nb::kFjRows, nb::kFjRows64},
    {(const void*)&nb::nb_fj_pk<nb::kFjNG>, (const void*)&nb::nb_fj64<double>},
    {(const void*)&nb::nb_fj_reduce<float, float>, (const void*)&nb::nb_fj_reduce<double, double>},
    {(const void*)&nb::nb_blk_fj_pk<2>, (const void*)&nb::nb_blk_fj64<double>}, (const void*)&nb::nb_blk_fj_pk<1>,
    NB_BOTH(nb_hermite_predict), NB_BOTH(nb_hermite_correct), NB_BOTH(nb_blk_predict),
    {(const void*)&nb::nb_blk_correct<float, float>, (const void*)&nb::nb_blk_correct<double, double>},
    &nb_sim::fj_part, &nb_sim::fj_chunks, &nb_sim::fj_per, false, false,
    NB_BOTH(nb_blkq_predict), {(const void*)&nb::nb_blkq_fj_pk<1>, (const void*)&nb::nb_blkq_fj64<double>},
    {(const void*)&nb::nb_blkq_correct<float, float>, (const void*)&nb::nb_blkq_correct<double, double>}};
// Order 4 with the encounter watch on (kernels/encounter.hip.h): kOrder4's kernels, shapes, j-chunks and partial rows; the gathered
// kernels are the same bodies with the watch compiled in.  Its batched mode (nb_set_block_batch_watch, kernels/encounter_batch.hip.h):
// kOrder4's slot with the watch compiled into the small pass (the thresholds last) and into the small corrector (the records, the
// words and the outer-step base last).
const hermite_order kWatch = {
    "hermite4_", 2, 2, 4, {nb::kFjRows, nb::kFjRows64}, {nb::kFjRows, nb::kFjRows64},
    {(const void*)&nb::nb_fj_pk<nb::kFjNG>, (const void*)&nb::nb_fj64<double>},
    {(const void*)&nb::nb_fj_reduce<float, float>, (const void*)&nb::nb_fj_reduce<double, double>},
    {(const void*)&nb::nb_enc_fj_pk<2>, (const void*)&nb::nb_enc_fj64<double>}, (const void*)&nb::nb_enc_fj_pk<1>,
    NB_BOTH(nb_hermite_predict), NB_BOTH(nb_hermite_correct), NB_BOTH(nb_blk_predict),
    {(const void*)&nb::nb_blk_correct<float, float>, (const void*)&nb::nb_blk_correct<double, double>},
    &nb_sim::fj_part, &nb_sim::fj_chunks, &nb_sim::fj_per, false, false,
    NB_BOTH(nb_blkq_predict), {(const void*)&nb::nb_encq_fj_pk<1>, (const void*)&nb::nb_encq_fj64<double>},
    {(const void*)&nb::nb_encq_correct<float, float>, (const void*)&nb::nb_encq_correct<double, double>}, true,
    {(const void*)&nb::nb_enc_fold<float, float>, (const void*)&nb::nb_enc_fold<double, double>}};
const hermite_order kOrder6 = {
    "hermite6_", 3, 3, 6, {nb::kH6Rows, nb::kH6Rows64}, {nb::kBlock * 4, nb::kH6Rows64},      // (the gathered kernels are NG = 2 and 1 whatever NB_H6_NG the full pass is built with)
    {(const void*)&nb::nb_h6_fjs_pk<nb::kH6NG>, (const void*)&nb::nb_h6_fjs64<double>},
    NB_BOTH(nb_h6_reduce),
    {(const void*)&nb::nb_blk6_fjs_pk<2>, (const void*)&nb::nb_blk6_fjs64<double>}, (const void*)&nb::nb_blk6_fjs_pk<1>,
    NB_BOTH(nb_h6_predict), NB_BOTH(nb_h6_correct), NB_BOTH(nb_blk6_predict),
    {(const void*)&nb::nb_blk6_correct<float, float>, (const void*)&nb::nb_blk6_correct<double, double>},
    &nb_sim::h6_part, &nb_sim::h6_chunks, &nb_sim::h6_per, false, false,
    NB_BOTH(nb_blkq6_predict), {(const void*)&nb::nb_blkq6_fjs_pk<1>, (const void*)&nb::nb_blkq6_fjs64<double>},
    {(const void*)&nb::nb_blkq6_correct<float, float>, (const void*)&nb::nb_blkq6_correct<double, double>}};
// The crackle pass of an order-6 start (nb_set_start6): a full pass only, in the order-6 pass's j-chunks and partial rows.
const hermite_order kStart6 = {
    "hermite6_", 1, 4, 6, {nb::kH6CrkRows, nb::kH6Rows64}, {0, 0},
    {(const void*)&nb::nb_h6_crk_pk<nb::kH6CrkNG>, (const void*)&nb::nb_h6_crk64<double>},
    NB_BOTH(nb_h6_reduce1),
    {nullptr, nullptr}, nullptr, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr},
    &nb_sim::h6_part, &nb_sim::h6_chunks, &nb_sim::h6_per, false};
#undef NB_BOTH
// Order 4 on an f64 handle with nb_set_pass_precision(NB_PASS_MIXED) (kernels/mixed.hip.h): the pass reads the three binary32
// streams (xh, xl, vf) the predictors write, in the f32 kernels' shapes, and leaves binary32 partial rows in fj_part; the reduce
// and the correctors sum them in fp64 into the fp64 state.  f64 handles only: the [0] entries are never read.
const hermite_order kMixed = {
    "hermite4_", 2, 3, 4, {nb::kFjRows, nb::kFjRows}, {nb::kFjRows, nb::kFjRows},
    {nullptr, (const void*)&nb::nb_mx_fj<nb::kFjNG>},
    {nullptr, (const void*)&nb::nb_fj_reduce<float, double>},
    {nullptr, (const void*)&nb::nb_mx_blk_fj<2>}, (const void*)&nb::nb_mx_blk_fj<1>,
    {nullptr, (const void*)&nb::nb_mx_predict<>}, {nullptr, (const void*)&nb::nb_hermite_correct<double>},
    {nullptr, (const void*)&nb::nb_mx_blk_predict<>}, {nullptr, (const void*)&nb::nb_blk_correct<float, double>},
    &nb_sim::fj_part, &nb_sim::mx_chunks, &nb_sim::mx_per, true, false,
    {nullptr, (const void*)&nb::nb_blkqm_predict<>}, {nullptr, (const void*)&nb::nb_blkqm_fj<1>},
    {nullptr, (const void*)&nb::nb_blkq_correct<float, double>}};
// ... and with a guard radius (nb_set_pass_guard, kernels/guard.hip.h): kMixed's streams, predictors, shapes and j-chunks; the passes
// leave fp64 partial rows, which the native pass's reduce and block corrector sum.  No batched mode.
const hermite_order kGuard = {
    "hermite4_", 2, 3, 4, {nb::kFjRows, nb::kFjRows}, {nb::kFjRows, nb::kFjRows},
    {nullptr, (const void*)&nb::nb_mxg_fj<nb::kFjNG>},
    {nullptr, (const void*)&nb::nb_fj_reduce<double, double>},
    {nullptr, (const void*)&nb::nb_mxg_blk_fj<2>}, (const void*)&nb::nb_mxg_blk_fj<1>,
    {nullptr, (const void*)&nb::nb_mx_predict<>}, {nullptr, (const void*)&nb::nb_hermite_correct<double>},
    {nullptr, (const void*)&nb::nb_mx_blk_predict<>}, {nullptr, (const void*)&nb::nb_blk_correct<double, double>},
    &nb_sim::fj_part, &nb_sim::mx_chunks, &nb_sim::mx_per, true, true};

// The one place the pass precision and the guard are read for a step: the description everything below works from.
// (the encounter watch is on only on native order-4 handles with block steps: its setter and the other setters see to it)
const hermite_order& order_of(const nb_sim* s) { return s->mx ? (s->mx_guard > 0.0 ? kGuard : kMixed) : s->h6 ? kOrder6 : s->enc && s->blk ? kWatch : kOrder4; }

// Sets the j-chunks of the order's full pass on the handle: chunk_shape with the pass's own rows per workgroup.
void set_chunks(nb_sim* s, const hermite_order& o) { chunk_shape(s->n, o.rows[s->f64], s->n_cu, &(s->*o.chunks), &(s->*o.per)); }

// The arrays of a handle in the order the kernels take them; an order reads its first `states`, `inputs` and `planes` of them.
// in: what the predictor writes and the pass reads -- the predicted arrays, or a mixed handle's three streams; pred: what the pass's
// reduce leaves for the corrector (a1, j1[, s1]).
struct hermite_arrays {
    void *state[6], *pred[3], *in[3];
    explicit hermite_arrays(nb_sim* s) : state{s->bodies[0], s->vel, s->acc, s->jerk, s->snap, s->crackle}, pred{s->hx, s->hv, s->ha},
        in{s->mx ? s->mx_in[0] : s->hx, s->mx ? s->mx_in[1] : s->hv, s->mx ? s->mx_in[2] : s->ha} {}
};

// The arguments of one launch, collected in the kernel's order: scalars one by one, the arrays of an order by their count.
struct kernel_args {
    void* v[32];
    uint32_t k = 0;
    kernel_args& operator()(void* p) { v[k++] = p; return *this; }
    kernel_args& operator()(void** arr, uint32_t count) { for (uint32_t i = 0; i < count; ++i) v[k++] = &arr[i]; return *this; }
};

// The launch shape of a gathered pass: `na` gathered i-rows against all n predicted rows.  Rows per workgroup and j-chunks are
// chosen so that a small active set still fills the machine (f32: half the rows, the NG = 1 kernel; chunks down to one 256-row tile),
// bounded by the partial rows the handle owns (owned_chunks x n per plane) and by kFjMaxChunk.  A function of its arguments alone:
// the summation order is fixed by (n, na).
struct pass_shape { uint32_t rows, chunks, per; };
pass_shape gathered_shape(uint32_t n, uint32_t na, uint32_t rows, bool f64, uint32_t owned_chunks, int n_cu)
{
    const uint32_t want = kFjWavesPerSimd * (uint32_t)n_cu, tiles = ceil_div(n, (uint32_t)nb::kTile);
    if (!f64 && (na <= rows / 2 || (uint64_t)ceil_div(na, rows) * tiles < want)) rows /= 2;      // NG = 1
    const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)owned_chunks * n / na, tiles);
    uint32_t c = std::min(ceil_div(want, ceil_div(na, rows)), cap);
    c = std::max(std::max(c, 1u), ceil_div(n, kFjMaxChunk));
    const uint32_t per = ceil_div(ceil_div(n, c), (uint32_t)nb::kTile) * nb::kTile;
    return {rows, ceil_div(n, per), per};
}

// What a gathered pass hands to the corrector: its j-chunks and where each plane of partial sums starts.
struct pass_parts { uint32_t chunks; void* plane[3]; };

// One O(N^2) pass of order `o` on the state in[0 .. o.inputs) = (pos, vel[, acc[, jerk]]) into the order's partial sums.
//   na == 0  the full pass with the handle's stored j-chunks, then the fp64 reduce into out[0 .. o.planes) (order 6: out[0] and
//            out[1] null together: the snap alone);
//   na > 0   the gathered pass of one block step over the rows blk_act[0 .. na), in gathered_shape's shape; no reduce: the block
//            corrector sums the planes handed back in *got.
// Errors are picked up by the caller's hipGetLastError.
void launch_pass(nb_sim* s, const hermite_order& o, void** in, void** out, uint32_t na = 0, pass_parts* got = nullptr)
{
    uint32_t n = s->n, irows = n;
    pass_shape sh = {o.rows[s->f64], s->*o.chunks, s->*o.per};
    const void* fn = o.pass[s->f64];
    const bool wide = s->f64 && !o.mixed;      // fp64 kernels and partial rows (a mixed pass: the f32 kernels' arguments, shapes and rows)
    if (na) {
        irows = na;
        sh = gathered_shape(n, na, o.gather_rows[s->f64], wide, s->*o.chunks, s->n_cu);
        fn = sh.rows == o.gather_rows[s->f64] ? o.gather[s->f64] : o.gather_ng1;
    }
    pass_parts part = {sh.chunks, {}};
    for (uint32_t p = 0; p < o.planes; ++p) part.plane[p] = (char*)(s->*o.part) + p * ((size_t)4 * (wide || o.guard ? 8 : 4) * sh.chunks * irows);
    double e2 = s->eps2, G = s->G;
    float e2f = (float)s->eps2, near2 = (float)(s->mx_guard * s->mx_guard);
    const void* zr = s->zero_row;
    kernel_args a;
    a(in, o.inputs);
    if (na) a(&s->blk_act)(&na);
    a(part.plane, o.planes)(&n)(&sh.per);
    if (wide) a(&e2); else a(&e2f)(&zr);
    if (o.guard) a(&near2);
    if (o.watch && na) a(&s->enc_w);
    (void)hipLaunchKernel(fn, dim3(ceil_div(irows, sh.rows), sh.chunks), dim3(nb::kBlock), a.v, 0, s->stream);
    if (na) {
        if (o.guard && part.chunks > nb::kGuardFoldFrom) {      // many fp64 chunk rows of few bodies: added here, in the corrector's order, into chunk row 0
            kernel_args f;
            f(part.plane, o.planes)(&na)(&part.chunks);
            (void)hipLaunchKernel((const void*)&nb::nb_mxg_fold<>, dim3(na), dim3(nb::kBlock), f.v, 0, s->stream);
            part.chunks = 1;
        }
        *got = part;
        return;
    }
    kernel_args r;
    r(part.plane, o.planes)(&n)(&part.chunks)(&G)(out, o.planes);
    (void)hipLaunchKernel(o.reduce[s->f64], dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), r.v, 0, s->stream);
}

int ensure_scheme(nb_sim* s, const char* who);

// A mixed handle's three streams from the stored state (the start, nb_force_pass: a step's come from its predictor).
void launch_split(nb_sim* s)
{
    uint32_t n = s->n;
    kernel_args a;
    a(&s->bodies[0])(&s->vel)(s->mx_in, 3)(&n);
    (void)hipLaunchKernel((const void*)&nb::nb_mx_split<>, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), a.v, 0, s->stream);
}

// Makes acc / jerk the derivatives of (bodies, vel) for the G in force (a no-op while they are current): the order-4 force+jerk
// pass, on handles of either order.  With the neighbour scheme on they are the scheme's totals and come from its start.
int ensure_derivs(nb_sim* s, const char* who)
{
    if (s->ac) return ensure_scheme(s, who);
    if (!s->params_set) return fail(s, NB_ERR_STATE, std::string(who) + ": nb_set_params has not been called (G)");
    if (s->derivs_ok && s->derivs_any_G) { s->derivs_any_G = false; s->derivs_G = s->G; }
    if (s->derivs_ok && s->derivs_G == s->G) return NB_OK;
    s->snap_ok = false;      // an order-6 handle's snap and crackle belong to the (a, j) replaced here, whoever asked for them: its start runs again
    void *in[] = {s->bodies[0], s->vel}, *out[] = {s->acc, s->jerk};
    if (s->mx) { launch_split(s); launch_pass(s, order_of(s), s->mx_in, out); }      // (a mixed handle is of order 4)
    else launch_pass(s, kOrder4, in, out);
    NB_HIP(s, hipGetLastError());
    s->derivs_ok = true; s->derivs_any_G = false; s->derivs_G = s->G;
    return NB_OK;
}

// The start of a step of the handle's order (a no-op while everything is current): ensure_derivs, and at order 6 the snap from the
// force+jerk+snap pass on (x, v, a) and crackle = 0 -- so an order-6 handle starts from the (a, j) bits an order-4 handle holds.
// With nb_set_start6(NB_START6_CRACKLE) the crackle is the direct sum on (x, v, a, j) instead; a, j and s are the same bits.
int ensure_start(nb_sim* s, const char* who)
{
    const bool snap_current = s->snap_ok && s->derivs_ok && (s->derivs_any_G || s->derivs_G == s->G);
    if (int rc = ensure_derivs(s, who)) return rc;
    if (!s->h6 || snap_current) return NB_OK;
    void *in[] = {s->bodies[0], s->vel, s->acc}, *out[] = {nullptr, nullptr, s->snap};
    launch_pass(s, kOrder6, in, out);
    if (s->start6 == NB_START6_CRACKLE) {
        void *in4[] = {s->bodies[0], s->vel, s->acc, s->jerk}, *out1[] = {s->crackle};
        launch_pass(s, kStart6, in4, out1);
    } else {
        NB_HIP(s, hipMemsetAsync(s->crackle, 0, 4 * s->esz * s->n, s->stream));
    }
    NB_HIP(s, hipGetLastError());
    s->snap_ok = true; s->start_own = true;
    return NB_OK;
}

// The predictor, state -> predicted arrays, or the corrector, state <- with the derivatives the pass left in the predicted arrays.
void launch_oc(nb_sim* s, const hermite_order& o, bool correct)
{
    hermite_arrays h(s);
    uint32_t n = s->n;
    double dt = s->dt;
    kernel_args a;
    if (correct) a(h.state, o.states)(h.pred, o.planes)(&n)(&dt);
    else a(h.state, o.states)(h.in, o.inputs)(&n)(&dt);
    (void)hipLaunchKernel((correct ? o.correct : o.predict)[s->f64], dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), a.v, 0, s->stream);
}

// nb_step of a Hermite handle: plain launches, nsteps x (predict, the order's pass at the predicted state, correct).
// Timed steps record e[6] predict e[0] pass, reduce e[1] correct e[2] (collect_times).
int hermite_step(nb_sim* s, uint32_t nsteps)
{
    if (int rc = ensure_start(s, "nb_step")) return rc;
    const hermite_order& o = order_of(s);
    hermite_arrays h(s);
    for (uint32_t k = 0; k < nsteps; ++k) {
        nb_events ev;
        const bool rec = s->timing && get_events(s, &ev) == 0;
        if (rec) NB_HIP(s, hipEventRecord(ev.e[6], s->stream));
        launch_oc(s, o, false);
        if (rec) NB_HIP(s, hipEventRecord(ev.e[0], s->stream));
        launch_pass(s, o, h.in, h.pred);      // (a1, j1[, s1]) over the predicted state: the reduce runs after every read of it
        if (rec) NB_HIP(s, hipEventRecord(ev.e[1], s->stream));
        launch_oc(s, o, true);
        if (rec) { NB_HIP(s, hipEventRecord(ev.e[2], s->stream)); s->pending.push_back(ev); }
        NB_HIP(s, hipGetLastError());
        ++s->steps_done;
        s->start_own = false;      // consumed: the state is a running one (nb_set_start6 leaves it alone)
    }
    return NB_OK;
}

void h6_release(nb_sim* s)
{
    for (void** p : {&s->snap, &s->crackle, &s->ha, &s->h6_part}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    s->h6 = false; s->snap_ok = false; s->start_own = false; s->start6 = NB_START6_ZERO;
}

void mx_release(nb_sim* s)
{
    for (void*& p : s->mx_in) { if (p) (void)hipFree(p); p = nullptr; }
    s->mx = false; s->mx_guard = 0.0;
}

// what nb_variant_name and nb_shape_info report: the pass a step of the handle runs
void hermite_names(nb_sim* s)
{
    const hermite_order& o = order_of(s);
    const uint32_t c = s->*o.chunks, per = s->*o.per;
    s->jsplit = c; s->j_per_split = per;
    s->variant = std::string(o.name) + (o.guard ? "f64mxg" : o.mixed ? "f64mx" : s->f64 ? "f64" : "f32pk") + "_c" + std::to_string(c) + "_j" + std::to_string(per);
}

// ---- block individual time steps (nb_set_block_steps, nb_set_block_steps6; kernels/block.hip.h, kernels/block6.hip.h) ----------
// Makes the levels current: the start rule on current derivatives (or every body at min_level on a frozen handle; uploaded levels
// are kept), and the clock of the outer step at 0.
int ensure_levels(nb_sim* s, const char* who)
{
    if (int rc = ensure_start(s, who)) return rc;      // also: a changed G re-evaluates them (order 6: its start, c = 0 or the direct sum)
    if (s->levels == 2) return NB_OK;
    s->levels_own = s->levels == 0;
    void *a = s->acc, *j = s->jerk;
    uint32_t n = s->n, lmin = s->blk_lmin, L = s->blk_L;
    int mode = s->levels == 1 ? 2 : s->blk_frozen ? 1 : 0;
    double eta = s->blk_eta, dt = s->dt;
    void* args[] = {&a, &j, &s->blk_lev, &s->blk_due, &s->blk_hdr, &n, &mode, &eta, &dt, &lmin, &L};
    const void* fn = s->f64 ? (const void*)&nb::nb_blk_start<double> : (const void*)&nb::nb_blk_start<float>;
    if (s->h6 && mode == 0 && s->start6 == NB_START6_CRACKLE) {      // the two-rule start on (a, j, s, c); dynamic levels of order 6 are f64 handles
        void* args6[] = {&a, &j, &s->snap, &s->crackle, &s->blk_lev, &s->blk_due, &s->blk_hdr, &n, &mode, &eta, &dt, &lmin, &L};
        (void)hipLaunchKernel((const void*)&nb::nb_blk6_start<double>, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args6, 0, s->stream);
    } else
        (void)hipLaunchKernel(fn, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream);
    NB_HIP(s, hipGetLastError());
    s->levels = 2;
    return NB_OK;
}

// The fold behind a gathered pass of a watched handle (block_step, and the host steps of block_batch_step): the answers in the .w
// lanes of the partial rows, into the records of the active bodies, at the block time t_next of the running outer step (exact:
// t_next <= 2^L <= 2^30).
void launch_enc_fold(nb_sim* s, const hermite_order& o, pass_parts& part, uint32_t na, uint32_t t_next)
{
    double t = (double)s->steps_done + std::ldexp((double)t_next, -(int)s->blk_L);
    kernel_args f;
    uint32_t lpr = 1;      // lanes that share a row's chunks: the next power of two, at most a wave, while the rows alone do not fill 256 workgroups
    while (lpr < part.chunks && lpr < 64 && (uint64_t)na * lpr * 2 <= 65536) lpr *= 2;
    f(part.plane, o.planes)(&s->blk_act)(&na)(&part.chunks)(&lpr)(&s->enc_rho2)(&s->enc_partner)(&s->enc_time)(&s->enc_count)(&s->enc_words)(&s->enc_pub)(&t);
    (void)hipLaunchKernel(o.enc_fold[s->f64], dim3(ceil_div(na, nb::kBlock / lpr)), dim3(nb::kBlock), f.v, 0, s->stream);
    ++s->enc_passes;
}

// nb_step of a block-step handle of either order: nsteps outer steps of dt.  Per block step: schedule and predict-all (launched
// right behind the previous corrector), ONE host wait for the header (the active count sizes the next launch), the order's gathered
// pass over the active bodies, reduce + correct + new levels.
int block_step(nb_sim* s, uint32_t nsteps)
{
    s->enc_stopped = 0; s->enc_steps_left = 0;
    if (int rc = ensure_levels(s, "nb_step")) return rc;
    const hermite_order& o = order_of(s);
    hermite_arrays h(s);
    const uint32_t L = s->blk_L, end = 1u << L;
    uint32_t n = s->n, lmin = s->blk_lmin, Lk = L;
    int frozen = s->blk_frozen ? 1 : 0;
    double eta = s->blk_eta, dt = s->dt, G = s->G, tick = std::ldexp(s->dt, -(int)L);
    auto schedule_and_predict = [&]() {
        void* sargs[] = {&s->blk_due, &s->blk_lev, &n, &s->blk_act, &s->blk_hdr, &s->blk_hdr_pub};
        (void)hipLaunchKernel((const void*)&nb::nb_blk_sched<nb::kBlkSched>, dim3(1), dim3(nb::kBlkSched), sargs, 0, s->stream);
        kernel_args p;
        p(h.state, o.states)(&s->blk_due)(&s->blk_lev)(h.in, o.inputs)(&n)(&s->blk_hdr)(&Lk)(&tick);
        (void)hipLaunchKernel(o.blk_predict[s->f64], dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), p.v, 0, s->stream);
    };
    bool ahead = false;      // the first schedule + predict of this outer step went out behind the previous one's last corrector
    for (uint32_t k = 0; k < nsteps; ++k) {
        nb_events ev;
        const bool rec = s->timing && get_events(s, &ev) == 0;
        if (rec) NB_HIP(s, hipEventRecord(ev.e[0], s->stream));
        if (!ahead) schedule_and_predict();
        ahead = false;
        for (;;) {
            NB_HIP(s, hipStreamSynchronize(s->stream));      // the one host wait of a block step
            uint32_t na = s->blk_hdr_host[nb::kBlkCount], t_next = s->blk_hdr_host[nb::kBlkNext];
            if (na == 0 || na > n || t_next == 0 || t_next > end)
                return fail(s, NB_ERR_HIP, "nb_step: block schedule out of range (active " + std::to_string(na) + ", tick " + std::to_string(t_next) + ")");
            pass_parts part;
            launch_pass(s, o, h.in, nullptr, na, &part);
            if (o.watch) launch_enc_fold(s, o, part, na, t_next);
            kernel_args c;
            c(part.plane, o.planes)(&s->blk_act)(&na)(&part.chunks)(&G)(h.state, o.states)(&s->blk_due)(&s->blk_lev)(&s->blk_hdr)(&t_next)(&Lk)(&lmin)(&frozen)(&eta)(&dt);
            (void)hipLaunchKernel(o.blk_correct[s->f64], dim3(ceil_div(na, nb::kBlock)), dim3(nb::kBlock), c.v, 0, s->stream);
            ++s->blk_steps; s->blk_body_steps += na;
            if (t_next == end) break;
            schedule_and_predict();
            NB_HIP(s, hipGetLastError());
        }
        if (rec) { NB_HIP(s, hipEventRecord(ev.e[1], s->stream)); ev.blk = true; s->pending.push_back(ev); }
        bool stop = false;
        if (o.watch && (s->enc_flags & NB_ENC_STOP)) {      // the one extra host wait per outer step: hits as the last fold published them
            NB_HIP(s, hipStreamSynchronize(s->stream));
            stop = *(volatile unsigned long long*)s->enc_host != 0;
        }
        if (k + 1 < nsteps && !s->timing && !stop) { schedule_and_predict(); ahead = true; }      // (timed steps launch it inside their own span)
        NB_HIP(s, hipGetLastError());
        ++s->blk_outer;
        ++s->steps_done;
        s->start_own = s->levels_own = false;      // consumed: state and levels are running ones (nb_set_start6 leaves them alone)
        if (stop) { s->enc_stopped = 1; s->enc_steps_left = nsteps - (k + 1); return NB_OK; }
    }
    return NB_OK;
}

// ---- nb_set_block_batch, nb_set_block_batch6, nb_set_block_batch_mixed: block steps sized on the device, many per host wait
// (kernels/block_batch.hip.h, kernels/block_batch6.hip.h, kernels/block_batch_mixed.hip.h) ----------
// The j-chunks of the small pass: a function of n and the CU count alone (a row's bits must not depend on |A|, small_max or depth).
// One chunk of whole tiles per CU: a wave's chain is a quarter of a chunk (64 rows of one tile up to 256 x CUs bodies), and the
// corrector shares a slot's chunk rows among nb::kBbSumLanes lanes.
void bb_shape(uint32_t n, int n_cu, uint32_t* chunks, uint32_t* per)
{
    const uint32_t tiles = ceil_div(n, (uint32_t)nb::kTile);
    const uint32_t c = std::max(1u, std::min((uint32_t)n_cu, tiles));
    *per = ceil_div(tiles, c) * nb::kTile;
    *chunks = ceil_div(n, *per);
}

// How many slots the next batch has: a function of what the host has read so far.  Nothing read yet: one.  Otherwise up to the next
// tick expected to park, that slot included: block times advance by the stride of the deepest level present, and ticks whose count
// of trailing zeros reaches bb_park_ctz are expected to park (|A(t)| grows with ctz(t); 2^L always parks).
uint32_t bb_plan_slots(const nb_sim* s)
{
    if (s->bb_fresh || s->bb_small_max == 0) return 1;
    const uint32_t L = s->blk_L, fin = std::min(s->bb_finest, L);
    const uint32_t z = std::max(std::min(s->bb_park_ctz, L), L - fin);
    const uint64_t step = 1ull << z, stride = 1ull << (L - fin);
    const uint64_t park = (s->bb_t / step + 1) * step;
    const uint64_t count = (park - s->bb_t + stride - 1) / stride;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, s->bb_depth));
}

// nb_step of a block-step handle of either order with nb_set_block_batch / nb_set_block_batch6 / nb_set_block_batch_mixed on: block_step's outer step, with
// the slots of a batch enqueued behind one another and ONE host wait per batch; the slot's kernels and argument lists are the order's.  A slot that parked left its schedule and prediction: the host runs that block
// step through the gathered path, as block_step does.
int block_batch_step(nb_sim* s, uint32_t nsteps)
{
    s->enc_stopped = 0; s->enc_steps_left = 0;
    const bool stale = s->levels != 2;
    if (int rc = ensure_levels(s, "nb_step")) return rc;
    if (stale) { s->bb_fresh = true; s->bb_t = 0; s->bb_park_ctz = s->blk_L; }
    const hermite_order& o = order_of(s);
    hermite_arrays h(s);
    const uint32_t L = s->blk_L;
    uint32_t n = s->n, lmin = s->blk_lmin, Lk = L, end = 1u << L, small_max = s->bb_small_max, chunks = s->bb_chunks, per = s->bb_per;
    int frozen = s->blk_frozen ? 1 : 0;
    double eta = s->blk_eta, dt = s->dt, G = s->G, tick = std::ldexp(s->dt, -(int)L), e2 = s->eps2;
    float e2f = (float)s->eps2;
    const void* zr = s->zero_row;
    const bool wide = s->f64 && !o.mixed;      // fp64 kernels and rows, as in launch_pass (a mixed slot: the f32 pass's shape and arguments)
    const size_t row = (size_t)4 * (s->f64 ? 8 : 4);      // the stride of a plane: bb_configure's (a mixed plane's 16-byte rows fill half of it)
    void* plane[3] = {nullptr, nullptr, nullptr};
    for (uint32_t p = 0; p < o.planes; ++p) plane[p] = (char*)s->bb_part + p * (row * chunks * nb::kBbMaxSmall);
    const uint32_t gx_small = std::max(1u, ceil_div(small_max, wide ? nb::kBbRows64 : nb::kBbRows));
    double tbase = 0.0;      // o.watch: the outer steps run when the running outer step began (the small corrector forms its block time from it)
    auto enqueue_slot = [&](uint32_t first) {
        void* sargs[] = {&s->blk_due, &s->blk_lev, &n, &s->blk_act, &s->blk_hdr, &s->blk_hdr_pub, &s->bb_words, &s->bb_pub, &first, &small_max, &end};
        (void)hipLaunchKernel((const void*)&nb::nb_blkq_sched<nb::kBlkSched>, dim3(1), dim3(nb::kBlkSched), sargs, 0, s->stream);
        kernel_args p;
        p(h.state, o.states)(&s->blk_due)(&s->blk_lev)(h.in, o.inputs)(&n)(&s->blk_hdr)(&Lk)(&tick)(&s->bb_words);
        (void)hipLaunchKernel(o.bb_predict[s->f64], dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), p.v, 0, s->stream);
        if (small_max == 0) return;      // no small steps: every slot parks
        kernel_args f;
        f(h.in, o.inputs)(&s->blk_act)(&s->blk_hdr)(&s->bb_words)(&small_max)(plane, o.planes)(&n)(&per);
        if (wide) f(&e2); else f(&e2f)(&zr);
        if (o.watch) f(&s->enc_w);
        (void)hipLaunchKernel(o.bb_pass[s->f64], dim3(gx_small, chunks), dim3(nb::kBlock), f.v, 0, s->stream);
        kernel_args c;
        c(plane, o.planes)(&s->blk_act)(&s->bb_words)(&small_max)(&chunks)(&G)(h.state, o.states)(&s->blk_due)(&s->blk_lev)(&s->blk_hdr)(&n)(&Lk)(&lmin)(&frozen)(&eta)(&dt);
        if (o.watch) c(&s->enc_rho2)(&s->enc_partner)(&s->enc_time)(&s->enc_count)(&s->enc_words)(&tbase);
        (void)hipLaunchKernel(o.bb_correct[s->f64], dim3(ceil_div(small_max * nb::kBbSumLanes, nb::kBlock)), dim3(nb::kBlock), c.v, 0, s->stream);
    };
    for (uint32_t k = 0; k < nsteps; ++k) {
        nb_events ev;
        const bool rec = s->timing && get_events(s, &ev) == 0;
        if (rec) NB_HIP(s, hipEventRecord(ev.e[0], s->stream));
        tbase = (double)s->steps_done;
        for (;;) {
            const uint32_t slots = bb_plan_slots(s);
            for (uint32_t q = 0; q < slots; ++q) enqueue_slot(q == 0 ? 1u : 0u);
            NB_HIP(s, hipGetLastError());
            NB_HIP(s, hipStreamSynchronize(s->stream));      // the one host wait of a batch
            ++s->bb_waits; s->bb_slots += slots;
            const uint32_t na = s->blk_hdr_host[nb::kBlkCount], t_next = s->blk_hdr_host[nb::kBlkNext];
            const uint32_t mode = s->bb_host[nb::kBbMode];
            const uint32_t dsmall = s->bb_host[nb::kBbSmall] - s->bb_seen_small, dbody = s->bb_host[nb::kBbBody] - s->bb_seen_body;
            s->bb_seen_small = s->bb_host[nb::kBbSmall]; s->bb_seen_body = s->bb_host[nb::kBbBody];
            const bool parked = mode != nb::kBbModeSmall;
            if (na == 0 || na > n || t_next == 0 || t_next > end || mode > nb::kBbModeParked || dsmall + (parked ? 1u : 0u) > slots ||
                (uint64_t)dbody > (uint64_t)dsmall * small_max || (!parked && (na > small_max || t_next == end)))
                return fail(s, NB_ERR_HIP, "nb_step: block schedule out of range (active " + std::to_string(na) + ", tick " + std::to_string(t_next) +
                            ", batch of " + std::to_string(slots) + ": " + std::to_string(dsmall) + " small steps, mode " + std::to_string(mode) + ")");
            s->bb_small += dsmall; s->blk_steps += dsmall; s->blk_body_steps += dbody;
            if (o.watch) s->enc_passes += dsmall;      // (a small step's fold is in its corrector)
            s->bb_idle += slots - dsmall - (parked ? 1u : 0u);
            // what the policy reads
            s->bb_fresh = false;
            s->bb_finest = s->bb_host[nb::kBbFinest];
            s->bb_t = t_next == end ? 0u : t_next;
            const uint32_t tz = (uint32_t)__builtin_ctz(t_next);
            if (parked && t_next != end) s->bb_park_ctz = std::min(s->bb_park_ctz, tz);
            else if (!parked && tz >= s->bb_park_ctz) s->bb_park_ctz = std::min(L, tz + 1);      // expected to park, and was small
            if (!parked) continue;
            pass_parts part;
            uint32_t nah = na, tn = t_next;
            launch_pass(s, o, h.in, nullptr, nah, &part);
            if (o.watch) launch_enc_fold(s, o, part, nah, tn);
            kernel_args c;
            c(part.plane, o.planes)(&s->blk_act)(&nah)(&part.chunks)(&G)(h.state, o.states)(&s->blk_due)(&s->blk_lev)(&s->blk_hdr)(&tn)(&Lk)(&lmin)(&frozen)(&eta)(&dt);
            (void)hipLaunchKernel(o.blk_correct[s->f64], dim3(ceil_div(nah, nb::kBlock)), dim3(nb::kBlock), c.v, 0, s->stream);
            ++s->bb_hoststeps; ++s->blk_steps; s->blk_body_steps += nah;
            if (t_next == end) break;
        }
        if (rec) { NB_HIP(s, hipEventRecord(ev.e[1], s->stream)); ev.blk = true; s->pending.push_back(ev); }
        bool stop = false;
        if (o.watch && (s->enc_flags & NB_ENC_STOP)) {      // the one extra host wait per outer step, as in block_step: the last (host) step's fold published the running hits, those of the small slots included
            NB_HIP(s, hipStreamSynchronize(s->stream));
            stop = *(volatile unsigned long long*)s->enc_host != 0;
        }
        NB_HIP(s, hipGetLastError());
        ++s->blk_outer;
        ++s->steps_done;
        s->start_own = s->levels_own = false;
        if (stop) { s->enc_stopped = 1; s->enc_steps_left = nsteps - (k + 1); return NB_OK; }
    }
    return NB_OK;
}

// ---- the Ahmad-Cohen neighbour scheme (nb_set_neighbor_scheme; kernels/ac_scheme.hip.h) ----------
// One list build at the bodies: nb_split_force's four outputs into (ai, ji, ar, jr) and nb_neighbor_lists' rows and counts into
// ac_list / ac_count, both through the engine's own entry points with device pointers, on the handle's stream -- or, where
// nb_split_lists cuts the request as nb_split_force does (nbi::ac_fused), that one call: the same bits from one pass over the pairs.
int ac_build(nb_sim* s, void* ai, void* ji, void* ar, void* jr, const char* who)
{
    const void* radii = s->ad ? s->ad_next : s->ac_radii;      // (with adaptation on the scheme's own copy is only the first `next`)
    if (nbi::ac_fused(s)) {
        nb_split_lists_request q;
        memset(&q, 0, sizeof q);
        q.struct_size = sizeof q; q.m = s->n; q.flags = NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE;
        q.radii = radii; q.radius = radii ? 0.0 : s->ac_radius;
        q.accel_irr = ai; q.jerk_irr = ji; q.accel_reg = ar; q.jerk_reg = jr;
        q.cap = s->ac_cap; q.list = s->ac_list; q.count = s->ac_count;
        if (int rc = nbi::split_lists(s, &q, s->n, who)) return rc;
        NB_HIP(s, hipMemsetAsync(s->ac_hdr, 0, sizeof(unsigned long long) * nb::kAcHdrWords, s->stream));
        return NB_OK;
    }
    nb_split_force_request sq;
    memset(&sq, 0, sizeof sq);
    sq.struct_size = sizeof sq; sq.m = s->n; sq.flags = NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE;
    sq.radii = radii; sq.radius = radii ? 0.0 : s->ac_radius;
    sq.accel_irr = ai; sq.jerk_irr = ji; sq.accel_reg = ar; sq.jerk_reg = jr;
    if (int rc = nbi::split_force(s, &sq, s->n, who)) return rc;
    nb_neighbor_list_request lq;
    memset(&lq, 0, sizeof lq);
    lq.struct_size = sizeof lq; lq.m = s->n; lq.flags = NB_NBR_AT_BODIES | NB_NBR_DEVICE;
    lq.radii = radii; lq.radius = radii ? 0.0 : s->ac_radius;
    lq.cap = s->ac_cap; lq.list = s->ac_list; lq.count = s->ac_count;
    if (int rc = nbi::neighbor_lists(s, &lq, s->n, who)) return rc;
    NB_HIP(s, hipMemsetAsync(s->ac_hdr, 0, sizeof(unsigned long long) * nb::kAcHdrWords, s->stream));
    return NB_OK;
}

// HOST SYNCHRONISATION: the header of a build (rows over cap, largest count, entries) is read here, after one wait for the stream.
// Returns true when some row holds more than cap members; *msg then names the numbers.
int ac_read_header(nb_sim* s, bool* over, std::string* msg)
{
    NB_HIP(s, hipMemcpyAsync(s->ac_hdr_host, s->ac_hdr, sizeof(unsigned long long) * nb::kAcHdrWords, hipMemcpyDeviceToHost, s->stream));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const unsigned long long rows = s->ac_hdr_host[nb::kAcOver], mx = s->ac_hdr_host[nb::kAcMax];
    ++s->ac_builds;
    s->ac_entries += s->ac_hdr_host[nb::kAcEntries];
    s->ac_max_count = (uint32_t)mx;
    s->ac_overflowed = (uint32_t)rows;
    *over = rows != 0;
    if (*over) *msg = "neighbour list overflow: " + std::to_string(rows) + " rows hold more than cap members (largest count " + std::to_string(mx) + ", cap " + std::to_string(s->ac_cap) + "); call nb_set_neighbor_scheme with a larger cap or a smaller radius";
    return NB_OK;
}

nb::AcRule ad_rule(const nb_sim* s) { return nb::AcRule{(double)s->ad_target, s->ad_gmax, s->ad_rmin, s->ad_rmax}; }

// A build with adaptation on (nb_set_neighbor_adapt): the pass cut by `next`, its header from the counts alone (ac_read_header's
// wait), and, while rows are over cap and rebuilds are left, the shrink of those rows and the pass again on the same state -- one
// more wait each.  keep: the first shrink saves `next` (a start that fails puts it back).  *over: rows are over after the last pass.
int ad_build(nb_sim* s, void* ai, void* ji, void* ar, void* jr, const char* who, bool keep, bool* over, std::string* msg)
{
    uint32_t n = s->n, cap = s->ac_cap, rebuilds = 0;
    double nt = (double)s->ad_target;
    const dim3 grid(ceil_div(n, nb::kBlock)), block(nb::kBlock);
    for (;;) {
        if (int rc = ac_build(s, ai, ji, ar, jr, who)) return rc;
        void* cargs[] = {&s->ac_count, &s->ac_hdr, &n, &cap};
        NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_ac_check<>, grid, block, cargs, 0, s->stream));
        if (int rc = ac_read_header(s, over, msg)) return rc;
        if (!*over || rebuilds == s->ad_max_rebuilds) break;
        if (keep && rebuilds == 0) NB_HIP(s, hipMemcpyAsync(s->ad_keep, s->ad_next, s->esz * n, hipMemcpyDeviceToDevice, s->stream));
        void* sargs[] = {&s->ad_next, &s->ac_count, &n, &cap, &nt};
        const void* fn = s->f64 ? (const void*)&nb::nb_ac_shrink<double> : (const void*)&nb::nb_ac_shrink<float>;
        NB_HIP(s, hipLaunchKernel(fn, grid, block, sargs, 0, s->stream));
        ++rebuilds;
        s->ad_rows_shrunk += s->ac_overflowed;
    }
    s->ad_rebuilds += rebuilds;
    s->ad_last_rebuilds = rebuilds;
    return NB_OK;
}

// The start with adaptation on: the build with its rebuilds, then the totals and the rule in one launch.
int ad_start(nb_sim* s, const char* who)
{
    bool over = false;
    std::string msg;
    if (int rc = ad_build(s, s->ac_ai, s->ac_ji, s->ac_ar, s->ac_jr, who, true, &over, &msg)) return rc;
    uint32_t n = s->n;
    if (over) {      // as without adaptation: the state is untouched, and so is `next`: every later call starts again
        if (s->ad_last_rebuilds) NB_HIP(s, hipMemcpyAsync(s->ad_next, s->ad_keep, s->esz * n, hipMemcpyDeviceToDevice, s->stream));
        return fail(s, NB_ERR_STATE, std::string(who) + ": " + msg);
    }
    nb::AcRule rule = ad_rule(s);
    void* args[] = {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->acc, &s->jerk, &s->ac_count, &s->ad_built, &s->ad_next, &n, &rule};
    const void* fn = s->f64 ? (const void*)&nb::nb_ac_start_ad<double> : (const void*)&nb::nb_ac_start_ad<float>;
    NB_HIP(s, hipLaunchKernel(fn, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    s->ac_ok = true; s->ac_over = false;
    s->derivs_ok = true; s->derivs_any_G = false; s->derivs_G = s->G;
    return NB_OK;
}

// The start: makes the scheme's arrays current for (bodies, vel) and the G in force (a no-op while they are).
int ensure_scheme(nb_sim* s, const char* who)
{
    if (!s->params_set) return fail(s, NB_ERR_STATE, std::string(who) + ": nb_set_params has not been called (G)");
    if (s->ac_ok && s->derivs_ok && s->derivs_any_G) { s->derivs_any_G = false; s->derivs_G = s->G; }      // (never set while the scheme is on)
    if (s->ac_ok && s->derivs_ok && s->derivs_G == s->G) return NB_OK;
    s->ac_ok = false; s->derivs_ok = false;
    s->lv_state = 0;      // the levels start again with the scheme (read only while nb_set_neighbor_levels is on)
    if (s->ad) return ad_start(s, who);
    if (int rc = ac_build(s, s->ac_ai, s->ac_ji, s->ac_ar, s->ac_jr, who)) return rc;
    uint32_t n = s->n, cap = s->ac_cap;
    void* args[] = {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->acc, &s->jerk, &s->ac_count, &s->ac_hdr, &n, &cap};
    const void* fn = s->f64 ? (const void*)&nb::nb_ac_start<double> : (const void*)&nb::nb_ac_start<float>;
    NB_HIP(s, hipLaunchKernel(fn, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    bool over = false;
    std::string msg;
    if (int rc = ac_read_header(s, &over, &msg)) return rc;
    if (over) return fail(s, NB_ERR_STATE, std::string(who) + ": " + msg);      // the state is untouched; every later call starts again
    s->ac_ok = true; s->ac_over = false;
    s->derivs_ok = true; s->derivs_any_G = false; s->derivs_G = s->G;
    return NB_OK;
}

nb::LvCfg lv_cfg(const nb_sim* s)
{
    uint32_t L = 0;
    while ((1u << L) < s->ac_nsub) ++L;
    return nb::LvCfg{L, s->lv_lmin, s->lv_frozen ? 1u : 0u, s->ac_nsub, s->lv_eta, s->dt, s->dt / (double)s->ac_nsub};
}

// The start of the levels (nb_set_neighbor_levels): runs where they are not current, behind the scheme's own start.  No host wait.
int ensure_levels(nb_sim* s)
{
    if (s->lv_state == 2) return NB_OK;
    uint32_t n = s->n;
    int mode = s->lv_state == 1 ? 2 : s->lv_frozen ? 1 : 0;
    nb::LvCfg c = lv_cfg(s);
    void* args[] = {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->lv_lev, &s->lv_rec, &n, &mode, &c};
    const void* fn = s->f64 ? (const void*)&nb::nb_ac_lv_start<double> : (const void*)&nb::nb_ac_lv_start<float>;
    NB_HIP(s, hipLaunchKernel(fn, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    s->lv_state = 2;
    return NB_OK;
}

// The irregular part of one regular step with levels on: the clock and the first prediction, then ONE launch for EVERY tick -- the
// corrector of the due bodies and the prediction of all bodies to the next tick -- which leaves at once where no body is due at
// the tick or the one behind it.  The host never learns which ticks those are: no wait.
int lv_ticks(nb_sim* s)
{
    uint32_t n = s->n, cap = s->ac_cap;
    const uint32_t nsub = s->ac_nsub;
    double G = s->G, eps2d = s->eps2;
    float eps2f = (float)s->eps2;
    void *x = s->bodies[0], *v = s->vel;
    void* P[2][2] = {{s->hx, s->hv}, {s->ac_px, s->ac_pv}};      // launch k reads P[k & 1] and writes P[(k + 1) & 1]
    nb::LvCfg c = lv_cfg(s);
    const dim3 rows_grid(ceil_div(n, nb::kBlock)), sub_grid(ceil_div(n, nb::lf_rows(s->f64))), block(nb::kBlock);
    NB_HIP(s, hipMemsetAsync(s->lv_words, 0, sizeof(uint32_t) * nb::lv_words(nsub), s->stream));
    {
        void* args[] = {&x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &P[1][0], &P[1][1], &s->lv_lev, &s->lv_due, &s->lv_words, &n, &c};
        const void* fn = s->f64 ? (const void*)&nb::nb_ac_lv_begin<double> : (const void*)&nb::nb_ac_lv_begin<float>;
        NB_HIP(s, hipLaunchKernel(fn, rows_grid, block, args, 0, s->stream));
    }
    for (uint32_t k = 1; k <= nsub; ++k) {
        void **pr = P[k & 1], **pw = P[(k + 1) & 1];
        void *wx = k < nsub ? pw[0] : nullptr, *wv = k < nsub ? pw[1] : nullptr;
        if (s->f64) {
            void* args[] = {&pr[0], &pr[1], &s->ac_list, &s->ac_count, &s->lv_words, &s->lv_cnt, &s->lv_rec, &n, &cap, &eps2d, &G, &x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->lv_lev, &s->lv_due, &k, &c, &wx, &wv};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_ac_lv_sub64<nb::kLfLanes64>, sub_grid, block, args, 0, s->stream));
        } else {
            void* args[] = {&pr[0], &pr[1], &s->ac_list, &s->ac_count, &s->lv_words, &s->lv_cnt, &s->lv_rec, &n, &cap, &eps2f, &G, &x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->lv_lev, &s->lv_due, &k, &c, &wx, &wv};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_ac_lv_sub32<nb::kLfLanes32>, sub_grid, block, args, 0, s->stream));
        }
    }
    ++s->lv_regular; s->lv_ticks += nsub;
    return NB_OK;
}

// nb_step of a handle with the neighbour scheme: nsteps regular steps of dt.  Per regular step: the first prediction, N_sub substep
// launches, the sums over the old list, the split pass and the list build at the arrived state, the regular correction, and ONE
// host wait for the header of the build.  Timed steps record e[0] .. e[1] around the regular step (as block steps).
int ac_step(nb_sim* s, uint32_t nsteps)
{
    if (s->ac_over) return fail(s, NB_ERR_STATE, "nb_step: " + s->ac_msg);
    if (int rc = ensure_scheme(s, "nb_step")) return rc;
    if (s->lv) { if (int rc = ensure_levels(s)) return rc; }
    uint32_t n = s->n, cap = s->ac_cap;
    const uint32_t nsub = s->ac_nsub;
    double dt = s->dt, hs = s->dt / (double)nsub, G = s->G, eps2d = s->eps2;
    float eps2f = (float)s->eps2;
    void *x = s->bodies[0], *v = s->vel;
    void* P[2][2] = {{s->hx, s->hv}, {s->ac_px, s->ac_pv}};
    const dim3 rows_grid(ceil_div(n, nb::kBlock)), sub_grid(ceil_div(n, nb::lf_rows(s->f64))), block(nb::kBlock);
    for (uint32_t k = 0; k < nsteps; ++k) {
        nb_events ev;
        const bool rec = s->timing && get_events(s, &ev) == 0;
        if (rec) NB_HIP(s, hipEventRecord(ev.e[0], s->stream));
        if (s->lv) {      // nb_set_neighbor_levels: every body on its own irregular step, one launch per tick in place of the shared substeps
            if (int rc = lv_ticks(s)) return rc;
        } else {
            void* args[] = {&x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &P[0][0], &P[0][1], &n, &hs};
            const void* fn = s->f64 ? (const void*)&nb::nb_ac_predict0<double> : (const void*)&nb::nb_ac_predict0<float>;
            NB_HIP(s, hipLaunchKernel(fn, rows_grid, block, args, 0, s->stream));
        }
        for (uint32_t q = 0; q < (s->lv ? 0u : nsub); ++q) {      // the shared substeps (none with levels on)
            double tau0 = (double)q * hs, tau1 = tau0 + hs;
            void **pr = P[q & 1], **pw = P[(q + 1) & 1];
            void *wx = q + 1 < nsub ? pw[0] : nullptr, *wv = q + 1 < nsub ? pw[1] : nullptr;
            if (s->f64) {
                void* args[] = {&pr[0], &pr[1], &s->ac_list, &s->ac_count, &n, &cap, &eps2d, &G, &x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &tau0, &tau1, &hs, &wx, &wv};
                NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_ac_sub64<nb::kLfLanes64>, sub_grid, block, args, 0, s->stream));
            } else {
                void* args[] = {&pr[0], &pr[1], &s->ac_list, &s->ac_count, &n, &cap, &eps2f, &G, &x, &v, &s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &tau0, &tau1, &hs, &wx, &wv};
                NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_ac_sub32<nb::kLfLanes32>, sub_grid, block, args, 0, s->stream));
            }
        }
        // the regular time: (aio, jio) over the OLD list into the first predicted pair, (ar', jr') into the second, (ai', ji') in
        // place (the old ones are not read again), the new list over the old one (the old-list sums are enqueued in front of it)
        nb_list_force_request fq;
        memset(&fq, 0, sizeof fq);
        fq.struct_size = sizeof fq; fq.m = n; fq.flags = NB_LISTF_AT_BODIES | NB_LISTF_DEVICE;
        fq.list = s->ac_list; fq.count = s->ac_count; fq.cap = cap; fq.accel = s->hx; fq.jerk = s->hv;
        if (int rc = nbi::list_force(s, &fq, n, "nb_step")) return rc;
        if (s->ad) {      // the list is accepted (the waits are ad_build's) in front of the correction, which moves x and v; then ONE launch
            bool over = false;
            if (int rc = ad_build(s, s->ac_ai, s->ac_ji, s->ac_px, s->ac_pv, "nb_step", false, &over, &s->ac_msg)) return rc;
            nb::AcRule rule = ad_rule(s);
            void* args[] = {&x, &v, &s->ac_ai, &s->ac_ji, &s->ac_px, &s->ac_pv, &s->hx, &s->hv, &s->ac_ar, &s->ac_jr, &s->acc, &s->jerk, &s->ac_count, &s->ad_built, &s->ad_next, &n, &dt, &rule};
            const void* fn = s->f64 ? (const void*)&nb::nb_ac_regular_ad<double> : (const void*)&nb::nb_ac_regular_ad<float>;
            NB_HIP(s, hipLaunchKernel(fn, rows_grid, block, args, 0, s->stream));
            if (rec) { NB_HIP(s, hipEventRecord(ev.e[1], s->stream)); ev.blk = true; s->pending.push_back(ev); }
            ++s->ac_regular; s->ac_substeps += nsub;
            ++s->steps_done;
            if (over) {      // rows are still over after the last allowed rebuild: the fixed-radii policy, to the letter
                s->ac_over = true;
                return fail(s, NB_ERR_STATE, "nb_step: " + s->ac_msg);
            }
            continue;
        }
        if (int rc = ac_build(s, s->ac_ai, s->ac_ji, s->ac_px, s->ac_pv, "nb_step")) return rc;
        {
            void* args[] = {&x, &v, &s->ac_ai, &s->ac_ji, &s->ac_px, &s->ac_pv, &s->hx, &s->hv, &s->ac_ar, &s->ac_jr, &s->acc, &s->jerk, &s->ac_count, &s->ac_hdr, &n, &cap, &dt};
            const void* fn = s->f64 ? (const void*)&nb::nb_ac_regular<double> : (const void*)&nb::nb_ac_regular<float>;
            NB_HIP(s, hipLaunchKernel(fn, rows_grid, block, args, 0, s->stream));
        }
        if (rec) { NB_HIP(s, hipEventRecord(ev.e[1], s->stream)); ev.blk = true; s->pending.push_back(ev); }
        bool over = false;
        if (int rc = ac_read_header(s, &over, &s->ac_msg)) return rc;
        ++s->ac_regular; s->ac_substeps += nsub;
        ++s->steps_done;
        if (over) {      // this step's state is complete and kept; the next interval has no consistent list
            s->ac_over = true;
            return fail(s, NB_ERR_STATE, "nb_step: " + s->ac_msg);
        }
    }
    return NB_OK;
}

}  // namespace

namespace nbi {

// Rank form of the symmetric pass, first half of a step: the force pass over the chunk lists of the handle's own super-blocks,
// then this rank's sums for every row of the system into sym_A.
template <typename T>
int sym_rank_phase_a_t(nb_sim* s, hipEvent_t after_force, bool split_at_gather, nb_events* stamps = nullptr)
{
    using V4 = typename nb::vec4<T>::type;
    const uint32_t npass = (uint32_t)s->sym_passes.size();
    for (uint32_t q = 0; q < npass; ++q) {
        s->sym_pass = q;
        if (split_at_gather && q == 0) {
            if (s->sym_passes[0].plan[13] == 0 || s->sym_passes[0].plan[14] == 0) stamps = nullptr;      // (WA, WB: a phase without waves launches nothing to stamp)
            // Two launches with the wait for the all-gather between them.  Timed steps stamp each launch at its own begin and end
            // (hipExtLaunchKernel: e[0]..e[7] and e[3]..e[4]), so that the wait for the other ranks' rows is NOT counted as force time.
            launch_force<T>(s, 1, stamps ? stamps->e[0] : nullptr, stamps ? stamps->e[7] : nullptr);     // own-row travelers: needs nothing from the other ranks
            if (int rc = finish_gather(s)) return rc;     // the engine stream waits for their rows here
            launch_force<T>(s, 2, stamps ? stamps->e[3] : nullptr, stamps ? stamps->e[4] : nullptr);
            if (stamps) { stamps->two = true; after_force = nullptr; }
        } else {
            launch_force<T>(s);
        }
        if (after_force && q + 1 == npass) NB_HIP(s, hipEventRecord(after_force, s->stream));
        // this pass's sums for every row: into sym_A (first pass) or on top of it
        const nbp::LaunchPlan::SymPass& ps = s->sym_passes[q];
        nb::SymRankPlan rp;
        memcpy(&rp, ps.plan, sizeof rp);
        const nb::SymRowT<T>* p = (const nb::SymRowT<T>*)s->partial;
        const uint32_t* tab = s->sym_tab + ps.tab_off;
        V4* A = (V4*)s->sym_A;
        uint32_t S = ipb_of(shape_of(s));
        const void* sp = s->sym_spill;
        uint32_t d0 = ps.d0, d1 = ps.k_hi == 0xffffffffu ? 0xffffffffu : ps.k_hi / (S / 64u), acc = q ? 1u : 0u;
        void* args[] = {&p, &tab, &A, &rp, &S, &sp, &d0, &d1, &acc};
        NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_sym_reduce<T>, dim3(ceil_div(rp.np, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    }
    s->sym_pass = 0;
    return NB_OK;
}

int sym_rank_phase_a(nb_sim* s, void* after_force, bool split_at_gather, nb_events* stamps)
{
    if (!s->sym_rank) return fail(s, NB_ERR_STATE, "sym_rank_phase_a: not a rank-form handle");
    if (int rc = ensure_gm(s)) return rc;
    return s->f64 ? sym_rank_phase_a_t<double>(s, (hipEvent_t)after_force, split_at_gather, stamps) : sym_rank_phase_a_t<float>(s, (hipEvent_t)after_force, split_at_gather, stamps);
}

template <typename T>
int sym_rank_phase_b_t(nb_sim* s)
{
    launch_integrate<T>(s);                          // its rank-form branch: nb_integrate<T, 1> on the handle's rows of sym_A
    NB_HIP(s, hipGetLastError());
    return NB_OK;
}

// Second half: the plain integrate kernel on the handle's rows of the (reduce-scattered) sym_A.
int sym_rank_phase_b(nb_sim* s)
{
    if (int rc = s->f64 ? sym_rank_phase_b_t<double>(s) : sym_rank_phase_b_t<float>(s)) return rc;
    ++s->steps_done;
    s->gm_ok = false;
    return NB_OK;
}

}  // namespace nbi

extern "C" {

#ifdef NB_STAMPS
/* Diagnostic build only (`make stamps`): the per-wave s_memtime stamps of the last launch that carries them (kernels/common.hip.h,
 * NB_STAMP): 16 words per wave, `waves` waves.  tools/stamps_symw.py. */
__attribute__((visibility("default"))) int nb_debug_stamps(uint64_t* out, uint32_t waves)
{
    static unsigned long long* buf = nullptr;
    constexpr size_t kWaves = 16384;
    if (!buf) {
        if (hipMalloc((void**)&buf, kWaves * 16 * sizeof(unsigned long long)) != hipSuccess) return NB_ERR_HIP;
        (void)hipMemset(buf, 0, kWaves * 16 * sizeof(unsigned long long));
        if (hipMemcpyToSymbol(HIP_SYMBOL(nb::nb_stamp_buf), &buf, sizeof buf) != hipSuccess) return NB_ERR_HIP;
    }
    if (out && waves) {
        if (waves > kWaves) waves = kWaves;
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, buf, (size_t)waves * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return NB_ERR_HIP;
    }
    return NB_OK;
}
#endif

uint32_t nb_abi_version(void) { return NB_ABI_VERSION; }
uint32_t nb_abi_minor(void) { return NB_ABI_MINOR; }

int nb_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

// nb_create's and nb_plan_query's reading of a caller's nb_config: a normalised copy, the shard and the softening
static int read_config(const nb_config* cfg_in, const char* who, nb_config* cfg, uint32_t* sb_out, uint32_t* sc_out, double* eps2_out)
{
    const std::string w(who);
    if (cfg_in->struct_size < offsetof(nb_config, integrator))
        return fail(nullptr, NB_ERR_INVALID, w + ": struct_size too small (set it to sizeof(nb_config))");
    memset(cfg, 0, sizeof *cfg);
    memcpy(cfg, cfg_in, cfg_in->struct_size < sizeof *cfg ? cfg_in->struct_size : sizeof *cfg);
    if (cfg->n == 0) return fail(nullptr, NB_ERR_INVALID, w + ": n must be >= 1");
    if (cfg->n > (1u << 30)) return fail(nullptr, NB_ERR_INVALID, w + ": n must be <= 2^30 (32-bit row arithmetic; the reference passes N as an f32, exact to 2^24: nbody3d.js:246)");
    if (cfg->precision > NB_F64) return fail(nullptr, NB_ERR_INVALID, w + ": unknown precision");
    if (cfg->tile != 0 && cfg->tile != (uint32_t)nb::kTile)
        return fail(nullptr, NB_ERR_INVALID, w + ": only tile = 256 is built (reference TILE_SIZE)");
    const double eps2 = cfg->eps2 == 0.0 ? 1e-4 : cfg->eps2;
    if (!(eps2 >= 1e-12))
        return fail(nullptr, NB_ERR_INVALID, w + ": eps2 must be >= 1e-12 (branch-free self term needs it)");
    uint32_t sb = cfg->shard_begin, sc = cfg->shard_count;
    if (sc == 0) { sb = 0; sc = cfg->n; }
    if ((uint64_t)sb + sc > cfg->n) return fail(nullptr, NB_ERR_INVALID, w + ": shard exceeds n");
    if (cfg->integrator > NB_INT_HERMITE4) return fail(nullptr, NB_ERR_INVALID, w + ": unknown integrator");
    if (cfg->integrator == NB_INT_HERMITE4) {
        // a Hermite handle is a whole system on one device with the one force+jerk kernel of its precision
        if (cfg->shard_count != 0) return fail(nullptr, NB_ERR_INVALID, w + ": integrator = NB_INT_HERMITE4 needs shard_count == 0 (whole system)");
        if (cfg->ext_bodies) return fail(nullptr, NB_ERR_INVALID, w + ": integrator = NB_INT_HERMITE4 does not take ext_bodies");
        if (cfg->force_variant != 0) return fail(nullptr, NB_ERR_INVALID, w + ": integrator = NB_INT_HERMITE4 does not take a force_variant");
        if (cfg->jsplit != 0) return fail(nullptr, NB_ERR_INVALID, w + ": integrator = NB_INT_HERMITE4 does not take a jsplit");
    }
    *sb_out = sb; *sc_out = sc; *eps2_out = eps2;
    return NB_OK;
}

int nb_create(const nb_config* cfg_in, nb_sim** out)
{
    if (out) *out = nullptr;
    if (!cfg_in || !out) return fail(nullptr, NB_ERR_INVALID, "nb_create: null argument");
    nb_config cfg;
    uint32_t sb, sc;
    double eps2;
    if (const int rc = read_config(cfg_in, "nb_create", &cfg, &sb, &sc, &eps2)) return rc;

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, NB_ERR_NO_DEVICE,
                    std::string("nb_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                        "); this engine has no CPU fallback");
    int dev = cfg.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= count) return fail(nullptr, NB_ERR_INVALID, "nb_create: device ordinal out of range");

    nb_sim* s = new (std::nothrow) nb_sim;
    if (!s) return fail(nullptr, NB_ERR_NOMEM, "nb_create: out of host memory");
    s->n = cfg.n; s->sb = sb; s->sc = sc;
    s->f64 = cfg.precision == NB_F64;
    s->esz = s->f64 ? 8 : 4;
    s->eps2 = eps2;
    s->device = dev;

    auto bail = [&](int code, const std::string& msg) {
        std::string m = msg;
        nb_destroy(s);
        return fail(nullptr, code, m);
    };
#define NB_HIPC(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return bail(NB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

    NB_HIPC(hipSetDevice(dev));
    hipDeviceProp_t prop;
    NB_HIPC(hipGetDeviceProperties(&prop, dev));
    if (cfg.ext_stream || (cfg.flags & NB_FLAG_EXT_STREAM)) { s->stream = (hipStream_t)cfg.ext_stream; s->own_stream = false; }
    else { NB_HIPC(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)); s->own_stream = true; }

    const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    s->n_cu = n_cu;
    const double clock_hz = prop.clockRate > 0 ? 1e3 * prop.clockRate : 2.4e9;     // clockRate is in kHz
    if (cfg.integrator == NB_INT_HERMITE4) {
        // plain unpadded arrays, no planner: (x, v) at one instant, the derived (a, j), the predicted state and the bounded partials
        s->hermite = true;
        s->ac_two_calls = (cfg.flags & NB_FLAG_AC_TWO_CALLS) != 0;      // (the scheme exists on these handles only)
        set_chunks(s, kOrder4);
        hermite_names(s);
        const size_t hrow = 4 * s->esz;
        NB_HIPC(hipMalloc(&s->bodies[0], hrow * s->n));
        s->own_bodies = true;
        for (void** p : {&s->vel, &s->acc, &s->jerk, &s->hx, &s->hv}) NB_HIPC(hipMalloc(p, hrow * s->n));
        s->fj_part_bytes = (size_t)2 * hrow * s->fj_chunks * s->n;
        NB_HIPC(hipMalloc(&s->fj_part, s->fj_part_bytes));
        NB_HIPC(hipMalloc(&s->zero_row, 64));
        NB_HIPC(hipMemsetAsync(s->zero_row, 0, 64, s->stream));
        s->diag_chunk = nb::kTile * std::min(16u, std::max(1u, s->n / 16384u));
        s->diag_blocks = ceil_div(s->sc, nb::kDiagRows) * ceil_div(s->n, s->diag_chunk);
        NB_HIPC(hipMalloc((void**)&s->diag, sizeof(double) * 5 * s->diag_blocks));
        *out = s;
        return NB_OK;
    }
    plan_handle(s, cfg, n_cu, clock_hz, (double)prop.totalGlobalMem);
    if (s->sym && (!s->sym_rank || s->sym_local) && !cfg.force_variant) {
        // The planner budgets the symmetric pass's layers against the device's TOTAL memory; what is FREE right now may be less
        // (other handles, other processes).  A whole-system handle then re-plans against the free memory instead of failing in
        // hipMalloc.  (A rank-form shard does not: its peers would still expect the reduce-scatter -- it fails loudly below.)
        size_t free_b = 0, total_b = 0;
        auto need = [&]() { return 3.0 * s->esz * (double)sym_layer_rows(s) * s->sym_layers + 12.0 * s->esz * s->sym_np; };
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need() > 0.9 * (double)free_b) {
            // first with a layer budget of what IS free: the ring distances then go in passes that reuse the layers (still every
            // unordered pair once); only if even that does not fit, the ordered-pair kernels
            nb_config fit = cfg;
            fit.layer_budget_mib = (uint32_t)std::max(1.0, 0.6 * (double)free_b / 1048576.0);
            plan_handle(s, fit, n_cu, clock_hz, (double)prop.totalGlobalMem);
            if (s->sym && need() > 0.9 * (double)free_b) {
                cfg.flags |= NB_FLAG_NO_SYM;
                plan_handle(s, cfg, n_cu, clock_hz, (double)prop.totalGlobalMem);
            }
        }
    }
    if (!kernel_of(s->f64, shape_of(s))) return bail(NB_ERR_INVALID, "nb_create: no kernel for shape " + s->variant);
    s->single_sweeps = (cfg.flags & NB_FLAG_SINGLE_SWEEPS) != 0;
    // the equal-mass kernels: a whole system in the wave-granular f32 form whose plan has no padding rows (zero-mass rows, and the padded
    // lanes of a short block Z, are not of the system's one mass)
    s->eqm_capable = !(cfg.flags & NB_FLAG_NO_EQM) && s->symw && !s->sym_rank && cfg.shard_count == 0 && !cfg.ext_bodies && s->sym_np == s->n
                     && eqm_shape(s->f64, shape_of(s));
    s->no_eqm_pow2 = (cfg.flags & NB_FLAG_NO_EQM_POW2) != 0;

    const size_t row = 4 * s->esz;
    if (cfg.ext_bodies) { s->bodies[0] = cfg.ext_bodies; s->own_bodies = false; }
    else {
        const size_t rows = s->sym ? s->sym_np : s->n;        // the symmetric pass reads whole super-blocks: zero-mass rows past n
        NB_HIPC(hipMalloc(&s->bodies[0], row * rows));
        if (s->sym) NB_HIPC(hipMemset(s->bodies[0], 0, row * rows));
        s->own_bodies = true;
        if (s->fused) NB_HIPC(hipMalloc(&s->bodies[1], row * s->n));
    }
    NB_HIPC(hipMalloc(&s->vel, row * s->sc));
    NB_HIPC(hipMalloc(&s->acc, row * s->sc));
    // `partial` is allocated exactly ONCE, with the size the handle's own kernels index (round 3's memory fault: an if / else-if
    // split allocated it a second time with the ordered-pair size -- 16 n q = 8.4 MB at N = 32,768, q = 16 -- under a
    // symmetric handle that needed 12 np (q + H + 1) = 9.4 MB; profiles/r03/README.md)
    auto alloc_partial = [&](size_t bytes) -> hipError_t {
        if (s->partial) return hipErrorInvalidValue;
        s->partial_bytes = bytes;
        return hipMalloc(&s->partial, bytes);
    };
    if (s->sym) {
        // layers of (x, y, z) rows: 12 bytes (24 in f64); a rank-form handle's layers hold the rows of its own super-blocks only
        NB_HIPC(alloc_partial((size_t)3 * s->esz * sym_layer_rows(s) * s->sym_layers));
        if (s->sym_rank) NB_HIPC(hipMalloc(&s->sym_A, 4 * s->esz * s->sym_np));
        if (s->sym_spill_rows) {
            // zeroed once: a wave that never spills (its range starts at a sweep boundary) leaves its row alone, and nobody reads it
            NB_HIPC(hipMalloc(&s->sym_spill, (size_t)3 * s->esz * s->sym_spill_rows));
            NB_HIPC(hipMemset(s->sym_spill, 0, (size_t)3 * s->esz * s->sym_spill_rows));
        }
        if (s->symw && s->sym_pieces) {
            NB_HIPC(hipMalloc((void**)&s->sym_queue, 64));
            NB_HIPC(hipMemset(s->sym_queue, 0, 64));
        }
        if (s->eqm_capable) NB_HIPC(hipMalloc((void**)&s->eqm_flag, 64));
        if (s->symw) {
            NB_HIPC(hipMalloc((void**)&s->sym_tab, sizeof(uint32_t) * s->sym_tab_host.size()));
            NB_HIPC(hipMemcpy(s->sym_tab, s->sym_tab_host.data(), sizeof(uint32_t) * s->sym_tab_host.size(), hipMemcpyHostToDevice));
        }
    } else if (!s->fused) {
        NB_HIPC(alloc_partial(row * s->sc * s->jsplit));
    }
    if (s->partial_bytes != (s->sym ? (size_t)3 * s->esz * sym_layer_rows(s) * s->sym_layers : s->fused ? (size_t)0 : row * s->sc * s->jsplit))
        return bail(NB_ERR_STATE, "nb_create: the partial-sum buffer does not have the size this handle's kernels index");
    if (s->jpk) {
        // pairs: whole 4-pair units (128 B) plus one spare the loop's last request may touch; everything past the
        // system stays zero (zero-mass bodies at the origin).  Partials: 64 rows per (split, i-block).
        const size_t pbytes = ((size_t)ceil_div(ceil_div(s->n, 2u), 4u) + 3) * 128;
        const uint32_t iblocks = ceil_div(s->n, 64u);
        for (auto& p : s->pairs) { NB_HIPC(hipMalloc(&p, pbytes)); NB_HIPC(hipMemset(p, 0, pbytes)); }
        NB_HIPC(hipMalloc((void**)&s->tickets, sizeof(uint32_t) * iblocks));
        NB_HIPC(hipMemset(s->tickets, 0, sizeof(uint32_t) * iblocks));
        if (s->jsplit > 1) {
            NB_HIPC(hipMalloc(&s->jpartial, (size_t)16 * 64 * iblocks * s->jsplit));
            NB_HIPC(hipMemset(s->jpartial, 0xff, (size_t)16 * 64 * iblocks * s->jsplit));   // NaN until written
        }
        NB_HIPC(hipDeviceSynchronize());
        s->poison = (cfg.flags & NB_FLAG_POISON) != 0;
        s->jpk_fenced = (cfg.flags & NB_FLAG_JPK_FENCED) != 0;
    }
    NB_HIPC(hipMalloc(&s->zero_row, 64));                     // a zero-mass body at the origin: what the LDS-DMA staging
    NB_HIPC(hipMemsetAsync(s->zero_row, 0, 64, s->stream));   // of the packed tile kernels reads for rows past the range (stream-ordered)
    // diagnostics: a grid of (row blocks) x (j-chunks); the chunk is sized so that a few thousand workgroups share the pairs
    s->diag_chunk = nb::kTile * std::min(16u, std::max(1u, s->n / 16384u));
    s->diag_blocks = ceil_div(s->sc, nb::kDiagRows) * ceil_div(s->n, s->diag_chunk);
    NB_HIPC(hipMalloc((void**)&s->diag, sizeof(double) * 5 * s->diag_blocks));
#undef NB_HIPC
    *out = s;
    return NB_OK;
}

void nb_destroy(nb_sim* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)finish_gather(s);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    nbi::rccl_release(s);
    drop_graph(s);
    free_frames(s);
    for (auto& t : s->pool)
        for (auto& e : t.e) (void)hipEventDestroy(e);
    if (s->own_bodies) {
        if (s->bodies[0]) (void)hipFree(s->bodies[0]);
        if (s->bodies[1]) (void)hipFree(s->bodies[1]);
    }
    if (s->vel) (void)hipFree(s->vel);
    if (s->acc) (void)hipFree(s->acc);
    if (s->partial) (void)hipFree(s->partial);
    for (auto& p : s->pairs) if (p) (void)hipFree(p);
    for (auto& p : s->gm) if (p) (void)hipFree(p);
    if (s->jpartial) (void)hipFree(s->jpartial);
    if (s->tickets) (void)hipFree(s->tickets);
    if (s->sym_tab) (void)hipFree(s->sym_tab);
    if (s->sym_spill) (void)hipFree(s->sym_spill);
    if (s->sym_queue) (void)hipFree(s->sym_queue);
    if (s->eqm_flag) (void)hipFree(s->eqm_flag);
    if (s->sym_A) (void)hipFree(s->sym_A);
    for (void* p : {s->jerk, s->hx, s->hv, s->fj_part, (void*)s->blk_lev, (void*)s->blk_due, (void*)s->blk_act, (void*)s->blk_hdr}) if (p) (void)hipFree(p);
    if (s->blk_hdr_host) (void)hipHostFree(s->blk_hdr_host);
    for (void* p : {(void*)s->bb_words, s->bb_part}) if (p) (void)hipFree(p);
    if (s->bb_host) (void)hipHostFree(s->bb_host);
    for (void* p : {s->enc_w, s->enc_rho2, (void*)s->enc_partner, (void*)s->enc_time, (void*)s->enc_count, (void*)s->enc_words}) if (p) (void)hipFree(p);
    if (s->enc_host) (void)hipHostFree(s->enc_host);
    ac_release(s);
    h6_release(s);
    mx_release(s);
    if (s->diag) (void)hipFree(s->diag);
    for (auto* b : {&s->q_in[0], &s->q_in[1], &s->q_in[2], &s->q_in[3], &s->q_out[0], &s->q_out[1], &s->q_out[2], &s->q_out[3], &s->q_out[4], &s->q_out[5], &s->q_part, &s->q_off, &s->q_work, &s->q_inf, &s->q_seg, &s->q_segcnt, &s->knn_stat})
        if (b->p) (void)hipFree(b->p);
    if (s->zero_row) (void)hipFree(s->zero_row);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

const char* nb_last_error(nb_sim* s) { return s ? s->err.c_str() : g_create_error.c_str(); }

static int enc_clear_records(nb_sim* s);

int nb_upload(nb_sim* s, const void* bodies, const void* vel, const void* accel)
{
    if (!s) return NB_ERR_INVALID;
    if (!bodies || !vel) return fail(s, NB_ERR_INVALID, "nb_upload: bodies and vel are required");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    const size_t row = 4 * s->esz;
    // the reference's writeBuffer copies out of the typed array before returning
    // (nbody3d.js:186,193): synchronous copies, host pointers are not retained
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->bodies[s->cur], bodies, row * s->n, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->vel, (const char*)vel + row * s->sb, row * s->sc, hipMemcpyHostToDevice));
    if (s->hermite) {          // accel is a derived array here: ignored, re-evaluated with the jerk when next needed
        s->uploaded = true;
        s->derivs_ok = false;
        s->ac_ok = false;
        s->levels = 0;
        if (s->enc) return enc_clear_records(s);      // the watch's records belonged to the state replaced here; its configuration and counters stay
        return NB_OK;
    }
    if (accel) NB_HIP(s, hipMemcpy(s->acc, (const char*)accel + row * s->sb, row * s->sc, hipMemcpyHostToDevice));
    else {
        // WebGPU zero-init, nbody3d.js:195-199.  On the ENGINE stream: a hipMemset on the null stream is
        // asynchronous for device memory and the engine's non-blocking stream does not wait for it
        // -- the fused step reads accel in its first microsecond.
        NB_HIP(s, hipMemsetAsync(s->acc, 0, row * s->sc, s->stream));
        NB_HIP(s, hipStreamSynchronize(s->stream));
    }
    s->uploaded = true;
    s->pairs_ok = false;
    s->gm_ok = false;
    if (s->eqm_capable) {
        // the host arrays are at hand: every mass lane the bits of row 0's, every vel.w and acc.w zero (what nb_eqm_check asks on the device)
        const float *hb = (const float*)bodies, *hv = (const float*)vel, *ha = (const float*)accel;
        uint32_t m0;
        memcpy(&m0, hb + 3, sizeof m0);
        bool same = true;
        for (uint32_t i = 0; i < s->n && same; ++i) {
            uint32_t m;
            memcpy(&m, hb + 4 * (size_t)i + 3, sizeof m);
            same = m == m0 && hv[4 * (size_t)i + 3] == 0.f && (!ha || ha[4 * (size_t)i + 3] == 0.f);
        }
        s->eqm = same ? nb_sim::kEqmYes : nb_sim::kEqmNo;
        s->eqm_m0 = m0;
    }
    return NB_OK;
}

int nb_set_params(nb_sim* s, double dt, double G)
{
    if (!s) return NB_ERR_INVALID;
    if (!(dt == dt) || !(G == G)) return fail(s, NB_ERR_INVALID, "nb_set_params: NaN");
    if (s->params_set && (dt != s->dt || G != s->G)) s->levels = 0;      // block steps: the levels belong to (dt, G)
    if (s->params_set && dt != s->dt) s->ac_ok = false;                  // the neighbour scheme starts again from (x, v) (a changed G: ensure_scheme)
    s->dt = dt; s->G = G; s->params_set = true;
    return NB_OK;
}

int nb_step(nb_sim* s, uint32_t nsteps)
{
    if (!s) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_step: nb_upload has not been called");
    if (!s->params_set) return fail(s, NB_ERR_STATE, "nb_step: nb_set_params has not been called");
    if (!(s->dt > 0.0)) return NB_OK;   // `if (dt > 0)` gate, nbody3d.js:474
    NB_HIP(s, hipSetDevice(s->device));
    if (s->hermite) return s->ac ? ac_step(s, nsteps) : s->blk ? (s->bb ? block_batch_step(s, nsteps) : block_step(s, nsteps)) : hermite_step(s, nsteps);
    const bool exchange = s->xfn || s->rccl;
    ensure_pairs(s);      // the j-packed step's position copy, if something outside the step rewrote the positions or G
    if (gm_active(s) && !s->gm_ok) { if (int rc = finish_gather(s)) return rc; }
    if (int rc = ensure_gm(s)) return rc;   // the packed K1 forms' (x, y, z, G*m) j-stream, likewise
    if (int rc = ensure_eqm(s)) return rc;  // whether the equal-mass kernels may run, if a pointer was handed out since it was last known
    // Multi-step calls on the engine's own stream replay a captured graph of
    // kGraphChunk steps (no exchange, no per-kernel timing requested).
    if (s->own_stream && s->graphs_ok && !exchange && !s->timing && !s->sym_rank && nsteps >= kGraphChunk) {
        for (int which = 1; which >= 0; --which) {
            while (nsteps >= kGraphSteps[which] && ensure_graph(s, which)) {
                NB_HIP(s, hipGraphLaunch(s->graphs[which].exec, s->stream));
                nsteps -= kGraphSteps[which];
                s->steps_done += kGraphSteps[which];
            }
        }
    }
    for (uint32_t k = 0; k < nsteps; ++k) {
        if (exchange && gm_active(s) && !s->gm_ok) {
            // G != 1 on a handle whose rows are exchanged: the other ranks' rows of the j-stream copy are rebuilt from the
            // gathered positions (one small launch per step; the overlapped form waits here, so it only overlaps at G == 1,
            // which every multi-GPU configuration of BASELINE.json uses)
            if (int rc = finish_gather(s)) return rc;
            if (int rc = ensure_gm(s)) return rc;
        }
        if (s->sym_rank) {
            // rank form of the symmetric pass: force pass -> this rank's sums for every row -> reduce-scatter across the ranks
            // -> integrate own rows -> all-gather of the new positions
            if (!s->rccl && !s->sym_local) return fail(s, NB_ERR_STATE, "nb_step: an NB_FLAG_SYM_SHARD handle needs nb_rccl_attach (or nb_multi) for its reduce-scatter");
            // an overlapped all-gather of the previous step still in flight: the sweeps whose travelers are this rank's own rows
            // (phase A, ~1 / ranks of the work) are issued before the engine stream waits for it
            const bool split = s->gather_pending;
            if (!split) { if (int rc = finish_gather(s)) return rc; }
            nb_events evr;
            const bool recr = s->timing && get_events(s, &evr) == 0;
            // one force launch: plain records around it; split at the gather: each launch stamped at its own begin / end (evr.two)
            if (recr) NB_HIP(s, hipEventRecord(evr.e[0], s->stream));
            if (int rc = nbi::sym_rank_phase_a(s, recr ? evr.e[7] : nullptr, split, recr && split ? &evr : nullptr)) return rc;
            if (recr) { NB_HIP(s, hipEventRecord(evr.e[1], s->stream)); evr.rs = true; }
            if (!s->sym_local) { if (int rc = nbi::rccl_reduce_scatter_A(s)) return rc; }
            if (recr) NB_HIP(s, hipEventRecord(evr.e[6], s->stream));
            if (int rc = nbi::sym_rank_phase_b(s)) return rc;
            if (recr) NB_HIP(s, hipEventRecord(evr.e[2], s->stream));
            NB_HIP(s, hipGetLastError());
            if (s->sym_local) { if (recr) s->pending.push_back(evr); continue; }      // a whole system on this device: nothing to exchange
            if (int rc = nbi::rccl_exchange_begin(s)) return rc;
            if (nbi::rccl_overlapped(s)) s->gather_pending = true;        // waited for inside the next force pass (or by whoever reads the positions first)
            else if (recr) { NB_HIP(s, hipEventRecord(evr.e[5], s->stream)); evr.xchg = true; }
            if (recr) s->pending.push_back(evr);
            continue;
        }
        nb_events ev;
        const bool rec = s->timing && get_events(s, &ev) == 0;
        hipEvent_t* e = rec ? ev.e : nullptr;
        if (s->fused) {
            launch_fused(s, e ? e[0] : nullptr, e ? e[1] : nullptr);
        } else {
            if (s->gather_pending) {
                // the previous step's all-gather is still in flight: own-row splits first
                if (s->f64) launch_force<double>(s, 1, e ? e[0] : nullptr, e ? e[1] : nullptr);
                else launch_force<float>(s, 1, e ? e[0] : nullptr, e ? e[1] : nullptr);
                if (int rc = finish_gather(s)) return rc;
                if (s->f64) launch_force<double>(s, 2, e ? e[3] : nullptr, e ? e[4] : nullptr);
                else launch_force<float>(s, 2, e ? e[3] : nullptr, e ? e[4] : nullptr);
                if (rec) ev.two = s->own_splits > 0 && s->own_splits < s->jsplit;
            } else {
                if (s->f64) launch_force<double>(s, 0, e ? e[0] : nullptr, e ? e[1] : nullptr);
                else launch_force<float>(s, 0, e ? e[0] : nullptr, e ? e[1] : nullptr);
            }
            if (s->f64) launch_integrate<double>(s, e ? e[6] : nullptr, e ? e[2] : nullptr);
            else launch_integrate<float>(s, e ? e[6] : nullptr, e ? e[2] : nullptr);
        }
        NB_HIP(s, hipGetLastError());
        if (s->force_err != hipSuccess) { const hipError_t queue_reset = s->force_err; s->force_err = hipSuccess; NB_HIP(s, queue_reset); }
        ++s->steps_done;
        if (exchange) s->gm_ok = false;
        if (s->rccl) {
            if (int rc = nbi::rccl_exchange_begin(s)) return rc;
            if (nbi::rccl_overlapped(s)) {
                s->gather_pending = true;
                if (s->own_splits == 0) { if (int rc2 = finish_gather(s)) return rc2; }
            } else if (rec) {
                NB_HIP(s, hipEventRecord(ev.e[5], s->stream));
                ev.xchg = true;
            }
        } else if (s->xfn) {
            int rc = s->xfn(s->xuser, s->bodies[s->cur], s->esz, s->n, s->sb, s->sc, (void*)s->stream);
            if (rc != 0) return fail(s, NB_ERR_COMM, "nb_step: exchange hook failed with code " + std::to_string(rc));
            if (s->xwait) {
                s->gather_pending = true;
                // nothing to overlap with: splits do not line up with the shard
                if (s->own_splits == 0) { if (int rc2 = finish_gather(s)) return rc2; }
            }
        }
        if (rec) s->pending.push_back(ev);
    }
    return NB_OK;
}

int nb_sync(nb_sim* s)
{
    if (!s) return NB_ERR_INVALID;
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    return NB_OK;
}

int nb_download(nb_sim* s, void* bodies, void* vel, void* accel)
{
    if (!s) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_download: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    if (s->hermite && accel) { if (int rc = ensure_derivs(s, "nb_download")) return rc; }
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const size_t row = 4 * s->esz;
    if (bodies) NB_HIP(s, hipMemcpy(bodies, s->bodies[s->cur], row * s->n, hipMemcpyDeviceToHost));
    if (vel) NB_HIP(s, hipMemcpy((char*)vel + row * s->sb, s->vel, row * s->sc, hipMemcpyDeviceToHost));
    if (accel) NB_HIP(s, hipMemcpy((char*)accel + row * s->sb, s->acc, row * s->sc, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_device_ptr(nb_sim* s, int which, void** out)
{
    if (!s || !out) return NB_ERR_INVALID;
    if (which == NB_JERK && !s->hermite) return fail(s, NB_ERR_STATE, "nb_device_ptr: NB_JERK needs a Hermite handle (nb_config.integrator)");
    if (s->hermite && (which == NB_ACCEL || which == NB_JERK)) {
        if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_device_ptr: nothing uploaded yet");
        NB_HIP(s, hipSetDevice(s->device));
        if (int rc = ensure_derivs(s, "nb_device_ptr")) return rc;
    }
    switch (which) {
        case NB_BODIES: *out = s->bodies[s->cur]; s->pairs_ok = false; s->gm_ok = false; s->derivs_ok = false; s->ac_ok = false; s->levels = 0; s->eqm = nb_sim::kEqmUnknown; break;   // the caller may write through it
        case NB_VEL: *out = s->vel; s->derivs_ok = false; s->ac_ok = false; s->levels = 0; s->eqm = nb_sim::kEqmUnknown; break;      // (the w lanes: see ensure_eqm)
        case NB_ACCEL: *out = s->acc; s->eqm = nb_sim::kEqmUnknown; break;
        case NB_JERK: *out = s->jerk; break;
        default: return fail(s, NB_ERR_INVALID, "nb_device_ptr: unknown array");
    }
    return NB_OK;
}

int nb_download_jerk(nb_sim* s, void* jerk)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_download_jerk: null handle");
    if (!jerk) return fail(s, NB_ERR_INVALID, "nb_download_jerk: jerk is NULL");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_download_jerk: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_download_jerk: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_derivs(s, "nb_download_jerk")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(jerk, s->jerk, 4 * s->esz * s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_upload_derivs(nb_sim* s, const void* accel, const void* jerk)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_upload_derivs: null handle");
    if (!accel || !jerk) return fail(s, NB_ERR_INVALID, "nb_upload_derivs: accel and jerk are required");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_upload_derivs: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_upload_derivs: the handle's order is 6 (nb_set_hermite_order): its checkpoint is four arrays, see nb_upload_derivs6");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_upload_derivs: nb_upload has not been called");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->acc, accel, 4 * s->esz * s->n, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->jerk, jerk, 4 * s->esz * s->n, hipMemcpyHostToDevice));
    s->derivs_ok = true;
    s->derivs_any_G = !s->params_set;
    s->derivs_G = s->G;
    s->ac_ok = false;      // the neighbour scheme keeps its own components: its start runs again (the uploaded totals are replaced)
    return NB_OK;
}

int nb_set_hermite_order(nb_sim* s, uint32_t order)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_hermite_order: null handle");
    if (order != 4 && order != 6) return fail(s, NB_ERR_INVALID, "nb_set_hermite_order: order must be 4 or 6");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (order == 6 && s->enc) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 6 while the encounter watch is switched on (nb_set_encounter_watch): it exists at order 4 only, switch it off first");
    if (order == 6 && s->bb && !s->h6) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 6 while batched block steps are switched on (nb_set_block_batch): they exist at order 4 only, switch them off first");
    if (order == 6 && s->blk && !s->h6) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 6 while block steps are switched on (nb_set_block_steps): they exclude each other");
    if (order == 4 && s->blk && s->h6) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 4 while block steps of order 6 are switched on (nb_set_block_steps6): switch them off first");
    if (order == 6 && s->mx) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 6 while the pass precision is NB_PASS_MIXED (nb_set_pass_precision): the mixed pass exists at order 4 only, set NB_PASS_NATIVE first");
    if (order == 6 && s->ac) return fail(s, NB_ERR_STATE, "nb_set_hermite_order: order = 6 while the neighbour scheme is switched on (nb_set_neighbor_scheme): they exclude each other");
    if ((order == 6) == s->h6) return NB_OK;
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    if (order == 4) {          // snap and crackle go, (a, j) stay current
        h6_release(s);
        hermite_names(s);
        return NB_OK;
    }
    set_chunks(s, kOrder6);
    const size_t rows = 4 * s->esz * s->n;
    hipError_t e = hipSuccess;
    for (void** p : {&s->snap, &s->crackle, &s->ha})
        if (e == hipSuccess) e = hipMalloc(p, rows);
    if (e == hipSuccess) e = hipMalloc(&s->h6_part, (size_t)3 * rows * s->h6_chunks);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h6_release(s);
        return fail(s, NB_ERR_HIP, std::string("nb_set_hermite_order: ") + hipGetErrorString(e));
    }
    s->h6 = true; s->snap_ok = false;
    hermite_names(s);
    return NB_OK;
}

int nb_hermite_order(nb_sim* s, uint32_t* order)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_hermite_order: null handle");
    if (!order) return fail(s, NB_ERR_INVALID, "nb_hermite_order: order is NULL");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_hermite_order: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    *order = s->h6 ? 6u : 4u;
    return NB_OK;
}

int nb_set_pass_precision(nb_sim* s, uint32_t mode)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_pass_precision: null handle");
    if (mode != NB_PASS_NATIVE && mode != NB_PASS_MIXED) return fail(s, NB_ERR_INVALID, "nb_set_pass_precision: mode must be NB_PASS_NATIVE or NB_PASS_MIXED");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!s->f64) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: precision NB_F32: the mixed pass keeps an fp64 state, it exists on NB_F64 handles only");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: the handle's order is 6 (nb_set_hermite_order): the mixed pass exists at order 4 only");
    if (s->ac) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: the neighbour scheme is switched on (nb_set_neighbor_scheme): it has no mixed kernels");
    if (mode == NB_PASS_MIXED && s->bb && !s->mx) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: NB_PASS_MIXED while batched block steps are switched on (nb_set_block_batch): they run the native pass only, switch them off first");
    if (mode == NB_PASS_NATIVE && s->bb && s->mx) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: NB_PASS_NATIVE while the batched block steps of a mixed handle are switched on (nb_set_block_batch_mixed): they run the mixed pass only, switch them off first");
    if (mode == NB_PASS_MIXED && s->enc) return fail(s, NB_ERR_STATE, "nb_set_pass_precision: NB_PASS_MIXED while the encounter watch is switched on (nb_set_encounter_watch): it runs in the native pass only, switch it off first");
    if ((mode == NB_PASS_MIXED) == s->mx) return NB_OK;
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    // Neither direction touches the state, the derivatives or the levels: what they hold stays what it is, the next pass runs in the new mode.
    if (mode == NB_PASS_NATIVE) {
        mx_release(s);
        hermite_names(s);
        return NB_OK;
    }
    chunk_shape(s->n, kMixed.rows[1], s->n_cu, &s->mx_chunks, &s->mx_per);
    hipError_t e = hipSuccess;
    for (void*& p : s->mx_in)
        if (e == hipSuccess) e = hipMalloc(&p, sizeof(float) * 4 * s->n);
    // the partial rows were sized for the native pass (kFjRows64 rows per workgroup, 32-byte rows): the mixed shape has up to four
    // times the chunks of 16-byte rows
    const size_t need = (size_t)2 * 16 * s->mx_chunks * s->n;
    if (e == hipSuccess && need > s->fj_part_bytes) {
        void* grown = nullptr;
        e = hipMalloc(&grown, need);
        if (e == hipSuccess) { (void)hipFree(s->fj_part); s->fj_part = grown; s->fj_part_bytes = need; }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        mx_release(s);
        return fail(s, NB_ERR_HIP, std::string("nb_set_pass_precision: ") + hipGetErrorString(e));
    }
    s->mx = true;
    hermite_names(s);
    return NB_OK;
}

int nb_pass_precision(nb_sim* s, uint32_t* mode)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_pass_precision: null handle");
    if (!mode) return fail(s, NB_ERR_INVALID, "nb_pass_precision: mode is NULL");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_pass_precision: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    *mode = s->mx ? NB_PASS_MIXED : NB_PASS_NATIVE;
    return NB_OK;
}

int nb_set_pass_guard(nb_sim* s, double r_near)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_pass_guard: null handle");
    if (!(r_near >= 0.0) || std::isinf(r_near)) return fail(s, NB_ERR_INVALID, "nb_set_pass_guard: r_near must be finite and >= 0 (0 switches the guard off)");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_pass_guard: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) whose pass precision is NB_PASS_MIXED (nb_set_pass_precision)");
    if (!s->f64) return fail(s, NB_ERR_STATE, "nb_set_pass_guard: precision NB_F32: the guard belongs to the mixed pass of NB_F64 handles (nb_set_pass_precision)");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_pass_guard: the handle's order is 6 (nb_set_hermite_order): the mixed pass (nb_set_pass_precision) and its guard exist at order 4 only");
    if (!s->mx) return fail(s, NB_ERR_STATE, "nb_set_pass_guard: the pass precision is NB_PASS_NATIVE: set NB_PASS_MIXED first (nb_set_pass_precision)");
    if (r_near > 0.0 && s->bb) return fail(s, NB_ERR_STATE, "nb_set_pass_guard: r_near > 0 while batched block steps are switched on (nb_set_block_batch_mixed): they have no guarded pass, switch them off first");
    if ((r_near > 0.0) == (s->mx_guard > 0.0)) { s->mx_guard = r_near; return NB_OK; }      // another radius, or off and off: the kernels and the rows stay
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    // Neither direction touches the state, the derivatives or the levels.  The guarded passes leave fp64 partial rows in the mixed
    // pass's j-chunks: twice the bytes.  (Grown once; a handle keeps the larger buffer.)
    const size_t need = (size_t)2 * 32 * s->mx_chunks * s->n;
    if (r_near > 0.0 && need > s->fj_part_bytes) {
        void* grown = nullptr;
        const hipError_t e = hipMalloc(&grown, need);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(s, NB_ERR_HIP, std::string("nb_set_pass_guard: ") + hipGetErrorString(e));
        }
        (void)hipFree(s->fj_part); s->fj_part = grown; s->fj_part_bytes = need;
    }
    s->mx_guard = r_near;
    hermite_names(s);
    return NB_OK;
}

int nb_pass_guard(nb_sim* s, double* r_near)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_pass_guard: null handle");
    if (!r_near) return fail(s, NB_ERR_INVALID, "nb_pass_guard: r_near is NULL");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_pass_guard: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    *r_near = s->mx ? s->mx_guard : 0.0;
    return NB_OK;
}

int nb_download_snap(nb_sim* s, void* snap, void* crackle)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_download_snap: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_download_snap: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_download_snap: the handle's order is 4: snap and crackle exist at order 6 (nb_set_hermite_order)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_download_snap: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_start(s, "nb_download_snap")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    if (snap) NB_HIP(s, hipMemcpy(snap, s->snap, 4 * s->esz * s->n, hipMemcpyDeviceToHost));
    if (crackle) NB_HIP(s, hipMemcpy(crackle, s->crackle, 4 * s->esz * s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_upload_derivs6(nb_sim* s, const void* accel, const void* jerk, const void* snap, const void* crackle)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_upload_derivs6: null handle");
    if (!accel || !jerk || !snap || !crackle) return fail(s, NB_ERR_INVALID, "nb_upload_derivs6: accel, jerk, snap and crackle are required");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_upload_derivs6: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_upload_derivs6: the handle's order is 4 (nb_set_hermite_order): see nb_upload_derivs");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_upload_derivs6: nb_upload has not been called");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const size_t rows = 4 * s->esz * s->n;
    NB_HIP(s, hipMemcpy(s->acc, accel, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->jerk, jerk, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->snap, snap, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->crackle, crackle, rows, hipMemcpyHostToDevice));
    s->derivs_ok = true;
    s->derivs_any_G = !s->params_set;
    s->derivs_G = s->G;
    s->snap_ok = true; s->start_own = false;
    return NB_OK;
}

int nb_set_start6(nb_sim* s, uint32_t mode)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_start6: null handle");
    if (mode != NB_START6_ZERO && mode != NB_START6_CRACKLE) return fail(s, NB_ERR_INVALID, "nb_set_start6: mode must be NB_START6_ZERO or NB_START6_CRACKLE");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_start6: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) of order 6 (nb_set_hermite_order)");
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_set_start6: the handle's order is 4 (nb_set_hermite_order): the start of an order-4 handle has no modes");
    if (mode == s->start6) return NB_OK;
    s->start6 = mode;
    // a start and levels the engine made itself and no step has consumed are made again in the new mode; an uploaded start, uploaded
    // levels and a running state stay as they are
    if (s->snap_ok && s->start_own) s->snap_ok = false;
    if (s->levels == 2 && s->levels_own) s->levels = 0;
    return NB_OK;
}

int nb_start6(nb_sim* s, uint32_t* mode)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_start6: null handle");
    if (!mode) return fail(s, NB_ERR_INVALID, "nb_start6: mode is NULL");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_start6: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) of order 6 (nb_set_hermite_order)");
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_start6: the handle's order is 4 (nb_set_hermite_order): the start of an order-4 handle has no modes");
    *mode = s->start6;
    return NB_OK;
}

// What nb_set_block_steps and nb_set_block_steps6 share: the checks of the configuration, the arrays (allocated when first switched
// on, each on its own: a failed call may be repeated) and the switch.  The levels go stale, nothing else.
static int blk_configure(nb_sim* s, const nb_block_steps* cfg, const char* who)
{
    const std::string w(who);
    if (cfg->struct_size != sizeof(nb_block_steps)) return fail(s, NB_ERR_INVALID, w + ": struct_size must be sizeof(nb_block_steps)");
    const uint32_t L = cfg->max_level ? cfg->max_level : 20u;
    if (cfg->max_level > 30) return fail(s, NB_ERR_INVALID, w + ": max_level is at most 30");
    if (cfg->min_level > L) return fail(s, NB_ERR_INVALID, w + ": min_level must not exceed max_level");
    if (cfg->flags & ~NB_BLOCK_FROZEN) return fail(s, NB_ERR_INVALID, w + ": unknown flags");
    if (!(cfg->eta >= 0.0)) return fail(s, NB_ERR_INVALID, w + ": eta must be > 0 (0: the default 0.02)");
    NB_HIP(s, hipSetDevice(s->device));
    if (!s->blk_lev) NB_HIP(s, hipMalloc((void**)&s->blk_lev, s->n));
    if (!s->blk_due) NB_HIP(s, hipMalloc((void**)&s->blk_due, sizeof(uint32_t) * s->n));
    if (!s->blk_act) NB_HIP(s, hipMalloc((void**)&s->blk_act, sizeof(uint32_t) * s->n));
    if (!s->blk_hdr) {
        NB_HIP(s, hipMalloc((void**)&s->blk_hdr, sizeof(uint32_t) * nb::kBlkWords));
        NB_HIP(s, hipMemsetAsync(s->blk_hdr, 0, sizeof(uint32_t) * nb::kBlkWords, s->stream));
    }
    if (!s->blk_hdr_host) NB_HIP(s, hipHostMalloc((void**)&s->blk_hdr_host, sizeof(uint32_t) * nb::kBlkWords, hipHostMallocDefault));
    if (!s->blk_hdr_pub) NB_HIP(s, hipHostGetDevicePointer((void**)&s->blk_hdr_pub, s->blk_hdr_host, 0));
    s->blk = true;
    s->blk_L = L; s->blk_lmin = cfg->min_level; s->blk_frozen = (cfg->flags & NB_BLOCK_FROZEN) != 0;
    s->blk_eta = cfg->eta > 0.0 ? cfg->eta : 0.02;
    s->levels = 0;
    return NB_OK;
}

int nb_set_block_steps(nb_sim* s, const nb_block_steps* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_steps: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_steps: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!cfg) { s->blk = false; s->bb = false; s->enc = false; s->levels = 0; return NB_OK; }      // (the batched mode and the encounter watch belong to the block steps: off with them)
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_steps: the handle's order is 6 (nb_set_hermite_order): block steps and the 6th-order scheme exclude each other here, see nb_set_block_steps6");
    if (s->ac) return fail(s, NB_ERR_STATE, "nb_set_block_steps: the neighbour scheme is switched on (nb_set_neighbor_scheme): block steps and the neighbour scheme exclude each other");
    return blk_configure(s, cfg, "nb_set_block_steps");
}

int nb_set_block_steps6(nb_sim* s, const nb_block_steps* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_steps6: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_steps6: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) of order 6 (nb_set_hermite_order)");
    if (!cfg) { s->blk = false; s->bb = false; s->levels = 0; return NB_OK; }      // (the batched mode belongs to the block steps: off with them)
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_steps6: the handle's order is 4 (nb_set_hermite_order): see nb_set_block_steps");
    if (cfg->struct_size == sizeof(nb_block_steps) && !s->f64 && !(cfg->flags & NB_BLOCK_FROZEN))
        return fail(s, NB_ERR_STATE, "nb_set_block_steps6: precision NB_F32 without flags = NB_BLOCK_FROZEN: the criterion's a4 and a5 cannot be formed from binary32 derivatives (rounding noise); dynamic levels of order 6 need an NB_F64 handle");
    return blk_configure(s, cfg, "nb_set_block_steps6");
}

int nb_block_stats(nb_sim* s, struct nb_block_stats* out, int reset)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_block_stats: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_block_stats: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!out || out->struct_size != sizeof(struct nb_block_stats)) return fail(s, NB_ERR_INVALID, "nb_block_stats: set out->struct_size to sizeof(nb_block_stats)");
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->enabled = s->blk ? 1u : 0u;
    if (!s->blk_hdr) return NB_OK;
    NB_HIP(s, hipSetDevice(s->device));
    uint32_t words[nb::kBlkWords];
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(words, s->blk_hdr, sizeof words, hipMemcpyDeviceToHost));
    out->outer_steps = s->blk_outer; out->block_steps = s->blk_steps; out->body_steps = s->blk_body_steps;
    out->clamped = words[nb::kBlkClamped];
    out->finest_level = words[nb::kBlkFinest];
    if (reset) {
        s->blk_outer = s->blk_steps = s->blk_body_steps = 0;
        NB_HIP(s, hipMemsetAsync(s->blk_hdr, 0, sizeof(uint32_t) * nb::kBlkWords, s->stream));
    }
    return NB_OK;
}

// The argument checks nb_set_block_batch, nb_set_block_batch6 and nb_set_block_batch_mixed share (who: the entry point's name).
int bb_check(nb_sim* s, const nb_block_batch* cfg, const std::string& who)
{
    if (cfg->struct_size != sizeof(nb_block_batch)) return fail(s, NB_ERR_INVALID, who + ": struct_size must be sizeof(nb_block_batch)");
    if (cfg->depth > 1024) return fail(s, NB_ERR_INVALID, who + ": depth is at most 1024 (0: the default 32)");
    if (cfg->small_max > nb::kBbMaxSmall && cfg->small_max != NB_BLOCK_BATCH_SMALL_DEFAULT)
        return fail(s, NB_ERR_INVALID, who + ": small_max is at most 1024 (NB_BLOCK_BATCH_SMALL_DEFAULT: the default 256)");
    if (cfg->flags != 0) return fail(s, NB_ERR_INVALID, who + ": flags must be 0");
    return NB_OK;
}

// ... and what they do behind their state checks: the mode on, for the order the handle has.
int bb_configure(nb_sim* s, const nb_block_batch* cfg)
{
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    bb_shape(s->n, s->n_cu, &s->bb_chunks, &s->bb_per);
    if (!s->bb_words) {
        NB_HIP(s, hipMalloc((void**)&s->bb_words, sizeof(uint32_t) * nb::kBbWords));
        NB_HIP(s, hipMemset(s->bb_words, 0, sizeof(uint32_t) * nb::kBbWords));
    }
    if (!s->bb_host) {
        NB_HIP(s, hipHostMalloc((void**)&s->bb_host, sizeof(uint32_t) * nb::kBbWords, hipHostMallocDefault));
        std::memset(s->bb_host, 0, sizeof(uint32_t) * nb::kBbWords);
    }
    if (!s->bb_pub) NB_HIP(s, hipHostGetDevicePointer((void**)&s->bb_pub, s->bb_host, 0));
    const uint32_t planes = order_of(s).planes;
    if (s->bb_part && s->bb_planes != planes) { NB_HIP(s, hipFree(s->bb_part)); s->bb_part = nullptr; }      // the order changed since
    if (!s->bb_part) {
        NB_HIP(s, hipMalloc(&s->bb_part, (size_t)planes * 4 * s->esz * s->bb_chunks * nb::kBbMaxSmall));
        s->bb_planes = planes;
    }
    // Touches no state, no derivatives and no levels; the policy starts over (one slot).
    s->bb = true;
    s->bb_depth = cfg->depth ? cfg->depth : 32u;
    s->bb_small_max = cfg->small_max == NB_BLOCK_BATCH_SMALL_DEFAULT ? 256u : cfg->small_max;
    s->bb_fresh = true; s->bb_t = 0; s->bb_park_ctz = s->blk_L;
    return NB_OK;
}

int nb_set_block_batch(nb_sim* s, const nb_block_batch* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_batch: null handle");
    if (!cfg) { s->bb = false; return NB_OK; }
    if (int rc = bb_check(s, cfg, "nb_set_block_batch")) return rc;
    if (s->enc) return fail(s, NB_ERR_STATE, "nb_set_block_batch: the encounter watch is switched on (nb_set_encounter_watch): it runs on the base path of block steps only, switch it off first");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_batch: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) with block steps switched on (nb_set_block_steps)");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_batch: the handle's order is 6 (nb_set_hermite_order): batched block steps exist at order 4 only");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_set_block_batch: block steps are not switched on (nb_set_block_steps)");
    if (s->mx) return fail(s, NB_ERR_STATE, "nb_set_block_batch: the pass precision is NB_PASS_MIXED (nb_set_pass_precision): batched block steps run the native pass only");
    return bb_configure(s, cfg);
}

int nb_set_block_batch6(nb_sim* s, const nb_block_batch* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_batch6: null handle");
    if (!cfg) { s->bb = false; return NB_OK; }
    if (int rc = bb_check(s, cfg, "nb_set_block_batch6")) return rc;
    if (s->enc) return fail(s, NB_ERR_STATE, "nb_set_block_batch6: the encounter watch is switched on (nb_set_encounter_watch): it runs on the base path of block steps only, switch it off first");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_batch6: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) of order 6 (nb_set_hermite_order) with block steps switched on (nb_set_block_steps6)");
    if (!s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_batch6: the handle's order is 4 (nb_set_hermite_order): see nb_set_block_batch");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_set_block_batch6: block steps are not switched on (nb_set_block_steps6)");
    return bb_configure(s, cfg);
}

int nb_set_block_batch_mixed(nb_sim* s, const nb_block_batch* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_batch_mixed: null handle");
    if (!cfg) { s->bb = false; return NB_OK; }
    if (int rc = bb_check(s, cfg, "nb_set_block_batch_mixed")) return rc;
    if (s->enc) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: the encounter watch is switched on (nb_set_encounter_watch): it runs on the base path of block steps only, switch it off first");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) with block steps switched on (nb_set_block_steps)");
    if (!s->f64) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: precision NB_F32: the mixed pass (nb_set_pass_precision) exists on NB_F64 handles only, see nb_set_block_batch");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: the handle's order is 6 (nb_set_hermite_order): the mixed pass exists at order 4 only, see nb_set_block_batch6");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: block steps are not switched on (nb_set_block_steps)");
    if (!s->mx) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: the pass precision is NB_PASS_NATIVE: set NB_PASS_MIXED first (nb_set_pass_precision), or see nb_set_block_batch");
    if (s->mx_guard > 0.0) return fail(s, NB_ERR_STATE, "nb_set_block_batch_mixed: a guard radius is set (nb_set_pass_guard): batched block steps have no guarded pass, call nb_set_pass_guard(0) first");
    return bb_configure(s, cfg);
}

// nb_set_block_batch's mode on a handle with the encounter watch on (the other three setters refuse such a handle): the slot's pass
// and corrector are kWatch's.
int nb_set_block_batch_watch(nb_sim* s, const nb_block_batch* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_block_batch_watch: null handle");
    if (!cfg) { s->bb = false; return NB_OK; }
    if (int rc = bb_check(s, cfg, "nb_set_block_batch_watch")) return rc;
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) with block steps (nb_set_block_steps) and the encounter watch (nb_set_encounter_watch) switched on");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: the handle's order is 6 (nb_set_hermite_order): the encounter watch exists at order 4 only, see nb_set_block_batch6");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: block steps are not switched on (nb_set_block_steps)");
    if (s->mx) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: the pass precision is NB_PASS_MIXED (nb_set_pass_precision, nb_set_pass_guard): the encounter watch runs in the native pass only, set NB_PASS_NATIVE first or see nb_set_block_batch_mixed");
    if (s->bb && !s->enc) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: another batched mode is switched on (nb_set_block_batch): switch it off first (nb_set_block_batch(s, NULL)), then nb_set_encounter_watch, then this call");
    if (!s->enc) return fail(s, NB_ERR_STATE, "nb_set_block_batch_watch: the encounter watch is not switched on: call nb_set_encounter_watch first, or nb_set_block_batch for the mode without a watch");
    return bb_configure(s, cfg);      // (while this mode is on: depth and small_max anew, as the other setters)
}

int nb_block_batch_stats(nb_sim* s, struct nb_block_batch_stats* out, int reset)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_block_batch_stats: null handle");
    if (!out || out->struct_size != sizeof(struct nb_block_batch_stats)) return fail(s, NB_ERR_INVALID, "nb_block_batch_stats: set out->struct_size to sizeof(nb_block_batch_stats)");
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->enabled = s->bb ? 1u : 0u;
    out->host_waits = s->bb_waits; out->slots = s->bb_slots; out->small_steps = s->bb_small; out->host_steps = s->bb_hoststeps; out->idle_slots = s->bb_idle;
    if (reset) s->bb_waits = s->bb_slots = s->bb_small = s->bb_hoststeps = s->bb_idle = 0;
    return NB_OK;
}

int nb_download_levels(nb_sim* s, uint8_t* levels)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_download_levels: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_download_levels: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!levels) return fail(s, NB_ERR_INVALID, "nb_download_levels: levels is NULL");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_download_levels: block steps are not switched on (nb_set_block_steps)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_download_levels: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_levels(s, "nb_download_levels")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(levels, s->blk_lev, s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_upload_levels(nb_sim* s, const uint8_t* levels)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_upload_levels: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_upload_levels: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!levels) return fail(s, NB_ERR_INVALID, "nb_upload_levels: levels is NULL");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_upload_levels: block steps are not switched on (nb_set_block_steps)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_upload_levels: nb_upload has not been called");
    for (uint32_t i = 0; i < s->n; ++i)
        if (levels[i] < s->blk_lmin || levels[i] > s->blk_L)
            return fail(s, NB_ERR_INVALID, "nb_upload_levels: levels[" + std::to_string(i) + "] = " + std::to_string(levels[i]) + " is outside [min_level, max_level]");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->blk_lev, levels, s->n, hipMemcpyHostToDevice));
    s->levels = 1;      // the start kernel keeps these levels and starts the clock (due_i = s_i)
    return NB_OK;
}

// ---- nb_set_encounter_watch: closest approaches seen inside block steps (kernels/encounter.hip.h) ----------
static int enc_clear_counters(nb_sim* s)
{
    const double inf = HUGE_VAL;
    unsigned long long w[nb::kEncWords] = {};
    std::memcpy(&w[nb::kEncFirst], &inf, sizeof inf);
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->enc_words, w, sizeof w, hipMemcpyHostToDevice));
    *s->enc_host = 0;
    s->enc_passes = 0;
    return NB_OK;
}

static int enc_clear_records(nb_sim* s)
{
    NB_HIP(s, hipStreamSynchronize(s->stream));
    std::vector<double> t(s->n, HUGE_VAL);
    NB_HIP(s, hipMemcpy(s->enc_time, t.data(), sizeof(double) * s->n, hipMemcpyHostToDevice));
    if (s->f64) NB_HIP(s, hipMemcpy(s->enc_rho2, t.data(), sizeof(double) * s->n, hipMemcpyHostToDevice));
    else {
        std::vector<float> r(s->n, HUGE_VALF);
        NB_HIP(s, hipMemcpy(s->enc_rho2, r.data(), sizeof(float) * s->n, hipMemcpyHostToDevice));
    }
    NB_HIP(s, hipMemset(s->enc_partner, 0xff, sizeof(uint32_t) * s->n));
    NB_HIP(s, hipMemset(s->enc_count, 0, sizeof(uint32_t) * s->n));
    NB_HIP(s, hipDeviceSynchronize());
    return NB_OK;
}

// the state checks the watch's calls other than the setter share
static int enc_on(nb_sim* s, const char* who)
{
    if (!s->hermite) return fail(s, NB_ERR_STATE, std::string(who) + ": needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) with the encounter watch switched on (nb_set_encounter_watch)");
    if (!s->enc) return fail(s, NB_ERR_STATE, std::string(who) + ": the encounter watch is not switched on (nb_set_encounter_watch)");
    NB_HIP(s, hipSetDevice(s->device));
    return NB_OK;
}

int nb_set_encounter_watch(nb_sim* s, const nb_encounter_watch* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_encounter_watch: null handle");
    if (!cfg) { if (s->enc) s->bb = false; s->enc = false; return NB_OK; }      // (its batched mode, nb_set_block_batch_watch, goes with it)
    if (cfg->flags & ~(uint32_t)NB_ENC_STOP) return fail(s, NB_ERR_INVALID, "nb_set_encounter_watch: unknown flags");
    if (!(cfg->radius >= 0.0) || std::isinf(cfg->radius)) return fail(s, NB_ERR_INVALID, "nb_set_encounter_watch: radius must be finite and >= 0");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4) with block steps switched on (nb_set_block_steps)");
    if (cfg->radii) {
        for (uint32_t i = 0; i < s->n; ++i) {
            const double h = s->f64 ? ((const double*)cfg->radii)[i] : (double)((const float*)cfg->radii)[i];
            if (!(h >= 0.0) || std::isinf(h)) return fail(s, NB_ERR_INVALID, "nb_set_encounter_watch: radii[" + std::to_string(i) + "] must be finite and >= 0");
        }
    }
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: the handle's order is 6 (nb_set_hermite_order): the watch exists at order 4 only");
    if (s->ac) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: the neighbour scheme is switched on (nb_set_neighbor_scheme): the watch runs in the gathered pass of block steps only");
    if (!s->blk) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: block steps are not switched on (nb_set_block_steps)");
    if (s->mx) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: the pass precision is NB_PASS_MIXED (nb_set_pass_precision, nb_set_pass_guard): the watch runs in the native pass only, set NB_PASS_NATIVE first");
    // (batched and watched: nb_set_block_batch_watch's mode, the one batched mode the watch has; the call re-configures radii and flags)
    if (s->bb && !s->enc) return fail(s, NB_ERR_STATE, "nb_set_encounter_watch: batched block steps are switched on (nb_set_block_batch): the watch runs on the base path of block steps only, switch them off first");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    if (!s->enc_w) NB_HIP(s, hipMalloc(&s->enc_w, s->esz * s->n));
    if (!s->enc_rho2) NB_HIP(s, hipMalloc(&s->enc_rho2, s->esz * s->n));
    if (!s->enc_partner) NB_HIP(s, hipMalloc((void**)&s->enc_partner, sizeof(uint32_t) * s->n));
    if (!s->enc_time) NB_HIP(s, hipMalloc((void**)&s->enc_time, sizeof(double) * s->n));
    if (!s->enc_count) NB_HIP(s, hipMalloc((void**)&s->enc_count, sizeof(uint32_t) * s->n));
    if (!s->enc_words) NB_HIP(s, hipMalloc((void**)&s->enc_words, sizeof(unsigned long long) * nb::kEncWords));
    if (!s->enc_host) NB_HIP(s, hipHostMalloc((void**)&s->enc_host, sizeof(unsigned long long), hipHostMallocDefault));
    if (!s->enc_pub) NB_HIP(s, hipHostGetDevicePointer((void**)&s->enc_pub, s->enc_host, 0));
    // w_i = h_i^2 + eps2 in fp64, rounded once to the handle's precision; h_i = 0: 0, below every rho^2
    auto w_of = [&](double h) { return h > 0.0 ? h * h + s->eps2 : 0.0; };
    if (s->f64) {
        std::vector<double> w(s->n);
        for (uint32_t i = 0; i < s->n; ++i) w[i] = w_of(cfg->radii ? ((const double*)cfg->radii)[i] : cfg->radius);
        NB_HIP(s, hipMemcpy(s->enc_w, w.data(), sizeof(double) * s->n, hipMemcpyHostToDevice));
    } else {
        std::vector<float> w(s->n);
        for (uint32_t i = 0; i < s->n; ++i) w[i] = (float)w_of(cfg->radii ? (double)((const float*)cfg->radii)[i] : cfg->radius);
        NB_HIP(s, hipMemcpy(s->enc_w, w.data(), sizeof(float) * s->n, hipMemcpyHostToDevice));
    }
    if (!s->enc) {      // switched on: the records and the counters start over (a call while it is on keeps them)
        if (int rc = enc_clear_records(s)) return rc;
        if (int rc = enc_clear_counters(s)) return rc;
        s->enc_stopped = s->enc_steps_left = 0;
    }
    s->enc = true;
    s->enc_flags = cfg->flags;
    return NB_OK;
}

int nb_encounter_stats(nb_sim* s, struct nb_encounter_stats* out, int reset)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_encounter_stats: null handle");
    if (!out) return fail(s, NB_ERR_INVALID, "nb_encounter_stats: out is NULL");
    if (int rc = enc_on(s, "nb_encounter_stats")) return rc;
    unsigned long long w[nb::kEncWords];
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(w, s->enc_words, sizeof w, hipMemcpyDeviceToHost));
    out->passes = s->enc_passes; out->hits = w[nb::kEncHits];
    std::memcpy(&out->first_time, &w[nb::kEncFirst], sizeof(double));
    out->stopped = s->enc_stopped; out->steps_left = s->enc_steps_left;
    if (reset) return enc_clear_counters(s);
    return NB_OK;
}

int nb_download_encounters(nb_sim* s, void* rho2, uint32_t* partner, double* time, uint32_t* count)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_download_encounters: null handle");
    if (int rc = enc_on(s, "nb_download_encounters")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    if (rho2) NB_HIP(s, hipMemcpy(rho2, s->enc_rho2, s->esz * s->n, hipMemcpyDeviceToHost));
    if (partner) NB_HIP(s, hipMemcpy(partner, s->enc_partner, sizeof(uint32_t) * s->n, hipMemcpyDeviceToHost));
    if (time) NB_HIP(s, hipMemcpy(time, s->enc_time, sizeof(double) * s->n, hipMemcpyDeviceToHost));
    if (count) NB_HIP(s, hipMemcpy(count, s->enc_count, sizeof(uint32_t) * s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_upload_encounters(nb_sim* s, const void* rho2, const uint32_t* partner, const double* time, const uint32_t* count)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_upload_encounters: null handle");
    if (!rho2 || !partner || !time || !count) return fail(s, NB_ERR_INVALID, "nb_upload_encounters: rho2, partner, time and count are required");
    if (int rc = enc_on(s, "nb_upload_encounters")) return rc;
    for (uint32_t i = 0; i < s->n; ++i)
        if (partner[i] != nb::kEncNone && (partner[i] >= s->n || partner[i] == i))
            return fail(s, NB_ERR_INVALID, "nb_upload_encounters: partner[" + std::to_string(i) + "] must be another body's index or 0xffffffff");
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->enc_rho2, rho2, s->esz * s->n, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->enc_partner, partner, sizeof(uint32_t) * s->n, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->enc_time, time, sizeof(double) * s->n, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->enc_count, count, sizeof(uint32_t) * s->n, hipMemcpyHostToDevice));
    return NB_OK;
}

int nb_reset_encounters(nb_sim* s)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_reset_encounters: null handle");
    if (int rc = enc_on(s, "nb_reset_encounters")) return rc;
    if (int rc = enc_clear_records(s)) return rc;
    s->enc_stopped = s->enc_steps_left = 0;
    return enc_clear_counters(s);
}

int nb_set_neighbor_scheme(nb_sim* s, const nb_neighbor_scheme* cfg)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_set_neighbor_scheme: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_set_neighbor_scheme: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!cfg) {
        if (s->ac) { NB_HIP(s, hipSetDevice(s->device)); NB_HIP(s, hipStreamSynchronize(s->stream)); s->derivs_ok = false; }      // acc / jerk held the scheme's totals
        ac_release(s);
        return NB_OK;
    }
    if (s->mx) return fail(s, NB_ERR_STATE, "nb_set_neighbor_scheme: the pass precision is NB_PASS_MIXED (nb_set_pass_precision): the neighbour scheme has no mixed kernels, set NB_PASS_NATIVE first");
    if (s->h6) return fail(s, NB_ERR_STATE, "nb_set_neighbor_scheme: the handle's order is 6 (nb_set_hermite_order): the neighbour scheme and the 6th-order scheme exclude each other");
    if (cfg->struct_size != sizeof(nb_neighbor_scheme)) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: struct_size must be sizeof(nb_neighbor_scheme)");
    const uint32_t nsub = cfg->substeps ? cfg->substeps : 8u, cap = cfg->cap ? cfg->cap : 128u;
    if (nsub > 1024 || (nsub & (nsub - 1))) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: substeps must be a power of two in 1 .. 1024 (0: the default 8)");
    if (cap > 4096) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: cap must be in 1 .. 4096 (0: the default 128)");
    if (cfg->flags != 0) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: flags must be 0");
    if (!cfg->radii && !(cfg->radius > 0.0)) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: radius must be > 0 when radii is NULL");
    if (cfg->radii) {
        for (uint32_t i = 0; i < s->n; ++i) {
            const double h = s->f64 ? ((const double*)cfg->radii)[i] : (double)((const float*)cfg->radii)[i];
            if (!(h >= 0.0) || std::isinf(h)) return fail(s, NB_ERR_INVALID, "nb_set_neighbor_scheme: radii[" + std::to_string(i) + "] must be finite and >= 0");
        }
    }
    if (s->blk) return fail(s, NB_ERR_STATE, "nb_set_neighbor_scheme: block steps are switched on (nb_set_block_steps): block steps and the neighbour scheme exclude each other");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    if (s->ac) s->derivs_ok = false;
    ac_release(s);
    const size_t rows = 4 * s->esz * s->n;
    hipError_t e = hipSuccess;
    for (void** p : {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->ac_px, &s->ac_pv})
        if (e == hipSuccess) e = hipMalloc(p, rows);
    if (e == hipSuccess) e = hipMalloc((void**)&s->ac_list, sizeof(uint32_t) * (size_t)s->n * cap);
    if (e == hipSuccess) e = hipMalloc((void**)&s->ac_count, sizeof(uint32_t) * s->n);
    if (e == hipSuccess) e = hipMalloc((void**)&s->ac_hdr, sizeof(unsigned long long) * nb::kAcHdrWords);
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->ac_hdr_host, sizeof(unsigned long long) * nb::kAcHdrWords, hipHostMallocDefault);
    if (e == hipSuccess && cfg->radii) {
        e = hipMalloc(&s->ac_radii, s->esz * s->n);
        if (e == hipSuccess) e = hipMemcpy(s->ac_radii, cfg->radii, s->esz * s->n, hipMemcpyHostToDevice);      // copied: the pointer is not kept
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ac_release(s);
        return fail(s, e == hipErrorOutOfMemory ? NB_ERR_NOMEM : NB_ERR_HIP, std::string("nb_set_neighbor_scheme: cannot allocate the scheme's arrays: ") + hipGetErrorString(e));
    }
    s->ac = true; s->ac_ok = false; s->ac_over = false;
    s->ac_nsub = nsub; s->ac_cap = cap; s->ac_radius = cfg->radius;
    return NB_OK;
}

int nb_neighbor_scheme_stats(nb_sim* s, struct nb_neighbor_scheme_stats* out, int reset)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_neighbor_scheme_stats: null handle");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_neighbor_scheme_stats: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    if (!out || out->struct_size != sizeof(struct nb_neighbor_scheme_stats)) return fail(s, NB_ERR_INVALID, "nb_neighbor_scheme_stats: set out->struct_size to sizeof(nb_neighbor_scheme_stats)");
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    if (!s->ac) return NB_OK;
    out->enabled = 1u;
    out->regular_steps = s->ac_regular; out->substeps = s->ac_substeps; out->entries = s->ac_entries; out->builds = s->ac_builds;
    out->max_count = s->ac_max_count; out->overflowed = s->ac_overflowed;
    if (reset) s->ac_regular = s->ac_substeps = s->ac_entries = s->ac_builds = 0;
    return NB_OK;
}

int nb_download_neighbor_scheme(nb_sim* s, void* accel_irr, void* jerk_irr, void* accel_reg, void* jerk_reg, uint32_t* list, uint32_t* count)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_download_neighbor_scheme: null handle");
    if (!s->ac) return fail(s, NB_ERR_STATE, "nb_download_neighbor_scheme: the neighbour scheme is not switched on (nb_set_neighbor_scheme)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_download_neighbor_scheme: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_scheme(s, "nb_download_neighbor_scheme")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const size_t rows = 4 * s->esz * s->n;
    if (accel_irr) NB_HIP(s, hipMemcpy(accel_irr, s->ac_ai, rows, hipMemcpyDeviceToHost));
    if (jerk_irr) NB_HIP(s, hipMemcpy(jerk_irr, s->ac_ji, rows, hipMemcpyDeviceToHost));
    if (accel_reg) NB_HIP(s, hipMemcpy(accel_reg, s->ac_ar, rows, hipMemcpyDeviceToHost));
    if (jerk_reg) NB_HIP(s, hipMemcpy(jerk_reg, s->ac_jr, rows, hipMemcpyDeviceToHost));
    if (list) NB_HIP(s, hipMemcpy(list, s->ac_list, sizeof(uint32_t) * (size_t)s->n * s->ac_cap, hipMemcpyDeviceToHost));
    if (count) NB_HIP(s, hipMemcpy(count, s->ac_count, sizeof(uint32_t) * s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

namespace {

// n elements of the handle's precision, every one `h` rounded once
void ad_fill(const nb_sim* s, double h, std::vector<char>* to)
{
    std::vector<char>& out = *to;
    out.resize(s->esz * (size_t)s->n);
    for (uint32_t i = 0; i < s->n; ++i) {
        if (s->f64) ((double*)out.data())[i] = h; else ((float*)out.data())[i] = (float)h;
    }
}

// what every call on the scheme's radii or checkpoint asks of the handle; nullptr: fine
const char* ad_bad_handle(const nb_sim* s)
{
    if (!s->hermite) return "needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)";
    return s->ac ? nullptr : "the neighbour scheme is not switched on (nb_set_neighbor_scheme)";
}

}  // namespace

int nb_set_neighbor_adapt(nb_sim* s, const nb_neighbor_adapt* cfg)
{
    const std::string F = "nb_set_neighbor_adapt: ";
    if (cfg) {      // the fields that need no handle first: the message names the field whatever else is wrong
        if (cfg->struct_size != sizeof(nb_neighbor_adapt)) return fail(s, NB_ERR_INVALID, F + "struct_size must be sizeof(nb_neighbor_adapt)");
        if (cfg->flags != 0) return fail(s, NB_ERR_INVALID, F + "flags must be 0");
        if (cfg->target == 0) return fail(s, NB_ERR_INVALID, F + "target must be >= 1");
        if (cfg->max_rebuilds > 16) return fail(s, NB_ERR_INVALID, F + "max_rebuilds is at most 16 (0: the default 4)");
        if (!(cfg->grow_max == 0.0 || cfg->grow_max >= 1.0) || std::isinf(cfg->grow_max)) return fail(s, NB_ERR_INVALID, F + "grow_max must be finite and >= 1 (0: the default cbrt(2))");
        if (!(cfg->radius_min >= 0.0) || std::isinf(cfg->radius_min)) return fail(s, NB_ERR_INVALID, F + "radius_min must be finite and >= 0 (0: none)");
        if (!(cfg->radius_max >= 0.0) || std::isinf(cfg->radius_max)) return fail(s, NB_ERR_INVALID, F + "radius_max must be finite and >= 0 (0: none)");
        if (cfg->radius_min > 0.0 && cfg->radius_max > 0.0 && cfg->radius_min > cfg->radius_max) return fail(s, NB_ERR_INVALID, F + "radius_min must not exceed radius_max");
    }
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    if (cfg && 2ull * cfg->target > s->ac_cap) return fail(s, NB_ERR_INVALID, F + "target must be at most cap / 2 of the scheme (cap " + std::to_string(s->ac_cap) + ")");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    ad_release(s);
    s->ac_ok = false;      // the start runs again, with or without adaptation
    if (!cfg) return NB_OK;
    const size_t bytes = s->esz * (size_t)s->n;
    hipError_t e = hipSuccess;
    for (void** p : {&s->ad_built, &s->ad_next, &s->ad_keep})
        if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess) {      // both from the scheme's radii, or from its radius; the scheme's own copy is never written
        if (s->ac_radii) {
            e = hipMemcpy(s->ad_built, s->ac_radii, bytes, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(s->ad_next, s->ac_radii, bytes, hipMemcpyDeviceToDevice);
        } else {
            std::vector<char> h;
            ad_fill(s, s->ac_radius, &h);
            e = hipMemcpy(s->ad_built, h.data(), bytes, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(s->ad_next, h.data(), bytes, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ad_release(s);
        return fail(s, e == hipErrorOutOfMemory ? NB_ERR_NOMEM : NB_ERR_HIP, F + "cannot allocate the radii: " + hipGetErrorString(e));
    }
    s->ad = true;
    s->ad_target = cfg->target;
    s->ad_max_rebuilds = cfg->max_rebuilds ? cfg->max_rebuilds : 4u;
    s->ad_gmax = cfg->grow_max > 0.0 ? cfg->grow_max : std::cbrt(2.0);
    s->ad_rmin = cfg->radius_min; s->ad_rmax = cfg->radius_max;
    return NB_OK;
}

int nb_neighbor_adapt_stats(nb_sim* s, struct nb_neighbor_adapt_stats* out, int reset)
{
    if (!s) return fail(nullptr, NB_ERR_INVALID, "nb_neighbor_adapt_stats: null handle");
    if (!out || out->struct_size != sizeof(struct nb_neighbor_adapt_stats)) return fail(s, NB_ERR_INVALID, "nb_neighbor_adapt_stats: set out->struct_size to sizeof(nb_neighbor_adapt_stats)");
    if (!s->hermite) return fail(s, NB_ERR_STATE, "nb_neighbor_adapt_stats: needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    if (!s->ad) return NB_OK;
    out->enabled = 1u;
    out->rebuilds = s->ad_rebuilds; out->rows_shrunk = s->ad_rows_shrunk; out->last_rebuilds = s->ad_last_rebuilds;
    if (reset) s->ad_rebuilds = s->ad_rows_shrunk = 0;
    return NB_OK;
}

int nb_download_neighbor_radii(nb_sim* s, void* built, void* next)
{
    const std::string F = "nb_download_neighbor_radii: ";
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    if (!s->uploaded) return fail(s, NB_ERR_STATE, F + "nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_scheme(s, "nb_download_neighbor_radii")) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const size_t bytes = s->esz * (size_t)s->n;
    if (s->ad || s->ac_radii) {
        if (built) NB_HIP(s, hipMemcpy(built, s->ad ? s->ad_built : s->ac_radii, bytes, hipMemcpyDeviceToHost));
        if (next) NB_HIP(s, hipMemcpy(next, s->ad ? s->ad_next : s->ac_radii, bytes, hipMemcpyDeviceToHost));
        return NB_OK;
    }
    std::vector<char> h;      // fixed radii: both arrays hold them
    ad_fill(s, s->ac_radius, &h);
    if (built) memcpy(built, h.data(), bytes);
    if (next) memcpy(next, h.data(), bytes);
    return NB_OK;
}

int nb_upload_neighbor_scheme(nb_sim* s, const nb_neighbor_checkpoint* ck)
{
    const std::string F = "nb_upload_neighbor_scheme: ";
    if (ck && ck->struct_size != sizeof(nb_neighbor_checkpoint)) return fail(s, NB_ERR_INVALID, F + "struct_size must be sizeof(nb_neighbor_checkpoint)");
    if (ck && ck->reserved != 0) return fail(s, NB_ERR_INVALID, F + "reserved must be 0");
    if (ck && !(ck->accel_irr && ck->jerk_irr && ck->accel_reg && ck->jerk_reg && ck->list && ck->count))
        return fail(s, NB_ERR_INVALID, F + "accel_irr, jerk_irr, accel_reg, jerk_reg, list and count are all required");
    if (!s || !ck) return fail(s, NB_ERR_INVALID, F + (!s ? "null handle" : "the checkpoint is NULL"));
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    if (!s->uploaded) return fail(s, NB_ERR_STATE, F + "nb_upload has not been called");
    if (!s->params_set) return fail(s, NB_ERR_STATE, F + "nb_set_params has not been called (G, dt)");
    if (s->ad && !ck->radii) return fail(s, NB_ERR_INVALID, F + "radii is required while adaptation is on (nb_set_neighbor_adapt)");
    if (!s->ad && ck->radii) return fail(s, NB_ERR_INVALID, F + "radii must be NULL while adaptation is off: the radii are the scheme's (nb_set_neighbor_scheme)");
    const uint32_t n = s->n, cap = s->ac_cap;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = ck->count[i];
        if (c > cap) return fail(s, NB_ERR_INVALID, F + "count[" + std::to_string(i) + "] = " + std::to_string(c) + " exceeds the scheme's cap " + std::to_string(cap));
        for (uint32_t e = 0; e < c; ++e) {
            const uint32_t j = ck->list[(size_t)i * cap + e];
            if (j >= n || j == i) return fail(s, NB_ERR_INVALID, F + "list[" + std::to_string(i) + "][" + std::to_string(e) + "] = " + std::to_string(j) + (j == i ? " is the row's own body" : " is not a body"));
        }
        if (ck->radii) {
            const double h = s->f64 ? ((const double*)ck->radii)[i] : (double)((const float*)ck->radii)[i];
            if (!(h >= 0.0) || std::isinf(h)) return fail(s, NB_ERR_INVALID, F + "radii[" + std::to_string(i) + "] must be finite and >= 0");
        }
    }
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    const size_t rows = 4 * s->esz * n;
    NB_HIP(s, hipMemcpy(s->ac_ai, ck->accel_irr, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->ac_ji, ck->jerk_irr, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->ac_ar, ck->accel_reg, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->ac_jr, ck->jerk_reg, rows, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->ac_list, ck->list, sizeof(uint32_t) * (size_t)n * cap, hipMemcpyHostToDevice));
    NB_HIP(s, hipMemcpy(s->ac_count, ck->count, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    if (ck->radii) {
        NB_HIP(s, hipMemcpy(s->ad_next, ck->radii, s->esz * n, hipMemcpyHostToDevice));
        NB_HIP(s, hipMemcpy(s->ad_built, ck->radii, s->esz * n, hipMemcpyHostToDevice));
    }
    uint32_t nn = n;
    void* args[] = {&s->ac_ai, &s->ac_ji, &s->ac_ar, &s->ac_jr, &s->acc, &s->jerk, &nn};
    const void* fn = s->f64 ? (const void*)&nb::nb_ac_restore<double> : (const void*)&nb::nb_ac_restore<float>;
    NB_HIP(s, hipLaunchKernel(fn, dim3(ceil_div(n, nb::kBlock)), dim3(nb::kBlock), args, 0, s->stream));
    s->ac_ok = true;      // current for the G and dt in force; it counts no build
    s->derivs_ok = true; s->derivs_any_G = false; s->derivs_G = s->G;
    s->lv_state = 0;      // the levels follow (nb_upload_neighbor_levels), or start by their rule on these components
    return NB_OK;
}

int nb_set_neighbor_levels(nb_sim* s, const nb_neighbor_levels* cfg)
{
    const std::string F = "nb_set_neighbor_levels: ";
    if (cfg) {      // the fields that need no handle first
        if (cfg->struct_size != sizeof(nb_neighbor_levels)) return fail(s, NB_ERR_INVALID, F + "struct_size must be sizeof(nb_neighbor_levels)");
        if (cfg->flags & ~NB_NLEV_FROZEN) return fail(s, NB_ERR_INVALID, F + "flags has unknown bits (NB_NLEV_FROZEN is the only one)");
        if (cfg->reserved != 0) return fail(s, NB_ERR_INVALID, F + "reserved must be 0");
        if (!(cfg->eta >= 0.0) || std::isinf(cfg->eta)) return fail(s, NB_ERR_INVALID, F + "eta must be finite and >= 0 (0: the default 0.02)");
    }
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    uint32_t L = 0;
    while ((1u << L) < s->ac_nsub) ++L;
    if (cfg && cfg->min_level > L) return fail(s, NB_ERR_INVALID, F + "min_level must not exceed log2(substeps) of the scheme (" + std::to_string(L) + ")");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    lv_release(s);
    if (!cfg) return NB_OK;
    hipError_t e = hipMalloc((void**)&s->lv_lev, s->n);
    if (e == hipSuccess) e = hipMalloc((void**)&s->lv_due, sizeof(uint32_t) * s->n);
    if (e == hipSuccess) e = hipMalloc((void**)&s->lv_words, sizeof(uint32_t) * nb::lv_words(s->ac_nsub));
    if (e == hipSuccess) e = hipMalloc((void**)&s->lv_cnt, sizeof(unsigned long long) * nb::kLvCntWords);
    if (e == hipSuccess) e = hipMemset(s->lv_cnt, 0, sizeof(unsigned long long) * nb::kLvCntWords);
    if (e == hipSuccess) e = hipMalloc((void**)&s->lv_rec, sizeof(unsigned long long) * nb::kLvRecWords * (size_t)s->n);
    if (e == hipSuccess) e = hipMemset(s->lv_rec, 0, sizeof(unsigned long long) * nb::kLvRecWords * (size_t)s->n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lv_release(s);
        return fail(s, e == hipErrorOutOfMemory ? NB_ERR_NOMEM : NB_ERR_HIP, F + "cannot allocate the levels: " + hipGetErrorString(e));
    }
    s->lv = true;
    s->lv_lmin = cfg->min_level; s->lv_frozen = (cfg->flags & NB_NLEV_FROZEN) != 0;
    s->lv_eta = cfg->eta > 0.0 ? cfg->eta : 0.02;
    s->lv_state = 0;
    return NB_OK;
}

int nb_neighbor_level_stats(nb_sim* s, struct nb_neighbor_level_stats* out, int reset)
{
    const std::string F = "nb_neighbor_level_stats: ";
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (!out || out->struct_size != sizeof(struct nb_neighbor_level_stats)) return fail(s, NB_ERR_INVALID, F + "set out->struct_size to sizeof(nb_neighbor_level_stats)");
    if (!s->hermite) return fail(s, NB_ERR_STATE, F + "needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    if (!s->lv) return NB_OK;
    out->enabled = 1u;
    NB_HIP(s, hipSetDevice(s->device));
    unsigned long long w[nb::kLvCntWords];
    std::vector<unsigned long long> rec((size_t)nb::kLvRecWords * s->n);      // the per-body records, summed here
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(w, s->lv_cnt, sizeof w, hipMemcpyDeviceToHost));
    NB_HIP(s, hipMemcpy(rec.data(), s->lv_rec, sizeof(unsigned long long) * rec.size(), hipMemcpyDeviceToHost));
    out->regular_steps = s->lv_regular; out->ticks = s->lv_ticks;
    out->block_steps = w[nb::kLvBlockSteps];
    for (uint32_t i = 0; i < s->n; ++i) {
        const unsigned long long* r = rec.data() + (size_t)nb::kLvRecWords * i;
        out->body_steps += r[nb::kLvBodySteps]; out->entries += r[nb::kLvEntries]; out->clamped += r[nb::kLvClamped];
        if (r[nb::kLvFinest] > out->finest_level) out->finest_level = (uint32_t)r[nb::kLvFinest];
    }
    if (reset) {
        s->lv_regular = s->lv_ticks = 0;
        NB_HIP(s, hipMemsetAsync(s->lv_cnt, 0, sizeof w, s->stream));
        NB_HIP(s, hipMemsetAsync(s->lv_rec, 0, sizeof(unsigned long long) * rec.size(), s->stream));
    }
    return NB_OK;
}

int nb_download_neighbor_levels(nb_sim* s, uint8_t* levels)
{
    const std::string F = "nb_download_neighbor_levels: ";
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (!levels) return fail(s, NB_ERR_INVALID, F + "levels is NULL");
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    if (!s->lv) return fail(s, NB_ERR_STATE, F + "the levels are not switched on (nb_set_neighbor_levels)");
    if (!s->uploaded) return fail(s, NB_ERR_STATE, F + "nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_scheme(s, "nb_download_neighbor_levels")) return rc;
    if (int rc = ensure_levels(s)) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(levels, s->lv_lev, s->n, hipMemcpyDeviceToHost));
    return NB_OK;
}

int nb_upload_neighbor_levels(nb_sim* s, const uint8_t* levels)
{
    const std::string F = "nb_upload_neighbor_levels: ";
    if (!s) return fail(nullptr, NB_ERR_INVALID, F + "null handle");
    if (!levels) return fail(s, NB_ERR_INVALID, F + "levels is NULL");
    if (const char* bad = ad_bad_handle(s)) return fail(s, NB_ERR_STATE, F + bad);
    if (!s->lv) return fail(s, NB_ERR_STATE, F + "the levels are not switched on (nb_set_neighbor_levels)");
    if (!(s->uploaded && s->params_set && s->ac_ok && s->derivs_ok && s->derivs_G == s->G))
        return fail(s, NB_ERR_STATE, F + "the scheme is not current: call it after nb_upload_neighbor_scheme (or after a call that ran the scheme's start)");
    const nb::LvCfg c = lv_cfg(s);
    for (uint32_t i = 0; i < s->n; ++i)
        if (levels[i] < c.lmin || levels[i] > c.L)
            return fail(s, NB_ERR_INVALID, F + "levels[" + std::to_string(i) + "] = " + std::to_string(levels[i]) + " is outside [min_level, log2(substeps)]");
    NB_HIP(s, hipSetDevice(s->device));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    NB_HIP(s, hipMemcpy(s->lv_lev, levels, s->n, hipMemcpyHostToDevice));
    s->lv_state = 1;      // current: the start rule does not run (the next step counts them into finest_level)
    return NB_OK;
}

int nb_set_exchange(nb_sim* s, nb_exchange_fn fn, void* user)
{
    if (!s) return NB_ERR_INVALID;
    if (s->hermite) return fail(s, NB_ERR_STATE, "nb_set_exchange: a Hermite handle is a whole system on one device: nothing to exchange");
    if (fn && s->fused) return fail(s, NB_ERR_STATE, "nb_set_exchange: a fused whole-system handle has nothing to exchange");
    if (fn && s->rccl) return fail(s, NB_ERR_STATE, "nb_set_exchange: a native RCCL communicator is attached (nb_rccl_detach first)");
    if (int rc = finish_gather(s)) return rc;
    s->xfn = fn; s->xwait = nullptr; s->xuser = user;
    return NB_OK;
}

int nb_set_exchange_overlapped(nb_sim* s, nb_exchange_fn begin, nb_exchange_wait_fn wait, void* user)
{
    if (!s) return NB_ERR_INVALID;
    if (!begin || !wait) return fail(s, NB_ERR_INVALID, "nb_set_exchange_overlapped: both hooks are required");
    if (s->hermite) return fail(s, NB_ERR_STATE, "nb_set_exchange_overlapped: a Hermite handle is a whole system on one device: nothing to exchange");
    if (s->fused) return fail(s, NB_ERR_STATE, "nb_set_exchange_overlapped: a fused whole-system handle has nothing to exchange");
    if (s->rccl) return fail(s, NB_ERR_STATE, "nb_set_exchange_overlapped: a native RCCL communicator is attached");
    if (int rc = finish_gather(s)) return rc;
    s->xfn = begin; s->xwait = wait; s->xuser = user;
    return NB_OK;
}

int nb_enable_timing(nb_sim* s, int on)
{
    if (!s) return NB_ERR_INVALID;
    s->timing = on != 0;
    return NB_OK;
}

// Averages of the recorded steps since the last call; clears the record.
static int collect_times(nb_sim* s, nb_step_timing* t)
{
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    NB_HIP(s, hipStreamSynchronize(s->stream));
    double f = 0, red = 0, rs = 0, g = 0, x = 0, span = 0;
    uint32_t nx = 0, nrs = 0;
    for (auto& ev : s->pending) {
        float a = 0, b = 0, c = 0, d = 0, r1 = 0, r2 = 0, sp = 0;
        if (ev.blk) {       // one outer step of a block-step handle: its whole span is force time (as a fused step's)
            NB_HIP(s, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
            f += a; span += a;
            continue;
        }
        if (s->hermite) {
            // e6 predict e0 force+jerk kernel, reduce e1 correct e2
            float pr = 0, co = 0;
            NB_HIP(s, hipEventElapsedTime(&pr, ev.e[6], ev.e[0]));
            NB_HIP(s, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
            NB_HIP(s, hipEventElapsedTime(&co, ev.e[1], ev.e[2]));
            NB_HIP(s, hipEventElapsedTime(&sp, ev.e[6], ev.e[2]));
            f += a; g += pr + co; span += sp;
            continue;
        }
        if (ev.rs) {
            // rank form: e0 force e7 nb_sym_reduce e1 reduce-scatter e6 integrate e2 [all-gather e5]; with the force pass split at the
            // gather: e0 own-row sweeps e7 [wait for the other ranks' rows] e3 the rest e4 nb_sym_reduce e1 ...
            NB_HIP(s, hipEventElapsedTime(&a, ev.e[0], ev.e[7]));
            NB_HIP(s, hipEventElapsedTime(&r1, ev.two ? ev.e[4] : ev.e[7], ev.e[1]));
            NB_HIP(s, hipEventElapsedTime(&r2, ev.e[1], ev.e[6]));
            ++nrs;
        } else {
            NB_HIP(s, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
        }
        if (ev.two) NB_HIP(s, hipEventElapsedTime(&c, ev.e[3], ev.e[4]));   // own-row work, [gather wait], the rest
        if (!s->fused) NB_HIP(s, hipEventElapsedTime(&b, ev.e[6], ev.e[2]));
        if (ev.xchg) { NB_HIP(s, hipEventElapsedTime(&d, ev.e[2], ev.e[5])); ++nx; }
        NB_HIP(s, hipEventElapsedTime(&sp, ev.e[0], ev.xchg ? ev.e[5] : s->fused ? ev.e[1] : ev.e[2]));
        f += a + c; red += r1; rs += r2; g += b; x += d; span += sp;
    }
    const uint32_t cnt = (uint32_t)s->pending.size();
    t->launches = cnt;
    t->force_ms = cnt ? f / cnt : 0.0;
    t->sym_reduce_ms = nrs ? red / nrs : 0.0;
    t->reduce_scatter_ms = nrs ? rs / nrs : 0.0;
    t->integrate_ms = cnt ? g / cnt : 0.0;
    t->allgather_ms = nx ? x / nx : 0.0;
    t->span_ms = cnt ? span / cnt : 0.0;
    t->reduce_scatters = nrs;
    t->allgathers = nx;
    s->pending.clear();
    s->pool_next = 0;
    return NB_OK;
}

int nb_step_times2(nb_sim* s, nb_step_timing* out)
{
    if (!s) return NB_ERR_INVALID;
    if (!out || out->struct_size < sizeof(nb_step_timing)) return fail(s, NB_ERR_INVALID, "nb_step_times2: set out->struct_size to sizeof(nb_step_timing)");
    nb_step_timing t;
    memset(&t, 0, sizeof t);
    if (int rc = collect_times(s, &t)) return rc;
    t.struct_size = out->struct_size;
    memcpy(out, &t, sizeof t);
    return NB_OK;
}

int nb_step_times(nb_sim* s, double* force_ms, double* integrate_ms, double* exchange_ms, uint32_t* launches)
{
    if (!s) return NB_ERR_INVALID;
    nb_step_timing t;
    memset(&t, 0, sizeof t);
    if (int rc = collect_times(s, &t)) return rc;
    if (force_ms) *force_ms = t.force_ms + t.sym_reduce_ms;        // the rank form's nb_sym_reduce counts as force work here
    if (integrate_ms) *integrate_ms = t.integrate_ms;
    if (exchange_ms) *exchange_ms = t.reduce_scatter_ms + t.allgather_ms;   // every native collective of a step
    if (launches) *launches = t.launches;
    return NB_OK;
}

int nb_kernel_times(nb_sim* s, double* force_ms, double* integrate_ms, uint32_t* launches)
{
    return nb_step_times(s, force_ms, integrate_ms, nullptr, launches);
}

int nb_integrate_pass(nb_sim* s, uint32_t reps, double* avg_ms)
{
    if (!s || !avg_ms) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_integrate_pass: nothing uploaded yet");
    if (s->hermite) return fail(s, NB_ERR_STATE, "nb_integrate_pass: a Hermite handle has no integrate kernel to run on its own (predictor and corrector belong to a step)");
    if (s->fused) return fail(s, NB_ERR_STATE, "nb_integrate_pass: a fused handle has no integrate kernel (create it with NB_FLAG_NO_FUSE)");
    if (reps == 0) return fail(s, NB_ERR_INVALID, "nb_integrate_pass: reps must be >= 1");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    const double dt = s->dt > 0 ? s->dt : 1e-3;
    const double keep = s->dt;
    s->dt = dt;
    if (s->steps_done == 0) {
        NB_HIP(s, hipMemsetAsync(s->partial, 0, s->sym ? (size_t)3 * s->esz * sym_layer_rows(s) * s->sym_layers : 4 * s->esz * s->sc * s->jsplit, s->stream));
        if (s->sym_rank) NB_HIP(s, hipMemsetAsync(s->sym_A, 0, 4 * s->esz * s->sym_np, s->stream));      // what a rank-form handle integrates from
    }
    hipEvent_t e0, e1;
    NB_HIP(s, hipEventCreate(&e0));
    NB_HIP(s, hipEventCreate(&e1));
    if (s->f64) launch_integrate<double>(s); else launch_integrate<float>(s);     // warm-up launch
    NB_HIP(s, hipEventRecord(e0, s->stream));
    for (uint32_t k = 0; k < reps; ++k) { if (s->f64) launch_integrate<double>(s); else launch_integrate<float>(s); }
    NB_HIP(s, hipEventRecord(e1, s->stream));
    NB_HIP(s, hipEventSynchronize(e1));
    float ms = 0;
    NB_HIP(s, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    NB_HIP(s, hipGetLastError());
    s->dt = keep;
    drop_graph(s);          // buffer roles may have changed parity
    *avg_ms = ms / reps;
    return NB_OK;
}

int nb_force_pass(nb_sim* s, uint32_t reps, double* avg_ms)
{
    if (!s || !avg_ms) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_force_pass: nothing uploaded yet");
    if (s->fused) return fail(s, NB_ERR_STATE, "nb_force_pass: a fused handle has no separate force kernel (create it with NB_FLAG_NO_FUSE)");
    if (reps == 0) return fail(s, NB_ERR_INVALID, "nb_force_pass: reps must be >= 1");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    if (int rc = ensure_gm(s)) return rc;
    if (int rc = ensure_eqm(s)) return rc;
    if (s->hermite && !s->params_set) return fail(s, NB_ERR_STATE, "nb_force_pass: nb_set_params has not been called (G)");
    if (s->h6) { if (int rc = ensure_start(s, "nb_force_pass")) return rc; }      // the pass streams the accelerations: they are made current, the state is untouched
    if (s->hermite && s->mx) launch_split(s);      // a mixed handle's pass reads its three streams: made from the stored state, once
    auto once = [&]() -> int {
        if (s->hermite) { hermite_arrays h(s); launch_pass(s, order_of(s), s->mx ? h.in : h.state, h.pred); return NB_OK; }      // the order's pass into the step's scratch: state and derivatives untouched
        if (s->sym_rank) return s->f64 ? nbi::sym_rank_phase_a_t<double>(s, nullptr, false) : nbi::sym_rank_phase_a_t<float>(s, nullptr, false);
        if (s->f64) launch_force<double>(s); else launch_force<float>(s);
        return NB_OK;
    };
    hipEvent_t e0, e1;
    NB_HIP(s, hipEventCreate(&e0));
    NB_HIP(s, hipEventCreate(&e1));
    if (int rc = once()) return rc;               // warm-up
    NB_HIP(s, hipEventRecord(e0, s->stream));
    for (uint32_t k = 0; k < reps; ++k) { if (int rc = once()) return rc; }
    NB_HIP(s, hipEventRecord(e1, s->stream));
    NB_HIP(s, hipEventSynchronize(e1));
    float ms = 0;
    NB_HIP(s, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    NB_HIP(s, hipGetLastError());
    if (s->force_err != hipSuccess) { const hipError_t queue_reset = s->force_err; s->force_err = hipSuccess; NB_HIP(s, queue_reset); }
    *avg_ms = ms / reps;
    return NB_OK;
}

const char* nb_variant_name(nb_sim* s) { return s ? s->variant.c_str() : ""; }

int nb_shape_info(nb_sim* s, uint32_t* jsplit, uint32_t* j_per_split, uint32_t* own_split0, uint32_t* own_splits)
{
    if (!s) return NB_ERR_INVALID;
    if (jsplit) *jsplit = s->jsplit;
    if (j_per_split) *j_per_split = s->j_per_split;
    if (own_split0) *own_split0 = s->own_split0;
    if (own_splits) *own_splits = s->own_splits;
    return NB_OK;
}

int nb_eqm_info(nb_sim* s, int* eqm)
{
    if (!s || !eqm) return NB_ERR_INVALID;
    *eqm = 0;
    if (!s->eqm_capable || !s->uploaded) return NB_OK;
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_eqm(s)) return rc;
    *eqm = eqm_active(s) ? 1 : 0;
    return NB_OK;
}

int nb_eqm_form(nb_sim* s, int* form)
{
    if (!s || !form) return NB_ERR_INVALID;
    *form = 0;
    if (!s->eqm_capable || !s->uploaded) return NB_OK;
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = ensure_eqm(s)) return rc;
    *form = eqm_form(s);
    return NB_OK;
}

int nb_plan_query(const nb_config* cfg_in, int n_cu, double clock_hz, nb_plan_info* out, uint32_t* tab, uint32_t tab_cap)
{
    if (!cfg_in || !out) return fail(nullptr, NB_ERR_INVALID, "nb_plan_query: null argument");
    if (out->struct_size < sizeof(nb_plan_info)) return fail(nullptr, NB_ERR_INVALID, "nb_plan_query: set out->struct_size to sizeof(nb_plan_info)");
    nb_config cfg;
    uint32_t sb, sc;
    double eps2;
    if (const int rc = read_config(cfg_in, "nb_plan_query", &cfg, &sb, &sc, &eps2)) return rc;
    if (cfg.integrator != NB_INT_LEAPFROG) return fail(nullptr, NB_ERR_INVALID, "nb_plan_query: integrator must be NB_INT_LEAPFROG (a Hermite handle has no launch plan: nb_shape_info reports its j-chunks)");
    int count = 0;
    double device_mem = 0.0;                      // 0: the planner's default (an MI355X's 288 GB)
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    if (n_cu <= 0 || !(clock_hz > 0)) {           // "as on the current device"
        if (count <= 0) return fail(nullptr, NB_ERR_NO_DEVICE, "nb_plan_query: n_cu / clock_hz not given and there is no HIP device to read them from");
        int dev = cfg.device;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
        hipDeviceProp_t prop;
        if (dev >= count || hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
            return fail(nullptr, NB_ERR_HIP, "nb_plan_query: cannot read the device properties");
        if (n_cu <= 0) n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (!(clock_hz > 0)) clock_hz = prop.clockRate > 0 ? 1e3 * prop.clockRate : 2.4e9;
        device_mem = (double)prop.totalGlobalMem;
    }
    nb_sim tmp;                                    // host fields only: nothing of it is ever allocated on a device
    tmp.n = cfg.n; tmp.sb = sb; tmp.sc = sc; tmp.f64 = cfg.precision == NB_F64; tmp.esz = tmp.f64 ? 8 : 4; tmp.eps2 = eps2;
    tmp.no_device = count <= 0;
    plan_handle(&tmp, cfg, n_cu, clock_hz, device_mem);
    const Shape sh = shape_of(&tmp);
    if (!kernel_of(tmp.f64, sh)) return fail(nullptr, NB_ERR_INVALID, "nb_plan_query: no kernel for shape " + tmp.variant);
    const uint32_t size = out->struct_size, want_pass = out->sym_pass;
    memset(out, 0, sizeof *out);
    out->struct_size = size;
    out->kind = (uint32_t)sh.kind; out->ipl = (uint32_t)sh.ipl; out->ls = (uint32_t)sh.ls; out->x = (uint32_t)sh.x;
    out->jsplit = tmp.jsplit; out->j_per_split = tmp.j_per_split; out->own_split0 = tmp.own_split0; out->own_splits = tmp.own_splits;
    out->sym = tmp.sym; out->symw = tmp.symw; out->sym_rank = tmp.sym_rank;
    out->sym_np = tmp.sym_np; out->sym_layers = tmp.sym_layers; out->sym_g0 = tmp.sym_g0; out->sym_g1 = tmp.sym_g1;
    static_assert(sizeof(out->sym_plan) == 11 * sizeof(uint32_t) && sizeof(tmp.sym_plan) >= 12 * sizeof(uint32_t), "nb_plan_info::sym_plan holds the first eleven words of nb_sim::sym_plan; the twelfth (ups) is sym_ups");
    memcpy(out->sym_plan, tmp.sym_plan, sizeof out->sym_plan);
    out->sym_ups = tmp.symw ? tmp.sym_plan[11] : 0;
    out->sym_spill_rows = tmp.sym_spill_rows;
    static_assert(sizeof(out->sym_rank_plan) == sizeof(tmp.sym_rank_plan), "nb_plan_info::sym_rank_plan mirrors nb_sim::sym_rank_plan");
    memcpy(out->sym_rank_plan, tmp.sym_rank_plan, sizeof out->sym_rank_plan);
    out->sym_passes = (uint32_t)tmp.sym_passes.size();
    out->sym_local = tmp.sym_local;
    size_t tab_from = 0, tab_to = tmp.sym_tab_host.size();
    if (!tmp.sym_passes.empty()) {
        if (want_pass >= tmp.sym_passes.size()) return fail(nullptr, NB_ERR_INVALID, "nb_plan_query: sym_pass out of range");
        const auto& ps = tmp.sym_passes[want_pass];
        out->sym_pass = want_pass;
        memcpy(out->sym_rank_plan, ps.plan, sizeof out->sym_rank_plan);
        out->sym_pass_k_lo = ps.k_lo; out->sym_pass_k_hi = ps.k_hi; out->sym_pass_d0 = ps.d0;
        tab_from = ps.tab_off;
        tab_to = want_pass + 1 < tmp.sym_passes.size() ? tmp.sym_passes[want_pass + 1].tab_off : tmp.sym_tab_host.size();
    }
    out->tab_len = (uint32_t)(tab_to - tab_from);
    snprintf(out->variant, sizeof out->variant, "%s", tmp.variant.c_str());
    if (tab) memcpy(tab, tmp.sym_tab_host.data() + tab_from, sizeof(uint32_t) * (out->tab_len < tab_cap ? out->tab_len : tab_cap));
    return NB_OK;
}

int nb_diagnostics(nb_sim* s, double out[5])
{
    if (!s || !out) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_diagnostics: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;
    dim3 grid(ceil_div(s->sc, nb::kDiagRows), ceil_div(s->n, s->diag_chunk)), block(nb::kBlock);
    if (s->f64)
        hipLaunchKernelGGL((nb::nb_diag<double>), grid, block, 0, s->stream, (const double4*)s->bodies[s->cur],
                           (const double4*)s->vel, s->n, s->sb, s->sc, s->diag_chunk, s->G, s->eps2, s->diag);
    else
        hipLaunchKernelGGL((nb::nb_diag<float>), grid, block, 0, s->stream, (const float4*)s->bodies[s->cur],
                           (const float4*)s->vel, s->n, s->sb, s->sc, s->diag_chunk, s->G, (float)s->eps2, s->diag);
    NB_HIP(s, hipGetLastError());
    std::vector<double> h((size_t)5 * s->diag_blocks);
    NB_HIP(s, hipMemcpyAsync(h.data(), s->diag, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s->stream));
    NB_HIP(s, hipStreamSynchronize(s->stream));
    for (int q = 0; q < 5; ++q) out[q] = 0.0;
    for (uint32_t b = 0; b < s->diag_blocks; ++b)
        for (int q = 0; q < 5; ++q) out[q] += h[(size_t)b * 5 + q];
    return NB_OK;
}

/* ---- field queries ------------------------------------------------------------------------ */

extern "C++" {      // (templates below)
namespace {

// Makes an engine-owned buffer hold at least `bytes` (a grown buffer is a new allocation: whatever the stream still runs on the
// old one is waited for first).
int field_reserve(nb_sim* s, nb_sim::field_buf& b, size_t bytes, const char* who)
{
    if (bytes <= b.cap) return NB_OK;
    if (b.p) { NB_HIP(s, hipStreamSynchronize(s->stream)); (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(s, NB_ERR_NOMEM, std::string(who) + ": cannot allocate " + std::to_string(bytes) + " bytes of device memory");
    }
    b.cap = bytes;
    return NB_OK;
}

constexpr uint32_t kFieldPartRows = 1u << 20;    // most (point, j-chunk) rows of partial sums in flight (or two launches' worth of workgroups, if that is more)
constexpr uint32_t kFieldWavesPerSimd = 8;       // waves per SIMD a launch is cut into, at least (when m x n gives that many): twice the four that are
                                                 // resident.  M = N = 262,144, both outputs, against nb_force_pass: 2 -> 1.285, 4 -> 1.21, 8 -> 1.18, 16 -> 1.165
constexpr uint32_t kFieldMinChunk = 2048;         // bodies of a j-chunk below which only the two-waves-per-SIMD floor cuts (m = 1,024 against N = 1,048,576:
                                                 // 0.33 ms with 512 chunks of 2,048 bodies, 0.42 ms with 2,048 chunks of 512)
constexpr uint32_t kFieldMaxChunk = 1u << 20;    // most bodies of one j-chunk (bounds the second-level sums of nb_field_pk)

// Workgroups a launch should have at least, however few the points are.
uint32_t field_blocks_wanted(const nb_sim* s)
{
    uint32_t per_simd = kFieldWavesPerSimd;
#ifdef NB_TUNING    // calibration build only: the launch-shape constant from the environment (tools/field_bench.py --only-big)
    if (const char* e = getenv("NB_FIELD_WAVES")) per_simd = (uint32_t)std::max(1, atoi(e));
#endif
    return per_simd * (uint32_t)s->n_cu;       // workgroups of 4 waves, one wave on each SIMD of a CU
}

// j-chunks for a batch of `pblocks` point blocks: that many workgroups -- but chunks shorter than kFieldMinChunk bodies only as far
// as a quarter of them needs it (two waves per SIMD is the floor a launch reaches whenever m x n gives it; past that, a short
// chunk pays more in its prologue and in nb_field_reduce than the finer cut returns) -- in whole 256-body tiles.
void field_shape(const nb_sim* s, uint32_t pblocks, uint32_t* chunks, uint32_t* j_per_chunk)
{
    const uint32_t want = field_blocks_wanted(s);
    const uint32_t c_hi = ceil_div(want, pblocks), c_lo = ceil_div(ceil_div(want, 4u), pblocks);
    uint32_t c = std::min(c_hi, std::max(c_lo, s->n / kFieldMinChunk));
    c = std::max(c, ceil_div(s->n, kFieldMaxChunk));
    c = std::max(1u, std::min(c, ceil_div(s->n, (uint32_t)nb::kTile)));
    const uint32_t per = ceil_div(ceil_div(s->n, c), (uint32_t)nb::kTile) * nb::kTile;
    *j_per_chunk = per;
    *chunks = ceil_div(s->n, per);
}

// ---- what the six queries share: one prologue, one staging path, one batch rule ----

// The six request structs open with the same fields (struct_size, m, flags, first_body, points) and the four flag families
// use the same bits.
constexpr uint32_t kQueryAtBodies = 1u, kQueryDevice = 4u;
static_assert(NB_FIELD_AT_BODIES == kQueryAtBodies && NB_NBR_AT_BODIES == kQueryAtBodies && NB_LISTF_AT_BODIES == kQueryAtBodies && NB_SPLIT_AT_BODIES == kQueryAtBodies, "one *_AT_BODIES bit");
static_assert(NB_FIELD_DEVICE == kQueryDevice && NB_NBR_DEVICE == kQueryDevice && NB_LISTF_DEVICE == kQueryDevice && NB_SPLIT_DEVICE == kQueryDevice, "one *_DEVICE bit");

// What the prologue has to know of a query: the names its messages carry, the flag bits it takes, whether its sums need G.
struct query_kind { const char* request; const char* at_bodies; uint32_t flags; bool needs_G; };
constexpr query_kind kQField = {"nb_field_request", "NB_FIELD_AT_BODIES", NB_FIELD_AT_BODIES | NB_FIELD_F64 | NB_FIELD_DEVICE, true};
constexpr query_kind kQNbr = {"nb_neighbor_request", "NB_NBR_AT_BODIES", NB_NBR_AT_BODIES | NB_NBR_DEVICE, false};
constexpr query_kind kQNbl = {"nb_neighbor_list_request", "NB_NBR_AT_BODIES", NB_NBR_AT_BODIES | NB_NBR_DEVICE, false};
constexpr query_kind kQKnn = {"nb_knn_request", "NB_NBR_AT_BODIES", NB_NBR_AT_BODIES | NB_NBR_DEVICE, false};
constexpr query_kind kQListF = {"nb_list_force_request", "NB_LISTF_AT_BODIES", NB_LISTF_AT_BODIES | NB_LISTF_DEVICE, true};
constexpr query_kind kQSplit = {"nb_split_force_request", "NB_SPLIT_AT_BODIES", NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE, true};

// (the text is only put together when a call fails: the Ahmad-Cohen scheme goes through these functions in every regular step)
int qfail(nb_sim* s, int code, const char* who, const std::string& what) { return fail(s, code, std::string(who) + ": " + what); }

// The prologue of every query against the first `rows` rows of the handle: the request's head, then `specific` (the checks of the
// fields only this query has: the text of the first one missed, or null), then the handle's state; every NB_ERR_INVALID comes
// before every NB_ERR_STATE.  `who` names the public function in the messages.
template <class R, class F>
int query_begin(nb_sim* s, const R* req, const query_kind& k, uint32_t rows, const char* who, F&& specific)
{
    if (!s) return qfail(nullptr, NB_ERR_INVALID, who, "null handle");
    if (!req) return qfail(s, NB_ERR_INVALID, who, "null request");
    if (req->struct_size != sizeof(R)) return qfail(s, NB_ERR_INVALID, who, std::string("struct_size must be sizeof(") + k.request + ")");
    if (req->flags & ~k.flags) return qfail(s, NB_ERR_INVALID, who, "unknown bits in flags");
    const bool at = (req->flags & kQueryAtBodies) != 0;
    if (at && req->points) return qfail(s, NB_ERR_INVALID, who, std::string("points must be NULL with ") + k.at_bodies);
    if (!at && !req->points) return qfail(s, NB_ERR_INVALID, who, std::string("points is NULL (and ") + k.at_bodies + " is not set)");
    if (req->m == 0) return qfail(s, NB_ERR_INVALID, who, "m must be >= 1");
    if (const char* bad = specific()) return qfail(s, NB_ERR_INVALID, who, bad);
    if (at && (uint64_t)req->first_body + req->m > rows) return qfail(s, NB_ERR_INVALID, who, "first_body + m exceeds n");
    if (!s->uploaded) return qfail(s, NB_ERR_STATE, who, "nothing uploaded yet");
    if (k.needs_G && !s->params_set) return qfail(s, NB_ERR_STATE, who, "nb_set_params has not been called (G)");
    NB_HIP(s, hipSetDevice(s->device));
    return finish_gather(s);     // other ranks' rows must have landed
}

// One array of a request: where the caller has it (null: not asked for), its bytes per point, its direction, the engine buffer
// that stages it for a host-pointer request (null: it is on the device whatever the request says -- the handle's own rows) and
// whether it is staged whole, ahead of the first batch, or batch by batch.
struct q_array {
    const void* user;
    size_t stride;
    bool out;
    nb_sim::field_buf* buf;
    bool whole;
    char* dev = nullptr;      // stage_in: the device address of point `first`
    size_t first = 0;
    char* at(size_t point) const { return dev ? dev + stride * (point - first) : nullptr; }
};

// The points of a request: the caller's, or with *_AT_BODIES the handle's own rows from first_body on.
template <class R>
q_array query_points(nb_sim* s, const R* req, bool whole = true)
{
    const size_t row = 4 * s->esz;
    if (req->flags & kQueryAtBodies) return {(const char*)s->bodies[s->cur] + row * req->first_body, row, false, nullptr, whole};
    return {req->points, row, false, &s->q_in[0], whole};
}

// Resolves points [first, first + count) of every array staged as `whole` says to device addresses: a device-pointer request's
// (`dev`) are the caller's own; a host-pointer request's get room in their engine buffer, the inputs copied in.
int stage_in(nb_sim* s, bool dev, std::initializer_list<q_array*> arrays, bool whole, size_t first, size_t count, const char* who)
{
    for (q_array* a : arrays) {
        if (!a->user || a->whole != whole) continue;
        if (dev || !a->buf) { a->dev = (char*)a->user; a->first = 0; continue; }
        if (int rc = field_reserve(s, *a->buf, a->stride * count, who)) return rc;
        a->dev = (char*)a->buf->p;
        a->first = first;
        if (!a->out) NB_HIP(s, hipMemcpyAsync(a->dev, (const char*)a->user + a->stride * first, a->stride * count, hipMemcpyHostToDevice, s->stream));
    }
    return NB_OK;
}

// The other way: copies the outputs that stage_in gave room back to a host-pointer request's arrays and, behind the arrays that
// are staged whole -- the end of the request --, waits for the stream.  A device-pointer request returns without waiting.
int stage_out(nb_sim* s, bool dev, std::initializer_list<q_array*> arrays, bool whole, size_t first, size_t count)
{
    if (dev) return NB_OK;
    for (q_array* a : arrays)
        if (a->user && a->out && a->buf && a->whole == whole)
            NB_HIP(s, hipMemcpyAsync((char*)a->user + a->stride * first, a->dev, a->stride * count, hipMemcpyDeviceToHost, s->stream));
    if (whole) NB_HIP(s, hipStreamSynchronize(s->stream));
    return NB_OK;
}

// One row at +inf: the LDS-DMA source of the f32 neighbour kernels for j past the range.  Written once per handle.
int ensure_inf_row(nb_sim* s, const char* who)
{
    if (s->f64 || s->q_inf.p) return NB_OK;
    static const float inf_row[4] = {HUGE_VALF, HUGE_VALF, HUGE_VALF, 0.0f};
    if (int rc = field_reserve(s, s->q_inf, 64, who)) return rc;
    NB_HIP(s, hipMemcpyAsync(s->q_inf.p, inf_row, sizeof inf_row, hipMemcpyHostToDevice, s->stream));
    return NB_OK;
}

// The batch rule: fewer points at once -- half as many, in whole workgroups' worth (prow) of points, one workgroup's being the
// floor -- while the batch is too big.  cut(mb) lays out a batch of mb points and returns the points it really takes.
template <class Cut, class Big>
uint32_t fit_batch(uint32_t mb, uint32_t prow, Cut&& cut, Big&& too_big)
{
    for (mb = cut(mb); too_big(mb) && mb > prow;) mb = cut(std::max(prow, (mb / 2 + prow - 1) / prow * prow));
    return mb;
}
uint32_t as_it_is(uint32_t mb) { return mb; }      // a cut that leaves the chunks alone

// The first batch of an m-point request whose kernel takes prow points per workgroup, under nb_field_eval's rule: at most 262,144
// points (65,536 in fp64), field_shape's j-chunks for them, halved until chunks x batch partial rows fit the bound of q_part.
uint32_t part_shape(const nb_sim* s, uint32_t m, uint32_t prow, bool wide, uint32_t* chunks, uint32_t* per)
{
    const uint64_t part_rows = std::max<uint64_t>(kFieldPartRows, (uint64_t)2 * field_blocks_wanted(s) * prow);
    return fit_batch(std::min(m, wide ? 65536u : 262144u), prow,
                     [&](uint32_t mb) { field_shape(s, ceil_div(mb, prow), chunks, per); return mb; },
                     [&](uint32_t mb) { return (uint64_t)*chunks * mb > part_rows; });
}

// What the *_shape getters share: the checks in front (`bad`: the text of a cap or k out of range, or null) and the outputs behind.
int shape_begin(nb_sim* s, const char* who, uint32_t m, const char* bad = nullptr)
{
    if (!s) return qfail(nullptr, NB_ERR_INVALID, who, "null handle");
    if (m == 0) return qfail(s, NB_ERR_INVALID, who, "m must be >= 1");
    return bad ? qfail(s, NB_ERR_INVALID, who, bad) : NB_OK;
}
int shape_put(uint32_t b, uint32_t c, uint32_t per, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk)
{
    if (batch) *batch = b;
    if (chunks) *chunks = c;
    if (j_per_chunk) *j_per_chunk = per;
    return NB_OK;
}

}  // namespace
}  // extern "C++"

int nb_field_eval(nb_sim* s, const nb_field_request* req)
{
    const char* who = "nb_field_eval";
    if (int rc = query_begin(s, req, kQField, s ? s->n : 0u, who, [&]() -> const char* {
            return !req->accel && !req->phi ? "accel and phi are both NULL" : nullptr; })) return rc;
    const bool at = (req->flags & NB_FIELD_AT_BODIES) != 0, dev = (req->flags & NB_FIELD_DEVICE) != 0;
    const bool wide = s->f64 || (req->flags & NB_FIELD_F64);      // fp64 arithmetic and outputs
    const size_t out_esz = wide ? 8 : 4;
    const uint32_t m = req->m;
    q_array pts = query_points(s, req), acc = {req->accel, 4 * out_esz, true, &s->q_out[0], true}, phi = {req->phi, out_esz, true, &s->q_out[1], true};
    if (int rc = stage_in(s, dev, {&pts, &acc, &phi}, true, 0, m, who)) return rc;

    const uint32_t rows = wide ? nb::kFieldRows64 : nb::kFieldRows;      // points per workgroup
    const void* bodies = s->bodies[s->cur];
    const void* zero_row = s->zero_row;
    uint32_t n = s->n, at_flag = at ? 1u : 0u;
    double G = s->G, eps2d = s->eps2;
    float eps2f = (float)s->eps2;
    for (uint32_t done = 0; done < m;) {
        uint32_t chunks, per, mb = part_shape(s, m - done, rows, wide, &chunks, &per);
        if (int rc = field_reserve(s, s->q_part, (size_t)4 * out_esz * chunks * mb, who)) return rc;
        const void* p = pts.at(done);
        void* part = s->q_part.p;
        void* a = acc.at(done);
        void* f = phi.at(done);
        uint32_t self0 = req->first_body + done;
        dim3 grid(ceil_div(mb, rows), chunks), block(nb::kBlock);
        if (wide) {
            void* args[] = {&bodies, &p, &part, &n, &mb, &per, &eps2d, &at_flag, &self0};
            const void* fn = s->f64 ? (const void*)&nb::nb_field64<double> : (const void*)&nb::nb_field64<float>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            void* rargs[] = {&part, &mb, &chunks, &G, &a, &f};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_field_reduce<double, double>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        } else {
            void* args[] = {&bodies, &p, &part, &n, &mb, &per, &eps2f, &at_flag, &self0, &zero_row};
            const void* fn = a && f ? (const void*)&nb::nb_field_pk<true, true>
                             : a ? (const void*)&nb::nb_field_pk<true, false> : (const void*)&nb::nb_field_pk<false, true>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            void* rargs[] = {&part, &mb, &chunks, &G, &a, &f};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_field_reduce<float, float>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        }
        done += mb;
    }
    return stage_out(s, dev, {&acc, &phi}, true, 0, m);
}

/* ---- neighbour queries -------------------------------------------------------------------- */

namespace {

uint32_t nbr_rows(const nb_sim* s) { return s->f64 ? nb::kNbrRows64 : nb::kNbrRows; }      // points per workgroup

// The first batch of an m-point request against `rows` bodies: its points, j-chunks and bodies per chunk -- nb_field_eval's rule
// (field_shape on the handle's n: the answer does not depend on the cut, and rows <= n only ever leaves chunks at the end empty).
void nbr_shape(const nb_sim* s, uint32_t m, uint32_t rows, uint32_t* batch, uint32_t* chunks, uint32_t* per)
{
    *batch = part_shape(s, m, nbr_rows(s), s->f64, chunks, per);
    *chunks = std::max(1u, std::min(*chunks, ceil_div(rows, *per)));      // chunks that start past the last row hold nothing
}

// the radius checks that nb_neighbor_lists and nb_split_force share with nb_neighbors
const char* bad_radius(double radius) { return radius >= 0.0 ? nullptr : "radius must be >= 0 (0: none given)"; }

}  // namespace

extern "C++" int nbi::neighbors(nb_sim* s, const nb_neighbor_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQNbr, rows, who, [&]() -> const char* {
            if (!req->index && !req->dist2 && !req->count) return "index, dist2 and count are all NULL";
            if (bad_radius(req->radius)) return bad_radius(req->radius);
            return req->count && !req->radii && !(req->radius > 0.0) ? "count needs radii or radius > 0" : nullptr; })) return rc;
    const bool at = (req->flags & NB_NBR_AT_BODIES) != 0, dev = (req->flags & NB_NBR_DEVICE) != 0;
    const size_t esz = s->esz;
    const uint32_t m = req->m;
    q_array pts = query_points(s, req), rad = {req->count ? req->radii : nullptr, esz, false, &s->q_in[1], true};      // the radius only enters the count
    q_array idx = {req->index, 4, true, &s->q_out[0], true}, d2 = {req->dist2, esz, true, &s->q_out[1], true}, cnt = {req->count, 4, true, &s->q_out[2], true};
    if (int rc = stage_in(s, dev, {&pts, &rad, &idx, &d2, &cnt}, true, 0, m, who)) return rc;
    if (int rc = ensure_inf_row(s, who)) return rc;

    const uint32_t prow = nbr_rows(s);
    const void* bodies = s->bodies[s->cur];
    const void* inf_row = s->q_inf.p;
    uint32_t n = rows, at_flag = at ? 1u : 0u;
    double rd = req->radius;
    float rf = (float)req->radius;
    for (uint32_t done = 0; done < m;) {
        uint32_t mb, chunks, per;
        nbr_shape(s, m - done, rows, &mb, &chunks, &per);
        if (int rc = field_reserve(s, s->q_part, (size_t)16 * chunks * mb, who)) return rc;
        const void* p = pts.at(done);
        const void* r = rad.at(done);
        void* part = s->q_part.p;
        void* oi = idx.at(done);
        void* od = d2.at(done);
        void* oc = cnt.at(done);
        uint32_t self0 = req->first_body + done;
        dim3 grid(ceil_div(mb, prow), chunks), block(nb::kBlock);
        void* rargs[] = {&part, &mb, &chunks, &oi, &od, &oc};
        if (s->f64) {
            void* args[] = {&bodies, &p, &r, &part, &n, &mb, &per, &rd, &at_flag, &self0};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbr64<double>, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbr_reduce<double>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        } else {
            void* args[] = {&bodies, &p, &r, &part, &n, &mb, &per, &rf, &at_flag, &self0, &inf_row};
            const void* fn = oc ? (const void*)&nb::nb_nbr_pk<true> : (const void*)&nb::nb_nbr_pk<false>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbr_reduce<float>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        }
        done += mb;
    }
    return stage_out(s, dev, {&idx, &d2, &cnt}, true, 0, m);
}

int nb_neighbors(nb_sim* s, const nb_neighbor_request* req) { return nbi::neighbors(s, req, s ? s->n : 0u, "nb_neighbors"); }

int nb_neighbors_shape(nb_sim* s, uint32_t m, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk)
{
    if (int rc = shape_begin(s, "nb_neighbors_shape", m)) return rc;
    uint32_t b, c, per;
    nbr_shape(s, m, s->n, &b, &c, &per);
    return shape_put(b, c, per, batch, chunks, j_per_chunk);
}

/* ---- neighbour lists ---------------------------------------------------------------------- */

namespace {

constexpr uint32_t kNblMaxCap = 4096;                   // most entries of one row
constexpr uint64_t kNblListBytes = 256ull << 20;        // most bytes of `list` one batch writes (or one workgroup's points x cap, if that is more)

const char* bad_cap(uint32_t cap) { return cap == 0 || cap > kNblMaxCap ? "cap must be in 1 .. 4096" : nullptr; }

// nbr_shape with the rows of `list` bounded too: the batch is halved until batch x cap x 4 <= kNblListBytes, the chunks follow the
// batch as in nbr_shape (which never takes more points than it is given).
void nbl_shape(const nb_sim* s, uint32_t m, uint32_t cap, uint32_t rows, uint32_t* batch, uint32_t* chunks, uint32_t* per)
{
    *batch = fit_batch(m, nbr_rows(s), [&](uint32_t mb) { nbr_shape(s, mb, rows, &mb, chunks, per); return mb; },
                       [&](uint32_t mb) { return (uint64_t)mb * cap * 4 > kNblListBytes; });
}

}  // namespace

extern "C++" int nbi::neighbor_lists(nb_sim* s, const nb_neighbor_list_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQNbl, rows, who, [&]() -> const char* {
            if (!req->list) return "list is NULL";
            if (bad_cap(req->cap)) return bad_cap(req->cap);
            if (req->reserved != 0) return "reserved must be 0";
            if (bad_radius(req->radius)) return bad_radius(req->radius);
            return !req->radii && !(req->radius > 0.0) ? "the lists need radii or radius > 0" : nullptr; })) return rc;
    const bool at = (req->flags & NB_NBR_AT_BODIES) != 0, dev = (req->flags & NB_NBR_DEVICE) != 0;
    const size_t esz = s->esz;
    const uint32_t m = req->m, cap = req->cap;
    q_array pts = query_points(s, req), rad = {req->radii, esz, false, &s->q_in[1], true}, lst = {req->list, (size_t)4 * cap, true, &s->q_out[3], false};
    q_array idx = {req->index, 4, true, &s->q_out[0], true}, d2 = {req->dist2, esz, true, &s->q_out[1], true}, cnt = {req->count, 4, true, &s->q_out[2], true};
    if (int rc = stage_in(s, dev, {&pts, &rad, &idx, &d2, &cnt}, true, 0, m, who)) return rc;
    if (int rc = ensure_inf_row(s, who)) return rc;

    const uint32_t prow = nbr_rows(s);
    const void* bodies = s->bodies[s->cur];
    const void* inf_row = s->q_inf.p;
    uint32_t n = rows, at_flag = at ? 1u : 0u, cap_arg = cap;
    double rd = req->radius;
    float rf = (float)req->radius;
    for (uint32_t done = 0; done < m;) {
        uint32_t mb, chunks, per;
        nbl_shape(s, m - done, cap, rows, &mb, &chunks, &per);
        if (int rc = field_reserve(s, s->q_part, (size_t)16 * chunks * mb, who)) return rc;
        if (int rc = field_reserve(s, s->q_off, (size_t)4 * chunks * mb, who)) return rc;
        if (int rc = stage_in(s, dev, {&lst}, false, done, mb, who)) return rc;      // a host-pointer request stages its rows batch by batch
        const void* p = pts.at(done);
        const void* r = rad.at(done);
        void* part = s->q_part.p;
        void* off = s->q_off.p;
        void* l = lst.at(done);
        void* oi = idx.at(done);
        void* od = d2.at(done);
        void* oc = cnt.at(done);
        uint32_t self0 = req->first_body + done;
        dim3 grid(ceil_div(mb, prow), chunks), block(nb::kBlock);
        NB_HIP(s, hipMemsetAsync(l, 0xff, (size_t)4 * cap * mb, s->stream));          // what pads the rows
        void* oargs[] = {&part, &mb, &chunks, &off, &oi, &od, &oc};
        if (s->f64) {
            void* args[] = {&bodies, &p, &r, &part, &n, &mb, &per, &rd, &at_flag, &self0};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbr64<double>, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbl_offsets<double>, dim3(ceil_div(mb, nb::kBlock)), block, oargs, 0, s->stream));
            void* fargs[] = {&bodies, &p, &r, &off, &l, &n, &mb, &per, &rd, &at_flag, &self0, &cap_arg};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbl64<double>, grid, block, fargs, 0, s->stream));
        } else {
            void* args[] = {&bodies, &p, &r, &part, &n, &mb, &per, &rf, &at_flag, &self0, &inf_row};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbr_pk<true>, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbl_offsets<float>, dim3(ceil_div(mb, nb::kBlock)), block, oargs, 0, s->stream));
            void* fargs[] = {&bodies, &p, &r, &off, &l, &n, &mb, &per, &rf, &at_flag, &self0, &cap_arg, &inf_row};
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_nbl_pk<>, grid, block, fargs, 0, s->stream));
        }
        if (int rc = stage_out(s, dev, {&lst}, false, done, mb)) return rc;
        done += mb;
    }
    return stage_out(s, dev, {&idx, &d2, &cnt}, true, 0, m);
}

int nb_neighbor_lists(nb_sim* s, const nb_neighbor_list_request* req) { return nbi::neighbor_lists(s, req, s ? s->n : 0u, "nb_neighbor_lists"); }

int nb_neighbor_lists_shape(nb_sim* s, uint32_t m, uint32_t cap, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk)
{
    if (int rc = shape_begin(s, "nb_neighbor_lists_shape", m, bad_cap(cap))) return rc;
    uint32_t b, c, per;
    nbl_shape(s, m, cap, s->n, &b, &c, &per);
    return shape_put(b, c, per, batch, chunks, j_per_chunk);
}

/* ---- k nearest neighbours ----------------------------------------------------------------- */

namespace {

constexpr uint64_t kKnnRowBytes = kNblListBytes;        // most bytes of partial rows (chunks x batch x k x 8) one batch leaves
constexpr uint32_t kKnnMaxChunks = 512;                 // most j-chunks: nb_knn_merge keeps 64 bytes of LDS per chunk (32 KiB)

const char* bad_k(uint32_t k) { return k == 0 || k > nb::kKnnMaxK ? "k must be in 1 .. 64" : nullptr; }

// The shape of a WHOLE m-point request: nbr_shape's batch and chunks for m points (at most kKnnMaxChunks chunks: few points against
// millions of bodies would get more); the batch is then halved, the chunks kept, until chunks x batch x k x 8 <= kKnnRowBytes.
// Every batch of the request, the last and shorter one included, runs against these chunks: fewer, longer chunks are what a
// k-nearest pass wants, since every chunk has to find its own k candidates first.
void knn_shape(const nb_sim* s, uint32_t m, uint32_t k, uint32_t rows, uint32_t* batch, uint32_t* chunks, uint32_t* per)
{
    uint32_t mb;
    nbr_shape(s, m, rows, &mb, chunks, per);
    if (*chunks > kKnnMaxChunks) {
        *per = ceil_div(ceil_div(rows, kKnnMaxChunks), (uint32_t)nb::kTile) * nb::kTile;
        *chunks = ceil_div(rows, *per);
    }
    *batch = fit_batch(mb, nbr_rows(s), as_it_is, [&](uint32_t b) { return (uint64_t)*chunks * b * k * 8 > kKnnRowBytes; });
}

#ifdef NB_TUNING    // calibration build only: what the passes did, summed over the calls since the last reset (tools/knn_bench.py --stats)
uint64_t g_knn_stats[5];      // (point, chunk) rows, candidates appended, compactions before the end of a chunk, groups on the slow path, groups
#endif

}  // namespace

#ifdef NB_TUNING
extern "C" __attribute__((visibility("default"))) void nb_tuning_knn_stats(uint64_t* out, int reset)
{
    for (int q = 0; q < 5; ++q) { if (out) out[q] = g_knn_stats[q]; if (reset) g_knn_stats[q] = 0; }
}
#endif

extern "C++" int nbi::knn(nb_sim* s, const nb_knn_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQKnn, rows, who, [&]() -> const char* {
            if (bad_k(req->k)) return bad_k(req->k);
            if (req->reserved != 0) return "reserved must be 0";
            return !req->index && !req->dist2 ? "index and dist2 are both NULL" : nullptr; })) return rc;
    const bool at = (req->flags & NB_NBR_AT_BODIES) != 0, dev = (req->flags & NB_NBR_DEVICE) != 0;
    const size_t esz = s->esz, ent = s->f64 ? 16 : 8;
    const uint32_t m = req->m, cap = nb::knn_cap(req->k);
    uint32_t n = rows, at_flag = at ? 1u : 0u, k = req->k;
    q_array pts = query_points(s, req), idx = {req->index, (size_t)4 * k, true, &s->q_out[0], false}, d2 = {req->dist2, esz * k, true, &s->q_out[1], false};
    if (int rc = stage_in(s, dev, {&pts}, true, 0, m, who)) return rc;
    if (int rc = ensure_inf_row(s, who)) return rc;

    const uint32_t prow = nbr_rows(s);
    const void* bodies = s->bodies[s->cur];
    const void* inf_row = s->q_inf.p;
    uint32_t batch, chunks, per;
    knn_shape(s, m, k, rows, &batch, &chunks, &per);      // once: every batch runs against the same chunks
    const size_t heads = (size_t)chunks * nb::kKnnMergeLanes;      // nb_knn_merge's dynamic LDS (chunks <= kKnnMaxChunks)
    for (uint32_t done = 0; done < m;) {
        uint32_t mb = std::min(batch, m - done);
        if (int rc = field_reserve(s, s->q_work, ent * cap * chunks * mb, who)) return rc;
        if (int rc = stage_in(s, dev, {&idx, &d2}, false, done, mb, who)) return rc;      // a host-pointer request stages its outputs batch by batch
        const void* p = pts.at(done);
        void* work = s->q_work.p;
        void* oi = idx.at(done);
        void* od = d2.at(done);
        uint32_t self0 = req->first_body + done;
        dim3 grid(ceil_div(mb, prow), chunks), block(nb::kBlock);
        void* margs[] = {&work, &mb, &chunks, &k, &oi, &od};
        const dim3 mgrid(ceil_div(mb, nb::kKnnMergeLanes)), mblock(nb::kKnnMergeLanes);
        void* stat_rows = nullptr;
        void* stat_waves = nullptr;
        const void* fn64 = (const void*)&nb::nb_knn64<double>;
        const void* fn32 = (const void*)&nb::nb_knn_pk<>;
#ifdef NB_TUNING
        const size_t stat_n = (size_t)chunks * mb, wave_n = (size_t)chunks * grid.x * (nb::kBlock / 64);
        const bool stats = getenv("NB_KNN_STATS") != nullptr;
        if (stats) {
            if (int rc = field_reserve(s, s->knn_stat, 8 * stat_n + 4 * wave_n, who)) return rc;
            stat_rows = s->knn_stat.p;
            stat_waves = (char*)s->knn_stat.p + 8 * stat_n;
            fn64 = (const void*)&nb::nb_knn64<double, true>;
            fn32 = (const void*)&nb::nb_knn_pk<true>;
        }
#endif
        if (s->f64) {
            void* args[] = {&bodies, &p, &work, &n, &mb, &per, &k, &at_flag, &self0, &stat_rows, &stat_waves};
            NB_HIP(s, hipLaunchKernel(fn64, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_knn_merge<double>, mgrid, mblock, margs, heads, s->stream));
        } else {
            void* args[] = {&bodies, &p, &work, &n, &mb, &per, &k, &at_flag, &self0, &inf_row, &stat_rows, &stat_waves};
            NB_HIP(s, hipLaunchKernel(fn32, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_knn_merge<float>, mgrid, mblock, margs, heads, s->stream));
        }
#ifdef NB_TUNING
        if (stats) {
            std::vector<uint32_t> h(2 * stat_n + wave_n);
            NB_HIP(s, hipMemcpyAsync(h.data(), s->knn_stat.p, 4 * h.size(), hipMemcpyDeviceToHost, s->stream));
            NB_HIP(s, hipStreamSynchronize(s->stream));
            g_knn_stats[0] += stat_n;
            for (size_t q = 0; q < stat_n; ++q) { g_knn_stats[1] += h[2 * q]; g_knn_stats[2] += h[2 * q + 1]; }
            for (size_t q = 0; q < wave_n; ++q) g_knn_stats[3] += h[2 * stat_n + q];
            for (uint32_t c = 0; c < chunks; ++c) {       // the groups a wave of chunk c walks: whole groups of 4 rows per tile
                const uint32_t r = std::min(per, n - c * per);
                g_knn_stats[4] += (uint64_t)grid.x * (nb::kBlock / 64) * ((r / nb::kTile) * (nb::kTile / nb::kKnnU) + (r % nb::kTile + nb::kKnnU - 1) / nb::kKnnU);
            }
        }
#endif
        if (int rc = stage_out(s, dev, {&idx, &d2}, false, done, mb)) return rc;
        done += mb;
    }
    return stage_out(s, dev, {}, true, 0, m);
}

int nb_knn(nb_sim* s, const nb_knn_request* req) { return nbi::knn(s, req, s ? s->n : 0u, "nb_knn"); }

int nb_knn_shape(nb_sim* s, uint32_t m, uint32_t k, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk)
{
    if (int rc = shape_begin(s, "nb_knn_shape", m, bad_k(k))) return rc;
    uint32_t b, c, per;
    knn_shape(s, m, k, s->n, &b, &c, &per);
    return shape_put(b, c, per, batch, chunks, j_per_chunk);
}

/* ---- forces over neighbour rows ------------------------------------------------------------- */

namespace {

// The rows of every batch but the last of a host-pointer request: nbl_shape's bound for the staged rows, batch x cap x 4 <= kNblListBytes.
uint32_t lf_batch(const nb_sim* s, uint32_t m, uint32_t cap)
{
    return fit_batch(m, nb::lf_rows(s->f64), as_it_is, [&](uint32_t mb) { return (uint64_t)mb * cap * 4 > kNblListBytes; });
}

#define NB_LF_TABLE(K) {nullptr, (const void*)&nb::K<false, false, true>, (const void*)&nb::K<false, true, false>, (const void*)&nb::K<false, true, true>, \
                        (const void*)&nb::K<true, false, false>, (const void*)&nb::K<true, false, true>, (const void*)&nb::K<true, true, false>,    \
                        (const void*)&nb::K<true, true, true>}
// the kernel for the outputs asked for: [accel << 2 | jerk << 1 | phi]
const void* lf_kernel(bool f64, bool a, bool j, bool p)
{
    static const void* const k32[8] = NB_LF_TABLE(nb_lf32);
    static const void* const k64[8] = NB_LF_TABLE(nb_lf64);
    return (f64 ? k64 : k32)[(a ? 4 : 0) | (j ? 2 : 0) | (p ? 1 : 0)];
}
#undef NB_LF_TABLE

}  // namespace

extern "C++" int nbi::list_force(nb_sim* s, const nb_list_force_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQListF, rows, who, [&]() -> const char* {
            const bool at = (req->flags & NB_LISTF_AT_BODIES) != 0;
            if (!req->list) return "list is NULL";
            if (bad_cap(req->cap)) return bad_cap(req->cap);
            if (req->reserved != 0) return "reserved must be 0";
            if (!req->accel && !req->jerk && !req->phi) return "accel, jerk and phi are all NULL";
            if (at && req->point_vel) return "point_vel must be NULL with NB_LISTF_AT_BODIES";
            if (!at && req->jerk && !req->point_vel) return "point_vel is NULL (the jerk at points needs their velocities)";
            return !at && !req->jerk && req->point_vel ? "point_vel must be NULL when jerk is NULL" : nullptr; })) return rc;
    if (req->jerk && !s->hermite) return qfail(s, NB_ERR_STATE, who, "jerk needs a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    const bool at = (req->flags & NB_LISTF_AT_BODIES) != 0, dev = (req->flags & NB_LISTF_DEVICE) != 0;
    const size_t esz = s->esz, row4 = 4 * esz;
    const uint32_t m = req->m;
    const bool wj = req->jerk != nullptr;
    const void* fn = lf_kernel(s->f64, req->accel != nullptr, wj, req->phi != nullptr);
    const void* bodies = s->bodies[s->cur];
    const void* vel = wj ? s->vel : nullptr;
    uint32_t n = rows, cap = req->cap, at_flag = at ? 1u : 0u;
    double G = s->G, eps2d = s->eps2;
    float eps2f = (float)s->eps2;
    // a host-pointer request stages its rows and its outputs batch by batch
    q_array lst = {req->list, (size_t)4 * cap, false, &s->q_in[3], false}, cnt = {req->count, 4, false, &s->q_in[1], false}, pts = query_points(s, req, false);
    q_array pvel = {!wj ? nullptr : at ? (const char*)s->vel + row4 * req->first_body : req->point_vel, row4, false, at ? nullptr : &s->q_in[2], false};
    q_array acc = {req->accel, row4, true, &s->q_out[0], false}, jerk = {req->jerk, row4, true, &s->q_out[1], false}, phi = {req->phi, esz, true, &s->q_out[2], false};
    const uint32_t batch = dev ? m : lf_batch(s, m, cap);        // device pointers are read in place: one launch
    for (uint32_t done = 0; done < m;) {
        uint32_t mb = std::min(batch, m - done);
        if (int rc = stage_in(s, dev, {&lst, &cnt, &pts, &pvel, &acc, &jerk, &phi}, false, done, mb, who)) return rc;
        const void* p = pts.at(done);
        const void* pv = pvel.at(done);
        const void* l = lst.at(done);
        const void* c = cnt.at(done);
        void* oa = acc.at(done);
        void* oj = jerk.at(done);
        void* op = phi.at(done);
        uint32_t self0 = req->first_body + done;
        const dim3 grid(ceil_div(mb, nb::lf_rows(s->f64))), block(nb::kBlock);
        if (s->f64) {
            void* args[] = {&bodies, &vel, &p, &pv, &l, &c, &n, &mb, &cap, &eps2d, &G, &at_flag, &self0, &oa, &oj, &op};
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
        } else {
            void* args[] = {&bodies, &vel, &p, &pv, &l, &c, &n, &mb, &cap, &eps2f, &G, &at_flag, &self0, &oa, &oj, &op};
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
        }
        if (int rc = stage_out(s, dev, {&acc, &jerk, &phi}, false, done, mb)) return rc;
        done += mb;
    }
    return stage_out(s, dev, {}, true, 0, m);
}

int nb_list_force(nb_sim* s, const nb_list_force_request* req) { return nbi::list_force(s, req, s ? s->n : 0u, "nb_list_force"); }

int nb_list_force_shape(nb_sim* s, uint32_t m, uint32_t cap, uint32_t* batch, uint32_t* lanes_per_row)
{
    if (int rc = shape_begin(s, "nb_list_force_shape", m, bad_cap(cap))) return rc;
    if (batch) *batch = lf_batch(s, m, cap);
    if (lanes_per_row) *lanes_per_row = nb::lf_lanes(s->f64);
    return NB_OK;
}

/* ---- regular and irregular force+jerk in one pass -------------------------------------------- */

namespace {

uint32_t split_rows(const nb_sim* s) { return s->f64 ? nb::kSplitRows64 : nb::kSplitRows; }      // points per workgroup

// The first batch of an m-point request against `rows` bodies: nbr_shape's rule for nb_split_pk's rows per workgroup, with
// `planes` partial rows per (point, j-chunk) counted against nb_field_eval's bound of q_part (the same bytes).  Where the j-chunks
// field_shape cuts for a batch do not fit, the chunks are made LONGER first (down to what kFieldMaxChunk allows: a workgroup's
// prologue, epilogue and its rows in nb_split_reduce are paid per chunk, and 2,048 workgroups are wanted, not 2,048-body chunks),
// and only then is the batch halved (measured: profiles/r15/split_force.md §3).
void split_shape(const nb_sim* s, uint32_t m, uint32_t rows, uint32_t planes, uint32_t* batch, uint32_t* chunks, uint32_t* per)
{
    const uint32_t prow = split_rows(s);
    const uint64_t part_rows = std::max<uint64_t>(kFieldPartRows, (uint64_t)2 * field_blocks_wanted(s) * (s->f64 ? nb::kFieldRows64 : nb::kFieldRows)) / planes;
    auto cut = [&](uint32_t mb) {
        field_shape(s, ceil_div(mb, prow), chunks, per);
        const uint64_t room = part_rows / mb;                       // the chunks the bound leaves a batch of mb points
        if (*chunks > room && room >= std::max(1u, ceil_div(s->n, kFieldMaxChunk))) {
            *per = ceil_div(ceil_div(s->n, (uint32_t)room), (uint32_t)nb::kTile) * nb::kTile;
            *chunks = ceil_div(s->n, *per);
        }
        return mb;
    };
    *batch = fit_batch(std::min(m, s->f64 ? 65536u : 262144u), prow, cut, [&](uint32_t mb) { return (uint64_t)*chunks * mb > part_rows; });
    *chunks = std::max(1u, std::min(*chunks, ceil_div(rows, *per)));      // chunks that start past the last row hold nothing
}

}  // namespace

extern "C++" int nbi::split_force(nb_sim* s, const nb_split_force_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQSplit, rows, who, [&]() -> const char* {
            const bool at = (req->flags & NB_SPLIT_AT_BODIES) != 0, wj = req->jerk_irr || req->jerk_reg;
            if (!req->accel_irr && !req->accel_reg && !wj) return "accel_irr, accel_reg, jerk_irr and jerk_reg are all NULL";
            if (at && req->point_vel) return "point_vel must be NULL with NB_SPLIT_AT_BODIES";
            if (!at && wj && !req->point_vel) return "point_vel is NULL (the jerk at points needs their velocities)";
            if (!at && !wj && req->point_vel) return "point_vel must be NULL when jerk_irr and jerk_reg are NULL";
            if (bad_radius(req->radius)) return bad_radius(req->radius);
            return !req->radii && !(req->radius > 0.0) ? "radii is NULL and radius is not > 0" : nullptr; })) return rc;
    const bool at = (req->flags & NB_SPLIT_AT_BODIES) != 0, dev = (req->flags & NB_SPLIT_DEVICE) != 0;
    const bool wj = req->jerk_irr || req->jerk_reg;
    if (wj && !s->hermite) return qfail(s, NB_ERR_STATE, who, "jerk_irr / jerk_reg need a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    const size_t esz = s->esz, row4 = 4 * esz;
    const uint32_t m = req->m;
    const void* bodies = s->bodies[s->cur];
    const void* vel = wj ? s->vel : nullptr;
    // a host-pointer request is staged whole, as nb_field_eval stages its own: O(m)
    q_array pts = query_points(s, req), rad = {req->radii, esz, false, &s->q_in[1], true};
    q_array pvel = {!wj ? nullptr : at ? (const char*)s->vel + row4 * req->first_body : req->point_vel, row4, false, at ? nullptr : &s->q_in[2], true};
    q_array out[4] = {{req->accel_irr, row4, true, &s->q_out[0], true}, {req->accel_reg, row4, true, &s->q_out[1], true},
                      {req->jerk_irr, row4, true, &s->q_out[2], true}, {req->jerk_reg, row4, true, &s->q_out[3], true}};
    if (int rc = stage_in(s, dev, {&pts, &pvel, &rad, &out[0], &out[1], &out[2], &out[3]}, true, 0, m, who)) return rc;

    const uint32_t prow = split_rows(s);
    const void* zero_row = s->zero_row;
    uint32_t n = rows, planes = wj ? 4u : 2u;
    double G = s->G, eps2d = s->eps2, rd = req->radius;
    float eps2f = (float)s->eps2, rf = (float)req->radius;
    for (uint32_t done = 0; done < m;) {
        uint32_t mb, chunks, per;
        split_shape(s, m - done, rows, planes, &mb, &chunks, &per);
        if (int rc = field_reserve(s, s->q_part, row4 * planes * chunks * mb, who)) return rc;
        const void* p = pts.at(done);
        const void* pv = pvel.at(done);
        const void* r = rad.at(done);
        void* part = s->q_part.p;
        void* o[4] = {out[0].at(done), out[1].at(done), out[2].at(done), out[3].at(done)};
        dim3 grid(ceil_div(mb, prow), chunks), block(nb::kBlock);
        void* rargs[] = {&part, &mb, &chunks, &planes, &G, &o[0], &o[1], &o[2], &o[3]};
        if (s->f64) {
            void* args[] = {&bodies, &vel, &p, &pv, &r, &part, &n, &mb, &per, &eps2d, &rd};
            const void* fn = wj ? (const void*)&nb::nb_split64<double, true> : (const void*)&nb::nb_split64<double, false>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_split_reduce<double, double>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        } else {
            void* args[] = {&bodies, &vel, &p, &pv, &r, &part, &n, &mb, &per, &eps2f, &rf, &zero_row};
            const void* fn = wj ? (const void*)&nb::nb_split_pk<nb::kSplitNG, true> : (const void*)&nb::nb_split_pk<nb::kSplitNG, false>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_split_reduce<float, float>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        }
        done += mb;
    }
    return stage_out(s, dev, {&out[0], &out[1], &out[2], &out[3]}, true, 0, m);
}

int nb_split_force(nb_sim* s, const nb_split_force_request* req) { return nbi::split_force(s, req, s ? s->n : 0u, "nb_split_force"); }

int nb_split_force_shape(nb_sim* s, uint32_t m, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk, uint32_t* rows_per_workgroup)
{
    if (int rc = shape_begin(s, "nb_split_force_shape", m)) return rc;
    uint32_t b, c, per;
    split_shape(s, m, s->n, s->hermite ? 4u : 2u, &b, &c, &per);      // (a Hermite handle: the shape of a request with the jerk pair)
    if (rows_per_workgroup) *rows_per_workgroup = split_rows(s);
    return shape_put(b, c, per, batch, chunks, j_per_chunk);
}

/* ---- the two sums and the neighbour rows from one pass ---------------------------------------- */

namespace {

constexpr query_kind kQSplitLists = {"nb_split_lists_request", "NB_SPLIT_AT_BODIES", NB_SPLIT_AT_BODIES | NB_SPLIT_DEVICE, true};
// Most bytes of segments (chunks x batch x cap x 4) one batch leaves: between kNblListBytes, what a batch of nb_neighbor_lists writes,
// and what nb_knn's working rows may take; N = 262,144 at cap 256 on a Hermite f32 handle (4 chunks of 65,536 bodies for one batch
// of 262,144 points) just keeps split_shape's shape under it.
constexpr uint64_t kSplSegBytes = 1ull << 30;

// split_shape's shape; the batch is halved further -- the chunks cut again by split_shape's rule at every candidate -- only while the
// segments exceed their bound (one workgroup's points being the floor, as for every batch rule).
void spl_shape(const nb_sim* s, uint32_t m, uint32_t cap, uint32_t rows, uint32_t planes, uint32_t* batch, uint32_t* chunks, uint32_t* per)
{
    const uint32_t prow = split_rows(s);
    split_shape(s, m, rows, planes, batch, chunks, per);
    while ((uint64_t)*chunks * *batch * cap * 4 > kSplSegBytes && *batch > prow)
        split_shape(s, std::max(prow, (*batch / 2 + prow - 1) / prow * prow), rows, planes, batch, chunks, per);
    // one workgroup's points against very many short chunks at a large cap: longer chunks are all that is left
    const uint32_t room = (uint32_t)std::max<uint64_t>(1, kSplSegBytes / ((uint64_t)*batch * cap * 4));
    if (*chunks > room) {
        *per = ceil_div(ceil_div(s->n, room), (uint32_t)nb::kTile) * nb::kTile;
        *chunks = std::max(1u, std::min(ceil_div(s->n, *per), ceil_div(rows, *per)));
    }
}

// Whether nb_split_lists cuts EVERY batch of a request at all n bodies as nb_split_force cuts it (then its sums are that call's bits).
bool spl_shape_is_splits(const nb_sim* s, uint32_t cap, uint32_t planes)
{
    for (uint32_t done = 0; done < s->n;) {
        uint32_t b0, c0, p0, b1, c1, p1;
        split_shape(s, s->n - done, s->n, planes, &b0, &c0, &p0);
        spl_shape(s, s->n - done, cap, s->n, planes, &b1, &c1, &p1);
        if (b0 != b1 || c0 != c1 || p0 != p1) return false;
        done += b0;
    }
    return true;
}

// the lanes of nb_spl_rows that share a row: the power of two from 8 to 64 that covers cap (or 64)
uint32_t spl_lanes(uint32_t cap)
{
    uint32_t l = 8;
    while (l < 64 && l < cap) l *= 2;
    return l;
}

}  // namespace

extern "C++" int nbi::split_lists(nb_sim* s, const nb_split_lists_request* req, uint32_t rows, const char* who)
{
    if (int rc = query_begin(s, req, kQSplitLists, rows, who, [&]() -> const char* {
            const bool at = (req->flags & NB_SPLIT_AT_BODIES) != 0, wj = req->jerk_irr || req->jerk_reg;
            if (!req->accel_irr && !req->accel_reg && !wj) return "accel_irr, accel_reg, jerk_irr and jerk_reg are all NULL (use nb_neighbor_lists for the rows alone)";
            if (at && req->point_vel) return "point_vel must be NULL with NB_SPLIT_AT_BODIES";
            if (!at && wj && !req->point_vel) return "point_vel is NULL (the jerk at points needs their velocities)";
            if (!at && !wj && req->point_vel) return "point_vel must be NULL when jerk_irr and jerk_reg are NULL";
            if (!req->list) return "list is NULL";
            if (bad_cap(req->cap)) return bad_cap(req->cap);
            if (req->reserved != 0) return "reserved must be 0";
            if (bad_radius(req->radius)) return bad_radius(req->radius);
            return !req->radii && !(req->radius > 0.0) ? "radii is NULL and radius is not > 0" : nullptr; })) return rc;
    const bool at = (req->flags & NB_SPLIT_AT_BODIES) != 0, dev = (req->flags & NB_SPLIT_DEVICE) != 0;
    const bool wj = req->jerk_irr || req->jerk_reg;
    if (wj && !s->hermite) return qfail(s, NB_ERR_STATE, who, "jerk_irr / jerk_reg need a Hermite handle (nb_config.integrator = NB_INT_HERMITE4)");
    const size_t esz = s->esz, row4 = 4 * esz;
    const uint32_t m = req->m;
    const void* bodies = s->bodies[s->cur];
    const void* vel = wj ? s->vel : nullptr;
    // a host-pointer request: everything O(m) is staged whole as nb_split_force stages it, the rows batch by batch as nb_neighbor_lists stages them
    q_array pts = query_points(s, req), rad = {req->radii, esz, false, &s->q_in[1], true};
    q_array pvel = {!wj ? nullptr : at ? (const char*)s->vel + row4 * req->first_body : req->point_vel, row4, false, at ? nullptr : &s->q_in[2], true};
    q_array out[4] = {{req->accel_irr, row4, true, &s->q_out[0], true}, {req->accel_reg, row4, true, &s->q_out[1], true},
                      {req->jerk_irr, row4, true, &s->q_out[2], true}, {req->jerk_reg, row4, true, &s->q_out[3], true}};
    q_array lst = {req->list, (size_t)4 * req->cap, true, &s->q_out[4], false}, cnt = {req->count, 4, true, &s->q_out[5], true};
    if (int rc = stage_in(s, dev, {&pts, &pvel, &rad, &out[0], &out[1], &out[2], &out[3], &cnt}, true, 0, m, who)) return rc;

    const uint32_t prow = split_rows(s);
    const void* zero_row = s->zero_row;
    uint32_t n = rows, planes = wj ? 4u : 2u, cap = req->cap, at_flag = at ? 1u : 0u, lanes = spl_lanes(cap);
    double G = s->G, eps2d = s->eps2, rd = req->radius;
    float eps2f = (float)s->eps2, rf = (float)req->radius;
    for (uint32_t done = 0; done < m;) {
        uint32_t mb, chunks, per;
        spl_shape(s, m - done, cap, rows, planes, &mb, &chunks, &per);
        if (int rc = field_reserve(s, s->q_part, row4 * planes * chunks * mb, who)) return rc;
        if (int rc = field_reserve(s, s->q_seg, (size_t)4 * cap * chunks * mb, who)) return rc;
        if (int rc = field_reserve(s, s->q_segcnt, (size_t)4 * chunks * mb, who)) return rc;
        if (int rc = stage_in(s, dev, {&lst}, false, done, mb, who)) return rc;
        const void* p = pts.at(done);
        const void* pv = pvel.at(done);
        const void* r = rad.at(done);
        void* part = s->q_part.p;
        void* seg = s->q_seg.p;
        void* segcnt = s->q_segcnt.p;
        void* l = lst.at(done);
        void* oc = cnt.at(done);
        void* o[4] = {out[0].at(done), out[1].at(done), out[2].at(done), out[3].at(done)};
        uint32_t self0 = req->first_body + done;
        dim3 grid(ceil_div(mb, prow), chunks), block(nb::kBlock);
        void* rargs[] = {&part, &mb, &chunks, &planes, &G, &o[0], &o[1], &o[2], &o[3]};
        void* gargs[] = {&seg, &segcnt, &mb, &chunks, &cap, &lanes, &l, &oc};
        if (s->f64) {
            void* args[] = {&bodies, &vel, &p, &pv, &r, &part, &n, &mb, &per, &eps2d, &rd, &seg, &segcnt, &cap, &at_flag, &self0};
            const void* fn = wj ? (const void*)&nb::nb_spl64<double, true> : (const void*)&nb::nb_spl64<double, false>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_split_reduce<double, double>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        } else {
            void* args[] = {&bodies, &vel, &p, &pv, &r, &part, &n, &mb, &per, &eps2f, &rf, &zero_row, &seg, &segcnt, &cap, &at_flag, &self0};
            const void* fn = wj ? (const void*)&nb::nb_spl_pk<nb::kSplitNG, true> : (const void*)&nb::nb_spl_pk<nb::kSplitNG, false>;
            NB_HIP(s, hipLaunchKernel(fn, grid, block, args, 0, s->stream));
            NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_split_reduce<float, float>, dim3(ceil_div(mb, nb::kBlock)), block, rargs, 0, s->stream));
        }
        NB_HIP(s, hipLaunchKernel((const void*)&nb::nb_spl_rows<>, dim3(ceil_div(mb, nb::kBlock / lanes)), block, gargs, 0, s->stream));
        if (int rc = stage_out(s, dev, {&lst}, false, done, mb)) return rc;
        done += mb;
    }
    return stage_out(s, dev, {&out[0], &out[1], &out[2], &out[3], &cnt}, true, 0, m);
}

extern "C++" bool nbi::ac_fused(const nb_sim* s) { return s->ac && !s->ac_two_calls && spl_shape_is_splits(s, s->ac_cap, 4u); }

int nb_neighbor_scheme_fused(nb_sim* s, int* fused)
{
    if (!s || !fused) return qfail(s, NB_ERR_INVALID, "nb_neighbor_scheme_fused", !s ? "null handle" : "fused is NULL");
    *fused = nbi::ac_fused(s) ? 1 : 0;
    return NB_OK;
}

int nb_split_lists(nb_sim* s, const nb_split_lists_request* req) { return nbi::split_lists(s, req, s ? s->n : 0u, "nb_split_lists"); }

int nb_split_lists_shape(nb_sim* s, uint32_t m, uint32_t cap, uint32_t* batch, uint32_t* chunks, uint32_t* j_per_chunk, uint32_t* rows_per_workgroup)
{
    if (int rc = shape_begin(s, "nb_split_lists_shape", m, bad_cap(cap))) return rc;
    uint32_t b, c, per;
    spl_shape(s, m, cap, s->n, s->hermite ? 4u : 2u, &b, &c, &per);      // (a Hermite handle: the shape of a request with the jerk pair)
    if (rows_per_workgroup) *rows_per_workgroup = split_rows(s);
    return shape_put(b, c, per, batch, chunks, j_per_chunk);
}

/* ---- viewer frame feed -------------------------------------------------------------------- */

int nb_frame_request(nb_sim* s)
{
    if (!s) return NB_ERR_INVALID;
    if (!s->uploaded) return fail(s, NB_ERR_STATE, "nb_frame_request: nothing uploaded yet");
    NB_HIP(s, hipSetDevice(s->device));
    if (int rc = finish_gather(s)) return rc;     // other ranks' rows must have landed
    if (!s->frame_stream) {
        // all or nothing: the stream is only published once every slot has its buffers and events -- a failed
        // allocation (4 x 20*n bytes pinned + device) returns an error and leaves the handle without a frame feed,
        // so that a later request starts over instead of packing into null buffers
        hipStream_t fs = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&fs, hipStreamNonBlocking);
        int slot = 0;
        for (auto& f : s->frame) {
            if (e != hipSuccess) break;
#ifdef NB_TUNING    // calibration / test build only: fail the k-th slot's allocation (tests/test_round3_gpu.py)
            if (const char* inj = getenv("NB_TEST_FAIL_FRAME_SLOT")) { if (atoi(inj) == slot) { e = hipErrorOutOfMemory; break; } }
#endif
            ++slot; (void)slot;
            // one allocation per side (bodies[4n] then speed[n]): ONE device-to-host copy per frame
            e = hipHostMalloc((void**)&f.h_bodies, sizeof(float) * 5 * s->n, hipHostMallocDefault);
            if (e != hipSuccess) break;
            f.h_speed = f.h_bodies + (size_t)4 * s->n;
            memset(f.h_speed, 0, sizeof(float) * s->n);
            e = hipMalloc((void**)&f.d_bodies, sizeof(float) * 5 * s->n);
            if (e != hipSuccess) break;
            f.d_speed = f.d_bodies + (size_t)4 * s->n;
            e = hipMemsetAsync(f.d_speed, 0, sizeof(float) * s->n, s->stream);   // ordered before the pack kernel
            if (e == hipSuccess) e = hipEventCreate(&f.packed);     // stamped by hipExtLaunchKernel
            if (e == hipSuccess) e = hipEventCreateWithFlags(&f.landed, hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s->stream);       // the memsets above
            s->frame_stream = fs;                        // free_frames destroys it with the partly built slots
            free_frames(s);
            return fail(s, e == hipErrorOutOfMemory ? NB_ERR_NOMEM : NB_ERR_HIP,
                        std::string("nb_frame_request: cannot set up the frame slots: ") + hipGetErrorString(e));
        }
        s->frame_stream = fs;
    }
    nb_frame_slot& f = s->frame[s->frame_next];
    if (!f.h_bodies || !f.d_bodies || !f.packed || !f.landed) return fail(s, NB_ERR_STATE, "nb_frame_request: frame slot is not initialised");
    // the host copy issued from this slot kFrameSlots requests ago must have finished reading its
    // staging buffer (normally long done; a host that runs further ahead than that is held back
    // here, on the host side); the step stream itself never waits for a copy
    if (f.in_flight) NB_HIP(s, hipEventSynchronize(f.landed));
    // the "packed" event rides on the pack kernel's own completion signal (hipExtLaunchKernel):
    // no marker packet on the step stream, so the next step's kernel is not held behind one
    {
        dim3 grid(ceil_div(s->n, nb::kBlock)), block(nb::kBlock);
        const void* b = s->bodies[s->cur];
        const void* v = s->vel;
        uint32_t n = s->n, sb = s->sb, sc = s->sc;
        float4* ob = (float4*)f.d_bodies;
        float* os = f.d_speed;
        void* args[] = {&b, &v, &n, &sb, &sc, &ob, &os};
        const void* fn = s->f64 ? (const void*)&nb::nb_frame_pack<double> : (const void*)&nb::nb_frame_pack<float>;
        NB_HIP(s, hipExtLaunchKernel(fn, grid, block, args, 0, s->stream, nullptr, f.packed, 0));
    }
    NB_HIP(s, hipStreamWaitEvent(s->frame_stream, f.packed, 0));
    NB_HIP(s, hipMemcpyAsync(f.h_bodies, f.d_bodies, sizeof(float) * 5 * s->n, hipMemcpyDeviceToHost, s->frame_stream));
    NB_HIP(s, hipEventRecord(f.landed, s->frame_stream));
    f.step = s->steps_done;
    f.in_flight = true; f.valid = true;
    s->frame_latest = s->frame_next;
    s->frame_next = (s->frame_next + 1) % nb_sim::kFrameSlots;
    return NB_OK;
}

int nb_frame_acquire(nb_sim* s, int wait, const float** bodies, const float** speed, uint64_t* step_index)
{
    if (!s) return NB_ERR_INVALID;
    if (s->frame_latest < 0) return fail(s, NB_ERR_STATE, "nb_frame_acquire: nb_frame_request has not been called");
    NB_HIP(s, hipSetDevice(s->device));
    int pick = -1;
    for (int k = 0; k < nb_sim::kFrameSlots && pick < 0; ++k) {          // newest first
        const int idx = (s->frame_latest - k + nb_sim::kFrameSlots) % nb_sim::kFrameSlots;
        nb_frame_slot& f = s->frame[idx];
        if (!f.valid) continue;
        if (f.in_flight) {
            if (wait && k == 0) NB_HIP(s, hipEventSynchronize(f.landed));
            const hipError_t q = hipEventQuery(f.landed);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); continue; }
            if (q != hipSuccess) return fail(s, NB_ERR_HIP, std::string("nb_frame_acquire: ") + hipGetErrorString(q));
            f.in_flight = false;
        }
        pick = idx;
    }
    if (pick < 0) return NB_NOT_READY;
    const nb_frame_slot& f = s->frame[pick];
    if (bodies) *bodies = f.h_bodies;
    if (speed) *speed = f.h_speed;
    if (step_index) *step_index = f.step;
    return NB_OK;
}

}  // extern "C"
