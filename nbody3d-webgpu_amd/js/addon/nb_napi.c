/*
 * nb_napi.c -- raw N-API binding of include/nbody3d_hip.h for Node.js.
 *
 * The reference's host side is browser JavaScript talking to WebGPU
 * (/root/reference nbody3d.js:136-521).  This addon is the thin FFI that lets
 * the same JavaScript-side calls reach the HIP engine: typed arrays are passed
 * by pointer (napi_get_typedarray_info, zero copy on the JS side), every C
 * status code becomes a thrown Error carrying nb_last_error().
 *
 * Built with plain gcc against /usr/include/node (no node-gyp, no network):
 *   gcc -O2 -fPIC -shared -I/usr/include/node -o nb_napi.node nb_napi.c -ldl
 * The engine library is dlopen()ed at load(path) time, so the addon itself
 * loads on a machine without ROCm and reports that as an ordinary error.
 */
#define NAPI_VERSION 6
#include <node_api.h>

#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/nbody3d_hip.h"
#include "../../../include/nbody3d_hip_plan.h"

/* ---- engine entry points, resolved at load() ---------------------------- */
static void *g_lib;
static uint32_t (*p_abi_version)(void);
static int (*p_device_count)(void);
static int (*p_create)(const nb_config *, nb_sim **);
static void (*p_destroy)(nb_sim *);
static int (*p_upload)(nb_sim *, const void *, const void *, const void *);
static int (*p_set_params)(nb_sim *, double, double);
static int (*p_step)(nb_sim *, uint32_t);
static int (*p_download)(nb_sim *, void *, void *, void *);
static int (*p_sync)(nb_sim *);
static const char *(*p_last_error)(nb_sim *);
static int (*p_enable_timing)(nb_sim *, int);
static int (*p_kernel_times)(nb_sim *, double *, double *, uint32_t *);
static const char *(*p_variant_name)(nb_sim *);
static int (*p_diagnostics)(nb_sim *, double *);
static int (*p_multi_create)(const nb_config *, uint32_t, const int32_t *, nb_multi **);
static void (*p_multi_destroy)(nb_multi *);
static int (*p_multi_upload)(nb_multi *, const void *, const void *, const void *);
static int (*p_multi_set_params)(nb_multi *, double, double);
static int (*p_multi_step)(nb_multi *, uint32_t);
static int (*p_multi_download)(nb_multi *, void *, void *, void *);
static int (*p_multi_sync)(nb_multi *);
static const char *(*p_multi_last_error)(nb_multi *);
static const char *(*p_multi_variant_name)(nb_multi *);
static int (*p_multi_diagnostics)(nb_multi *, double *);
static int (*p_multi_set_collective)(nb_multi *, int);
static int (*p_multi_collective_info)(nb_multi *, int *, int *, int *);
static int (*p_step_times)(nb_sim *, double *, double *, double *, uint32_t *);
static int (*p_step_times2)(nb_sim *, nb_step_timing *);
static int (*p_frame_request)(nb_sim *);
static int (*p_frame_acquire)(nb_sim *, int, const float **, const float **, uint64_t *);
static int (*p_plan_query)(const nb_config *, int, double, nb_plan_info *, uint32_t *, uint32_t);
static int (*p_field_eval)(nb_sim *, const nb_field_request *);
static int (*p_multi_field_eval)(nb_multi *, const nb_field_request *);
static int (*p_download_jerk)(nb_sim *, void *);                        /* the Hermite additions within ABI 2.4: optional symbols */
static int (*p_upload_derivs)(nb_sim *, const void *, const void *);
static int (*p_set_hermite_order)(nb_sim *, uint32_t);                  /* the 6th-order scheme, also within ABI 2.4: optional symbols */
static int (*p_hermite_order)(nb_sim *, uint32_t *);
static int (*p_download_snap)(nb_sim *, void *, void *);
static int (*p_upload_derivs6)(nb_sim *, const void *, const void *, const void *, const void *);
static int (*p_set_block_steps6)(nb_sim *, const nb_block_steps *);     /* block steps on order-6 handles (round 21): optional */
static int (*p_set_start6)(nb_sim *, uint32_t);                         /* the start mode of order-6 handles (round 22): optional */
static int (*p_start6)(nb_sim *, uint32_t *);
static int (*p_set_pass_precision)(nb_sim *, uint32_t);                 /* the mixed-precision pass of f64 Hermite handles (round 23): optional */
static int (*p_pass_precision)(nb_sim *, uint32_t *);
static int (*p_set_pass_guard)(nb_sim *, double);                       /* the guard radius of the mixed pass (round 24): optional */
static int (*p_pass_guard)(nb_sim *, double *);
static int (*p_set_block_steps)(nb_sim *, const nb_block_steps *);      /* block time steps, also within ABI 2.4: optional symbols */
static int (*p_block_stats)(nb_sim *, struct nb_block_stats *, int);
static int (*p_set_block_batch)(nb_sim *, const nb_block_batch *);      /* batched block steps (round 25): optional */
static int (*p_block_batch_stats)(nb_sim *, struct nb_block_batch_stats *, int);
static int (*p_set_block_batch6)(nb_sim *, const nb_block_batch *);     /* ... on order-6 handles (round 26): optional */
static int (*p_set_block_batch_mixed)(nb_sim *, const nb_block_batch *);     /* ... on mixed-precision handles (round 27): optional */
static int (*p_set_block_batch_watch)(nb_sim *, const nb_block_batch *);     /* ... on watched handles (round 29): optional */
static int (*p_set_encounter_watch)(nb_sim *, const nb_encounter_watch *);     /* the encounter watch of block steps (round 28): optional */
static int (*p_encounter_stats)(nb_sim *, struct nb_encounter_stats *, int);
static int (*p_download_encounters)(nb_sim *, void *, uint32_t *, double *, uint32_t *);
static int (*p_upload_encounters)(nb_sim *, const void *, const uint32_t *, const double *, const uint32_t *);
static int (*p_reset_encounters)(nb_sim *);
static int (*p_download_levels)(nb_sim *, uint8_t *);
static int (*p_upload_levels)(nb_sim *, const uint8_t *);
static int (*p_neighbors)(nb_sim *, const nb_neighbor_request *);       /* neighbour queries, also within ABI 2.4: optional symbols */
static int (*p_multi_neighbors)(nb_multi *, const nb_neighbor_request *);
static int (*p_neighbor_lists)(nb_sim *, const nb_neighbor_list_request *);       /* neighbour lists, likewise: optional symbols */
static int (*p_multi_neighbor_lists)(nb_multi *, const nb_neighbor_list_request *);
static int (*p_knn)(nb_sim *, const nb_knn_request *);                              /* k nearest neighbours, likewise: optional symbols */
static int (*p_multi_knn)(nb_multi *, const nb_knn_request *);
static int (*p_list_force)(nb_sim *, const nb_list_force_request *);                /* forces over neighbour rows, likewise: optional symbols */
static int (*p_multi_list_force)(nb_multi *, const nb_list_force_request *);
static int (*p_split_force)(nb_sim *, const nb_split_force_request *);              /* regular + irregular force+jerk in one pass, likewise */
static int (*p_multi_split_force)(nb_multi *, const nb_split_force_request *);
static int (*p_set_neighbor_scheme)(nb_sim *, const nb_neighbor_scheme *);          /* the Ahmad-Cohen neighbour scheme, likewise: optional symbols */
static int (*p_neighbor_scheme_stats)(nb_sim *, struct nb_neighbor_scheme_stats *, int);
static int (*p_download_neighbor_scheme)(nb_sim *, void *, void *, void *, void *, uint32_t *, uint32_t *);
static int (*p_set_neighbor_adapt)(nb_sim *, const nb_neighbor_adapt *);            /* its radii that follow a target count and its checkpoint, likewise */
static int (*p_neighbor_adapt_stats)(nb_sim *, struct nb_neighbor_adapt_stats *, int);
static int (*p_download_neighbor_radii)(nb_sim *, void *, void *);
static int (*p_upload_neighbor_scheme)(nb_sim *, const nb_neighbor_checkpoint *);
static int (*p_set_neighbor_levels)(nb_sim *, const nb_neighbor_levels *);         /* block individual irregular steps inside the scheme, likewise */
static int (*p_neighbor_level_stats)(nb_sim *, struct nb_neighbor_level_stats *, int);
static int (*p_download_neighbor_levels)(nb_sim *, uint8_t *);
static int (*p_upload_neighbor_levels)(nb_sim *, const uint8_t *);
static int (*p_split_lists)(nb_sim *, const nb_split_lists_request *);              /* the two sums and the neighbour rows from one pass, likewise */
static int (*p_multi_split_lists)(nb_multi *, const nb_split_lists_request *);
static int (*p_neighbor_scheme_fused)(nb_sim *, int *);
static int (*p_eqm_info)(nb_sim *, int *);                              /* the equal-mass kernels' report, also within ABI 2.4: optional symbol */
static int (*p_eqm_form)(nb_sim *, int *);                              /* which equal-mass form, likewise */

/* one JS handle = a single-device nb_sim or a single-process multi-device nb_multi */
typedef struct { nb_sim *sim; nb_multi *multi; uint32_t n; int f64; uint32_t ac_cap; /* entries per row of the neighbour scheme, 0: off */ } handle_t;

#define CHECK_NAPI(env, call)                                                        \
    do {                                                                             \
        if ((call) != napi_ok) {                                                     \
            napi_throw_error((env), NULL, "N-API call failed: " #call);              \
            return NULL;                                                             \
        }                                                                            \
    } while (0)

static napi_value throw_msg(napi_env env, int code, const char *msg, const char *where)
{
    char buf[768];
    snprintf(buf, sizeof buf, "%s: status %d: %s", where, code, msg ? msg : "");
    char codes[16];
    snprintf(codes, sizeof codes, "NB_%d", code);
    napi_throw_error(env, codes, buf);
    return NULL;
}

static napi_value throw_nb(napi_env env, int code, nb_sim *s, const char *where)
{
    char buf[768];
    const char *msg = p_last_error ? p_last_error(s) : "engine not loaded";
    snprintf(buf, sizeof buf, "%s: status %d: %s", where, code, msg ? msg : "");
    char codes[16];
    snprintf(codes, sizeof codes, "NB_%d", code);
    napi_throw_error(env, codes, buf);
    return NULL;
}

static int need_lib(napi_env env)
{
    if (!g_lib) { napi_throw_error(env, "NB_NOLIB", "libnbody3d_hip.so is not loaded; call load(path) first"); return 0; }
    return 1;
}

static napi_value undefined(napi_env env) { napi_value u; napi_get_undefined(env, &u); return u; }

/* load(path) -> abi version */
static napi_value js_load(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    char path[4096]; size_t len = 0;
    if (argc < 1 || napi_get_value_string_utf8(env, argv[0], path, sizeof path, &len) != napi_ok) {
        napi_throw_type_error(env, NULL, "load(path): path string required"); return NULL;
    }
    if (!g_lib) {
        void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            char buf[4600]; snprintf(buf, sizeof buf, "cannot load HIP engine %s: %s", path, dlerror());
            napi_throw_error(env, "NB_NOLIB", buf); return NULL;
        }
#define SYM(var, name)                                                                            \
    do {                                                                                          \
        *(void **)(&var) = dlsym(h, name);                                                        \
        if (!var) { dlclose(h); napi_throw_error(env, "NB_NOLIB", "missing symbol " name); return NULL; } \
    } while (0)
        SYM(p_abi_version, "nb_abi_version"); SYM(p_device_count, "nb_device_count");
        SYM(p_create, "nb_create"); SYM(p_destroy, "nb_destroy"); SYM(p_upload, "nb_upload");
        SYM(p_set_params, "nb_set_params"); SYM(p_step, "nb_step"); SYM(p_download, "nb_download");
        SYM(p_sync, "nb_sync"); SYM(p_last_error, "nb_last_error"); SYM(p_enable_timing, "nb_enable_timing");
        SYM(p_kernel_times, "nb_kernel_times"); SYM(p_variant_name, "nb_variant_name");
        SYM(p_diagnostics, "nb_diagnostics");
        SYM(p_multi_create, "nb_multi_create"); SYM(p_multi_destroy, "nb_multi_destroy");
        SYM(p_multi_upload, "nb_multi_upload"); SYM(p_multi_set_params, "nb_multi_set_params");
        SYM(p_multi_step, "nb_multi_step"); SYM(p_multi_download, "nb_multi_download");
        SYM(p_multi_sync, "nb_multi_sync"); SYM(p_multi_last_error, "nb_multi_last_error");
        SYM(p_multi_variant_name, "nb_multi_variant_name"); SYM(p_multi_diagnostics, "nb_multi_diagnostics");
        SYM(p_multi_set_collective, "nb_multi_set_collective"); SYM(p_multi_collective_info, "nb_multi_collective_info");
        SYM(p_step_times, "nb_step_times"); SYM(p_step_times2, "nb_step_times2"); SYM(p_frame_request, "nb_frame_request"); SYM(p_frame_acquire, "nb_frame_acquire");
        SYM(p_plan_query, "nb_plan_query");
        SYM(p_field_eval, "nb_field_eval"); SYM(p_multi_field_eval, "nb_multi_field_eval");
#undef SYM
        /* present from the library that has NB_INT_HERMITE4; an older 2.4 library still loads */
        *(void **)(&p_download_jerk) = dlsym(h, "nb_download_jerk");
        *(void **)(&p_upload_derivs) = dlsym(h, "nb_upload_derivs");
        *(void **)(&p_set_hermite_order) = dlsym(h, "nb_set_hermite_order");
        *(void **)(&p_hermite_order) = dlsym(h, "nb_hermite_order");
        *(void **)(&p_download_snap) = dlsym(h, "nb_download_snap");
        *(void **)(&p_upload_derivs6) = dlsym(h, "nb_upload_derivs6");
        *(void **)(&p_set_block_steps) = dlsym(h, "nb_set_block_steps");
        *(void **)(&p_set_block_steps6) = dlsym(h, "nb_set_block_steps6");
        *(void **)(&p_set_start6) = dlsym(h, "nb_set_start6");
        *(void **)(&p_start6) = dlsym(h, "nb_start6");
        *(void **)(&p_set_pass_precision) = dlsym(h, "nb_set_pass_precision");
        *(void **)(&p_pass_precision) = dlsym(h, "nb_pass_precision");
        *(void **)(&p_set_pass_guard) = dlsym(h, "nb_set_pass_guard");
        *(void **)(&p_pass_guard) = dlsym(h, "nb_pass_guard");
        *(void **)(&p_block_stats) = dlsym(h, "nb_block_stats");
        *(void **)(&p_set_block_batch) = dlsym(h, "nb_set_block_batch");
        *(void **)(&p_block_batch_stats) = dlsym(h, "nb_block_batch_stats");
        *(void **)(&p_set_block_batch6) = dlsym(h, "nb_set_block_batch6");
        *(void **)(&p_set_block_batch_mixed) = dlsym(h, "nb_set_block_batch_mixed");
        *(void **)(&p_set_block_batch_watch) = dlsym(h, "nb_set_block_batch_watch");
        *(void **)(&p_set_encounter_watch) = dlsym(h, "nb_set_encounter_watch");
        *(void **)(&p_encounter_stats) = dlsym(h, "nb_encounter_stats");
        *(void **)(&p_download_encounters) = dlsym(h, "nb_download_encounters");
        *(void **)(&p_upload_encounters) = dlsym(h, "nb_upload_encounters");
        *(void **)(&p_reset_encounters) = dlsym(h, "nb_reset_encounters");
        *(void **)(&p_download_levels) = dlsym(h, "nb_download_levels");
        *(void **)(&p_upload_levels) = dlsym(h, "nb_upload_levels");
        *(void **)(&p_neighbors) = dlsym(h, "nb_neighbors");
        *(void **)(&p_multi_neighbors) = dlsym(h, "nb_multi_neighbors");
        *(void **)(&p_neighbor_lists) = dlsym(h, "nb_neighbor_lists");
        *(void **)(&p_multi_neighbor_lists) = dlsym(h, "nb_multi_neighbor_lists");
        *(void **)(&p_knn) = dlsym(h, "nb_knn");
        *(void **)(&p_multi_knn) = dlsym(h, "nb_multi_knn");
        *(void **)(&p_list_force) = dlsym(h, "nb_list_force");
        *(void **)(&p_multi_list_force) = dlsym(h, "nb_multi_list_force");
        *(void **)(&p_split_force) = dlsym(h, "nb_split_force");
        *(void **)(&p_multi_split_force) = dlsym(h, "nb_multi_split_force");
        *(void **)(&p_set_neighbor_scheme) = dlsym(h, "nb_set_neighbor_scheme");
        *(void **)(&p_neighbor_scheme_stats) = dlsym(h, "nb_neighbor_scheme_stats");
        *(void **)(&p_download_neighbor_scheme) = dlsym(h, "nb_download_neighbor_scheme");
        *(void **)(&p_set_neighbor_adapt) = dlsym(h, "nb_set_neighbor_adapt");
        *(void **)(&p_neighbor_adapt_stats) = dlsym(h, "nb_neighbor_adapt_stats");
        *(void **)(&p_download_neighbor_radii) = dlsym(h, "nb_download_neighbor_radii");
        *(void **)(&p_upload_neighbor_scheme) = dlsym(h, "nb_upload_neighbor_scheme");
        *(void **)(&p_set_neighbor_levels) = dlsym(h, "nb_set_neighbor_levels");
        *(void **)(&p_neighbor_level_stats) = dlsym(h, "nb_neighbor_level_stats");
        *(void **)(&p_download_neighbor_levels) = dlsym(h, "nb_download_neighbor_levels");
        *(void **)(&p_upload_neighbor_levels) = dlsym(h, "nb_upload_neighbor_levels");
        *(void **)(&p_split_lists) = dlsym(h, "nb_split_lists");
        *(void **)(&p_multi_split_lists) = dlsym(h, "nb_multi_split_lists");
        *(void **)(&p_neighbor_scheme_fused) = dlsym(h, "nb_neighbor_scheme_fused");
        *(void **)(&p_eqm_info) = dlsym(h, "nb_eqm_info");
        *(void **)(&p_eqm_form) = dlsym(h, "nb_eqm_form");
        g_lib = h;
    }
    if (p_abi_version() != NB_ABI_VERSION) { napi_throw_error(env, "NB_ABI", "ABI version mismatch"); return NULL; }
    napi_value v; CHECK_NAPI(env, napi_create_uint32(env, p_abi_version(), &v)); return v;
}

static napi_value js_device_count(napi_env env, napi_callback_info info)
{
    (void)info;
    if (!need_lib(env)) return NULL;
    napi_value v; CHECK_NAPI(env, napi_create_int32(env, p_device_count(), &v)); return v;
}

static void finalize_handle(napi_env env, void *data, void *hint)
{
    (void)env; (void)hint;
    handle_t *h = (handle_t *)data;
    if (h) {
        if (h->sim && p_destroy) p_destroy(h->sim);
        if (h->multi && p_multi_destroy) p_multi_destroy(h->multi);
        free(h);
    }
}

static int get_u32_prop(napi_env env, napi_value obj, const char *name, uint32_t *out)
{
    bool has = false; napi_value v;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    napi_valuetype t; napi_typeof(env, v, &t);
    if (t != napi_number) return 0;
    double d; napi_get_value_double(env, v, &d);
    *out = (uint32_t)d; return 1;
}

static int get_f64_prop(napi_env env, napi_value obj, const char *name, double *out)
{
    bool has = false; napi_value v;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    napi_valuetype t; napi_typeof(env, v, &t);
    if (t != napi_number) return 0;
    napi_get_value_double(env, v, out); return 1;
}

/* create({n, f64, eps2, device, shardBegin, shardCount, variant, jsplit, flags, shards, collective}) -> external */
/* options object -> nb_config (create and planQuery read the same keys) */
static void read_config(napi_env env, napi_value opts, nb_config *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg; cfg->device = -1;
    uint32_t u; double d;
    if (get_u32_prop(env, opts, "n", &u)) cfg->n = u;
    if (get_u32_prop(env, opts, "f64", &u)) cfg->precision = u ? NB_F64 : NB_F32;
    if (get_f64_prop(env, opts, "eps2", &d)) cfg->eps2 = d;
    if (get_f64_prop(env, opts, "device", &d)) cfg->device = (int32_t)d;
    if (get_u32_prop(env, opts, "shardBegin", &u)) cfg->shard_begin = u;
    if (get_u32_prop(env, opts, "shardCount", &u)) cfg->shard_count = u;
    if (get_u32_prop(env, opts, "variant", &u)) cfg->force_variant = u;
    if (get_u32_prop(env, opts, "jsplit", &u)) cfg->jsplit = u;
    if (get_u32_prop(env, opts, "tile", &u)) cfg->tile = u;
    if (get_u32_prop(env, opts, "flags", &u)) cfg->flags = u;
    if (get_u32_prop(env, opts, "layerBudgetMiB", &u)) cfg->layer_budget_mib = u;
    if (get_u32_prop(env, opts, "integrator", &u)) cfg->integrator = u;     /* nb_integrator: 0 leapfrog, 1 Hermite 4th order */
}

/* planQuery(options) -> {variant, kind, ipl, ls, x, jsplit, jPerSplit, sym, symRows, symLayers, symUnitsPerSweep, symSpillRows, layerBytes}: nb_plan_query -- the launch
 * plan nb_create would build, from host arithmetic alone (options.nCU + options.clockHz given: no GPU needed) */
static napi_value js_plan_query(napi_env env, napi_callback_info info)
{
    if (!need_lib(env)) return NULL;
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "planQuery(options) requires an object"); return NULL; }
    nb_config cfg; read_config(env, argv[0], &cfg);
    uint32_t n_cu = 0; double clock = 0.0;
    get_u32_prop(env, argv[0], "nCU", &n_cu);
    get_f64_prop(env, argv[0], "clockHz", &clock);
    nb_plan_info pi; memset(&pi, 0, sizeof pi); pi.struct_size = sizeof pi;
    int rc = p_plan_query(&cfg, (int)n_cu, clock, &pi, NULL, 0);
    if (rc != NB_OK) return throw_nb(env, rc, NULL, "nb_plan_query");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    CHECK_NAPI(env, napi_create_string_utf8(env, pi.variant, NAPI_AUTO_LENGTH, &v)); napi_set_named_property(env, o, "variant", v);
#define PUT_U32(name, val) do { napi_create_uint32(env, (val), &v); napi_set_named_property(env, o, name, v); } while (0)
    PUT_U32("kind", pi.kind); PUT_U32("ipl", pi.ipl); PUT_U32("ls", pi.ls); PUT_U32("x", pi.x);
    PUT_U32("jsplit", pi.jsplit); PUT_U32("jPerSplit", pi.j_per_split);
    PUT_U32("sym", pi.sym); PUT_U32("symRows", pi.sym_np); PUT_U32("symLayers", pi.sym_layers);
    PUT_U32("symUnitsPerSweep", pi.sym_ups); PUT_U32("symSpillRows", pi.sym_spill_rows);
#undef PUT_U32
    napi_create_double(env, 3.0 * (cfg.precision == NB_F64 ? 8.0 : 4.0) * (double)pi.sym_np * (double)pi.sym_layers, &v);
    napi_set_named_property(env, o, "layerBytes", v);
    return o;
}

static napi_value js_create(napi_env env, napi_callback_info info)
{
    if (!need_lib(env)) return NULL;
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "create(options) requires an object"); return NULL; }
    nb_config cfg; read_config(env, argv[0], &cfg);
    if (cfg.integrator != NB_INT_LEAPFROG && !p_download_jerk) {
        napi_throw_error(env, "NB_1", "create: the loaded library has no Hermite integrator (nb_download_jerk is missing)"); return NULL;
    }
    uint32_t shards = 0, collective = 0;
    get_u32_prop(env, argv[0], "shards", &shards);
    get_u32_prop(env, argv[0], "collective", &collective);   /* 0 peer copies, 1 RCCL (nb_multi_collective) */
    nb_sim *sim = NULL;
    nb_multi *multi = NULL;
    if (shards > 1 || (shards == 1 && collective)) {   /* single-process multi-device: shards round-robin over the visible GPUs */
        cfg.device = -1; cfg.shard_begin = cfg.shard_count = 0;
        int rc = p_multi_create(&cfg, shards, NULL, &multi);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(NULL), "nb_multi_create");
        if (collective) {
            rc = p_multi_set_collective(multi, (int)collective);
            if (rc != NB_OK) {
                char msg[512]; snprintf(msg, sizeof msg, "%s", p_multi_last_error(multi));
                p_multi_destroy(multi);
                return throw_msg(env, rc, msg, "nb_multi_set_collective");
            }
        }
    } else {
        int rc = p_create(&cfg, &sim);
        if (rc != NB_OK) return throw_nb(env, rc, NULL, "nb_create");
    }
    handle_t *h = (handle_t *)calloc(1, sizeof *h);
    if (!h) { if (sim) p_destroy(sim); if (multi) p_multi_destroy(multi); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    h->sim = sim; h->multi = multi; h->n = cfg.n; h->f64 = cfg.precision == NB_F64; h->ac_cap = 0;
    napi_value ext;
    if (napi_create_external(env, h, finalize_handle, NULL, &ext) != napi_ok) {
        finalize_handle(env, h, NULL); napi_throw_error(env, NULL, "napi_create_external failed"); return NULL;
    }
    return ext;
}

static handle_t *get_handle(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || (!((handle_t *)p)->sim && !((handle_t *)p)->multi)) {
        napi_throw_error(env, "NB_1", "invalid or destroyed simulation handle"); return NULL;
    }
    return (handle_t *)p;
}

/* typed array -> pointer; NULL allowed when nullable; checks element type + length */
static int get_array(napi_env env, napi_value v, const handle_t *h, int nullable, void **out, const char *name)
{
    napi_valuetype t; napi_typeof(env, v, &t);
    *out = NULL;
    if (t == napi_null || t == napi_undefined) {
        if (nullable) return 1;
        napi_throw_type_error(env, NULL, name); return 0;
    }
    bool is_ta = false; napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) { napi_throw_type_error(env, NULL, name); return 0; }
    napi_typedarray_type tt; size_t len; void *data; napi_value ab; size_t off;
    if (napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok) { napi_throw_type_error(env, NULL, name); return 0; }
    if ((h->f64 && tt != napi_float64_array) || (!h->f64 && tt != napi_float32_array)) {
        napi_throw_type_error(env, NULL, h->f64 ? "expected Float64Array (f64 simulation)" : "expected Float32Array");
        return 0;
    }
    if (len != (size_t)4 * h->n) {
        char buf[160]; snprintf(buf, sizeof buf, "%s: expected %zu elements (4*n), got %zu", name, (size_t)4 * h->n, len);
        napi_throw_range_error(env, NULL, buf); return 0;
    }
    *out = data; return 1;
}

static napi_value js_upload(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_type_error(env, NULL, "upload(handle, bodies, vel[, accel])"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    void *b, *v, *a = NULL;
    if (!get_array(env, argv[1], h, 0, &b, "bodies must be a typed array of 4*n elements")) return NULL;
    if (!get_array(env, argv[2], h, 0, &v, "vel must be a typed array of 4*n elements")) return NULL;
    if (argc >= 4 && !get_array(env, argv[3], h, 1, &a, "accel must be a typed array of 4*n elements or null")) return NULL;
    if (h->multi) {
        int rc = p_multi_upload(h->multi, b, v, a);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_upload");
        return undefined(env);
    }
    int rc = p_upload(h->sim, b, v, a);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_upload");
    return undefined(env);
}

static napi_value js_set_params(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_type_error(env, NULL, "setParams(handle, dt, G)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    double dt, G;
    if (napi_get_value_double(env, argv[1], &dt) != napi_ok || napi_get_value_double(env, argv[2], &G) != napi_ok) {
        napi_throw_type_error(env, NULL, "dt and G must be numbers"); return NULL;
    }
    if (h->multi) {
        int rc = p_multi_set_params(h->multi, dt, G);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_set_params");
        return undefined(env);
    }
    int rc = p_set_params(h->sim, dt, G);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_params");
    return undefined(env);
}

static napi_value js_step(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "step(handle[, nsteps])"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    uint32_t n = 1;
    if (argc >= 2) { double d; if (napi_get_value_double(env, argv[1], &d) == napi_ok && d >= 0) n = (uint32_t)d; }
    if (h->multi) {
        int rc = p_multi_step(h->multi, n);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_step");
        return undefined(env);
    }
    int rc = p_step(h->sim, n);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_step");
    return undefined(env);
}

static napi_value js_download(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_type_error(env, NULL, "download(handle, bodies|null, vel|null, accel|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    void *b, *v, *a;
    if (!get_array(env, argv[1], h, 1, &b, "bodies: typed array of 4*n elements or null")) return NULL;
    if (!get_array(env, argv[2], h, 1, &v, "vel: typed array of 4*n elements or null")) return NULL;
    if (!get_array(env, argv[3], h, 1, &a, "accel: typed array of 4*n elements or null")) return NULL;
    if (h->multi) {
        int rc = p_multi_download(h->multi, b, v, a);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_download");
        return undefined(env);
    }
    int rc = p_download(h->sim, b, v, a);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download");
    return undefined(env);
}

static napi_value js_sync(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    if (h->multi) {
        int rc = p_multi_sync(h->multi);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_sync");
        return undefined(env);
    }
    int rc = p_sync(h->sim);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_sync");
    return undefined(env);
}

static napi_value js_destroy(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void *p = NULL;
    if (argc && napi_get_value_external(env, argv[0], &p) == napi_ok && p) {
        handle_t *h = (handle_t *)p;
        if (h->sim) { p_destroy(h->sim); h->sim = NULL; }   /* idempotent; finalizer frees the shell */
        if (h->multi) { p_multi_destroy(h->multi); h->multi = NULL; }
    }
    return undefined(env);
}

static napi_value js_enable_timing(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    if (h->multi) { napi_throw_error(env, "NB_1", "per-kernel timing is not available on a multi-device handle"); return NULL; }
    bool on = true; if (argc >= 2) napi_get_value_bool(env, argv[1], &on);
    int rc = p_enable_timing(h->sim, on ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_enable_timing");
    return undefined(env);
}

/* kernelTimes(handle) -> {forceMs, integrateMs, launches} */
static napi_value js_kernel_times(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    if (h->multi) { napi_throw_error(env, "NB_1", "per-kernel timing is not available on a multi-device handle"); return NULL; }
    double f, g; uint32_t c;
    int rc = p_kernel_times(h->sim, &f, &g, &c);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_kernel_times");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_create_double(env, f, &v); napi_set_named_property(env, o, "forceMs", v);
    napi_create_double(env, g, &v); napi_set_named_property(env, o, "integrateMs", v);
    napi_create_uint32(env, c, &v); napi_set_named_property(env, o, "launches", v);
    return o;
}

static napi_value js_variant(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    napi_value v;
    CHECK_NAPI(env, napi_create_string_utf8(env, h->multi ? p_multi_variant_name(h->multi) : p_variant_name(h->sim), NAPI_AUTO_LENGTH, &v));
    return v;
}

/* eqm(handle) -> whether the next force pass runs the equal-mass kernels (nb_eqm_info; false on a multi-device handle or an older library) */
static napi_value js_eqm(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    int eqm = 0;
    if (h->sim && p_eqm_info) {
        int rc = p_eqm_info(h->sim, &eqm);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_eqm_info");
    }
    napi_value v;
    CHECK_NAPI(env, napi_get_boolean(env, eqm != 0, &v));
    return v;
}

/* eqmForm(handle) -> 0 / 1 / 2: the general kernels, the equal-mass kernels, the equal-mass kernels with unit mass product (nb_eqm_form;
 * an older library: nb_eqm_info's 0 / 1) */
static napi_value js_eqm_form(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    int form = 0;
    if (h->sim && (p_eqm_form || p_eqm_info)) {
        int rc = p_eqm_form ? p_eqm_form(h->sim, &form) : p_eqm_info(h->sim, &form);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, p_eqm_form ? "nb_eqm_form" : "nb_eqm_info");
    }
    napi_value v;
    CHECK_NAPI(env, napi_create_int32(env, form, &v));
    return v;
}

/* diagnostics(handle) -> {kinetic, potential, momentum:[3]} */
static napi_value js_diagnostics(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    double out[5];
    if (h->multi) {
        int rcm = p_multi_diagnostics(h->multi, out);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_diagnostics");
    } else {
        int rc = p_diagnostics(h->sim, out);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_diagnostics");
    }
    napi_value o, v, arr;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_create_double(env, out[0], &v); napi_set_named_property(env, o, "kinetic", v);
    napi_create_double(env, out[1], &v); napi_set_named_property(env, o, "potential", v);
    napi_create_array_with_length(env, 3, &arr);
    for (uint32_t i = 0; i < 3; ++i) { napi_create_double(env, out[2 + i], &v); napi_set_element(env, arr, i, v); }
    napi_set_named_property(env, o, "momentum", arr);
    return o;
}


/* stepTimes(handle) -> {forceMs, integrateMs, exchangeMs, launches, symReduceMs, reduceScatterMs, allgatherMs, spanMs}
 * (nb_step_times2; forceMs / exchangeMs keep nb_step_times's meaning: force pass + nb_sym_reduce, every native collective) */
static napi_value js_step_times(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    if (h->multi) { napi_throw_error(env, "NB_1", "per-kernel timing is not available on a multi-device handle"); return NULL; }
    nb_step_timing t;
    memset(&t, 0, sizeof t);
    t.struct_size = sizeof t;
    int rc = p_step_times2(h->sim, &t);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_step_times2");
    const double f = t.force_ms + t.sym_reduce_ms, g = t.integrate_ms, x = t.reduce_scatter_ms + t.allgather_ms;
    const uint32_t c = t.launches;
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_create_double(env, t.sym_reduce_ms, &v); napi_set_named_property(env, o, "symReduceMs", v);
    napi_create_double(env, t.reduce_scatter_ms, &v); napi_set_named_property(env, o, "reduceScatterMs", v);
    napi_create_double(env, t.allgather_ms, &v); napi_set_named_property(env, o, "allgatherMs", v);
    napi_create_double(env, t.span_ms, &v); napi_set_named_property(env, o, "spanMs", v);
    napi_create_double(env, f, &v); napi_set_named_property(env, o, "forceMs", v);
    napi_create_double(env, g, &v); napi_set_named_property(env, o, "integrateMs", v);
    napi_create_double(env, x, &v); napi_set_named_property(env, o, "exchangeMs", v);
    napi_create_uint32(env, c, &v); napi_set_named_property(env, o, "launches", v);
    return o;
}

/* collectiveInfo(handle) -> {mode: 'peer'|'rccl'|'none', nranks, rcclVersion} */
static napi_value js_collective_info(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    int mode = -1, nranks = 0, ver = 0;
    if (h->multi) {
        int rc = p_multi_collective_info(h->multi, &mode, &nranks, &ver);
        if (rc != NB_OK) return throw_msg(env, rc, p_multi_last_error(h->multi), "nb_multi_collective_info");
    }
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_create_string_utf8(env, mode == NB_MULTI_RCCL ? "rccl" : (mode == NB_MULTI_PEER ? "peer" : "none"), NAPI_AUTO_LENGTH, &v);
    napi_set_named_property(env, o, "mode", v);
    napi_create_int32(env, nranks, &v); napi_set_named_property(env, o, "nranks", v);
    napi_create_int32(env, ver, &v); napi_set_named_property(env, o, "rcclVersion", v);
    return o;
}

/* requestFrame(handle): enqueue a viewer snapshot behind the steps issued so far (returns at once) */
static napi_value js_request_frame(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t *h = argc ? get_handle(env, argv[0]) : NULL; if (!h) return NULL;
    if (h->multi) { napi_throw_error(env, "NB_1", "the frame feed is not available on a multi-device handle"); return NULL; }
    int rc = p_frame_request(h->sim);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_frame_request");
    return undefined(env);
}

/* frame(handle, wait, bodiesOut Float32Array(4n), speedOut Float32Array(n)) -> step index, or -1 when
 * wait is false and no frame has landed yet.  Copies out of the engine's pinned frame slot. */
static napi_value js_frame(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 4) { napi_throw_type_error(env, NULL, "frame(handle, wait, bodiesOut, speedOut)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (h->multi) { napi_throw_error(env, "NB_1", "the frame feed is not available on a multi-device handle"); return NULL; }
    bool wait = true; napi_get_value_bool(env, argv[1], &wait);
    void *dst[2]; const size_t want[2] = {(size_t)4 * h->n, (size_t)h->n};
    for (int k = 0; k < 2; ++k) {
        bool is_ta = false; napi_is_typedarray(env, argv[2 + k], &is_ta);
        napi_typedarray_type tt; size_t len = 0; napi_value ab; size_t off;
        if (!is_ta || napi_get_typedarray_info(env, argv[2 + k], &tt, &len, &dst[k], &ab, &off) != napi_ok ||
            tt != napi_float32_array || len != want[k]) {
            napi_throw_type_error(env, NULL, k ? "speedOut must be a Float32Array of n elements" : "bodiesOut must be a Float32Array of 4*n elements");
            return NULL;
        }
    }
    const float *b = NULL, *sp = NULL; uint64_t step = 0;
    int rc = p_frame_acquire(h->sim, wait ? 1 : 0, &b, &sp, &step);
    napi_value v;
    if (rc == NB_NOT_READY) { napi_create_double(env, -1.0, &v); return v; }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_frame_acquire");
    memcpy(dst[0], b, sizeof(float) * want[0]);
    memcpy(dst[1], sp, sizeof(float) * want[1]);
    napi_create_double(env, (double)step, &v);
    return v;
}

/* fieldEval(handle, points|null, firstBody, count, accelOut|null, phiOut|null): nb_field_eval / nb_multi_field_eval.
 * points: typed array of the handle's precision with 4*m elements (x, y, z, ignored) -- or null, and then the points are
 * the bodies [firstBody, firstBody + count) themselves (NB_FIELD_AT_BODIES).  accelOut (4*m) / phiOut (m): typed arrays of the
 * handle's precision, written in place; no copy beyond the engine's own. */
static napi_value js_field_eval(napi_env env, napi_callback_info info)
{
    size_t argc = 6; napi_value argv[6];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_type_error(env, NULL, "fieldEval(handle, points|null, firstBody, count, accelOut|null, phiOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    const napi_typedarray_type want = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[3] = {NULL, NULL, NULL}; size_t len[3] = {0, 0, 0};
    static const int arg_of[3] = {1, 4, 5};
    static const char *const what[3] = {"points", "accelOut", "phiOut"};
    for (int k = 0; k < 3; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "fieldEval: %s must be a %s or null", what[k], h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0;
    napi_get_value_double(env, argv[2], &first); napi_get_value_double(env, argv[3], &count);
    nb_field_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    if (ptr[0]) {
        if (len[0] % 4 != 0 || len[0] / 4 > 0xffffffffu) { napi_throw_range_error(env, NULL, "fieldEval: points must hold 4*m elements"); return NULL; }
        req.m = (uint32_t)(len[0] / 4);
        req.points = ptr[0];
    } else {
        if (!(first >= 0 && first <= 4294967295.0 && count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "fieldEval: firstBody / count out of range"); return NULL; }
        req.flags = NB_FIELD_AT_BODIES;
        req.first_body = (uint32_t)first; req.m = (uint32_t)count;
    }
    if ((ptr[1] && len[1] != (size_t)4 * req.m) || (ptr[2] && len[2] != (size_t)req.m)) {
        napi_throw_range_error(env, NULL, "fieldEval: accelOut must hold 4*m elements and phiOut m"); return NULL;
    }
    req.accel = ptr[1]; req.phi = ptr[2];
    if (h->multi) {
        int rcm = p_multi_field_eval(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_field_eval");
    } else {
        int rc = p_field_eval(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_field_eval");
    }
    return undefined(env);
}

/* neighbors(handle, points|null, firstBody, count, radii|null, radius, indexOut|null, dist2Out|null, countOut|null): nb_neighbors /
 * nb_multi_neighbors.  points (4*m) / radii (m) / dist2Out (m): typed arrays of the handle's precision; indexOut / countOut:
 * Uint32Array of m elements, written in place.  points null: the points are the bodies [firstBody, firstBody + count)
 * themselves (NB_NBR_AT_BODIES). */
static napi_value js_neighbors(napi_env env, napi_callback_info info)
{
    size_t argc = 9; napi_value argv[9];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 9) { napi_throw_type_error(env, NULL, "neighbors(handle, points|null, firstBody, count, radii|null, radius, indexOut|null, dist2Out|null, countOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_neighbors || !p_multi_neighbors) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_neighbors", "nb_neighbors");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[5] = {NULL, NULL, NULL, NULL, NULL}; size_t len[5] = {0, 0, 0, 0, 0};
    static const int arg_of[5] = {1, 4, 6, 7, 8};
    static const int is_u32[5] = {0, 0, 1, 0, 1};
    static const char *const what[5] = {"points", "radii", "indexOut", "dist2Out", "countOut"};
    for (int k = 0; k < 5; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        const napi_typedarray_type want = is_u32[k] ? napi_uint32_array : real;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "neighbors: %s must be a %s or null", what[k], is_u32[k] ? "Uint32Array" : h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0, radius = 0;
    napi_get_value_double(env, argv[2], &first); napi_get_value_double(env, argv[3], &count); napi_get_value_double(env, argv[5], &radius);
    nb_neighbor_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    if (ptr[0]) {
        if (len[0] % 4 != 0 || len[0] / 4 > 0xffffffffu) { napi_throw_range_error(env, NULL, "neighbors: points must hold 4*m elements"); return NULL; }
        req.m = (uint32_t)(len[0] / 4);
        req.points = ptr[0];
    } else {
        if (!(first >= 0 && first <= 4294967295.0 && count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "neighbors: firstBody / count out of range"); return NULL; }
        req.flags = NB_NBR_AT_BODIES;
        req.first_body = (uint32_t)first; req.m = (uint32_t)count;
    }
    for (int k = 1; k < 5; ++k)
        if (ptr[k] && len[k] != (size_t)req.m) { napi_throw_range_error(env, NULL, "neighbors: radii, indexOut, dist2Out and countOut must hold m elements"); return NULL; }
    req.radii = ptr[1]; req.radius = radius;
    req.index = (uint32_t *)ptr[2]; req.dist2 = ptr[3]; req.count = (uint32_t *)ptr[4];
    if (h->multi) {
        int rcm = p_multi_neighbors(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_neighbors");
    } else {
        int rc = p_neighbors(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbors");
    }
    return undefined(env);
}

/* neighborLists(handle, points|null, firstBody, count, radii|null, radius, cap, listOut, countOut|null): nb_neighbor_lists /
 * nb_multi_neighbor_lists.  points (4*m) / radii (m): typed arrays of the handle's precision; listOut: Uint32Array of m*cap
 * elements, countOut: Uint32Array of m elements, written in place.  points null: the points are the bodies [firstBody,
 * firstBody + count) themselves (NB_NBR_AT_BODIES). */
static napi_value js_neighbor_lists(napi_env env, napi_callback_info info)
{
    size_t argc = 9; napi_value argv[9];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 9) { napi_throw_type_error(env, NULL, "neighborLists(handle, points|null, firstBody, count, radii|null, radius, cap, listOut, countOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_neighbor_lists || !p_multi_neighbor_lists) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_neighbor_lists", "nb_neighbor_lists");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[4] = {NULL, NULL, NULL, NULL}; size_t len[4] = {0, 0, 0, 0};
    static const int arg_of[4] = {1, 4, 7, 8};
    static const int is_u32[4] = {0, 0, 1, 1};
    static const char *const what[4] = {"points", "radii", "listOut", "countOut"};
    for (int k = 0; k < 4; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        const napi_typedarray_type want = is_u32[k] ? napi_uint32_array : real;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "neighborLists: %s must be a %s or null", what[k], is_u32[k] ? "Uint32Array" : h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0, radius = 0, cap = 0;
    napi_get_value_double(env, argv[2], &first); napi_get_value_double(env, argv[3], &count); napi_get_value_double(env, argv[5], &radius);
    napi_get_value_double(env, argv[6], &cap);
    if (!(cap >= 0 && cap <= 4294967295.0)) { napi_throw_range_error(env, NULL, "neighborLists: cap out of range"); return NULL; }
    nb_neighbor_list_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    if (ptr[0]) {
        if (len[0] % 4 != 0 || len[0] / 4 > 0xffffffffu) { napi_throw_range_error(env, NULL, "neighborLists: points must hold 4*m elements"); return NULL; }
        req.m = (uint32_t)(len[0] / 4);
        req.points = ptr[0];
    } else {
        if (!(first >= 0 && first <= 4294967295.0 && count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "neighborLists: firstBody / count out of range"); return NULL; }
        req.flags = NB_NBR_AT_BODIES;
        req.first_body = (uint32_t)first; req.m = (uint32_t)count;
    }
    req.cap = (uint32_t)cap;
    if ((ptr[1] && len[1] != (size_t)req.m) || (ptr[3] && len[3] != (size_t)req.m)) { napi_throw_range_error(env, NULL, "neighborLists: radii and countOut must hold m elements"); return NULL; }
    if (ptr[2] && len[2] != (size_t)req.m * (size_t)req.cap) { napi_throw_range_error(env, NULL, "neighborLists: listOut must hold m * cap elements"); return NULL; }
    req.radii = ptr[1]; req.radius = radius;
    req.list = (uint32_t *)ptr[2]; req.count = (uint32_t *)ptr[3];
    if (h->multi) {
        int rcm = p_multi_neighbor_lists(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_neighbor_lists");
    } else {
        int rc = p_neighbor_lists(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbor_lists");
    }
    return undefined(env);
}

/* knn(handle, points|null, firstBody, count, k, indexOut|null, dist2Out|null): nb_knn / nb_multi_knn.  points (4*m): a typed array
 * of the handle's precision; indexOut: Uint32Array, dist2Out: typed array of the handle's precision, m*k elements each, written in
 * place.  points null: the points are the bodies [firstBody, firstBody + count) themselves (NB_NBR_AT_BODIES). */
static napi_value js_knn(napi_env env, napi_callback_info info)
{
    size_t argc = 7; napi_value argv[7];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_type_error(env, NULL, "knn(handle, points|null, firstBody, count, k, indexOut|null, dist2Out|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_knn || !p_multi_knn) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_knn", "nb_knn");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[3] = {NULL, NULL, NULL}; size_t len[3] = {0, 0, 0};
    static const int arg_of[3] = {1, 5, 6};
    static const int is_u32[3] = {0, 1, 0};
    static const char *const what[3] = {"points", "indexOut", "dist2Out"};
    for (int k = 0; k < 3; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        const napi_typedarray_type want = is_u32[k] ? napi_uint32_array : real;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "knn: %s must be a %s or null", what[k], is_u32[k] ? "Uint32Array" : h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0, kk = 0;
    napi_get_value_double(env, argv[2], &first); napi_get_value_double(env, argv[3], &count); napi_get_value_double(env, argv[4], &kk);
    if (!(kk >= 0 && kk <= 4294967295.0)) { napi_throw_range_error(env, NULL, "knn: k out of range"); return NULL; }
    nb_knn_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    if (ptr[0]) {
        if (len[0] % 4 != 0 || len[0] / 4 > 0xffffffffu) { napi_throw_range_error(env, NULL, "knn: points must hold 4*m elements"); return NULL; }
        req.m = (uint32_t)(len[0] / 4);
        req.points = ptr[0];
    } else {
        if (!(first >= 0 && first <= 4294967295.0 && count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "knn: firstBody / count out of range"); return NULL; }
        req.flags = NB_NBR_AT_BODIES;
        req.first_body = (uint32_t)first; req.m = (uint32_t)count;
    }
    req.k = (uint32_t)kk;
    if ((ptr[1] && len[1] != (size_t)req.m * (size_t)req.k) || (ptr[2] && len[2] != (size_t)req.m * (size_t)req.k)) {
        napi_throw_range_error(env, NULL, "knn: indexOut and dist2Out must hold m * k elements"); return NULL;
    }
    req.index = (uint32_t *)ptr[1]; req.dist2 = ptr[2];
    if (h->multi) {
        int rcm = p_multi_knn(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_knn");
    } else {
        int rc = p_knn(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_knn");
    }
    return undefined(env);
}

/* listForce(handle, list, cap, points|null, pointVel|null, firstBody, count|null, accelOut|null, jerkOut|null, phiOut|null):
 * nb_list_force / nb_multi_list_force.  list: Uint32Array of m * cap entries, count: Uint32Array of m elements or null; points / pointVel
 * (4*m) and the outputs (4*m, 4*m, m elements): typed arrays of the handle's precision, the outputs written in place.  points null:
 * row k belongs to body firstBody + k (NB_LISTF_AT_BODIES). */
static napi_value js_list_force(napi_env env, napi_callback_info info)
{
    size_t argc = 10; napi_value argv[10];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 10) { napi_throw_type_error(env, NULL, "listForce(handle, list, cap, points|null, pointVel|null, firstBody, count|null, accelOut|null, jerkOut|null, phiOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_list_force || !p_multi_list_force) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_list_force", "nb_list_force");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL}; size_t len[7] = {0, 0, 0, 0, 0, 0, 0};
    static const int arg_of[7] = {1, 3, 4, 6, 7, 8, 9};
    static const int is_u32[7] = {1, 0, 0, 1, 0, 0, 0};
    static const char *const what[7] = {"list", "points", "pointVel", "count", "accelOut", "jerkOut", "phiOut"};
    for (int k = 0; k < 7; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        const napi_typedarray_type want = is_u32[k] ? napi_uint32_array : real;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "listForce: %s must be a %s or null", what[k], is_u32[k] ? "Uint32Array" : h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double cap = 0, first = 0;
    napi_get_value_double(env, argv[2], &cap); napi_get_value_double(env, argv[5], &first);
    if (!ptr[0] || !(cap >= 1 && cap <= 4294967295.0) || len[0] % (size_t)cap != 0 || len[0] / (size_t)cap > 0xffffffffu || len[0] == 0) {
        napi_throw_range_error(env, NULL, "listForce: list must hold m * cap entries, m >= 1"); return NULL;
    }
    if (!(first >= 0 && first <= 4294967295.0)) { napi_throw_range_error(env, NULL, "listForce: firstBody out of range"); return NULL; }
    nb_list_force_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    req.cap = (uint32_t)cap;
    req.m = (uint32_t)(len[0] / (size_t)cap);
    const size_t m = req.m;
    if ((ptr[1] && len[1] != 4 * m) || (ptr[2] && len[2] != 4 * m) || (ptr[3] && len[3] != m) || (ptr[4] && len[4] != 4 * m) ||
        (ptr[5] && len[5] != 4 * m) || (ptr[6] && len[6] != m)) {
        napi_throw_range_error(env, NULL, "listForce: points, pointVel, accelOut and jerkOut must hold 4*m elements, count and phiOut m"); return NULL;
    }
    if (!ptr[1]) { req.flags = NB_LISTF_AT_BODIES; req.first_body = (uint32_t)first; }
    req.points = ptr[1]; req.point_vel = ptr[2];
    req.list = (const uint32_t *)ptr[0]; req.count = (const uint32_t *)ptr[3];
    req.accel = ptr[4]; req.jerk = ptr[5]; req.phi = ptr[6];
    if (h->multi) {
        int rcm = p_multi_list_force(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_list_force");
    } else {
        int rc = p_list_force(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_list_force");
    }
    return undefined(env);
}

/* splitForce(handle, points|null, pointVel|null, firstBody, m, radii|null, radius, accelIrrOut|null, accelRegOut|null, jerkIrrOut|null,
 * jerkRegOut|null): nb_split_force / nb_multi_split_force.  points / pointVel and the outputs (4*m elements), radii (m elements): typed
 * arrays of the handle's precision, the outputs written in place.  points null: point k is body firstBody + k (NB_SPLIT_AT_BODIES). */
static napi_value js_split_force(napi_env env, napi_callback_info info)
{
    size_t argc = 11; napi_value argv[11];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 11) { napi_throw_type_error(env, NULL, "splitForce(handle, points|null, pointVel|null, firstBody, m, radii|null, radius, accelIrrOut|null, accelRegOut|null, jerkIrrOut|null, jerkRegOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_split_force || !p_multi_split_force) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_split_force", "nb_split_force");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL}; size_t len[7] = {0, 0, 0, 0, 0, 0, 0};
    static const int arg_of[7] = {1, 2, 5, 7, 8, 9, 10};
    static const char *const what[7] = {"points", "pointVel", "radii", "accelIrrOut", "accelRegOut", "jerkIrrOut", "jerkRegOut"};
    for (int k = 0; k < 7; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != real) {
            char buf[160]; snprintf(buf, sizeof buf, "splitForce: %s must be a %s or null", what[k], h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0, radius = 0;
    napi_get_value_double(env, argv[3], &first); napi_get_value_double(env, argv[4], &count); napi_get_value_double(env, argv[6], &radius);
    if (!(first >= 0 && first <= 4294967295.0) || !(count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "splitForce: firstBody / m out of range"); return NULL; }
    nb_split_force_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    req.m = (uint32_t)count;
    const size_t m = req.m;
    if ((ptr[0] && len[0] != 4 * m) || (ptr[1] && len[1] != 4 * m) || (ptr[2] && len[2] != m) || (ptr[3] && len[3] != 4 * m) ||
        (ptr[4] && len[4] != 4 * m) || (ptr[5] && len[5] != 4 * m) || (ptr[6] && len[6] != 4 * m)) {
        napi_throw_range_error(env, NULL, "splitForce: points, pointVel and the outputs must hold 4*m elements, radii m"); return NULL;
    }
    if (!ptr[0]) { req.flags = NB_SPLIT_AT_BODIES; req.first_body = (uint32_t)first; }
    req.points = ptr[0]; req.point_vel = ptr[1]; req.radii = ptr[2]; req.radius = radius;
    req.accel_irr = ptr[3]; req.accel_reg = ptr[4]; req.jerk_irr = ptr[5]; req.jerk_reg = ptr[6];
    if (h->multi) {
        int rcm = p_multi_split_force(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_split_force");
    } else {
        int rc = p_split_force(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_split_force");
    }
    return undefined(env);
}

/* splitLists(handle, points|null, pointVel|null, firstBody, m, radii|null, radius, accelIrrOut|null, accelRegOut|null, jerkIrrOut|null,
 * jerkRegOut|null, cap, listOut, countOut|null): nb_split_lists / nb_multi_split_lists.  As splitForce, and listOut (m * cap) / countOut
 * (m): Uint32Array, written in place. */
static napi_value js_split_lists(napi_env env, napi_callback_info info)
{
    size_t argc = 14; napi_value argv[14];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 14) { napi_throw_type_error(env, NULL, "splitLists(handle, points|null, pointVel|null, firstBody, m, radii|null, radius, accelIrrOut|null, accelRegOut|null, jerkIrrOut|null, jerkRegOut|null, cap, listOut, countOut|null)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (!p_split_lists || !p_multi_split_lists) return throw_msg(env, NB_ERR_STATE, "the loaded library has no nb_split_lists", "nb_split_lists");
    const napi_typedarray_type real = h->f64 ? napi_float64_array : napi_float32_array;
    void *ptr[9] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL}; size_t len[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    static const int arg_of[9] = {1, 2, 5, 7, 8, 9, 10, 12, 13};
    static const int is_u32[9] = {0, 0, 0, 0, 0, 0, 0, 1, 1};
    static const char *const what[9] = {"points", "pointVel", "radii", "accelIrrOut", "accelRegOut", "jerkIrrOut", "jerkRegOut", "listOut", "countOut"};
    for (int k = 0; k < 9; ++k) {
        napi_valuetype vt; napi_typeof(env, argv[arg_of[k]], &vt);
        if (vt == napi_null || vt == napi_undefined) continue;
        bool is_ta = false; napi_is_typedarray(env, argv[arg_of[k]], &is_ta);
        napi_typedarray_type tt; napi_value ab; size_t off;
        const napi_typedarray_type want = is_u32[k] ? napi_uint32_array : real;
        if (!is_ta || napi_get_typedarray_info(env, argv[arg_of[k]], &tt, &len[k], &ptr[k], &ab, &off) != napi_ok || tt != want) {
            char buf[160]; snprintf(buf, sizeof buf, "splitLists: %s must be a %s or null", what[k], is_u32[k] ? "Uint32Array" : h->f64 ? "Float64Array" : "Float32Array");
            napi_throw_type_error(env, NULL, buf); return NULL;
        }
    }
    double first = 0, count = 0, radius = 0, cap = 0;
    napi_get_value_double(env, argv[3], &first); napi_get_value_double(env, argv[4], &count); napi_get_value_double(env, argv[6], &radius);
    napi_get_value_double(env, argv[11], &cap);
    if (!(first >= 0 && first <= 4294967295.0) || !(count >= 0 && count <= 4294967295.0)) { napi_throw_range_error(env, NULL, "splitLists: firstBody / m out of range"); return NULL; }
    if (!(cap >= 1 && cap <= 4096)) { napi_throw_range_error(env, NULL, "splitLists: cap must be in 1 .. 4096"); return NULL; }
    nb_split_lists_request req;
    memset(&req, 0, sizeof req);
    req.struct_size = sizeof req;
    req.m = (uint32_t)count;
    req.cap = (uint32_t)cap;
    const size_t m = req.m;
    if ((ptr[0] && len[0] != 4 * m) || (ptr[1] && len[1] != 4 * m) || (ptr[2] && len[2] != m) || (ptr[3] && len[3] != 4 * m) ||
        (ptr[4] && len[4] != 4 * m) || (ptr[5] && len[5] != 4 * m) || (ptr[6] && len[6] != 4 * m) || !ptr[7] || len[7] != m * (size_t)req.cap ||
        (ptr[8] && len[8] != m)) {
        napi_throw_range_error(env, NULL, "splitLists: points, pointVel and the sums must hold 4*m elements, radii and countOut m, listOut m * cap"); return NULL;
    }
    if (!ptr[0]) { req.flags = NB_SPLIT_AT_BODIES; req.first_body = (uint32_t)first; }
    req.points = ptr[0]; req.point_vel = ptr[1]; req.radii = ptr[2]; req.radius = radius;
    req.accel_irr = ptr[3]; req.accel_reg = ptr[4]; req.jerk_irr = ptr[5]; req.jerk_reg = ptr[6];
    req.list = (uint32_t *)ptr[7]; req.count = (uint32_t *)ptr[8];
    if (h->multi) {
        int rcm = p_multi_split_lists(h->multi, &req);
        if (rcm != NB_OK) return throw_msg(env, rcm, p_multi_last_error(h->multi), "nb_multi_split_lists");
    } else {
        int rc = p_split_lists(h->sim, &req);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_split_lists");
    }
    return undefined(env);
}

/* neighborSchemeFused(handle) -> whether the next list build of the neighbour scheme is one nb_split_lists call (nb_neighbor_scheme_fused;
 * false on a multi-device handle or an older library) */
static napi_value js_neighbor_scheme_fused(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "neighborSchemeFused(handle)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    int fused = 0;
    if (h->sim && p_neighbor_scheme_fused) {
        int rc = p_neighbor_scheme_fused(h->sim, &fused);
        if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbor_scheme_fused");
    }
    napi_value out;
    CHECK_NAPI(env, napi_get_boolean(env, fused != 0, &out));
    return out;
}

/* downloadJerk(handle, jerkOut): nb_download_jerk -- 4*n elements (jx, jy, jz, 0) of a Hermite handle, written in place. */
static napi_value js_download_jerk(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "downloadJerk(handle, jerkOut)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (h->multi || !p_download_jerk) return throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_download_jerk", "nb_download_jerk");
    void *j;
    if (!get_array(env, argv[1], h, 0, &j, "jerkOut must be a typed array of 4*n elements")) return NULL;
    int rc = p_download_jerk(h->sim, j);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download_jerk");
    return undefined(env);
}

/* uploadDerivs(handle, accel, jerk): nb_upload_derivs -- the checkpoint restore of a Hermite handle, after upload(). */
static napi_value js_upload_derivs(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_type_error(env, NULL, "uploadDerivs(handle, accel, jerk)"); return NULL; }
    handle_t *h = get_handle(env, argv[0]); if (!h) return NULL;
    if (h->multi || !p_upload_derivs) return throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_upload_derivs", "nb_upload_derivs");
    void *a, *j;
    if (!get_array(env, argv[1], h, 0, &a, "accel must be a typed array of 4*n elements")) return NULL;
    if (!get_array(env, argv[2], h, 0, &j, "jerk must be a typed array of 4*n elements")) return NULL;
    int rc = p_upload_derivs(h->sim, a, j);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_upload_derivs");
    return undefined(env);
}

/* the single-device handle of an order-6 call, or NULL with an exception pending */
static handle_t *order_handle(napi_env env, napi_value v, const void *sym, const char *where)
{
    handle_t *h = get_handle(env, v); if (!h) return NULL;
    if (h->multi || !sym) { throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_set_hermite_order", where); return NULL; }
    return h;
}

/* setHermiteOrder(handle, order): nb_set_hermite_order -- 4 or 6. */
static napi_value js_set_hermite_order(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setHermiteOrder(handle, order)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_set_hermite_order, "nb_set_hermite_order"); if (!h) return NULL;
    uint32_t order = 0;
    CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &order));
    int rc = p_set_hermite_order(h->sim, order);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_hermite_order");
    return undefined(env);
}

/* hermiteOrder(handle) -> 4 or 6: nb_hermite_order. */
static napi_value js_hermite_order(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "hermiteOrder(handle)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_hermite_order, "nb_hermite_order"); if (!h) return NULL;
    uint32_t order = 0;
    int rc = p_hermite_order(h->sim, &order);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_hermite_order");
    napi_value out;
    CHECK_NAPI(env, napi_create_uint32(env, order, &out));
    return out;
}

/* setStart6(handle, mode): nb_set_start6 -- NB_START6_ZERO (0) or NB_START6_CRACKLE (1). */
static napi_value js_set_start6(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setStart6(handle, mode)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_set_start6, "nb_set_start6"); if (!h) return NULL;
    uint32_t mode = 0;
    CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &mode));
    int rc = p_set_start6(h->sim, mode);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_start6");
    return undefined(env);
}

/* the single-device handle of a pass-precision call, or NULL with an exception pending */
static handle_t *pass_handle(napi_env env, napi_value v, const void *sym, const char *where)
{
    handle_t *h = get_handle(env, v); if (!h) return NULL;
    if (h->multi || !sym) { throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_set_pass_precision", where); return NULL; }
    return h;
}

/* setPassPrecision(handle, mode): nb_set_pass_precision -- NB_PASS_NATIVE (0) or NB_PASS_MIXED (1). */
static napi_value js_set_pass_precision(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setPassPrecision(handle, mode)"); return NULL; }
    handle_t *h = pass_handle(env, argv[0], (const void *)p_set_pass_precision, "nb_set_pass_precision"); if (!h) return NULL;
    uint32_t mode = 0;
    CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &mode));
    int rc = p_set_pass_precision(h->sim, mode);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_pass_precision");
    return undefined(env);
}

/* passPrecision(handle) -> 0 or 1: nb_pass_precision. */
static napi_value js_pass_precision(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "passPrecision(handle)"); return NULL; }
    handle_t *h = pass_handle(env, argv[0], (const void *)p_pass_precision, "nb_pass_precision"); if (!h) return NULL;
    uint32_t mode = 0;
    int rc = p_pass_precision(h->sim, &mode);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_pass_precision");
    napi_value out;
    CHECK_NAPI(env, napi_create_uint32(env, mode, &out));
    return out;
}

/* setPassGuard(handle, rNear): nb_set_pass_guard -- 0 switches the guard off. */
static napi_value js_set_pass_guard(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setPassGuard(handle, rNear)"); return NULL; }
    handle_t *h = pass_handle(env, argv[0], (const void *)p_set_pass_guard, "nb_set_pass_guard"); if (!h) return NULL;
    double r_near = 0.0;
    CHECK_NAPI(env, napi_get_value_double(env, argv[1], &r_near));
    int rc = p_set_pass_guard(h->sim, r_near);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_pass_guard");
    return undefined(env);
}

/* passGuard(handle) -> the guard radius (0: off): nb_pass_guard. */
static napi_value js_pass_guard(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "passGuard(handle)"); return NULL; }
    handle_t *h = pass_handle(env, argv[0], (const void *)p_pass_guard, "nb_pass_guard"); if (!h) return NULL;
    double r_near = 0.0;
    int rc = p_pass_guard(h->sim, &r_near);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_pass_guard");
    napi_value out;
    CHECK_NAPI(env, napi_create_double(env, r_near, &out));
    return out;
}

/* start6(handle) -> 0 or 1: nb_start6. */
static napi_value js_start6(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "start6(handle)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_start6, "nb_start6"); if (!h) return NULL;
    uint32_t mode = 0;
    int rc = p_start6(h->sim, &mode);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_start6");
    napi_value out;
    CHECK_NAPI(env, napi_create_uint32(env, mode, &out));
    return out;
}

/* downloadSnap(handle, snapOut, crackleOut): nb_download_snap -- 4*n elements each, written in place; either may be null. */
static napi_value js_download_snap(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_type_error(env, NULL, "downloadSnap(handle, snapOut, crackleOut)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_download_snap, "nb_download_snap"); if (!h) return NULL;
    void *s, *c;
    if (!get_array(env, argv[1], h, 1, &s, "snapOut must be null or a typed array of 4*n elements")) return NULL;
    if (!get_array(env, argv[2], h, 1, &c, "crackleOut must be null or a typed array of 4*n elements")) return NULL;
    int rc = p_download_snap(h->sim, s, c);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download_snap");
    return undefined(env);
}

/* uploadDerivs6(handle, accel, jerk, snap, crackle): nb_upload_derivs6 -- the checkpoint restore of an order-6 handle, after upload(). */
static napi_value js_upload_derivs6(napi_env env, napi_callback_info info)
{
    size_t argc = 5; napi_value argv[5];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_type_error(env, NULL, "uploadDerivs6(handle, accel, jerk, snap, crackle)"); return NULL; }
    handle_t *h = order_handle(env, argv[0], (const void *)p_upload_derivs6, "nb_upload_derivs6"); if (!h) return NULL;
    void *p[4];
    static const char *const what[4] = {"accel must be a typed array of 4*n elements", "jerk must be a typed array of 4*n elements",
                                        "snap must be a typed array of 4*n elements", "crackle must be a typed array of 4*n elements"};
    for (int k = 0; k < 4; ++k)
        if (!get_array(env, argv[1 + k], h, 0, &p[k], what[k])) return NULL;
    int rc = p_upload_derivs6(h->sim, p[0], p[1], p[2], p[3]);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_upload_derivs6");
    return undefined(env);
}

/* the single-device handle of a block-step call, or NULL with an exception pending */
static handle_t *block_handle(napi_env env, napi_value v, const void *sym, const char *where)
{
    handle_t *h = get_handle(env, v); if (!h) return NULL;
    if (h->multi || !sym) { throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_set_block_steps", where); return NULL; }
    return h;
}

/* setBlockSteps(handle, null) | setBlockSteps(handle, eta, maxLevel, minLevel, frozen): nb_set_block_steps (eta 0 / maxLevel 0: the defaults) */
static napi_value set_block_steps_with(napi_env env, napi_callback_info info, int (*fn)(nb_sim *, const nb_block_steps *), const char *where)
{
    size_t argc = 5; napi_value argv[5];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setBlockSteps(handle, null | eta, maxLevel, minLevel, frozen)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&fn, where); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (t == napi_null || t == napi_undefined) rc = fn(h->sim, NULL);
    else {
        if (argc < 5) { napi_throw_type_error(env, NULL, "setBlockSteps(handle, eta, maxLevel, minLevel, frozen)"); return NULL; }
        nb_block_steps cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg;
        uint32_t u = 0; bool frozen = false;
        CHECK_NAPI(env, napi_get_value_double(env, argv[1], &cfg.eta));
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[2], &u)); cfg.max_level = u;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[3], &u)); cfg.min_level = u;
        CHECK_NAPI(env, napi_get_value_bool(env, argv[4], &frozen));
        cfg.flags = frozen ? NB_BLOCK_FROZEN : 0u;
        rc = fn(h->sim, &cfg);
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, where);
    return undefined(env);
}

static napi_value js_set_block_steps(napi_env env, napi_callback_info info)
{
    return set_block_steps_with(env, info, p_set_block_steps, "nb_set_block_steps");
}

/* setBlockSteps6(handle, null) | setBlockSteps6(handle, eta, maxLevel, minLevel, frozen): nb_set_block_steps6, on an order-6 handle */
static napi_value js_set_block_steps6(napi_env env, napi_callback_info info)
{
    return set_block_steps_with(env, info, p_set_block_steps6, "nb_set_block_steps6");
}

/* blockStats(handle, reset) -> {enabled, outerSteps, blockSteps, bodySteps, clamped, finestLevel} (counts as doubles) */
static napi_value js_block_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "blockStats(handle, reset)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_block_stats, "nb_block_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_block_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_block_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_block_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_get_boolean(env, st.enabled != 0, &v); napi_set_named_property(env, o, "enabled", v);
    napi_create_double(env, (double)st.outer_steps, &v); napi_set_named_property(env, o, "outerSteps", v);
    napi_create_double(env, (double)st.block_steps, &v); napi_set_named_property(env, o, "blockSteps", v);
    napi_create_double(env, (double)st.body_steps, &v); napi_set_named_property(env, o, "bodySteps", v);
    napi_create_double(env, (double)st.clamped, &v); napi_set_named_property(env, o, "clamped", v);
    napi_create_uint32(env, st.finest_level, &v); napi_set_named_property(env, o, "finestLevel", v);
    return o;
}

/* setBlockBatch(handle, null) | setBlockBatch(handle, depth, smallMax): nb_set_block_batch (depth 0: the default; smallMax < 0: the
 * default); setBlockBatch6, setBlockBatchMixed and setBlockBatchWatch likewise through nb_set_block_batch6, nb_set_block_batch_mixed
 * and nb_set_block_batch_watch */
static napi_value set_block_batch_by(napi_env env, napi_callback_info info, int (*fn)(nb_sim *, const nb_block_batch *), const char *sym)
{
    size_t argc = 3; napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setBlockBatch[6](handle, null | depth, smallMax)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&fn, sym); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (t == napi_null || t == napi_undefined) rc = fn(h->sim, NULL);
    else {
        if (argc < 3) { napi_throw_type_error(env, NULL, "setBlockBatch[6](handle, depth, smallMax)"); return NULL; }
        nb_block_batch cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg;
        uint32_t u = 0; double sm = -1.0;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &u)); cfg.depth = u;
        CHECK_NAPI(env, napi_get_value_double(env, argv[2], &sm));
        cfg.small_max = sm < 0.0 ? NB_BLOCK_BATCH_SMALL_DEFAULT : sm > 4294967294.0 ? 0xfffffffeu : (uint32_t)sm;
        rc = fn(h->sim, &cfg);
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, sym);
    return undefined(env);
}
static napi_value js_set_block_batch(napi_env env, napi_callback_info info) { return set_block_batch_by(env, info, p_set_block_batch, "nb_set_block_batch"); }
static napi_value js_set_block_batch6(napi_env env, napi_callback_info info) { return set_block_batch_by(env, info, p_set_block_batch6, "nb_set_block_batch6"); }
static napi_value js_set_block_batch_mixed(napi_env env, napi_callback_info info) { return set_block_batch_by(env, info, p_set_block_batch_mixed, "nb_set_block_batch_mixed"); }
static napi_value js_set_block_batch_watch(napi_env env, napi_callback_info info) { return set_block_batch_by(env, info, p_set_block_batch_watch, "nb_set_block_batch_watch"); }

/* blockBatchStats(handle, reset) -> {enabled, hostWaits, slots, smallSteps, hostSteps, idleSlots} (counts as doubles) */
static napi_value js_block_batch_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "blockBatchStats(handle, reset)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_block_batch_stats, "nb_block_batch_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_block_batch_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_block_batch_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_block_batch_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_get_boolean(env, st.enabled != 0, &v); napi_set_named_property(env, o, "enabled", v);
    napi_create_double(env, (double)st.host_waits, &v); napi_set_named_property(env, o, "hostWaits", v);
    napi_create_double(env, (double)st.slots, &v); napi_set_named_property(env, o, "slots", v);
    napi_create_double(env, (double)st.small_steps, &v); napi_set_named_property(env, o, "smallSteps", v);
    napi_create_double(env, (double)st.host_steps, &v); napi_set_named_property(env, o, "hostSteps", v);
    napi_create_double(env, (double)st.idle_slots, &v); napi_set_named_property(env, o, "idleSlots", v);
    return o;
}

/* a Uint8Array of n elements */
static int get_levels(napi_env env, napi_value v, const handle_t *h, uint8_t **out)
{
    bool is_ta = false; napi_is_typedarray(env, v, &is_ta);
    napi_typedarray_type tt = napi_int8_array; size_t len = 0; void *data = NULL; napi_value ab; size_t off;
    if (!is_ta || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok || tt != napi_uint8_array) {
        napi_throw_type_error(env, NULL, "levels must be a Uint8Array of n elements"); return 0;
    }
    if (len != (size_t)h->n) { napi_throw_range_error(env, NULL, "levels must be a Uint8Array of n elements"); return 0; }
    *out = (uint8_t *)data; return 1;
}

/* downloadLevels(handle, levelsOut): nb_download_levels -- n levels, written in place */
static napi_value js_download_levels(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "downloadLevels(handle, levelsOut)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_download_levels, "nb_download_levels"); if (!h) return NULL;
    uint8_t *lv;
    if (!get_levels(env, argv[1], h, &lv)) return NULL;
    int rc = p_download_levels(h->sim, lv);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download_levels");
    return undefined(env);
}

/* uploadLevels(handle, levels): nb_upload_levels -- the last call of a block-step checkpoint restore */
static napi_value js_upload_levels(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "uploadLevels(handle, levels)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_upload_levels, "nb_upload_levels"); if (!h) return NULL;
    uint8_t *lv;
    if (!get_levels(env, argv[1], h, &lv)) return NULL;
    int rc = p_upload_levels(h->sim, lv);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_upload_levels");
    return undefined(env);
}

/* the single-device handle of a neighbour-scheme call, or NULL with an exception pending */
static handle_t *scheme_handle(napi_env env, napi_value v, const void *sym, const char *where)
{
    handle_t *h = get_handle(env, v); if (!h) return NULL;
    if (h->multi || !sym) { throw_msg(env, NB_ERR_STATE, "needs a single-device Hermite handle and a library with nb_set_neighbor_scheme", where); return NULL; }
    return h;
}

/* a typed array of `want` elements of the given type, or null when nullable */
static int get_typed(napi_env env, napi_value v, napi_typedarray_type type, size_t want, int nullable, void **out, const char *name)
{
    napi_valuetype t; napi_typeof(env, v, &t);
    *out = NULL;
    if (t == napi_null || t == napi_undefined) {
        if (nullable) return 1;
        napi_throw_type_error(env, NULL, name); return 0;
    }
    bool is_ta = false; napi_is_typedarray(env, v, &is_ta);
    napi_typedarray_type tt = napi_int8_array; size_t len = 0; void *data = NULL; napi_value ab; size_t off;
    if (!is_ta || napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off) != napi_ok || tt != type) { napi_throw_type_error(env, NULL, name); return 0; }
    if (len != want) { napi_throw_range_error(env, NULL, name); return 0; }
    *out = data; return 1;
}

/* setNeighborScheme(handle, null) | setNeighborScheme(handle, radius, radii | null, substeps, cap): nb_set_neighbor_scheme (substeps 0 /
 * cap 0: the defaults 8 / 128); radii: n elements of the handle's precision, copied by the call */
static napi_value js_set_neighbor_scheme(napi_env env, napi_callback_info info)
{
    size_t argc = 5; napi_value argv[5];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setNeighborScheme(handle, null | radius, radii, substeps, cap)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_set_neighbor_scheme, "nb_set_neighbor_scheme"); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (argc < 5 && (t == napi_null || t == napi_undefined)) { rc = p_set_neighbor_scheme(h->sim, NULL); if (rc == NB_OK) h->ac_cap = 0; }
    else {
        if (argc < 5) { napi_throw_type_error(env, NULL, "setNeighborScheme(handle, radius, radii, substeps, cap)"); return NULL; }
        nb_neighbor_scheme cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg;
        uint32_t u = 0; void *radii = NULL;
        CHECK_NAPI(env, napi_get_value_double(env, argv[1], &cfg.radius));
        if (!get_typed(env, argv[2], h->f64 ? napi_float64_array : napi_float32_array, h->n, 1, &radii, "radii must be null or a typed array of n elements of the simulation's precision")) return NULL;
        cfg.radii = radii;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[3], &u)); cfg.substeps = u;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[4], &u)); cfg.cap = u;
        rc = p_set_neighbor_scheme(h->sim, &cfg);
        if (rc == NB_OK) h->ac_cap = cfg.cap ? cfg.cap : 128u;
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_neighbor_scheme");
    return undefined(env);
}

/* setEncounterWatch(handle, null) | setEncounterWatch(handle, radius, radii | null, stop): nb_set_encounter_watch; radii: n elements of
 * the handle's precision, copied by the call */
static napi_value js_set_encounter_watch(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setEncounterWatch(handle, null | radius, radii, stop)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_set_encounter_watch, "nb_set_encounter_watch"); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (argc < 4 && (t == napi_null || t == napi_undefined)) rc = p_set_encounter_watch(h->sim, NULL);
    else {
        if (argc < 4) { napi_throw_type_error(env, NULL, "setEncounterWatch(handle, radius, radii, stop)"); return NULL; }
        nb_encounter_watch cfg;
        memset(&cfg, 0, sizeof cfg);
        void *radii = NULL; bool stop = false;
        CHECK_NAPI(env, napi_get_value_double(env, argv[1], &cfg.radius));
        if (!get_typed(env, argv[2], h->f64 ? napi_float64_array : napi_float32_array, h->n, 1, &radii, "radii must be null or a typed array of n elements of the simulation's precision")) return NULL;
        cfg.radii = radii;
        napi_get_value_bool(env, argv[3], &stop);
        cfg.flags = stop ? NB_ENC_STOP : 0u;
        rc = p_set_encounter_watch(h->sim, &cfg);
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_encounter_watch");
    return undefined(env);
}

/* encounterStats(handle, reset) -> {passes, hits, firstTime, stopped, stepsLeft} (counts as doubles) */
static napi_value js_encounter_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "encounterStats(handle, reset)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_encounter_stats, "nb_encounter_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_encounter_stats st;
    memset(&st, 0, sizeof st);
    int rc = p_encounter_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_encounter_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_create_double(env, (double)st.passes, &v); napi_set_named_property(env, o, "passes", v);
    napi_create_double(env, (double)st.hits, &v); napi_set_named_property(env, o, "hits", v);
    napi_create_double(env, st.first_time, &v); napi_set_named_property(env, o, "firstTime", v);
    napi_get_boolean(env, st.stopped != 0, &v); napi_set_named_property(env, o, "stopped", v);
    napi_create_uint32(env, st.steps_left, &v); napi_set_named_property(env, o, "stepsLeft", v);
    return o;
}

/* downloadEncounters(handle, rho2Out, partnerOut, timeOut, countOut) / uploadEncounters(handle, rho2, partner, time, count): the
 * records, n elements each -- rho2 of the handle's precision, partner and count Uint32Array, time Float64Array */
static napi_value encounters_by(napi_env env, napi_callback_info info, int upload)
{
    size_t argc = 5; napi_value argv[5];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 5) { napi_throw_type_error(env, NULL, "downloadEncounters | uploadEncounters(handle, rho2, partner, time, count)"); return NULL; }
    const char *sym = upload ? "nb_upload_encounters" : "nb_download_encounters";
    handle_t *h = block_handle(env, argv[0], upload ? *(void **)&p_upload_encounters : *(void **)&p_download_encounters, sym); if (!h) return NULL;
    void *rho2, *partner, *time, *count;
    if (!get_typed(env, argv[1], h->f64 ? napi_float64_array : napi_float32_array, h->n, 0, &rho2, "rho2 must be a typed array of n elements of the simulation's precision")) return NULL;
    if (!get_typed(env, argv[2], napi_uint32_array, h->n, 0, &partner, "partner must be a Uint32Array of n elements")) return NULL;
    if (!get_typed(env, argv[3], napi_float64_array, h->n, 0, &time, "time must be a Float64Array of n elements")) return NULL;
    if (!get_typed(env, argv[4], napi_uint32_array, h->n, 0, &count, "count must be a Uint32Array of n elements")) return NULL;
    int rc = upload ? p_upload_encounters(h->sim, rho2, (const uint32_t *)partner, (const double *)time, (const uint32_t *)count)
                    : p_download_encounters(h->sim, rho2, (uint32_t *)partner, (double *)time, (uint32_t *)count);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, sym);
    return undefined(env);
}
static napi_value js_download_encounters(napi_env env, napi_callback_info info) { return encounters_by(env, info, 0); }
static napi_value js_upload_encounters(napi_env env, napi_callback_info info) { return encounters_by(env, info, 1); }

/* resetEncounters(handle): nb_reset_encounters */
static napi_value js_reset_encounters(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "resetEncounters(handle)"); return NULL; }
    handle_t *h = block_handle(env, argv[0], *(void **)&p_reset_encounters, "nb_reset_encounters"); if (!h) return NULL;
    int rc = p_reset_encounters(h->sim);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_reset_encounters");
    return undefined(env);
}

/* neighborSchemeStats(handle, reset) -> {enabled, regularSteps, substeps, entries, builds, maxCount, overflowed} (counts as doubles) */
static napi_value js_neighbor_scheme_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "neighborSchemeStats(handle, reset)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_neighbor_scheme_stats, "nb_neighbor_scheme_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_neighbor_scheme_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_neighbor_scheme_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbor_scheme_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_get_boolean(env, st.enabled != 0, &v); napi_set_named_property(env, o, "enabled", v);
    napi_create_double(env, (double)st.regular_steps, &v); napi_set_named_property(env, o, "regularSteps", v);
    napi_create_double(env, (double)st.substeps, &v); napi_set_named_property(env, o, "substeps", v);
    napi_create_double(env, (double)st.entries, &v); napi_set_named_property(env, o, "entries", v);
    napi_create_double(env, (double)st.builds, &v); napi_set_named_property(env, o, "builds", v);
    napi_create_uint32(env, st.max_count, &v); napi_set_named_property(env, o, "maxCount", v);
    napi_create_uint32(env, st.overflowed, &v); napi_set_named_property(env, o, "overflowed", v);
    return o;
}

/* downloadNeighborScheme(handle, accelIrr, jerkIrr, accelReg, jerkReg, list, count): nb_download_neighbor_scheme, written in place; any
 * of the six may be null.  list: Uint32Array of n * cap (the cap the scheme was set with), count: Uint32Array of n */
static napi_value js_download_neighbor_scheme(napi_env env, napi_callback_info info)
{
    size_t argc = 7; napi_value argv[7];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 7) { napi_throw_type_error(env, NULL, "downloadNeighborScheme(handle, accelIrr, jerkIrr, accelReg, jerkReg, list, count)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_download_neighbor_scheme, "nb_download_neighbor_scheme"); if (!h) return NULL;
    void *row[4], *list, *count;
    for (int k = 0; k < 4; ++k)
        if (!get_array(env, argv[1 + k], h, 1, &row[k], "accelIrr / jerkIrr / accelReg / jerkReg must be null or typed arrays of 4*n elements")) return NULL;
    if (!get_typed(env, argv[5], napi_uint32_array, (size_t)h->n * h->ac_cap, 1, &list, "list must be null or a Uint32Array of n * cap elements")) return NULL;
    if (!get_typed(env, argv[6], napi_uint32_array, h->n, 1, &count, "count must be null or a Uint32Array of n elements")) return NULL;
    int rc = p_download_neighbor_scheme(h->sim, row[0], row[1], row[2], row[3], (uint32_t *)list, (uint32_t *)count);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download_neighbor_scheme");
    return undefined(env);
}

/* setNeighborAdapt(handle, null) | setNeighborAdapt(handle, target, growMax, maxRebuilds, radiusMin, radiusMax): nb_set_neighbor_adapt
 * (growMax 0 / maxRebuilds 0: the defaults cbrt(2) / 4; radiusMin / radiusMax 0: none) */
static napi_value js_set_neighbor_adapt(napi_env env, napi_callback_info info)
{
    size_t argc = 6; napi_value argv[6];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setNeighborAdapt(handle, null | target, growMax, maxRebuilds, radiusMin, radiusMax)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_set_neighbor_adapt, "nb_set_neighbor_adapt"); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (argc < 6 && (t == napi_null || t == napi_undefined)) rc = p_set_neighbor_adapt(h->sim, NULL);
    else {
        if (argc < 6) { napi_throw_type_error(env, NULL, "setNeighborAdapt(handle, target, growMax, maxRebuilds, radiusMin, radiusMax)"); return NULL; }
        nb_neighbor_adapt cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg;
        uint32_t u = 0;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &u)); cfg.target = u;
        CHECK_NAPI(env, napi_get_value_double(env, argv[2], &cfg.grow_max));
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[3], &u)); cfg.max_rebuilds = u;
        CHECK_NAPI(env, napi_get_value_double(env, argv[4], &cfg.radius_min));
        CHECK_NAPI(env, napi_get_value_double(env, argv[5], &cfg.radius_max));
        rc = p_set_neighbor_adapt(h->sim, &cfg);
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_neighbor_adapt");
    return undefined(env);
}

/* neighborAdaptStats(handle, reset) -> {enabled, rebuilds, rowsShrunk, lastRebuilds} (counts as doubles) */
static napi_value js_neighbor_adapt_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "neighborAdaptStats(handle, reset)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_neighbor_adapt_stats, "nb_neighbor_adapt_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_neighbor_adapt_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_neighbor_adapt_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbor_adapt_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_get_boolean(env, st.enabled != 0, &v); napi_set_named_property(env, o, "enabled", v);
    napi_create_double(env, (double)st.rebuilds, &v); napi_set_named_property(env, o, "rebuilds", v);
    napi_create_double(env, (double)st.rows_shrunk, &v); napi_set_named_property(env, o, "rowsShrunk", v);
    napi_create_uint32(env, st.last_rebuilds, &v); napi_set_named_property(env, o, "lastRebuilds", v);
    return o;
}

/* downloadNeighborRadii(handle, built, next): nb_download_neighbor_radii, written in place; either may be null.  n elements of the
 * simulation's precision each */
static napi_value js_download_neighbor_radii(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) { napi_throw_type_error(env, NULL, "downloadNeighborRadii(handle, built, next)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_download_neighbor_radii, "nb_download_neighbor_radii"); if (!h) return NULL;
    void *r[2];
    for (int k = 0; k < 2; ++k)
        if (!get_typed(env, argv[1 + k], h->f64 ? napi_float64_array : napi_float32_array, h->n, 1, &r[k], "built / next must be null or typed arrays of n elements of the simulation's precision")) return NULL;
    int rc = p_download_neighbor_radii(h->sim, r[0], r[1]);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_download_neighbor_radii");
    return undefined(env);
}

/* uploadNeighborScheme(handle, accelIrr, jerkIrr, accelReg, jerkReg, list, count, radii | null): nb_upload_neighbor_scheme, the last call
 * of a restore.  The shapes of downloadNeighborScheme; radii: n elements (`next`), null with adaptation off */
static napi_value js_upload_neighbor_scheme(napi_env env, napi_callback_info info)
{
    size_t argc = 8; napi_value argv[8];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 8) { napi_throw_type_error(env, NULL, "uploadNeighborScheme(handle, accelIrr, jerkIrr, accelReg, jerkReg, list, count, radii)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_upload_neighbor_scheme, "nb_upload_neighbor_scheme"); if (!h) return NULL;
    void *row[4], *list, *count, *radii;
    for (int k = 0; k < 4; ++k)
        if (!get_array(env, argv[1 + k], h, 1, &row[k], "accelIrr / jerkIrr / accelReg / jerkReg must be typed arrays of 4*n elements")) return NULL;
    if (!get_typed(env, argv[5], napi_uint32_array, (size_t)h->n * h->ac_cap, 1, &list, "list must be a Uint32Array of n * cap elements")) return NULL;
    if (!get_typed(env, argv[6], napi_uint32_array, h->n, 1, &count, "count must be a Uint32Array of n elements")) return NULL;
    if (!get_typed(env, argv[7], h->f64 ? napi_float64_array : napi_float32_array, h->n, 1, &radii, "radii must be null or a typed array of n elements of the simulation's precision")) return NULL;
    nb_neighbor_checkpoint ck;
    memset(&ck, 0, sizeof ck);
    ck.struct_size = sizeof ck;
    ck.accel_irr = row[0]; ck.jerk_irr = row[1]; ck.accel_reg = row[2]; ck.jerk_reg = row[3];
    ck.list = (const uint32_t *)list; ck.count = (const uint32_t *)count; ck.radii = radii;
    int rc = p_upload_neighbor_scheme(h->sim, &ck);      /* (a missing array is the library's NB_ERR_INVALID) */
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_upload_neighbor_scheme");
    return undefined(env);
}

/* setNeighborLevels(handle, null) | setNeighborLevels(handle, minLevel, eta, frozen): nb_set_neighbor_levels (eta 0: the default 0.02) */
static napi_value js_set_neighbor_levels(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 2) { napi_throw_type_error(env, NULL, "setNeighborLevels(handle, null | minLevel, eta, frozen)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_set_neighbor_levels, "nb_set_neighbor_levels"); if (!h) return NULL;
    napi_valuetype t; napi_typeof(env, argv[1], &t);
    int rc;
    if (argc < 4 && (t == napi_null || t == napi_undefined)) rc = p_set_neighbor_levels(h->sim, NULL);
    else {
        if (argc < 4) { napi_throw_type_error(env, NULL, "setNeighborLevels(handle, minLevel, eta, frozen)"); return NULL; }
        nb_neighbor_levels cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.struct_size = sizeof cfg;
        uint32_t u = 0;
        bool frozen = false;
        CHECK_NAPI(env, napi_get_value_uint32(env, argv[1], &u)); cfg.min_level = u;
        CHECK_NAPI(env, napi_get_value_double(env, argv[2], &cfg.eta));
        CHECK_NAPI(env, napi_get_value_bool(env, argv[3], &frozen));
        cfg.flags = frozen ? NB_NLEV_FROZEN : 0u;
        rc = p_set_neighbor_levels(h->sim, &cfg);
    }
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_set_neighbor_levels");
    return undefined(env);
}

/* neighborLevelStats(handle, reset) -> {enabled, regularSteps, ticks, blockSteps, bodySteps, entries, clamped, finestLevel} (counts as doubles) */
static napi_value js_neighbor_level_stats(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1) { napi_throw_type_error(env, NULL, "neighborLevelStats(handle, reset)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], *(void **)&p_neighbor_level_stats, "nb_neighbor_level_stats"); if (!h) return NULL;
    bool reset = false;
    if (argc > 1) napi_get_value_bool(env, argv[1], &reset);
    struct nb_neighbor_level_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_neighbor_level_stats(h->sim, &st, reset ? 1 : 0);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, "nb_neighbor_level_stats");
    napi_value o, v;
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_get_boolean(env, st.enabled != 0, &v); napi_set_named_property(env, o, "enabled", v);
    napi_create_double(env, (double)st.regular_steps, &v); napi_set_named_property(env, o, "regularSteps", v);
    napi_create_double(env, (double)st.ticks, &v); napi_set_named_property(env, o, "ticks", v);
    napi_create_double(env, (double)st.block_steps, &v); napi_set_named_property(env, o, "blockSteps", v);
    napi_create_double(env, (double)st.body_steps, &v); napi_set_named_property(env, o, "bodySteps", v);
    napi_create_double(env, (double)st.entries, &v); napi_set_named_property(env, o, "entries", v);
    napi_create_double(env, (double)st.clamped, &v); napi_set_named_property(env, o, "clamped", v);
    napi_create_uint32(env, st.finest_level, &v); napi_set_named_property(env, o, "finestLevel", v);
    return o;
}

/* downloadNeighborLevels(handle, levels) / uploadNeighborLevels(handle, levels): a Uint8Array of n elements, written in place / read */
static napi_value js_neighbor_levels_io(napi_env env, napi_callback_info info, int up)
{
    size_t argc = 2; napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *what = up ? "nb_upload_neighbor_levels" : "nb_download_neighbor_levels";
    if (argc < 2) { napi_throw_type_error(env, NULL, up ? "uploadNeighborLevels(handle, levels)" : "downloadNeighborLevels(handle, levels)"); return NULL; }
    handle_t *h = scheme_handle(env, argv[0], up ? *(void **)&p_upload_neighbor_levels : *(void **)&p_download_neighbor_levels, what); if (!h) return NULL;
    void *lev;
    if (!get_typed(env, argv[1], napi_uint8_array, h->n, 0, &lev, "levels must be a Uint8Array of n elements")) return NULL;
    int rc = up ? p_upload_neighbor_levels(h->sim, (const uint8_t *)lev) : p_download_neighbor_levels(h->sim, (uint8_t *)lev);
    if (rc != NB_OK) return throw_nb(env, rc, h->sim, what);
    return undefined(env);
}
static napi_value js_download_neighbor_levels(napi_env env, napi_callback_info info) { return js_neighbor_levels_io(env, info, 0); }
static napi_value js_upload_neighbor_levels(napi_env env, napi_callback_info info) { return js_neighbor_levels_io(env, info, 1); }

static napi_value init_module(napi_env env, napi_value exports)
{
    static const struct { const char *name; napi_callback fn; } fns[] = {
        {"load", js_load}, {"deviceCount", js_device_count}, {"create", js_create}, {"upload", js_upload},
        {"setParams", js_set_params}, {"step", js_step}, {"download", js_download}, {"sync", js_sync},
        {"destroy", js_destroy}, {"enableTiming", js_enable_timing}, {"kernelTimes", js_kernel_times},
        {"variant", js_variant}, {"eqm", js_eqm}, {"eqmForm", js_eqm_form}, {"diagnostics", js_diagnostics}, {"stepTimes", js_step_times},
        {"collectiveInfo", js_collective_info}, {"requestFrame", js_request_frame}, {"frame", js_frame}, {"planQuery", js_plan_query},
        {"fieldEval", js_field_eval}, {"downloadJerk", js_download_jerk}, {"uploadDerivs", js_upload_derivs},
        {"setHermiteOrder", js_set_hermite_order}, {"hermiteOrder", js_hermite_order}, {"downloadSnap", js_download_snap}, {"uploadDerivs6", js_upload_derivs6},
        {"setStart6", js_set_start6}, {"start6", js_start6}, {"setPassPrecision", js_set_pass_precision}, {"passPrecision", js_pass_precision},
        {"setPassGuard", js_set_pass_guard}, {"passGuard", js_pass_guard},
        {"setBlockSteps", js_set_block_steps}, {"setBlockSteps6", js_set_block_steps6}, {"blockStats", js_block_stats}, {"setBlockBatch", js_set_block_batch}, {"setBlockBatch6", js_set_block_batch6}, {"setBlockBatchMixed", js_set_block_batch_mixed}, {"setBlockBatchWatch", js_set_block_batch_watch}, {"blockBatchStats", js_block_batch_stats}, {"downloadLevels", js_download_levels},
        {"setEncounterWatch", js_set_encounter_watch}, {"encounterStats", js_encounter_stats}, {"downloadEncounters", js_download_encounters},
        {"uploadEncounters", js_upload_encounters}, {"resetEncounters", js_reset_encounters},
        {"uploadLevels", js_upload_levels}, {"neighbors", js_neighbors}, {"neighborLists", js_neighbor_lists},
        {"knn", js_knn}, {"listForce", js_list_force}, {"splitForce", js_split_force}, {"splitLists", js_split_lists}, {"neighborSchemeFused", js_neighbor_scheme_fused},
        {"setNeighborScheme", js_set_neighbor_scheme}, {"neighborSchemeStats", js_neighbor_scheme_stats},
        {"downloadNeighborScheme", js_download_neighbor_scheme},
        {"setNeighborAdapt", js_set_neighbor_adapt}, {"neighborAdaptStats", js_neighbor_adapt_stats},
        {"downloadNeighborRadii", js_download_neighbor_radii}, {"uploadNeighborScheme", js_upload_neighbor_scheme},
        {"setNeighborLevels", js_set_neighbor_levels}, {"neighborLevelStats", js_neighbor_level_stats},
        {"downloadNeighborLevels", js_download_neighbor_levels}, {"uploadNeighborLevels", js_upload_neighbor_levels},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; ++i) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
    }
    return exports;
}

NAPI_MODULE(nb_napi, init_module)
