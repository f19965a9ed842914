"""ctypes binding of include/nbody3d_hip.h.

Mirrors the reference's host-side protocol for the hot path (file:line relative
to /root/reference):

    Simulation(n).init(bodies, vel)   nbody3d.js:177-199  (create + writeBuffer)
    sim.step(dt)                      nbody3d.js:470,474-480,489-490
    sim.simulate(k, dt)               k back-to-back frames of the above
    sim.read()                        util.js:163-178     (exportSimulation copies)
    sim.restore(bodies, vel, accel)   util.js:230-244     (importSimulation)
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# NB_ENGINE_LIB: load another build of the same library (the -DNB_TUNING calibration build of csrc/Makefile)
_LIB_PATH = os.environ.get("NB_ENGINE_LIB") or os.path.normpath(os.path.join(_PKG, "..", "csrc", "libnbody3d_hip.so"))

NB_F32, NB_F64 = 0, 1
NB_FLAG_EXT_STREAM = 1
NB_FLAG_LDS_ONLY = 4
NB_FLAG_NO_FUSE = 8
NB_FLAG_POISON = 16
NB_FLAG_JPK_FENCED = 32
NB_FLAG_NO_SYM = 64
NB_FLAG_SYM_SHARD = 128
NB_FLAG_WHOLE_SWEEPS = 256
NB_FLAG_SINGLE_SWEEPS = 512
NB_FLAG_NO_EQM = 1024
NB_FLAG_NO_EQM_POW2 = 2048
NB_FLAG_AC_TWO_CALLS = 4096
NB_RCCL_ID_BYTES = 128
NB_RCCL_OVERLAP = 1
NB_MULTI_PEER, NB_MULTI_RCCL, NB_MULTI_PEER_OVERLAP = 0, 1, 2
NB_NOT_READY = 7
NB_FIELD_AT_BODIES, NB_FIELD_F64, NB_FIELD_DEVICE = 1, 2, 4      # nb_field_request.flags (ABI 2.4)
NB_NBR_AT_BODIES, NB_NBR_DEVICE = 1, 4                           # nb_neighbor_request.flags (added within ABI 2.4)
NB_NBR_NONE = 0xffffffff                                         # the index of "no neighbour"
NB_INT_LEAPFROG, NB_INT_HERMITE4 = 0, 1                          # nb_config.integrator (added within ABI 2.4)
INTEGRATORS = {"leapfrog": NB_INT_LEAPFROG, "hermite4": NB_INT_HERMITE4}
STATUS = {0: "NB_OK", 1: "NB_ERR_INVALID", 2: "NB_ERR_NO_DEVICE", 3: "NB_ERR_HIP",
          4: "NB_ERR_STATE", 5: "NB_ERR_NOMEM", 6: "NB_ERR_COMM", 7: "NB_NOT_READY"}
ABI_VERSION = 2      # NB_ABI_VERSION (major)
ABI_MINOR = 3        # NB_ABI_MINOR this binding was written against


class NBodyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS.get(code, code), msg))
        self.code = code


class nb_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n", C.c_uint32), ("precision", C.c_uint32), ("tile", C.c_uint32),
        ("eps2", C.c_double), ("device", C.c_int32), ("shard_begin", C.c_uint32), ("shard_count", C.c_uint32),
        ("ext_stream", C.c_void_p), ("ext_bodies", C.c_void_p),
        ("force_variant", C.c_uint32), ("jsplit", C.c_uint32), ("flags", C.c_uint32), ("layer_budget_mib", C.c_uint32),
        ("integrator", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


class nb_plan_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_uint32) for k in (
        "kind", "ipl", "ls", "x", "jsplit", "j_per_split", "own_split0", "own_splits",
        "sym", "symw", "sym_rank", "sym_np", "sym_layers", "sym_g0", "sym_g1")] + [
        ("sym_plan", C.c_uint32 * 11), ("tab_len", C.c_uint32), ("variant", C.c_char * 112),
        ("sym_ups", C.c_uint32), ("sym_spill_rows", C.c_uint32), ("sym_rank_plan", C.c_uint32 * 16),
        ("sym_pass", C.c_uint32), ("sym_passes", C.c_uint32), ("sym_pass_k_lo", C.c_uint32), ("sym_pass_k_hi", C.c_uint32),
        ("sym_pass_d0", C.c_uint32), ("sym_local", C.c_uint32)]


class nb_step_timing(C.Structure):          # include/nbody3d_hip.h
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_uint32), ("force_ms", C.c_double), ("sym_reduce_ms", C.c_double),
                ("reduce_scatter_ms", C.c_double), ("integrate_ms", C.c_double), ("allgather_ms", C.c_double),
                ("span_ms", C.c_double), ("reduce_scatters", C.c_uint32), ("allgathers", C.c_uint32)]


class nb_field_request(C.Structure):        # include/nbody3d_hip.h (ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("accel", C.c_void_p), ("phi", C.c_void_p)]


class nb_neighbor_request(C.Structure):     # include/nbody3d_hip.h (neighbour queries, added within ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("radii", C.c_void_p), ("radius", C.c_double),
                ("index", C.c_void_p), ("dist2", C.c_void_p), ("count", C.c_void_p)]


class nb_neighbor_list_request(C.Structure):     # include/nbody3d_hip.h (neighbour lists, added within ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("radii", C.c_void_p), ("radius", C.c_double),
                ("cap", C.c_uint32), ("reserved", C.c_uint32),
                ("list", C.c_void_p), ("count", C.c_void_p), ("index", C.c_void_p), ("dist2", C.c_void_p)]


class nb_knn_request(C.Structure):          # include/nbody3d_hip.h (k nearest neighbours, added within ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("k", C.c_uint32), ("reserved", C.c_uint32),
                ("index", C.c_void_p), ("dist2", C.c_void_p)]


class nb_list_force_request(C.Structure):   # include/nbody3d_hip.h (forces over neighbour rows, added within ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("point_vel", C.c_void_p), ("list", C.c_void_p), ("count", C.c_void_p),
                ("cap", C.c_uint32), ("reserved", C.c_uint32),
                ("accel", C.c_void_p), ("jerk", C.c_void_p), ("phi", C.c_void_p)]


NB_LISTF_AT_BODIES, NB_LISTF_DEVICE = 1, 4


class nb_split_force_request(C.Structure):  # include/nbody3d_hip.h (regular and irregular force+jerk in one pass, added within ABI 2.4)
    _fields_ = [("struct_size", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("first_body", C.c_uint32),
                ("points", C.c_void_p), ("point_vel", C.c_void_p), ("radii", C.c_void_p), ("radius", C.c_double),
                ("accel_irr", C.c_void_p), ("accel_reg", C.c_void_p), ("jerk_irr", C.c_void_p), ("jerk_reg", C.c_void_p)]


NB_SPLIT_AT_BODIES, NB_SPLIT_DEVICE = 1, 4


class nb_split_lists_request(C.Structure):  # include/nbody3d_hip.h (the two sums and the neighbour rows from one pass, added within ABI 2.4)
    _fields_ = nb_split_force_request._fields_ + [("cap", C.c_uint32), ("reserved", C.c_uint32), ("list", C.c_void_p), ("count", C.c_void_p)]


NB_BLOCK_FROZEN = 1


class nb_block_steps(C.Structure):          # include/nbody3d_hip.h (block individual time steps of a Hermite handle)
    _fields_ = [("struct_size", C.c_uint32), ("max_level", C.c_uint32), ("min_level", C.c_uint32), ("flags", C.c_uint32),
                ("eta", C.c_double)]


BLOCK_BATCH_SMALL_DEFAULT = 0xffffffff     # nb_block_batch.small_max: the default (256); 0 itself means "no small steps"


class nb_block_batch(C.Structure):          # include/nbody3d_hip.h (block steps sized on the device, many per host wait)
    _fields_ = [("struct_size", C.c_uint32), ("depth", C.c_uint32), ("small_max", C.c_uint32), ("flags", C.c_uint32)]


NB_ENC_STOP = 1                             # nb_encounter_watch.flags
ENC_NONE = 0xffffffff                       # the partner of a body without a record


class nb_encounter_watch(C.Structure):      # include/nbody3d_hip.h (closest approaches seen inside block steps)
    _fields_ = [("radius", C.c_double), ("radii", C.c_void_p), ("flags", C.c_uint32)]


class nb_encounter_stats(C.Structure):
    _fields_ = [("passes", C.c_uint64), ("hits", C.c_uint64), ("first_time", C.c_double), ("stopped", C.c_uint32),
                ("steps_left", C.c_uint32)]


class nb_block_batch_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("host_waits", C.c_uint64), ("slots", C.c_uint64),
                ("small_steps", C.c_uint64), ("host_steps", C.c_uint64), ("idle_slots", C.c_uint64)]


class nb_block_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("outer_steps", C.c_uint64), ("block_steps", C.c_uint64),
                ("body_steps", C.c_uint64), ("clamped", C.c_uint64), ("finest_level", C.c_uint32), ("reserved", C.c_uint32)]


class nb_neighbor_scheme(C.Structure):      # include/nbody3d_hip.h (the Ahmad-Cohen neighbour scheme of a Hermite handle)
    _fields_ = [("struct_size", C.c_uint32), ("substeps", C.c_uint32), ("cap", C.c_uint32), ("flags", C.c_uint32),
                ("radius", C.c_double), ("radii", C.c_void_p)]


class nb_neighbor_scheme_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("regular_steps", C.c_uint64), ("substeps", C.c_uint64),
                ("entries", C.c_uint64), ("builds", C.c_uint64), ("max_count", C.c_uint32), ("overflowed", C.c_uint32)]


class nb_neighbor_adapt(C.Structure):       # include/nbody3d_hip.h (the scheme's radii follow a target count)
    _fields_ = [("struct_size", C.c_uint32), ("target", C.c_uint32), ("max_rebuilds", C.c_uint32), ("flags", C.c_uint32),
                ("grow_max", C.c_double), ("radius_min", C.c_double), ("radius_max", C.c_double)]


class nb_neighbor_adapt_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("rebuilds", C.c_uint64), ("rows_shrunk", C.c_uint64),
                ("last_rebuilds", C.c_uint32), ("reserved", C.c_uint32)]


class nb_neighbor_checkpoint(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("accel_irr", C.c_void_p), ("jerk_irr", C.c_void_p),
                ("accel_reg", C.c_void_p), ("jerk_reg", C.c_void_p), ("list", C.c_void_p), ("count", C.c_void_p), ("radii", C.c_void_p)]


class nb_neighbor_levels(C.Structure):      # include/nbody3d_hip.h (block individual irregular steps inside the scheme)
    _fields_ = [("struct_size", C.c_uint32), ("min_level", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("eta", C.c_double)]


class nb_neighbor_level_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_uint32), ("regular_steps", C.c_uint64), ("ticks", C.c_uint64),
                ("block_steps", C.c_uint64), ("body_steps", C.c_uint64), ("entries", C.c_uint64), ("clamped", C.c_uint64),
                ("finest_level", C.c_uint32), ("reserved", C.c_uint32)]


NLEV_FROZEN = 1

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
EXCHANGE_WAIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)

# every symbol include/nbody3d_hip.h and include/nbody3d_hip_plan.h declare (tests check the export list)
SYMBOLS = ["nb_abi_version", "nb_device_count", "nb_create", "nb_destroy", "nb_upload", "nb_set_params", "nb_step",
           "nb_download", "nb_sync", "nb_last_error", "nb_device_ptr", "nb_set_exchange",
           "nb_set_exchange_overlapped", "nb_enable_timing",
           "nb_kernel_times", "nb_variant_name", "nb_diagnostics",
           "nb_multi_create", "nb_multi_destroy", "nb_multi_upload", "nb_multi_set_params", "nb_multi_step",
           "nb_multi_download", "nb_multi_sync", "nb_multi_last_error", "nb_multi_variant_name",
           "nb_multi_diagnostics", "nb_multi_set_collective", "nb_multi_collective_info",
           "nb_rccl_unique_id", "nb_rccl_attach", "nb_rccl_detach", "nb_rccl_info",
           "nb_step_times", "nb_step_times2", "nb_integrate_pass", "nb_force_pass", "nb_frame_request", "nb_frame_acquire", "nb_shape_info", "nb_plan_query",
           "nb_abi_minor", "nb_field_eval", "nb_multi_field_eval", "nb_download_jerk", "nb_upload_derivs",
           "nb_set_block_steps", "nb_block_stats", "nb_download_levels", "nb_upload_levels",
           "nb_neighbors", "nb_multi_neighbors", "nb_neighbors_shape", "nb_eqm_info", "nb_eqm_form",
           "nb_neighbor_lists", "nb_multi_neighbor_lists", "nb_neighbor_lists_shape",
           "nb_knn", "nb_multi_knn", "nb_knn_shape",
           "nb_list_force", "nb_multi_list_force", "nb_list_force_shape",
           "nb_split_force", "nb_multi_split_force", "nb_split_force_shape",
           "nb_set_neighbor_scheme", "nb_neighbor_scheme_stats", "nb_download_neighbor_scheme",
           "nb_split_lists", "nb_multi_split_lists", "nb_split_lists_shape", "nb_neighbor_scheme_fused",
           "nb_set_neighbor_adapt", "nb_neighbor_adapt_stats", "nb_download_neighbor_radii", "nb_upload_neighbor_scheme",
           "nb_set_neighbor_levels", "nb_neighbor_level_stats", "nb_download_neighbor_levels", "nb_upload_neighbor_levels",
           "nb_set_hermite_order", "nb_hermite_order", "nb_download_snap", "nb_upload_derivs6",
           "nb_set_block_steps6", "nb_set_start6", "nb_start6", "nb_set_pass_precision", "nb_pass_precision",
           "nb_set_pass_guard", "nb_pass_guard", "nb_set_block_batch", "nb_block_batch_stats", "nb_set_block_batch6",
           "nb_set_block_batch_mixed",
           "nb_set_encounter_watch", "nb_encounter_stats", "nb_download_encounters", "nb_upload_encounters", "nb_reset_encounters",
           "nb_set_block_batch_watch"]

START6_ZERO, START6_CRACKLE = 0, 1      # nb_set_start6
PASS_NATIVE, PASS_MIXED = 0, 1          # nb_set_pass_precision
_PASS_MODES = {"native": PASS_NATIVE, "mixed": PASS_MIXED}

_lib = None


def library_path():
    return _LIB_PATH


def load_library():
    """Loads libnbody3d_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise NBodyError(3, "HIP engine not built: %s is missing (run __graft_entry__.build() or "
                            "make -C nbody3d-webgpu_amd/csrc)" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    vp = C.c_void_p
    L.nb_abi_version.restype = C.c_uint32
    L.nb_abi_minor.restype = C.c_uint32
    L.nb_device_count.restype = C.c_int
    L.nb_create.argtypes = [C.POINTER(nb_config), C.POINTER(vp)]
    L.nb_destroy.argtypes = [vp]
    L.nb_destroy.restype = None
    L.nb_upload.argtypes = [vp, vp, vp, vp]
    L.nb_set_params.argtypes = [vp, C.c_double, C.c_double]
    L.nb_step.argtypes = [vp, C.c_uint32]
    L.nb_download.argtypes = [vp, vp, vp, vp]
    L.nb_sync.argtypes = [vp]
    L.nb_last_error.argtypes = [vp]
    L.nb_last_error.restype = C.c_char_p
    L.nb_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.nb_set_exchange.argtypes = [vp, EXCHANGE_FN, vp]
    L.nb_set_exchange_overlapped.argtypes = [vp, EXCHANGE_FN, EXCHANGE_WAIT_FN, vp]
    L.nb_enable_timing.argtypes = [vp, C.c_int]
    L.nb_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.nb_variant_name.argtypes = [vp]
    L.nb_variant_name.restype = C.c_char_p
    L.nb_diagnostics.argtypes = [vp, C.POINTER(C.c_double)]
    L.nb_multi_create.argtypes = [C.POINTER(nb_config), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(vp)]
    L.nb_multi_destroy.argtypes = [vp]
    L.nb_multi_destroy.restype = None
    L.nb_multi_upload.argtypes = [vp, vp, vp, vp]
    L.nb_multi_set_params.argtypes = [vp, C.c_double, C.c_double]
    L.nb_multi_step.argtypes = [vp, C.c_uint32]
    L.nb_multi_download.argtypes = [vp, vp, vp, vp]
    L.nb_multi_sync.argtypes = [vp]
    L.nb_multi_last_error.argtypes = [vp]
    L.nb_multi_last_error.restype = C.c_char_p
    L.nb_multi_variant_name.argtypes = [vp]
    L.nb_multi_variant_name.restype = C.c_char_p
    L.nb_multi_diagnostics.argtypes = [vp, C.POINTER(C.c_double)]
    L.nb_multi_set_collective.argtypes = [vp, C.c_int]
    L.nb_multi_collective_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.nb_rccl_unique_id.argtypes = [vp]
    L.nb_rccl_attach.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32]
    L.nb_rccl_detach.argtypes = [vp]
    L.nb_rccl_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.nb_step_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_uint32)]
    L.nb_step_times2.argtypes = [vp, C.POINTER(nb_step_timing)]
    L.nb_integrate_pass.argtypes = [vp, C.c_uint32, C.POINTER(C.c_double)]
    L.nb_force_pass.argtypes = [vp, C.c_uint32, C.POINTER(C.c_double)]
    L.nb_shape_info.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4
    L.nb_plan_query.argtypes = [C.POINTER(nb_config), C.c_int, C.c_double, C.POINTER(nb_plan_info), C.POINTER(C.c_uint32), C.c_uint32]
    L.nb_frame_request.argtypes = [vp]
    L.nb_frame_acquire.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                   C.POINTER(C.c_uint64)]
    if L.nb_abi_minor() >= 4:       # an older library of the same major still loads; field() then raises
        L.nb_field_eval.argtypes = [vp, C.POINTER(nb_field_request)]
        L.nb_multi_field_eval.argtypes = [vp, C.POINTER(nb_field_request)]
    if hasattr(L, "nb_download_jerk"):      # the Hermite additions within 2.4: detected by the symbol, not by the minor
        L.nb_download_jerk.argtypes = [vp, vp]
        L.nb_upload_derivs.argtypes = [vp, vp, vp]
    if hasattr(L, "nb_set_block_steps"):    # block time steps, also within 2.4 and detected by the symbol
        L.nb_set_block_steps.argtypes = [vp, C.POINTER(nb_block_steps)]
        L.nb_block_stats.argtypes = [vp, C.POINTER(nb_block_stats), C.c_int]
        L.nb_download_levels.argtypes = [vp, vp]
        L.nb_upload_levels.argtypes = [vp, vp]
    if hasattr(L, "nb_neighbors"):          # neighbour queries, also within 2.4 and detected by the symbol
        L.nb_neighbors.argtypes = [vp, C.POINTER(nb_neighbor_request)]
        L.nb_multi_neighbors.argtypes = [vp, C.POINTER(nb_neighbor_request)]
        L.nb_neighbors_shape.argtypes = [vp, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    if hasattr(L, "nb_neighbor_lists"):     # neighbour lists, also within 2.4 and detected by the symbol
        L.nb_neighbor_lists.argtypes = [vp, C.POINTER(nb_neighbor_list_request)]
        L.nb_multi_neighbor_lists.argtypes = [vp, C.POINTER(nb_neighbor_list_request)]
        L.nb_neighbor_lists_shape.argtypes = [vp, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    if hasattr(L, "nb_knn"):                # k nearest neighbours, also within 2.4 and detected by the symbol
        L.nb_knn.argtypes = [vp, C.POINTER(nb_knn_request)]
        L.nb_multi_knn.argtypes = [vp, C.POINTER(nb_knn_request)]
        L.nb_knn_shape.argtypes = [vp, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    if hasattr(L, "nb_list_force"):         # forces over neighbour rows, also within 2.4 and detected by the symbol
        L.nb_list_force.argtypes = [vp, C.POINTER(nb_list_force_request)]
        L.nb_multi_list_force.argtypes = [vp, C.POINTER(nb_list_force_request)]
        L.nb_list_force_shape.argtypes = [vp, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 2
    if hasattr(L, "nb_split_force"):        # regular and irregular force+jerk in one pass, also within 2.4 and detected by the symbol
        L.nb_split_force.argtypes = [vp, C.POINTER(nb_split_force_request)]
        L.nb_multi_split_force.argtypes = [vp, C.POINTER(nb_split_force_request)]
        L.nb_split_force_shape.argtypes = [vp, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4
    if hasattr(L, "nb_set_neighbor_scheme"):    # the Ahmad-Cohen neighbour scheme, also within 2.4 and detected by the symbol
        L.nb_set_neighbor_scheme.argtypes = [vp, C.POINTER(nb_neighbor_scheme)]
        L.nb_neighbor_scheme_stats.argtypes = [vp, C.POINTER(nb_neighbor_scheme_stats), C.c_int]
        L.nb_download_neighbor_scheme.argtypes = [vp] * 7
    if hasattr(L, "nb_split_lists"):        # the two sums and the neighbour rows from one pass, also within 2.4 and detected by the symbol
        L.nb_split_lists.argtypes = [vp, C.POINTER(nb_split_lists_request)]
        L.nb_multi_split_lists.argtypes = [vp, C.POINTER(nb_split_lists_request)]
        L.nb_split_lists_shape.argtypes = [vp, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4
        L.nb_neighbor_scheme_fused.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "nb_set_neighbor_adapt"):     # radii that follow a target count and the scheme's checkpoint, also within 2.4
        L.nb_set_neighbor_adapt.argtypes = [vp, C.POINTER(nb_neighbor_adapt)]
        L.nb_neighbor_adapt_stats.argtypes = [vp, C.POINTER(nb_neighbor_adapt_stats), C.c_int]
        L.nb_download_neighbor_radii.argtypes = [vp, vp, vp]
        L.nb_upload_neighbor_scheme.argtypes = [vp, C.POINTER(nb_neighbor_checkpoint)]
    if hasattr(L, "nb_set_block_batch"):        # batched block steps, likewise
        L.nb_set_block_batch.argtypes = [vp, C.POINTER(nb_block_batch)]
        L.nb_block_batch_stats.argtypes = [vp, C.POINTER(nb_block_batch_stats), C.c_int]
    if hasattr(L, "nb_set_block_batch6"):       # ... on order-6 handles, likewise
        L.nb_set_block_batch6.argtypes = [vp, C.POINTER(nb_block_batch)]
    if hasattr(L, "nb_set_block_batch_mixed"):  # ... on mixed-precision handles, likewise
        L.nb_set_block_batch_mixed.argtypes = [vp, C.POINTER(nb_block_batch)]
    if hasattr(L, "nb_set_encounter_watch"):    # the encounter watch of block steps, likewise
        L.nb_set_encounter_watch.argtypes = [vp, C.POINTER(nb_encounter_watch)]
        L.nb_encounter_stats.argtypes = [vp, C.POINTER(nb_encounter_stats), C.c_int]
        L.nb_download_encounters.argtypes = [vp, vp, vp, vp, vp]
        L.nb_upload_encounters.argtypes = [vp, vp, vp, vp, vp]
        L.nb_reset_encounters.argtypes = [vp]
    if hasattr(L, "nb_set_block_batch_watch"):  # batched block steps on a watched handle, likewise
        L.nb_set_block_batch_watch.argtypes = [vp, C.POINTER(nb_block_batch)]
    if hasattr(L, "nb_set_neighbor_levels"):    # block individual irregular steps inside the scheme, also within 2.4
        L.nb_set_neighbor_levels.argtypes = [vp, C.POINTER(nb_neighbor_levels)]
        L.nb_neighbor_level_stats.argtypes = [vp, C.POINTER(nb_neighbor_level_stats), C.c_int]
        L.nb_download_neighbor_levels.argtypes = [vp, vp]
        L.nb_upload_neighbor_levels.argtypes = [vp, vp]
    if hasattr(L, "nb_set_hermite_order"):      # the 6th-order scheme on force, jerk and snap, also within 2.4 and detected by the symbol
        L.nb_set_hermite_order.argtypes = [vp, C.c_uint32]
        L.nb_hermite_order.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.nb_download_snap.argtypes = [vp, vp, vp]
        L.nb_upload_derivs6.argtypes = [vp, vp, vp, vp, vp]
    if hasattr(L, "nb_set_block_steps6"):       # block steps on order-6 handles, likewise
        L.nb_set_block_steps6.argtypes = [vp, C.POINTER(nb_block_steps)]
    if hasattr(L, "nb_set_start6"):             # the start mode of order-6 handles, likewise
        L.nb_set_start6.argtypes = [vp, C.c_uint32]
        L.nb_start6.argtypes = [vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "nb_set_pass_precision"):     # the mixed-precision force+jerk pass of f64 Hermite handles, likewise
        L.nb_set_pass_precision.argtypes = [vp, C.c_uint32]
        L.nb_pass_precision.argtypes = [vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "nb_set_pass_guard"):         # the guard radius of the mixed pass, likewise
        L.nb_set_pass_guard.argtypes = [vp, C.c_double]
        L.nb_pass_guard.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(L, "nb_eqm_info"):           # the equal-mass kernels' report, also within 2.4 and detected by the symbol
        L.nb_eqm_info.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "nb_eqm_form"):           # which of the equal-mass forms, likewise
        L.nb_eqm_form.argtypes = [vp, C.POINTER(C.c_int)]
    _lib = L
    return L


def abi_version():
    return load_library().nb_abi_version()


def abi_minor():
    return load_library().nb_abi_minor()


def device_count():
    return load_library().nb_device_count()


def rccl_unique_id():
    """ncclGetUniqueId through the engine: 128 bytes that rank 0 hands to every other rank."""
    L = load_library()
    buf = C.create_string_buffer(NB_RCCL_ID_BYTES)
    rc = L.nb_rccl_unique_id(buf)
    if rc != 0:
        raise NBodyError(rc, L.nb_last_error(None).decode())
    return buf.raw


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _need(symbol, what):
    """``what`` (the caller's name) needs ``symbol``: the queries after nb_field_eval were added within ABI 2.4, one by one."""
    if not hasattr(load_library(), symbol):
        raise NBodyError(1, "%s: the loaded library has no %s" % (what, symbol))


def _rows4(a, dtype, who, what="points"):
    """``a`` as contiguous (m, 4) rows of ``dtype``: (m, 3) gets a fourth column of zeros, a flat array is read as rows."""
    a = np.asarray(a, dtype=dtype)
    if a.ndim == 1:
        a = a.reshape(-1, 3 if a.size % 4 else 4)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError("%s: %s must have shape (m, 3) or (m, 4)" % (who, what))
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((len(a), 1), dtype)], axis=1)
    return np.ascontiguousarray(a)


def _targets(who, req, dtype, points, bodies, at_bodies):
    """The "``bodies=(first, count)`` or ``points``" part of ``who``'s request: sets flags, first_body, points and m (the count of
    the bodies if they are given, else the number of points).  Returns (points array to keep alive | None, count | None).  Both or
    neither of the two: passed on as they are -- the engine's NB_ERR_INVALID names the field."""
    pts = count = None
    if bodies is not None:
        first, count = int(bodies[0]), int(bodies[1])
        if not (0 <= first < 2 ** 32 and 0 <= count < 2 ** 32):
            raise ValueError("%s: bodies=(first, count) out of range" % who)
        req.flags |= at_bodies
        req.first_body, req.m = first, count
    if points is not None:
        pts = _rows4(points, dtype, who)
        if bodies is None:
            req.m = len(pts)
        req.points = _ptr(pts) if len(pts) else None
    return pts, count


def _radii(who, req, dtype, radii):
    """The ``radii`` part of ``who``'s request (after _targets: one radius per point): the array to keep alive, or None."""
    if radii is None:
        return None
    rad = np.ascontiguousarray(radii, dtype=dtype).reshape(-1)
    if len(rad) != req.m:
        raise ValueError("%s: radii must hold one radius per point" % who)
    req.radii = _ptr(rad) if len(rad) else None
    return rad


def _new_request(cls):
    req = cls()
    req.struct_size = C.sizeof(cls)
    return req


def _device_request(cls, flags, at_bodies, m, bodies, points_ptr):
    """What the ``*_device`` methods share: ``bodies=(first, count)`` selects the bodies themselves (``m`` is ignored then)."""
    # (the head of every request, in the structs' order: struct_size, m, flags, first_body, points)
    if bodies is not None:
        return cls(C.sizeof(cls), int(bodies[1]), flags | at_bodies, int(bodies[0]), points_ptr or None)
    return cls(C.sizeof(cls), int(m), flags, 0, points_ptr or None)


def _field_request(n, dtype, points, bodies, accel, phi, f64):
    """The nb_field_request of field(): (request, points array kept alive, accel array | None, phi array | None)."""
    if load_library().nb_abi_minor() < 4:
        raise NBodyError(1, "field(): the loaded library is ABI %d.%d; nb_field_eval needs 2.4" % (abi_version(), abi_minor()))
    req = _new_request(nb_field_request)
    pts, _ = _targets("field()", req, dtype, points, bodies, NB_FIELD_AT_BODIES)
    out_t = np.float64 if (f64 or dtype == np.float64) else np.float32
    if f64:
        req.flags |= NB_FIELD_F64
    a = np.zeros((req.m, 4), out_t) if accel else None
    f = np.zeros((req.m,), out_t) if phi else None
    req.accel = _ptr(a) if a is not None and a.size else None
    req.phi = _ptr(f) if f is not None and f.size else None
    return req, pts, a, f


def _neighbor_request(dtype, points, bodies, radius, radii):
    """The nb_neighbor_request of neighbors(): (request, arrays kept alive, index, dist2, count | None)."""
    _need("nb_neighbors", "neighbors()")
    req = _new_request(nb_neighbor_request)
    pts, _ = _targets("neighbors()", req, dtype, points, bodies, NB_NBR_AT_BODIES)
    rad = _radii("neighbors()", req, dtype, radii)
    if radius is not None:
        req.radius = float(radius)
    index = np.zeros((req.m,), np.uint32)
    dist2 = np.zeros((req.m,), dtype)
    count = np.zeros((req.m,), np.uint32) if (radius is not None or radii is not None) else None
    req.index = _ptr(index) if req.m else None
    req.dist2 = _ptr(dist2) if req.m else None
    req.count = _ptr(count) if count is not None and req.m else None
    return req, (pts, rad), index, dist2, count


def _neighbor_list_request(dtype, points, bodies, radius, radii, cap, nearest):
    """The nb_neighbor_list_request of neighbor_lists(): (request, arrays kept alive, lists, count, index | None, dist2 | None)."""
    _need("nb_neighbor_lists", "neighbor_lists()")
    req = _new_request(nb_neighbor_list_request)
    pts, _ = _targets("neighbor_lists()", req, dtype, points, bodies, NB_NBR_AT_BODIES)
    rad = _radii("neighbor_lists()", req, dtype, radii)
    if radius is not None:
        req.radius = float(radius)
    cap = int(cap)
    if not 0 <= cap < 2 ** 32:
        raise ValueError("neighbor_lists(): cap out of range")
    req.cap = cap
    rows = cap if 1 <= cap <= 4096 else 1              # (an invalid cap is the engine's to refuse: nothing is written then)
    lists = np.zeros((req.m, rows), np.uint32)
    count = np.zeros((req.m,), np.uint32)
    index = np.zeros((req.m,), np.uint32) if nearest else None
    dist2 = np.zeros((req.m,), dtype) if nearest else None
    req.list = _ptr(lists) if req.m else None
    req.count = _ptr(count) if req.m else None
    req.index = _ptr(index) if nearest and req.m else None
    req.dist2 = _ptr(dist2) if nearest and req.m else None
    return req, (pts, rad), lists, count, index, dist2


def _list_force_request(dtype, lists, bodies, points, point_vel, count, accel, jerk, phi):
    """The nb_list_force_request of list_force(): (request, arrays kept alive, accel | None, jerk | None, phi | None)."""
    _need("nb_list_force", "list_force()")
    req = _new_request(nb_list_force_request)
    lists = np.ascontiguousarray(lists, dtype=np.uint32)
    if lists.ndim != 2:
        raise ValueError("list_force(): lists must have shape (m, cap)")
    m, cap = lists.shape
    if not (m < 2 ** 32 and cap < 2 ** 32):
        raise ValueError("list_force(): lists out of range")
    pv = cnt = None
    # (point_vel without a jerk, a cap out of range: passed on as they are -- the engine's NB_ERR_INVALID names the field)
    pts, nb = _targets("list_force()", req, dtype, points, bodies, NB_LISTF_AT_BODIES)
    if nb is not None and nb != m:
        raise ValueError("list_force(): bodies=(first, count) must name one body per row of lists")
    if pts is not None and len(pts) != m:
        raise ValueError("list_force(): points must hold one point per row of lists")
    req.m, req.cap = m, cap
    if point_vel is not None:
        pv = _rows4(point_vel, dtype, "list_force()", "point_vel")
        if len(pv) != m:
            raise ValueError("list_force(): point_vel must hold one velocity per row of lists")
        req.point_vel = _ptr(pv) if m else None
    if count is not None:
        cnt = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
        if len(cnt) != m:
            raise ValueError("list_force(): count must hold one length per row of lists")
        req.count = _ptr(cnt) if m else None
    req.list = _ptr(lists) if lists.size else None
    a = np.zeros((m, 4), dtype) if accel else None
    j = np.zeros((m, 4), dtype) if jerk else None
    f = np.zeros((m,), dtype) if phi else None
    req.accel = _ptr(a) if accel and m else None
    req.jerk = _ptr(j) if jerk and m else None
    req.phi = _ptr(f) if phi and m else None
    return req, (lists, pts, pv, cnt), a, j, f


SPLIT_OUTPUTS = ("accel_irr", "accel_reg", "jerk_irr", "jerk_reg")


def _split_force_request(dtype, points, bodies, point_vel, radius, radii, jerk):
    """The nb_split_force_request of split_force(): (request, arrays kept alive, {output name: (m, 4) array})."""
    _need("nb_split_force", "split_force()")
    req = _new_request(nb_split_force_request)
    if points is None and bodies is None:
        raise ValueError("split_force(): give points or bodies=(first, count)")
    # (both of points / bodies, point_vel without a jerk, no radius at all: passed on as they are -- the engine's NB_ERR_INVALID
    # names the field)
    pts, _ = _targets("split_force()", req, dtype, points, bodies, NB_SPLIT_AT_BODIES)
    m = req.m
    pv = None
    if point_vel is not None:
        pv = _rows4(point_vel, dtype, "split_force()", "point_vel")
        if len(pv) != m:
            raise ValueError("split_force(): point_vel must hold one velocity per point")
        req.point_vel = _ptr(pv) if m else None
    rad = _radii("split_force()", req, dtype, radii)
    req.radius = 0.0 if radius is None else float(radius)
    out = {}
    for name in SPLIT_OUTPUTS[:4 if jerk else 2]:
        out[name] = np.zeros((m, 4), dtype)
        setattr(req, name, _ptr(out[name]) if m else None)
    return req, (pts, pv, rad), out


def _split_lists_request(dtype, points, bodies, point_vel, radius, radii, jerk, cap):
    """The nb_split_lists_request of split_lists(): (request, arrays kept alive, {output name: array}) -- split_force()'s four sums
    plus ``list`` ((m, cap) uint32) and ``count`` ((m,) uint32)."""
    _need("nb_split_lists", "split_lists()")
    req = _new_request(nb_split_lists_request)
    if points is None and bodies is None:
        raise ValueError("split_lists(): give points or bodies=(first, count)")
    pts, _ = _targets("split_lists()", req, dtype, points, bodies, NB_SPLIT_AT_BODIES)
    m = req.m
    pv = None
    if point_vel is not None:
        pv = _rows4(point_vel, dtype, "split_lists()", "point_vel")
        if len(pv) != m:
            raise ValueError("split_lists(): point_vel must hold one velocity per point")
        req.point_vel = _ptr(pv) if m else None
    rad = _radii("split_lists()", req, dtype, radii)
    req.radius = 0.0 if radius is None else float(radius)
    cap = int(cap)
    if not 0 <= cap < 2 ** 32:
        raise ValueError("split_lists(): cap out of range")
    req.cap = cap
    out = {}
    for name in SPLIT_OUTPUTS[:4 if jerk else 2]:
        out[name] = np.zeros((m, 4), dtype)
        setattr(req, name, _ptr(out[name]) if m else None)
    out["list"] = np.zeros((m, cap if 1 <= cap <= 4096 else 1), np.uint32)      # (an invalid cap is the engine's to refuse: nothing is written then)
    out["count"] = np.zeros((m,), np.uint32)
    req.list = _ptr(out["list"]) if m else None
    req.count = _ptr(out["count"]) if m else None
    return req, (pts, pv, rad), out


def _knn_request(dtype, points, bodies, k, want_dist2):
    """The nb_knn_request of knn(): (request, arrays kept alive, index, dist2 | None)."""
    _need("nb_knn", "knn()")
    req = _new_request(nb_knn_request)
    pts, _ = _targets("knn()", req, dtype, points, bodies, NB_NBR_AT_BODIES)
    k = int(k)
    if not 0 <= k < 2 ** 32:
        raise ValueError("knn(): k out of range")
    req.k = k
    cols = k if 1 <= k <= 64 else 1                    # (an invalid k is the engine's to refuse: nothing is written then)
    index = np.zeros((req.m, cols), np.uint32)
    dist2 = np.zeros((req.m, cols), dtype) if want_dist2 else None
    req.index = _ptr(index) if req.m else None
    req.dist2 = _ptr(dist2) if want_dist2 and req.m else None
    return req, (pts,), index, dist2


def density_from_knn(bodies, index, dist2):
    """The Casertano-Hut local density of each row of a knn() result, in float64: the masses of the first k - 1 neighbours over the
    volume of the sphere that reaches the k-th, ``rho = sum(m[index[:, :k-1]]) / (4 pi / 3 * dist2[:, k-1] ** 1.5)`` -- the point
    itself and the k-th neighbour left out.  ``bodies``: (n, 4) rows (x, y, z, m) or the n masses; k >= 2.  ``nan`` where the row
    holds fewer than k neighbours."""
    b = np.asarray(bodies, np.float64)
    mass = b[:, 3] if b.ndim == 2 else b
    index = np.asarray(index, np.uint32)
    d2 = np.asarray(dist2, np.float64)
    if index.ndim != 2 or d2.shape != index.shape:
        raise ValueError("density_from_knn(): index and dist2 must both be (m, k)")
    k = index.shape[1]
    if k < 2:
        raise ValueError("density_from_knn(): k must be >= 2")
    full = index[:, k - 1] != NB_NBR_NONE
    inner = np.where(full[:, None], index[:, :k - 1].astype(np.int64), 0)
    msum = mass[inner].sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = msum / (4.0 * np.pi / 3.0 * np.where(full, d2[:, k - 1], 1.0) ** 1.5)
    return np.where(full, rho, np.nan)


def lists_to_csr(lists, count):
    """The rows of a neighbor_lists() result without their padding: ``(offsets (m + 1,) int64, indices uint32, truncated (m,) bool)``
    -- row k is ``indices[offsets[k]:offsets[k + 1]]``, its min(count[k], cap) entries in ascending order; ``truncated[k]`` says that
    count[k] > cap, i.e. that the row holds only the cap smallest of its members."""
    lists = np.asarray(lists, np.uint32)
    count = np.asarray(count, np.uint32).astype(np.int64)
    if lists.ndim != 2 or count.shape != (lists.shape[0],):
        raise ValueError("lists_to_csr(): lists must be (m, cap) and count (m,)")
    m, cap = lists.shape
    kept = np.minimum(count, cap)
    offsets = np.zeros(m + 1, np.int64)
    np.cumsum(kept, out=offsets[1:])
    mask = np.arange(cap, dtype=np.int64)[None, :] < kept[:, None]
    return offsets, lists[mask], count > cap


def pairs_from_lists(lists, count, first=0):
    """Every unordered pair (i, j), i < j, of the rows of an all-bodies neighbor_lists() result (row k = body first + k):
    ``(k, 2) uint32`` sorted by i, then j.  Membership is symmetric, so each pair is taken from the row of its smaller index.
    Raises if a row was truncated."""
    offsets, indices, truncated = lists_to_csr(lists, count)
    if truncated.any():
        raise ValueError("pairs_from_lists(): %d rows hold more members than cap (the largest count is %d): ask again with a larger cap"
                         % (int(truncated.sum()), int(np.asarray(count).max())))
    i = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64) + int(first), np.diff(offsets))
    j = indices.astype(np.int64)
    ok = i < j
    return np.stack([i[ok], j[ok]], axis=1).astype(np.uint32).reshape(-1, 2)


def mutual_pairs(index, dist2, radius):
    """The mutual nearest-neighbour pairs of an all-bodies neighbour result closer than ``radius``: ``(pairs (k, 2) uint32 sorted by
    i, d2 (k,))`` with i < j, index[i] == j, index[j] == i and dist2[i] < radius * radius in the precision of dist2."""
    index = np.asarray(index, np.uint32)
    dist2 = np.asarray(dist2)
    n = len(index)
    i = np.arange(n, dtype=np.int64)
    j = index.astype(np.int64)
    ok = j < n                                         # NB_NBR_NONE: no neighbour
    jj = np.where(ok, j, 0)
    h = dist2.dtype.type(radius)
    ok &= (i < j) & (index[jj].astype(np.int64) == i) & (dist2 < h * h)
    return np.stack([i[ok], j[ok]], axis=1).astype(np.uint32).reshape(-1, 2), dist2[ok].copy()


SYMW_PLAN_WORDS = ("np", "nsb", "W", "total_hi", "total_lo", "n_hi", "H", "r_layer0", "t_layer0", "L", "zc")
SYM_RANK_PLAN_WORDS = ("np", "nsb", "total_hi", "total_lo", "n_hi", "H", "r_layer0", "rb_layer0", "t_layer0", "g0", "g1", "LA", "LB", "WA", "WB", "ups")
SYM_PLAN_WORDS = ("np", "nsb", "q", "total_hi", "total_lo", "n_hi", "H", "r_layer0", "t_layer0")


def plan_query(n, precision="f32", shard=None, force_variant=0, jsplit=0, flags=0, n_cu=256, clock_hz=2.4e9, device=-1,
               layer_budget_mib=0, sym_pass=0):
    """nb_plan_query: the launch plan nb_create would build -- the engine's planner run on the host alone (works without a
    GPU when n_cu and clock_hz are given; 0 means "as on the device").  Returns a dict: the shape digits, the j-partitions,
    and for the symmetric pass `plan` (the words the kernels receive, by name) and `tab` (first wave, resident layers per super-block)."""
    L = load_library()
    cfg = nb_config()
    cfg.struct_size = C.sizeof(nb_config)
    cfg.n = int(n)
    cfg.precision = NB_F64 if precision in ("f64", NB_F64, np.float64) else NB_F32
    cfg.device = device
    if shard is not None:
        cfg.shard_begin, cfg.shard_count = int(shard[0]), int(shard[1])
    cfg.force_variant, cfg.jsplit, cfg.flags = int(force_variant), int(jsplit), int(flags)
    cfg.layer_budget_mib = int(layer_budget_mib)
    info = nb_plan_info()
    info.struct_size = C.sizeof(nb_plan_info)
    info.sym_pass = int(sym_pass)
    rc = L.nb_plan_query(C.byref(cfg), int(n_cu), float(clock_hz), C.byref(info), None, 0)
    if rc != 0:
        raise NBodyError(rc, L.nb_last_error(None).decode())
    tab = np.zeros(info.tab_len, np.uint32)
    if info.tab_len:
        info.sym_pass = int(sym_pass)
        rc = L.nb_plan_query(C.byref(cfg), int(n_cu), float(clock_hz), C.byref(info), tab.ctypes.data_as(C.POINTER(C.c_uint32)), tab.size)
        if rc != 0:
            raise NBodyError(rc, L.nb_last_error(None).decode())
    out = {k: int(getattr(info, k)) for k, _ in nb_plan_info._fields_[1:16]}
    out["variant"] = info.variant.decode()
    out["flags"] = int(flags)
    out.update(passes=int(info.sym_passes), local=int(info.sym_local), pass_k_lo=int(info.sym_pass_k_lo), pass_k_hi=int(info.sym_pass_k_hi),
               pass_d0=int(info.sym_pass_d0))
    if info.sym:
        out["plan"] = dict(zip(SYMW_PLAN_WORDS if info.symw else SYM_PLAN_WORDS, (int(w) for w in info.sym_plan)))
        nsb = out["plan"]["nsb"]
        if info.sym_rank:
            # the rank form: two phases (own-row travelers first), {first A wave, A waves, first B wave, B waves} per super-block
            rp = dict(zip(SYM_RANK_PLAN_WORDS, (int(w) for w in info.sym_rank_plan)))
            ng = rp["g1"] - rp["g0"]
            out["rank_plan"] = rp
            out["rank_tab"] = tab[:4 * nsb].reshape(-1, 4)
            out["prefix_a"] = tab[4 * nsb:4 * nsb + ng + 1]
            out["prefix_b"] = tab[4 * nsb + ng + 1:4 * nsb + 2 * (ng + 1)]
            if rp["ups"] > 1:
                nch = rp["np"] // 64
                base = 4 * nsb + 2 * (ng + 1)
                out["spill_tab"] = tab[base:base + 2 * nch].reshape(-1, 2)
                out["spill_ids"] = tab[base + 2 * nch:]
            out["tab"] = out["rank_tab"][:, :2]
        else:
            if info.symw:
                # one {first wave, resident layers} pair per block of S rows: the nsb whole super-blocks of the ring, then the short block Z
                nsb = out["plan"]["np"] // (64 * int(info.ipl))
            out["tab"] = tab[:2 * nsb].reshape(-1, 2)
            if info.symw:
                # four words per physical wave: {first unit, end, resident layer of the super-block the range ends in, spill row}.  The ranges
                # partition the list; "order" lists the waves in list order ("positions"), "starts" the first unit of every position + the list's end
                W = out["plan"]["W"]
                out["waves"] = tab[2 * nsb:2 * nsb + 4 * W].reshape(-1, 4)
                out["order"] = np.argsort(out["waves"][:, 0], kind="stable")
                out["starts"] = np.concatenate([out["waves"][out["order"], 0], [out["plan"]["L"] * int(info.sym_ups)]]).astype(np.uint32)
                # (a wave's record ends where its OWN part ends: with whole sweeps and two waves per SIMD the last sweeps of an older
                # wave's range are left to a queue -- {first unit, resident layer | sweeps << 16} per queued piece, in queue order, behind the records)
                out["pieces"] = tab[2 * nsb + 4 * W:].reshape(-1, 2) if int(info.sym_ups) == 1 else np.zeros((0, 2), np.uint32)
        out["ups"], out["spill_rows"] = int(info.sym_ups), int(info.sym_spill_rows)
        if info.symw:
            out["plan"]["ups"] = int(info.sym_ups)
        if info.sym_ups > 1 and not info.sym_rank:
            # the spill rows (wave ranges cut inside sweeps): {first row, count} per traveler chunk, then the wave numbers in row order
            # (a wave's own row is word 3 of its record)
            ch = 128 if info.x == 1 else 64
            nch = out["plan"]["np"] // ch
            W = out["plan"]["W"]
            base = 2 * nsb + 4 * W
            out["spill_slot"] = out["waves"][:, 3]
            out["spill_tab"] = tab[base:base + 2 * nch].reshape(-1, 2)
            out["spill_ids"] = tab[base + 2 * nch:]
    return out


class Simulation:
    """One engine handle = the reference's (bodyBuffer, velBuffer, accelBuffer,
    uniforms, compute pipeline) bundle, nbody3d.js:13,179-204,296-311."""

    def __init__(self, n, precision="f32", eps2=None, device=-1, shard=None, stream=None, ext_bodies=None,
                 force_variant=0, jsplit=0, tile=0, flags=0, layer_budget_mib=0, integrator="leapfrog"):
        L = load_library()
        self._L = L
        self.n = int(n)
        if integrator not in INTEGRATORS and integrator != "hermite6":
            raise ValueError("integrator must be one of %s, got %r" % (sorted(INTEGRATORS) + ["hermite6"], integrator))
        if integrator == "hermite6" and not hasattr(L, "nb_set_hermite_order"):
            raise NBodyError(1, "integrator='hermite6': the loaded library has no nb_set_hermite_order")
        if integrator != "leapfrog" and not hasattr(L, "nb_download_jerk"):
            raise NBodyError(1, "integrator=%r: the loaded library has no Hermite integrator (nb_download_jerk is missing)" % (integrator,))
        self.integrator = integrator
        self.dtype = np.float64 if precision in ("f64", NB_F64, np.float64) else np.float32
        cfg = nb_config()
        cfg.struct_size = C.sizeof(nb_config)
        cfg.n = self.n
        cfg.precision = NB_F64 if self.dtype == np.float64 else NB_F32
        cfg.tile = tile
        cfg.eps2 = 0.0 if eps2 is None else float(eps2)
        cfg.device = device
        self._device = int(device)
        self.shard_begin, self.shard_count = (0, self.n) if shard is None else (int(shard[0]), int(shard[1]))
        if shard is not None:      # shard_count = 0 means "whole system, not a shard" (eligible for the fused step)
            cfg.shard_begin, cfg.shard_count = self.shard_begin, self.shard_count
        if stream is not None:
            cfg.ext_stream = stream if stream else None
            cfg.flags |= NB_FLAG_EXT_STREAM
        if ext_bodies is not None:
            cfg.ext_bodies = ext_bodies
        cfg.force_variant = force_variant
        cfg.jsplit = jsplit
        cfg.flags |= int(flags)
        cfg.layer_budget_mib = int(layer_budget_mib)
        cfg.integrator = INTEGRATORS["hermite4" if integrator == "hermite6" else integrator]      # "hermite6": hermite4 + set_hermite_order(6)
        h = C.c_void_p()
        rc = L.nb_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise NBodyError(rc, L.nb_last_error(None).decode())
        self._h = h
        self._hook = None
        self.dt = 0.0
        self.G = 0.0
        if integrator == "hermite6":
            try:
                self.set_hermite_order(6)
            except Exception:
                self.close()
                raise

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.nb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise NBodyError(rc, self._L.nb_last_error(self._h).decode())

    def _arr(self, a, name):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.size != 4 * self.n:
            raise ValueError("%s must hold 4*n = %d elements, got %d" % (name, 4 * self.n, a.size))
        return a

    # -- reference-shaped surface -------------------------------------------
    def init(self, bodies, vel, accel=None):
        """nbody3d.js:177-199: upload packed [x,y,z,m] / [vx,vy,vz,0]; accel zero."""
        b = self._arr(bodies, "bodies")
        v = self._arr(vel, "vel")
        a = None if accel is None else self._arr(accel, "accel")
        self._check(self._L.nb_upload(self._h, _ptr(b), _ptr(v), _ptr(a)))
        return self

    restore = init  # util.js:230-244 writes the same three arrays back

    def set_params(self, dt, G):
        self.dt, self.G = float(dt), float(G)
        self._check(self._L.nb_set_params(self._h, self.dt, self.G))

    def step(self, dt=None, G=None):
        """One frame's compute pass (nbody3d.js:470-490); dt <= 0 is a no-op (:474)."""
        if dt is not None or G is not None:
            self.set_params(self.dt if dt is None else dt, self.G if G is None else G)
        self._check(self._L.nb_step(self._h, 1))

    def simulate(self, nsteps, dt=None, G=None):
        if dt is not None or G is not None:
            self.set_params(self.dt if dt is None else dt, self.G if G is None else G)
        self._check(self._L.nb_step(self._h, int(nsteps)))

    def sync(self):
        self._check(self._L.nb_sync(self._h))

    def read(self, bodies=True, vel=True, accel=True):
        """util.js:163-178: fresh host copies of (bodies, vel, accel), shape (N,4).
        On a shard handle vel/accel rows outside the shard are zero."""
        out = [np.zeros((self.n, 4), self.dtype) if f else None for f in (bodies, vel, accel)]
        self._check(self._L.nb_download(self._h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    # -- Hermite handles (integrator="hermite4") -----------------------------
    def read_jerk(self):
        """nb_download_jerk: the jerk (jx, jy, jz, 0) of the state as it stands, shape (N,4).  With read() this is the whole
        checkpoint of a Hermite handle: (bodies, vel) at one instant and the derivatives the next step starts from."""
        if not hasattr(self._L, "nb_download_jerk"):
            raise NBodyError(1, "read_jerk(): the loaded library has no nb_download_jerk")
        out = np.zeros((self.n, 4), self.dtype)
        self._check(self._L.nb_download_jerk(self._h, _ptr(out)))
        return out

    def upload_derivs(self, accel, jerk):
        """nb_upload_derivs: after init() / restore(), hands a checkpoint's (accel, jerk) back, so that the next step continues
        bit-identically (a step leaves derivatives evaluated at the PREDICTED state: recomputing them from (x, v) is close, not equal)."""
        if not hasattr(self._L, "nb_upload_derivs"):
            raise NBodyError(1, "upload_derivs(): the loaded library has no nb_upload_derivs")
        a, j = self._arr(accel, "accel"), self._arr(jerk, "jerk")
        self._check(self._L.nb_upload_derivs(self._h, _ptr(a), _ptr(j)))
        return self

    # -- the 6th-order scheme of a Hermite handle (force, jerk and snap) --------
    def _need_order(self, what):
        if not hasattr(self._L, "nb_set_hermite_order"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_hermite_order" % what)

    def set_hermite_order(self, order):
        """nb_set_hermite_order: 6 switches the handle to the 6th-order predictor-corrector on force, jerk and snap (the snap is
        evaluated when next needed), 4 back to the 4th-order one (snap and crackle are freed, accel and jerk stay current)."""
        self._need_order("set_hermite_order()")
        self._check(self._L.nb_set_hermite_order(self._h, int(order)))
        return self

    def hermite_order(self):
        """nb_hermite_order: 4 or 6."""
        self._need_order("hermite_order()")
        o = C.c_uint32()
        self._check(self._L.nb_hermite_order(self._h, C.byref(o)))
        return int(o.value)

    def read_snap(self):
        """nb_download_snap: (snap, crackle) of the state as it stands, shape (N,4) each.  With read() and read_jerk() this is the
        whole checkpoint of an order-6 handle."""
        self._need_order("read_snap()")
        s, c = np.zeros((self.n, 4), self.dtype), np.zeros((self.n, 4), self.dtype)
        self._check(self._L.nb_download_snap(self._h, _ptr(s), _ptr(c)))
        return s, c

    def upload_derivs6(self, accel, jerk, snap, crackle):
        """nb_upload_derivs6: after init() / restore() and set_hermite_order(6), hands a checkpoint's (accel, jerk, snap, crackle)
        back, so that the next step continues bit-identically."""
        self._need_order("upload_derivs6()")
        a, j, s, c = self._arr(accel, "accel"), self._arr(jerk, "jerk"), self._arr(snap, "snap"), self._arr(crackle, "crackle")
        self._check(self._L.nb_upload_derivs6(self._h, _ptr(a), _ptr(j), _ptr(s), _ptr(c)))
        return self

    def set_start6(self, mode):
        """nb_set_start6: how the engine makes the starts of an order-6 handle itself.  START6_ZERO (0): snap from the pass, crackle
        0, block levels from (eta / 2)|a|/|j|; START6_CRACKLE (1): the crackle is the direct sum on (x, v, a, j) and dynamic block
        levels come from the two-rule start.  A start or levels the engine made that no step has consumed are made again; uploaded
        ones and a running state are kept."""
        if not hasattr(self._L, "nb_set_start6"):
            raise NBodyError(1, "set_start6(): the loaded library has no nb_set_start6")
        self._check(self._L.nb_set_start6(self._h, int(mode)))
        return self

    @property
    def start6(self):
        """nb_start6: START6_ZERO or START6_CRACKLE."""
        if not hasattr(self._L, "nb_start6"):
            raise NBodyError(1, "start6: the loaded library has no nb_start6")
        m = C.c_uint32()
        self._check(self._L.nb_start6(self._h, C.byref(m)))
        return int(m.value)

    def set_pass_precision(self, mode):
        """nb_set_pass_precision: "native" (0), the handle's own precision, or "mixed" (1): every force+jerk pass of an f64 Hermite
        handle of order 4 runs binary32 pair arithmetic on double-single position differences, with fp64 sums across the j-chunks
        into the unchanged fp64 state.  Touches no state, derivatives or levels; takes effect from the next pass on."""
        if isinstance(mode, str):
            if mode not in _PASS_MODES:
                raise ValueError("set_pass_precision(): mode must be 'native', 'mixed', 0 or 1, not %r" % (mode,))
            mode = _PASS_MODES[mode]
        if not hasattr(self._L, "nb_set_pass_precision"):
            raise NBodyError(1, "set_pass_precision(): the loaded library has no nb_set_pass_precision")
        self._check(self._L.nb_set_pass_precision(self._h, int(mode)))
        return self

    def pass_precision(self):
        """nb_pass_precision: "native" or "mixed"."""
        if not hasattr(self._L, "nb_pass_precision"):
            raise NBodyError(1, "pass_precision(): the loaded library has no nb_pass_precision")
        m = C.c_uint32()
        self._check(self._L.nb_pass_precision(self._h, C.byref(m)))
        return "mixed" if m.value == PASS_MIXED else "native"

    def set_pass_guard(self, r_near):
        """nb_set_pass_guard: the guard radius of the mixed pass (0: off).  The terms of pairs closer than r_near are summed apart
        from the binary32 registers, compensated (TwoSum), so that a hard pair's members -- and the pair's barycentre -- keep the
        field of the rest of the system.  Valid while the pass precision is "mixed"; touches no state, derivatives or levels."""
        try:
            r_near = float(r_near)
        except (TypeError, ValueError):
            raise ValueError("set_pass_guard(): r_near must be a number, not %r" % (r_near,))
        if not hasattr(self._L, "nb_set_pass_guard"):
            raise NBodyError(1, "set_pass_guard(): the loaded library has no nb_set_pass_guard")
        self._check(self._L.nb_set_pass_guard(self._h, r_near))
        return self

    def pass_guard(self):
        """nb_pass_guard: the guard radius, 0.0 where the guard is off."""
        if not hasattr(self._L, "nb_pass_guard"):
            raise NBodyError(1, "pass_guard(): the loaded library has no nb_pass_guard")
        r = C.c_double()
        self._check(self._L.nb_pass_guard(self._h, C.byref(r)))
        return float(r.value)

    # -- block individual time steps of a Hermite handle -----------------------
    def _need_block(self, what):
        if not hasattr(self._L, "nb_set_block_steps"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_block_steps" % what)

    def set_block_steps(self, *args, **kw):
        """set_block_steps(eta=None, max_level=None, min_level=0, frozen=False): nb_set_block_steps -- every body steps by
        dt / 2^level, level in [min_level, max_level], chosen from its own (a, j, a2, a3) with the accuracy parameter eta (None:
        the library's defaults, eta 0.02 and max_level 20); frozen=True keeps the levels as initialised or uploaded.  step() /
        simulate() still advance by whole dt.  set_block_steps(None) switches back to one shared step."""
        self._need_block("set_block_steps()")
        return self._set_block(self._L.nb_set_block_steps, args, kw)

    def _set_block(self, fn, args, kw):
        if args == (None,) and not kw:
            self._check(fn(self._h, None))
            return self

        def bind(eta=None, max_level=None, min_level=0, frozen=False):
            return eta, max_level, min_level, frozen
        eta, max_level, min_level, frozen = bind(*args, **kw)
        cfg = nb_block_steps()
        cfg.struct_size = C.sizeof(nb_block_steps)
        cfg.max_level = 0 if max_level is None else int(max_level)
        cfg.min_level = int(min_level)
        cfg.flags = NB_BLOCK_FROZEN if frozen else 0
        cfg.eta = 0.0 if eta is None else float(eta)
        self._check(fn(self._h, C.byref(cfg)))
        return self

    def set_block_steps6(self, *args, **kw):
        """set_block_steps6(eta=None, max_level=None, min_level=0, frozen=False): nb_set_block_steps6 -- block steps on an order-6
        handle (after set_hermite_order(6)): every body steps by dt / 2^level, chosen from its own (a, j, s, c, a4, a5) with the
        accuracy parameter eta.  Dynamic levels need an f64 handle; an f32 handle takes frozen=True.  block_stats(), read_levels()
        and upload_levels() work as with set_block_steps().  set_block_steps6(None) switches back to the shared order-6 step."""
        if not hasattr(self._L, "nb_set_block_steps6"):
            raise NBodyError(1, "set_block_steps6(): the loaded library has no nb_set_block_steps6")
        return self._set_block(self._L.nb_set_block_steps6, args, kw)

    def block_stats(self, reset=False):
        """nb_block_stats: {enabled, outer_steps, block_steps, body_steps, clamped, finest_level} since the last reset."""
        self._need_block("block_stats()")
        st = nb_block_stats()
        st.struct_size = C.sizeof(nb_block_stats)
        self._check(self._L.nb_block_stats(self._h, C.byref(st), 1 if reset else 0))
        return {k: int(getattr(st, k)) for k in ("enabled", "outer_steps", "block_steps", "body_steps", "clamped", "finest_level")}

    def set_block_batch(self, *args, **kw):
        """set_block_batch(depth=None, small_max=None): nb_set_block_batch -- on an order-4 block-step handle with the native pass,
        block steps with at most small_max active bodies (None: 256; 0: none; at most 1024) run from the device's own header, up
        to depth (None: 32; at most 1024) of them per host wait.  No stored bit depends on depth.  Touches no state, derivatives
        or levels.  set_block_batch(None) switches the mode off (so does set_block_steps(None))."""
        return self._set_block_batch("nb_set_block_batch", args, kw)

    def set_block_batch6(self, *args, **kw):
        """set_block_batch6(depth=None, small_max=None): nb_set_block_batch6 -- set_block_batch()'s mode on an order-6 handle with
        set_block_steps6() on (f64: dynamic or frozen levels; f32: frozen levels).  The same arguments, defaults and refusals;
        block_batch_stats() serves both.  set_block_batch6(None) switches the mode off (so do set_block_batch(None),
        set_block_steps6(None) and set_block_steps(None))."""
        return self._set_block_batch("nb_set_block_batch6", args, kw)

    def set_block_batch_mixed(self, *args, **kw):
        """set_block_batch_mixed(depth=None, small_max=None): nb_set_block_batch_mixed -- set_block_batch()'s mode on an f64 order-4
        handle with set_block_steps() on, set_pass_precision("mixed") and no guard: the small steps run the double-single pass.
        The same arguments, defaults and refusals; block_batch_stats() serves all three.  set_block_batch_mixed(None) switches
        the mode off (so do set_block_batch(None), set_block_batch6(None) and set_block_steps(None))."""
        return self._set_block_batch("nb_set_block_batch_mixed", args, kw)

    def set_block_batch_watch(self, *args, **kw):
        """set_block_batch_watch(depth=None, small_max=None): nb_set_block_batch_watch -- set_block_batch()'s mode on a handle with
        the encounter watch on (order 4, the native pass; call set_block_steps(), set_encounter_watch(), then this): the small
        steps watch too, and the records and counters depend on depth as little as the state does.  The same arguments, defaults
        and refusals; block_batch_stats() serves all four.  set_block_batch_watch(None) switches the mode off and keeps the watch
        (so do the three other batch setters with None); set_encounter_watch(None) switches off both."""
        return self._set_block_batch("nb_set_block_batch_watch", args, kw)

    def _set_block_batch(self, symbol, args, kw):
        who = symbol[3:]
        if not hasattr(self._L, symbol):
            raise NBodyError(1, "%s(): the loaded library has no %s" % (who, symbol))
        if args == (None,) and not kw:
            self._check(getattr(self._L, symbol)(self._h, None))
            return self

        def bind(depth=None, small_max=None):
            return depth, small_max
        depth, small_max = bind(*args, **kw)
        if depth is not None and not 0 <= int(depth) <= 1024:
            raise ValueError("depth must be in [0, 1024] (0 or None: 32)")
        if small_max is not None and not 0 <= int(small_max) <= 1024:
            raise ValueError("small_max must be in [0, 1024] (None: 256; 0: no small steps)")
        cfg = nb_block_batch()
        cfg.struct_size = C.sizeof(nb_block_batch)
        cfg.depth = 0 if depth is None else int(depth)
        cfg.small_max = BLOCK_BATCH_SMALL_DEFAULT if small_max is None else int(small_max)
        cfg.flags = 0
        self._check(getattr(self._L, symbol)(self._h, C.byref(cfg)))
        return self

    def block_batch_stats(self, reset=False):
        """nb_block_batch_stats: {enabled, host_waits, slots, small_steps, host_steps, idle_slots} since the last reset."""
        if not hasattr(self._L, "nb_block_batch_stats"):
            raise NBodyError(1, "block_batch_stats(): the loaded library has no nb_block_batch_stats")
        st = nb_block_batch_stats()
        st.struct_size = C.sizeof(nb_block_batch_stats)
        self._check(self._L.nb_block_batch_stats(self._h, C.byref(st), 1 if reset else 0))
        return {k: int(getattr(st, k)) for k in ("enabled", "host_waits", "slots", "small_steps", "host_steps", "idle_slots")}

    # -- the encounter watch of a block-step handle -----------------------------
    def _need_watch(self, what):
        if not hasattr(self._L, "nb_set_encounter_watch"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_encounter_watch" % what)

    def set_encounter_watch(self, *args, **kw):
        """set_encounter_watch(radius=None, radii=None, stop=False): nb_set_encounter_watch -- on an order-4 block-step handle with
        the native pass, every body with a watch radius > 0 (``radius`` for all, or ``radii`` of shape (N,); 0: not watched)
        records the closest body it meets below that radius at its OWN block steps: download_encounters().  stop=True makes
        step() return after the first outer step that had a hit (encounter_stats()["stopped"], ["steps_left"]).  Changes no bit of
        the state.  set_encounter_watch(None) switches the watch off (so does set_block_steps(None))."""
        self._need_watch("set_encounter_watch()")
        if args == (None,) and not kw:
            self._check(self._L.nb_set_encounter_watch(self._h, None))
            return self

        def bind(radius=None, radii=None, stop=False):
            return radius, radii, stop
        radius, radii, stop = bind(*args, **kw)
        if (radius is None) == (radii is None):
            raise ValueError("set_encounter_watch(): give exactly one of radius and radii")
        cfg = nb_encounter_watch()
        cfg.flags = NB_ENC_STOP if stop else 0
        keep = None
        if radii is None:
            try:
                radius = float(radius)
            except (TypeError, ValueError):
                raise ValueError("set_encounter_watch(): radius must be a number, not %r" % (radius,))
            if not (radius >= 0.0) or radius == float("inf"):
                raise ValueError("set_encounter_watch(): radius must be finite and >= 0")
            cfg.radius = radius
        else:
            keep = np.ascontiguousarray(radii, dtype=self.dtype)
            if keep.shape != (self.n,):
                raise ValueError("radii must have shape (%d,)" % self.n)
            if not (np.isfinite(keep).all() and (keep >= 0).all()):
                raise ValueError("set_encounter_watch(): radii must be finite and >= 0")
            cfg.radii = _ptr(keep)
        self._check(self._L.nb_set_encounter_watch(self._h, C.byref(cfg)))
        return self

    def encounter_stats(self, reset=False):
        """nb_encounter_stats: {passes, hits, first_time, stopped, steps_left}; reset=True zeroes the counters (not the records)."""
        self._need_watch("encounter_stats()")
        st = nb_encounter_stats()
        self._check(self._L.nb_encounter_stats(self._h, C.byref(st), 1 if reset else 0))
        return {"passes": int(st.passes), "hits": int(st.hits), "first_time": float(st.first_time), "stopped": int(st.stopped),
                "steps_left": int(st.steps_left)}

    def download_encounters(self):
        """nb_download_encounters: {rho2 (the handle's dtype; +inf: none), partner (uint32; ENC_NONE: none), time (float64),
        count (uint32)}, each of shape (N,)."""
        self._need_watch("download_encounters()")
        out = {"rho2": np.zeros(self.n, self.dtype), "partner": np.zeros(self.n, np.uint32), "time": np.zeros(self.n, np.float64),
               "count": np.zeros(self.n, np.uint32)}
        self._check(self._L.nb_download_encounters(self._h, _ptr(out["rho2"]), _ptr(out["partner"]), _ptr(out["time"]), _ptr(out["count"])))
        return out

    def upload_encounters(self, rho2, partner, time, count):
        """nb_upload_encounters: the records of a checkpoint (what download_encounters() gave), behind set_encounter_watch()."""
        self._need_watch("upload_encounters()")
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((rho2, self.dtype), (partner, np.uint32), (time, np.float64), (count, np.uint32))]
        for a, name in zip(arrs, ("rho2", "partner", "time", "count")):
            if a.shape != (self.n,):
                raise ValueError("%s must have shape (%d,)" % (name, self.n))
        self._check(self._L.nb_upload_encounters(self._h, *[_ptr(a) for a in arrs]))
        return self

    def reset_encounters(self):
        """nb_reset_encounters: the records to their start values and the counters to 0."""
        self._need_watch("reset_encounters()")
        self._check(self._L.nb_reset_encounters(self._h))
        return self

    def read_levels(self):
        """nb_download_levels: the level of every body (uint8, shape (N,)); initialises them first if they are not current."""
        self._need_block("read_levels()")
        out = np.zeros(self.n, np.uint8)
        self._check(self._L.nb_download_levels(self._h, _ptr(out)))
        return out

    def upload_levels(self, levels):
        """nb_upload_levels: the last call of a checkpoint restore (init, upload_derivs, set_block_steps, upload_levels)."""
        self._need_block("upload_levels()")
        lv = np.ascontiguousarray(levels, np.uint8)
        if lv.shape != (self.n,):
            raise ValueError("levels must have shape (%d,)" % self.n)
        self._check(self._L.nb_upload_levels(self._h, _ptr(lv)))
        return self

    # -- the Ahmad-Cohen neighbour scheme of a Hermite handle -------------------
    def _need_scheme(self, what):
        if not hasattr(self._L, "nb_set_neighbor_scheme"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_neighbor_scheme" % what)

    def set_neighbor_scheme(self, *args, **kw):
        """set_neighbor_scheme(radius=None, radii=None, substeps=None, cap=None): nb_set_neighbor_scheme -- a body's force is
        split at its neighbour radius; the sums over its neighbour list run every dt / substeps, the rest once per dt.  ``radius``
        is one number, ``radii`` one per body (copied by the call); substeps a power of two (None: the library's 8), cap the
        entries of a list row (None: 128).  A list that does not fit its row makes step() raise NB_ERR_STATE until the scheme is
        set again.  set_neighbor_scheme(None) switches back to plain Hermite steps."""
        self._need_scheme("set_neighbor_scheme()")
        if args == (None,) and not kw:
            self._check(self._L.nb_set_neighbor_scheme(self._h, None))
            return self

        def bind(radius=None, radii=None, substeps=None, cap=None):
            return radius, radii, substeps, cap
        radius, radii, substeps, cap = bind(*args, **kw)
        cfg = nb_neighbor_scheme()
        cfg.struct_size = C.sizeof(nb_neighbor_scheme)
        cfg.substeps = 0 if substeps is None else int(substeps)
        cfg.cap = 0 if cap is None else int(cap)
        cfg.flags = 0
        cfg.radius = 0.0 if radius is None else float(radius)
        keep = None
        if radii is not None:
            keep = np.ascontiguousarray(radii, dtype=self.dtype)
            if keep.shape != (self.n,):
                raise ValueError("radii must have shape (%d,)" % self.n)
            cfg.radii = _ptr(keep)
        self._check(self._L.nb_set_neighbor_scheme(self._h, C.byref(cfg)))
        return self

    def neighbor_scheme_stats(self, reset=False):
        """nb_neighbor_scheme_stats: {enabled, regular_steps, substeps, entries, builds, max_count, overflowed}; entries is the
        sum of min(count, cap) over the list builds (the start included), max_count and overflowed belong to the last build."""
        self._need_scheme("neighbor_scheme_stats()")
        st = nb_neighbor_scheme_stats()
        st.struct_size = C.sizeof(nb_neighbor_scheme_stats)
        self._check(self._L.nb_neighbor_scheme_stats(self._h, C.byref(st), 1 if reset else 0))
        return {k: int(getattr(st, k)) for k in ("enabled", "regular_steps", "substeps", "entries", "builds", "max_count", "overflowed")}

    @property
    def neighbor_scheme_fused(self):
        """nb_neighbor_scheme_fused: whether the next list build of the neighbour scheme is ONE nb_split_lists call (True) or
        nb_split_force followed by nb_neighbor_lists (False: NB_FLAG_AC_TWO_CALLS, a launch shape that differs, the scheme off, or
        an older library).  Both routes leave the same bits."""
        if not hasattr(self._L, "nb_neighbor_scheme_fused"):
            return False
        v = C.c_int()
        self._check(self._L.nb_neighbor_scheme_fused(self._h, C.byref(v)))
        return bool(v.value)

    def download_neighbor_scheme(self, cap):
        """nb_download_neighbor_scheme: {accel_irr, jerk_irr, accel_reg, jerk_reg ((N, 4)), list ((N, cap), uint32), count ((N,),
        uint32)} at the handle's instant; runs the scheme's start first if they are not current.  ``cap`` is the scheme's."""
        self._need_scheme("download_neighbor_scheme()")
        out = {k: np.zeros((self.n, 4), self.dtype) for k in ("accel_irr", "jerk_irr", "accel_reg", "jerk_reg")}
        out["list"] = np.zeros((self.n, int(cap)), np.uint32)
        out["count"] = np.zeros(self.n, np.uint32)
        self._check(self._L.nb_download_neighbor_scheme(self._h, *[_ptr(out[k]) for k in ("accel_irr", "jerk_irr", "accel_reg", "jerk_reg", "list", "count")]))
        return out

    # -- the scheme on a long run: radii that follow a target count, bit-exact restore --
    def _need_adapt(self, what):
        if not hasattr(self._L, "nb_set_neighbor_adapt"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_neighbor_adapt" % what)

    def set_neighbor_adapt(self, *args, **kw):
        """set_neighbor_adapt(target, grow_max=None, max_rebuilds=None, radius_min=None, radius_max=None): nb_set_neighbor_adapt --
        after every list build each radius moves towards the one that would hold ``target`` members (by at most grow_max per
        build, None: cbrt(2)), and a build with rows over cap shrinks those rows and runs again, up to max_rebuilds times (None: 4).
        radius_min / radius_max clamp a non-zero radius.  Needs set_neighbor_scheme first; 2 * target <= its cap.
        set_neighbor_adapt(None) goes back to the scheme's fixed radii."""
        self._need_adapt("set_neighbor_adapt()")
        if args == (None,) and not kw:
            self._check(self._L.nb_set_neighbor_adapt(self._h, None))
            return self

        def bind(target, grow_max=None, max_rebuilds=None, radius_min=None, radius_max=None):
            return target, grow_max, max_rebuilds, radius_min, radius_max
        target, grow_max, max_rebuilds, radius_min, radius_max = bind(*args, **kw)
        cfg = nb_neighbor_adapt()
        cfg.struct_size = C.sizeof(nb_neighbor_adapt)
        cfg.target = int(target)
        cfg.max_rebuilds = 0 if max_rebuilds is None else int(max_rebuilds)
        cfg.flags = 0
        cfg.grow_max = 0.0 if grow_max is None else float(grow_max)
        cfg.radius_min = 0.0 if radius_min is None else float(radius_min)
        cfg.radius_max = 0.0 if radius_max is None else float(radius_max)
        self._check(self._L.nb_set_neighbor_adapt(self._h, C.byref(cfg)))
        return self

    def neighbor_adapt_stats(self, reset=False):
        """nb_neighbor_adapt_stats: {enabled, rebuilds, rows_shrunk, last_rebuilds}; last_rebuilds belongs to the last build."""
        self._need_adapt("neighbor_adapt_stats()")
        st = nb_neighbor_adapt_stats()
        st.struct_size = C.sizeof(nb_neighbor_adapt_stats)
        self._check(self._L.nb_neighbor_adapt_stats(self._h, C.byref(st), 1 if reset else 0))
        return {k: int(getattr(st, k)) for k in ("enabled", "rebuilds", "rows_shrunk", "last_rebuilds")}

    def download_neighbor_radii(self):
        """nb_download_neighbor_radii: (built, next), each (N,): the radii the current list was cut by and those the next build
        will use (with adaptation off both are the scheme's fixed radii); runs the scheme's start first if it is not current."""
        self._need_adapt("download_neighbor_radii()")
        built, nxt = np.zeros(self.n, self.dtype), np.zeros(self.n, self.dtype)
        self._check(self._L.nb_download_neighbor_radii(self._h, _ptr(built), _ptr(nxt)))
        return built, nxt

    def upload_neighbor_scheme(self, accel_irr=None, jerk_irr=None, accel_reg=None, jerk_reg=None, list=None, count=None, radii=None):
        """nb_upload_neighbor_scheme: the last call of a restore -- the arrays of download_neighbor_scheme() and, with adaptation on,
        ``radii`` = the `next` of download_neighbor_radii().  The next step continues bit for bit."""
        self._need_adapt("upload_neighbor_scheme()")
        ck = nb_neighbor_checkpoint()
        ck.struct_size = C.sizeof(nb_neighbor_checkpoint)
        keep = []
        for name, a in (("accel_irr", accel_irr), ("jerk_irr", jerk_irr), ("accel_reg", accel_reg), ("jerk_reg", jerk_reg)):
            if a is not None:
                keep.append(self._arr(a, name))
                setattr(ck, name, _ptr(keep[-1]))
        if count is not None:
            keep.append(np.ascontiguousarray(count, np.uint32))
            if keep[-1].shape != (self.n,):
                raise ValueError("count must have shape (%d,)" % self.n)
            ck.count = _ptr(keep[-1])
        if list is not None:
            keep.append(np.ascontiguousarray(list, np.uint32))
            if keep[-1].ndim != 2 or keep[-1].shape[0] != self.n:
                raise ValueError("list must have shape (%d, cap)" % self.n)
            ck.list = _ptr(keep[-1])
        if radii is not None:
            keep.append(np.ascontiguousarray(radii, self.dtype))
            if keep[-1].shape != (self.n,):
                raise ValueError("radii must have shape (%d,)" % self.n)
            ck.radii = _ptr(keep[-1])
        self._check(self._L.nb_upload_neighbor_scheme(self._h, C.byref(ck)))
        return self

    def neighbor_scheme_checkpoint(self, cap):
        """Everything a restore of a handle with the neighbour scheme needs, as host arrays: {bodies, vel, dt, G, scheme (the arrays
        of download_neighbor_scheme(cap)), radii (`next`), adaptive}.  The scheme's and the adaptation's settings are the caller's."""
        b, v, _ = self.read(accel=False)
        ck = {"bodies": b, "vel": v, "dt": self.dt, "G": self.G, "scheme": self.download_neighbor_scheme(cap),
              "adaptive": bool(self.neighbor_adapt_stats()["enabled"])}
        ck["radii"] = self.download_neighbor_radii()[1]
        if hasattr(self._L, "nb_set_neighbor_levels") and self.neighbor_level_stats()["enabled"]:
            ck["levels"] = self.download_neighbor_levels()
        return ck

    def restore_neighbor_scheme(self, ck, scheme=None, adapt=None, levels=None):
        """The calls of a restore in their order: init, set_params, set_neighbor_scheme(**scheme), set_neighbor_adapt(**adapt) and
        set_neighbor_levels(**levels) where given (a handle that already has them set keeps them otherwise), upload_neighbor_scheme
        and, where the checkpoint holds levels and the handle has them switched on, upload_neighbor_levels last."""
        self.init(ck["bodies"], ck["vel"])
        self.set_params(ck["dt"], ck["G"])
        if scheme is not None:
            self.set_neighbor_scheme(**scheme)
        if adapt is not None:
            self.set_neighbor_adapt(**adapt)
        if levels is not None:
            self.set_neighbor_levels(**levels)
        self.upload_neighbor_scheme(radii=ck["radii"] if self.neighbor_adapt_stats()["enabled"] else None, **ck["scheme"])
        if ck.get("levels") is not None and self.neighbor_level_stats()["enabled"]:
            self.upload_neighbor_levels(ck["levels"])
        return self

    # -- block individual irregular steps inside the scheme --
    def _need_levels(self, what):
        if not hasattr(self._L, "nb_set_neighbor_levels"):
            raise NBodyError(1, "%s: the loaded library has no nb_set_neighbor_levels" % what)

    def set_neighbor_levels(self, *args, **kw):
        """set_neighbor_levels(min_level=0, eta=None, frozen=False): nb_set_neighbor_levels -- inside the neighbour scheme every
        body re-evaluates its list force at a step of its own, dt / 2^l with l in [min_level, log2(substeps)], chosen by the step
        criterion (eta None: 0.02); frozen keeps every body at min_level, or at what upload_neighbor_levels gave.  min_level is
        the accuracy floor of a run.  Needs set_neighbor_scheme first.  set_neighbor_levels(None): the shared substeps again."""
        self._need_levels("set_neighbor_levels()")
        if args == (None,) and not kw:
            self._check(self._L.nb_set_neighbor_levels(self._h, None))
            return self

        def bind(min_level=0, eta=None, frozen=False, flags=None, reserved=0):
            return min_level, eta, frozen, flags, reserved
        min_level, eta, frozen, flags, reserved = bind(*args, **kw)
        cfg = nb_neighbor_levels()
        cfg.struct_size = C.sizeof(nb_neighbor_levels)
        cfg.min_level = int(min_level)
        cfg.flags = (NLEV_FROZEN if frozen else 0) if flags is None else int(flags)
        cfg.reserved = int(reserved)
        cfg.eta = 0.0 if eta is None else float(eta)
        self._check(self._L.nb_set_neighbor_levels(self._h, C.byref(cfg)))
        return self

    def neighbor_level_stats(self, reset=False):
        """nb_neighbor_level_stats: {enabled, regular_steps, ticks, block_steps (ticks with a due body), body_steps, entries (the sum
        of min(count, cap) over the body-steps), clamped, finest_level}.  Blocks."""
        self._need_levels("neighbor_level_stats()")
        st = nb_neighbor_level_stats()
        st.struct_size = C.sizeof(nb_neighbor_level_stats)
        self._check(self._L.nb_neighbor_level_stats(self._h, C.byref(st), 1 if reset else 0))
        return {k: int(getattr(st, k)) for k in ("enabled", "regular_steps", "ticks", "block_steps", "body_steps", "entries", "clamped", "finest_level")}

    def download_neighbor_levels(self):
        """nb_download_neighbor_levels: (N,) uint8; runs the scheme's start and the levels' start first where they are not current."""
        self._need_levels("download_neighbor_levels()")
        lev = np.zeros(self.n, np.uint8)
        self._check(self._L.nb_download_neighbor_levels(self._h, _ptr(lev)))
        return lev

    def upload_neighbor_levels(self, levels):
        """nb_upload_neighbor_levels: after upload_neighbor_scheme (or any call that left the scheme current) -- the levels are
        these and the start rule does not run."""
        self._need_levels("upload_neighbor_levels()")
        lev = np.ascontiguousarray(levels, np.uint8)
        if lev.shape != (self.n,):
            raise ValueError("levels must have shape (%d,)" % self.n)
        self._check(self._L.nb_upload_neighbor_levels(self._h, _ptr(lev)))
        return self

    # -- multi-GPU / measurement / diagnostics ------------------------------
    def device_ptr(self, which):
        p = C.c_void_p()
        self._check(self._L.nb_device_ptr(self._h, {"bodies": 0, "vel": 1, "accel": 2, "jerk": 3}[which], C.byref(p)))
        return p.value

    def set_exchange(self, fn):
        """fn(bodies_dev_ptr, elem_size, n, shard_begin, shard_count, stream) -> 0."""
        if fn is None:
            self._hook = None
            self._check(self._L.nb_set_exchange(self._h, C.cast(None, EXCHANGE_FN), None))
            return

        def tramp(user, bodies, esz, n, sb, sc, stream):
            try:
                return int(fn(bodies, esz, n, sb, sc, stream) or 0)
            except Exception:  # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return -1

        self._hook = EXCHANGE_FN(tramp)  # keep alive
        self._check(self._L.nb_set_exchange(self._h, self._hook, None))

    def set_exchange_overlapped(self, begin, wait):
        """Two-phase hook (nb_set_exchange_overlapped): begin(bodies_ptr, esz, n, sb, sc,
        stream) starts the all-gather, wait(stream) makes the stream wait for it."""
        def t_begin(user, bodies, esz, n, sb, sc, stream):
            try:
                return int(begin(bodies, esz, n, sb, sc, stream) or 0)
            except Exception:
                import traceback
                traceback.print_exc()
                return -1

        def t_wait(user, stream):
            try:
                return int(wait(stream) or 0)
            except Exception:
                import traceback
                traceback.print_exc()
                return -1

        self._hook = (EXCHANGE_FN(t_begin), EXCHANGE_WAIT_FN(t_wait))  # keep alive
        self._check(self._L.nb_set_exchange_overlapped(self._h, self._hook[0], self._hook[1], None))

    def enable_timing(self, on=True):
        self._check(self._L.nb_enable_timing(self._h, 1 if on else 0))

    def kernel_times(self):
        """(avg force-kernel ms, avg integrate-kernel ms, launches) since last call."""
        f, g, c = C.c_double(), C.c_double(), C.c_uint32()
        self._check(self._L.nb_kernel_times(self._h, C.byref(f), C.byref(g), C.byref(c)))
        return f.value, g.value, c.value

    def step_times(self):
        """(force ms, integrate ms, native-RCCL exchange ms, launches) since last call."""
        f, g, x, c = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        self._check(self._L.nb_step_times(self._h, C.byref(f), C.byref(g), C.byref(x), C.byref(c)))
        return f.value, g.value, x.value, c.value

    def step_breakdown(self):
        """The parts of a step as the engine stream runs them (nb_step_times2; averages in ms since the last call):
        dict(launches, force_ms, sym_reduce_ms, reduce_scatter_ms, integrate_ms, allgather_ms, span_ms, reduce_scatters,
        allgathers)."""
        t = nb_step_timing()
        t.struct_size = C.sizeof(nb_step_timing)
        self._check(self._L.nb_step_times2(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in nb_step_timing._fields_ if k != "struct_size"}

    def integrate_pass(self, reps):
        """Average ms of the integrate kernel alone over ``reps`` launches (measurement only:
        the particle state is garbage afterwards)."""
        ms = C.c_double()
        self._check(self._L.nb_integrate_pass(self._h, int(reps), C.byref(ms)))
        return ms.value

    def force_pass(self, reps):
        """Average ms of the force pass alone over ``reps`` runs (a rank-form shard: both phases + nb_sym_reduce); no communicator
        needed, the state is left untouched.  What one rank of an N-rank partition spends in its force pass, timed on one GPU."""
        ms = C.c_double()
        self._check(self._L.nb_force_pass(self._h, int(reps), C.byref(ms)))
        return ms.value

    # -- native RCCL collective (one process per GPU) ------------------------
    def rccl_attach(self, unique_id, nranks, rank, overlap=False):
        if len(unique_id) != NB_RCCL_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % NB_RCCL_ID_BYTES)
        buf = C.create_string_buffer(bytes(unique_id), NB_RCCL_ID_BYTES)
        self._check(self._L.nb_rccl_attach(self._h, buf, int(nranks), int(rank), NB_RCCL_OVERLAP if overlap else 0))

    def rccl_detach(self):
        self._check(self._L.nb_rccl_detach(self._h))

    def rccl_info(self):
        """(nranks, rank, rccl version code) of the attached communicator; zeros when none."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.nb_rccl_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- viewer frame feed (nbody3d.js:408-415,482-487; colour input :380) ----
    def request_frame(self):
        self._check(self._L.nb_frame_request(self._h))

    def frame(self, wait=True):
        """Newest finished frame: (bodies f32 (n,4), speed f32 (n,), step index) -- views of the
        engine's pinned host memory, valid until the fourth request_frame() after the one that
        produced them AND no longer than the handle itself (close() frees the memory: copy what
        must outlive it); None when wait=False and nothing has landed yet."""
        pb, ps, st = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_uint64()
        rc = self._L.nb_frame_acquire(self._h, 1 if wait else 0, C.byref(pb), C.byref(ps), C.byref(st))
        if rc == NB_NOT_READY:
            return None
        self._check(rc)
        b = np.ctypeslib.as_array(pb, shape=(self.n, 4))
        sp = np.ctypeslib.as_array(ps, shape=(self.n,))
        return b, sp, st.value

    @property
    def variant(self):
        return self._L.nb_variant_name(self._h).decode()

    def shape_info(self):
        """{jsplit, j_per_split, own_split0, own_splits}: the force pass's j-partitions and those that lie entirely
        inside this handle's own rows (what the overlapped exchange issues before waiting for the gather)."""
        v = [C.c_uint32() for _ in range(4)]
        self._check(self._L.nb_shape_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("jsplit", "j_per_split", "own_split0", "own_splits"), (x.value for x in v)))

    @property
    def eqm(self):
        """Whether the next force pass runs the equal-mass kernels (NB_FLAG_NO_EQM; nb_eqm_info).  A property of its own and not a key
        of shape_info(): that dict is compared whole with the planner's answer, and this is a fact of the uploaded state, not of the plan."""
        if not hasattr(self._L, "nb_eqm_info"):
            return False
        v = C.c_int()
        self._check(self._L.nb_eqm_info(self._h, C.byref(v)))
        return bool(v.value)

    @property
    def eqm_form(self):
        """The form of the force kernels the next force pass runs (nb_eqm_form): 0 the general kernels, 1 the equal-mass kernels, 2 the
        equal-mass kernels with unit mass product (G*m a power of two; NB_FLAG_NO_EQM_POW2 keeps form 1).  An older library: eqm as 0 / 1."""
        if not hasattr(self._L, "nb_eqm_form"):
            return int(self.eqm)
        v = C.c_int()
        self._check(self._L.nb_eqm_form(self._h, C.byref(v)))
        return int(v.value)

    def diagnostics(self):
        """(kinetic, potential share, momentum[3]) of this handle's shard, fp64 on device."""
        out = (C.c_double * 5)()
        self._check(self._L.nb_diagnostics(self._h, out))
        return out[0], out[1], np.array(out[2:5])

    def _shape(self, getter, names, *args):
        """What the ``*_shape`` methods share: {name: value} of the uint32 outputs of an nb_*_shape getter."""
        v = [C.c_uint32() for _ in names]
        self._check(getter(self._h, *args, *[C.byref(x) for x in v]))
        return dict(zip(names, (x.value for x in v)))

    def field(self, points=None, *, bodies=None, accel=True, phi=True, f64=False):
        """nb_field_eval: acceleration and potential of the system at ``points`` ((m, 3) or (m, 4); the fourth column is ignored)
        or, with ``bodies=(first, count)``, at the current positions of those bodies, each leaving itself out of its sums.
        Returns ``(accel (m, 4) | None, phi (m,) | None)`` in the handle's precision, float64 with ``f64=True`` (fp64 arithmetic on
        the stored rows: the audit of the f32 sums).  Uses the handle's eps2 and the G of the last set_params(); the positions are
        those behind every step issued so far; the simulation state is not touched."""
        req, pts, a, f = _field_request(self.n, self.dtype, points, bodies, accel, phi, f64)
        self._check(self._L.nb_field_eval(self._h, C.byref(req)))
        return a, f

    def field_device(self, points_ptr, m, accel_ptr, phi_ptr, *, bodies=None, f64=False):
        """The device-pointer form (NB_FIELD_DEVICE): ``points_ptr`` / ``accel_ptr`` / ``phi_ptr`` are device addresses on the handle's
        device (e.g. ``tensor.data_ptr()``; 0 or None for an output that is not wanted), element types as for field().  The work is
        enqueued on the handle's stream and the call returns without waiting.  ``bodies=(first, count)`` selects the bodies' own
        positions (``points_ptr`` must then be None and ``m`` is ignored)."""
        if self._L.nb_abi_minor() < 4:
            raise NBodyError(1, "field_device(): the loaded library is ABI %d.%d; nb_field_eval needs 2.4" % (abi_version(), abi_minor()))
        req = _device_request(nb_field_request, NB_FIELD_DEVICE | (NB_FIELD_F64 if f64 else 0), NB_FIELD_AT_BODIES, m, bodies, points_ptr)
        req.accel = accel_ptr or None
        req.phi = phi_ptr or None
        self._check(self._L.nb_field_eval(self._h, C.byref(req)))

    def neighbors(self, points=None, *, bodies=None, radius=None, radii=None):
        """nb_neighbors: for each of ``points`` ((m, 3) or (m, 4); the fourth column is ignored) -- or, with ``bodies=(first, count)``,
        for each of those bodies, itself left out by index -- the nearest body, its squared distance (plain, unsoftened, the handle's
        precision) and, with ``radius`` (one for all) or ``radii`` (one per point), the number of bodies strictly closer than that.
        Returns ``(index (m,) uint32, dist2 (m,), count (m,) uint32 | None)``; index is NB_NBR_NONE and dist2 +inf where there is no
        candidate.  Equal distances: the smallest index.  The positions are those behind every step issued so far; the simulation
        state is not touched; the answer for a point does not depend on the other points of the request."""
        req, keep, index, dist2, count = _neighbor_request(self.dtype, points, bodies, radius, radii)
        self._check(self._L.nb_neighbors(self._h, C.byref(req)))
        return index, dist2, count

    def neighbors_device(self, points_ptr, m, index_ptr, dist2_ptr, count_ptr=None, *, bodies=None, radius=None, radii_ptr=None):
        """The device-pointer form (NB_NBR_DEVICE): device addresses on the handle's device (e.g. ``tensor.data_ptr()``; 0 or None for
        what is not wanted), element types as for neighbors().  The work is enqueued on the handle's stream and the call returns
        without waiting.  ``bodies=(first, count)`` selects the bodies themselves (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_neighbors", "neighbors_device()")
        req = _device_request(nb_neighbor_request, NB_NBR_DEVICE, NB_NBR_AT_BODIES, m, bodies, points_ptr)
        req.radii = radii_ptr or None
        req.radius = 0.0 if radius is None else float(radius)
        req.index = index_ptr or None
        req.dist2 = dist2_ptr or None
        req.count = count_ptr or None
        self._check(self._L.nb_neighbors(self._h, C.byref(req)))

    def neighbors_shape(self, m):
        """{batch, chunks, j_per_chunk}: the launch shape nb_neighbors gives an m-point request (the answers do not depend on it)."""
        _need("nb_neighbors", "neighbors_shape()")
        return self._shape(self._L.nb_neighbors_shape, ("batch", "chunks", "j_per_chunk"), int(m))

    def neighbor_lists(self, points=None, *, bodies=None, radius=None, radii=None, cap=64, nearest=False):
        """nb_neighbor_lists: WHICH bodies lie strictly inside ``radius`` (one for all) or ``radii`` (one per point) of each of
        ``points`` -- or, with ``bodies=(first, count)``, of each of those bodies, itself left out by index.  Returns ``(lists (m, cap)
        uint32, count (m,) uint32)``, and with ``nearest`` also ``index`` and ``dist2`` as neighbors() returns them.  Row k holds the
        members in ascending order, padded with NB_NBR_NONE; ``count`` is the true number of members (what neighbors() counts, bit
        for bit): where it exceeds ``cap`` the row holds the cap smallest indices.  See lists_to_csr()."""
        req, keep, lists, count, index, dist2 = _neighbor_list_request(self.dtype, points, bodies, radius, radii, cap, nearest)
        self._check(self._L.nb_neighbor_lists(self._h, C.byref(req)))
        return (lists, count, index, dist2) if nearest else (lists, count)

    def neighbor_lists_device(self, points_ptr, m, list_ptr, cap, count_ptr=None, index_ptr=None, dist2_ptr=None, *, bodies=None,
                              radius=None, radii_ptr=None):
        """The device-pointer form (NB_NBR_DEVICE): device addresses on the handle's device (0 or None for what is not wanted);
        ``list_ptr``: m * cap uint32.  Enqueued on the handle's stream, returns without waiting.  ``bodies=(first, count)`` selects the
        bodies themselves (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_neighbor_lists", "neighbor_lists_device()")
        req = _device_request(nb_neighbor_list_request, NB_NBR_DEVICE, NB_NBR_AT_BODIES, m, bodies, points_ptr)
        req.radii = radii_ptr or None
        req.radius = 0.0 if radius is None else float(radius)
        req.cap = int(cap)
        req.list = list_ptr or None
        req.count = count_ptr or None
        req.index = index_ptr or None
        req.dist2 = dist2_ptr or None
        self._check(self._L.nb_neighbor_lists(self._h, C.byref(req)))

    def neighbor_lists_shape(self, m, cap):
        """{batch, chunks, j_per_chunk}: the launch shape nb_neighbor_lists gives an m-point request with rows of ``cap`` entries (the
        answers do not depend on it)."""
        _need("nb_neighbor_lists", "neighbor_lists_shape()")
        return self._shape(self._L.nb_neighbor_lists_shape, ("batch", "chunks", "j_per_chunk"), int(m), int(cap))

    def list_force(self, lists, *, bodies=None, points=None, point_vel=None, count=None, accel=True, jerk=False, phi=False):
        """nb_list_force: acceleration, jerk and potential summed over the entries of each row of ``lists`` ((m, cap) uint32: the
        rows neighbor_lists() or knn() return, or any other) at ``points`` ((m, 3) or (m, 4)) -- or, with ``bodies=(first, m)``, at
        those bodies, an entry equal to the row's own body skipped.  ``count`` ((m,) uint32): only the first min(count, cap) entries
        of a row are read.  An entry >= n (the padding NB_NBR_NONE, wherever it stands) adds nothing.  ``jerk`` needs a Hermite handle
        and, at points, ``point_vel``.  Returns ``(accel (m, 4) | None, jerk (m, 4) | None, phi (m,) | None)``.  A row's outputs depend
        on its entries, its point and the bodies only -- bit for bit, whatever m, cap and count are."""
        req, keep, a, j, f = _list_force_request(self.dtype, lists, bodies, points, point_vel, count, accel, jerk, phi)
        self._check(self._L.nb_list_force(self._h, C.byref(req)))
        return a, j, f

    def list_force_device(self, list_ptr, m, cap, *, bodies=None, points_ptr=None, point_vel_ptr=None, count_ptr=None,
                          accel_ptr=None, jerk_ptr=None, phi_ptr=None):
        """The device-pointer form (NB_LISTF_DEVICE): device addresses on the handle's device (0 or None for what is not wanted);
        ``list_ptr``: m * cap uint32, ``count_ptr``: m uint32, the outputs as list_force() returns them.  Read and written in place,
        enqueued on the handle's stream, returns without waiting.  ``bodies=(first, count)`` selects the bodies themselves
        (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_list_force", "list_force_device()")
        req = _device_request(nb_list_force_request, NB_LISTF_DEVICE, NB_LISTF_AT_BODIES, m, bodies, points_ptr)
        req.point_vel = point_vel_ptr or None
        req.list = list_ptr or None
        req.count = count_ptr or None
        req.cap = int(cap)
        req.accel = accel_ptr or None
        req.jerk = jerk_ptr or None
        req.phi = phi_ptr or None
        self._check(self._L.nb_list_force(self._h, C.byref(req)))

    def list_force_shape(self, m, cap):
        """{batch, lanes_per_row}: the rows of every batch but the last that a host-pointer nb_list_force request of m rows at ``cap``
        entries is staged in, and the lanes that share one row (the answers depend on neither m nor the batch)."""
        _need("nb_list_force", "list_force_shape()")
        return self._shape(self._L.nb_list_force_shape, ("batch", "lanes_per_row"), int(m), int(cap))

    def irregular_force(self, radius, cap=128, *, jerk=None, phi=False):
        """The irregular force of an Ahmad-Cohen split at every body: nb_neighbor_lists with ``radius`` and rows of ``cap`` entries,
        then nb_list_force over those rows, both with device pointers on the handle's stream -- the rows never visit the host.
        ``jerk`` defaults to what the handle can give (Hermite handles: True).  Returns ``(accel (n, 4), jerk (n, 4) | None, phi (n,) |
        None, count (n,) uint32)``; where count exceeds cap the sums run over the cap members with the smallest indices."""
        _need("nb_list_force", "irregular_force()")
        import torch
        jerk = (self.integrator != "leapfrog") if jerk is None else bool(jerk)
        n, cap = self.n, int(cap)
        if not 1 <= cap <= 4096:
            raise ValueError("irregular_force(): cap must be in 1 .. 4096")
        dev = torch.device("cuda", torch.cuda.current_device() if self._device < 0 else self._device)
        tt = torch.float64 if self.dtype == np.float64 else torch.float32
        lst = torch.empty((n, cap), dtype=torch.int32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev)
        a = torch.empty((n, 4), dtype=tt, device=dev)
        j = torch.empty((n, 4), dtype=tt, device=dev) if jerk else None
        f = torch.empty((n,), dtype=tt, device=dev) if phi else None
        # The buffers come from torch's allocator on torch's CURRENT stream and are used on the HANDLE's stream.  Two waits make that
        # safe, and both are needed: this one (whatever torch still runs on a recycled block has finished before the engine writes
        # it) and self.sync() below (the engine has finished before torch reads the buffers or takes them back).
        torch.cuda.current_stream(dev).synchronize()
        self.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=radius)
        self.list_force_device(lst.data_ptr(), 0, cap, bodies=(0, n), count_ptr=cnt.data_ptr(), accel_ptr=a.data_ptr(),
                               jerk_ptr=j.data_ptr() if jerk else None, phi_ptr=f.data_ptr() if phi else None)
        self.sync()
        host = lambda t: None if t is None else t.cpu().numpy()
        return host(a), host(j), host(f), cnt.cpu().numpy().view(np.uint32)

    def split_force(self, points=None, *, bodies=None, point_vel=None, radius=None, radii=None, jerk=None):
        """nb_split_force: the acceleration (and, on Hermite handles, the jerk) of ALL bodies at ``points`` ((m, 3) or (m, 4)) -- or,
        with ``bodies=(first, m)``, at those bodies --, every pair's term added to exactly one of two sums: ``*_irr`` over the bodies
        with d2 < h^2 (``radius``, or one of ``radii`` per point; nb_neighbors' strict rule), ``*_reg`` over every other row.  One
        pass, nothing subtracted.  ``jerk`` defaults to what the handle can give (Hermite handles: True) and needs, at points,
        ``point_vel``.  Returns a dict of (m, 4) arrays: accel_irr, accel_reg[, jerk_irr, jerk_reg]."""
        jerk = (self.integrator != "leapfrog") if jerk is None else bool(jerk)
        req, keep, out = _split_force_request(self.dtype, points, bodies, point_vel, radius, radii, jerk)
        self._check(self._L.nb_split_force(self._h, C.byref(req)))
        return out

    def split_force_device(self, m, *, bodies=None, points_ptr=None, point_vel_ptr=None, radius=None, radii_ptr=None,
                           accel_irr_ptr=None, accel_reg_ptr=None, jerk_irr_ptr=None, jerk_reg_ptr=None):
        """The device-pointer form (NB_SPLIT_DEVICE): device addresses on the handle's device (0 or None for what is not wanted), the
        outputs as split_force() returns them.  Read and written in place, enqueued on the handle's stream, returns without
        waiting.  ``bodies=(first, count)`` selects the bodies themselves (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_split_force", "split_force_device()")
        req = _device_request(nb_split_force_request, NB_SPLIT_DEVICE, NB_SPLIT_AT_BODIES, m, bodies, points_ptr)
        req.point_vel = point_vel_ptr or None
        req.radii = radii_ptr or None
        req.radius = 0.0 if radius is None else float(radius)
        req.accel_irr = accel_irr_ptr or None
        req.accel_reg = accel_reg_ptr or None
        req.jerk_irr = jerk_irr_ptr or None
        req.jerk_reg = jerk_reg_ptr or None
        self._check(self._L.nb_split_force(self._h, C.byref(req)))

    def split_force_shape(self, m):
        """{batch, chunks, j_per_chunk, rows_per_workgroup}: the launch shape nb_split_force gives an m-point request (on a Hermite
        handle: one with the jerk pair)."""
        _need("nb_split_force", "split_force_shape()")
        return self._shape(self._L.nb_split_force_shape, ("batch", "chunks", "j_per_chunk", "rows_per_workgroup"), int(m))

    def split_lists(self, points=None, *, bodies=None, point_vel=None, radius=None, radii=None, jerk=None, cap=64):
        """nb_split_lists: split_force()'s sums AND neighbor_lists()' rows from one pass over the pairs, cut by one comparison.
        Returns split_force()'s dict with two more keys: ``list`` ((m, cap) uint32: the members in ascending order, padded with
        NB_NBR_NONE, the cap smallest where there are more) and ``count`` ((m,) uint32: the true number of members) -- bit for bit
        what neighbor_lists() returns; with ``bodies=(first, m)`` a body leaves itself out of its row by index (not out of its
        sums, where it adds an exact 0).  The sums are split_force()'s bits wherever split_lists_shape() equals split_force_shape()."""
        jerk = (self.integrator != "leapfrog") if jerk is None else bool(jerk)
        req, keep, out = _split_lists_request(self.dtype, points, bodies, point_vel, radius, radii, jerk, cap)
        self._check(self._L.nb_split_lists(self._h, C.byref(req)))
        return out

    def split_lists_device(self, m, list_ptr, cap, count_ptr=None, *, bodies=None, points_ptr=None, point_vel_ptr=None, radius=None,
                           radii_ptr=None, accel_irr_ptr=None, accel_reg_ptr=None, jerk_irr_ptr=None, jerk_reg_ptr=None):
        """The device-pointer form (NB_SPLIT_DEVICE): device addresses on the handle's device (0 or None for what is not wanted);
        ``list_ptr``: m * cap uint32, ``count_ptr``: m uint32, the sums as split_force_device() takes them.  Read and written in
        place, enqueued on the handle's stream, returns without waiting.  ``bodies=(first, count)`` selects the bodies themselves
        (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_split_lists", "split_lists_device()")
        req = _device_request(nb_split_lists_request, NB_SPLIT_DEVICE, NB_SPLIT_AT_BODIES, m, bodies, points_ptr)
        req.point_vel = point_vel_ptr or None
        req.radii = radii_ptr or None
        req.radius = 0.0 if radius is None else float(radius)
        req.accel_irr = accel_irr_ptr or None
        req.accel_reg = accel_reg_ptr or None
        req.jerk_irr = jerk_irr_ptr or None
        req.jerk_reg = jerk_reg_ptr or None
        req.cap = int(cap)
        req.list = list_ptr or None
        req.count = count_ptr or None
        self._check(self._L.nb_split_lists(self._h, C.byref(req)))

    def split_lists_shape(self, m, cap):
        """{batch, chunks, j_per_chunk, rows_per_workgroup}: the launch shape nb_split_lists gives an m-point request with rows of
        ``cap`` entries (on a Hermite handle: one with the jerk pair) -- split_force_shape()'s wherever the segments fit their bound."""
        _need("nb_split_lists", "split_lists_shape()")
        return self._shape(self._L.nb_split_lists_shape, ("batch", "chunks", "j_per_chunk", "rows_per_workgroup"), int(m), int(cap))

    def knn(self, points=None, *, bodies=None, k=6, dist2=True):
        """nb_knn: the ``k`` nearest bodies (1 <= k <= 64) of each of ``points`` ((m, 3) or (m, 4); the fourth column is ignored) --
        or, with ``bodies=(first, count)``, of each of those bodies, itself left out by index.  Returns ``(index (m, k) uint32,
        dist2 (m, k) | None)``: row r holds the k smallest candidates in the order (d2 ascending, then index ascending), d2 the
        plain squared distance of neighbors(); with fewer than k candidates the rest of the row is NB_NBR_NONE / +inf.  Column 0
        is what neighbors() returns, bit for bit; the row for a smaller k is the start of the row for a larger one."""
        req, keep, index, d2 = _knn_request(self.dtype, points, bodies, k, dist2)
        self._check(self._L.nb_knn(self._h, C.byref(req)))
        return index, d2

    def knn_device(self, points_ptr, m, k, index_ptr, dist2_ptr=None, *, bodies=None):
        """The device-pointer form (NB_NBR_DEVICE): device addresses on the handle's device (0 or None for what is not wanted);
        ``index_ptr``: m * k uint32, ``dist2_ptr``: m * k elements of the handle's precision.  Enqueued on the handle's stream, returns
        without waiting.  ``bodies=(first, count)`` selects the bodies themselves (``points_ptr`` must then be None, ``m`` is ignored)."""
        _need("nb_knn", "knn_device()")
        req = _device_request(nb_knn_request, NB_NBR_DEVICE, NB_NBR_AT_BODIES, m, bodies, points_ptr)
        req.k = int(k)
        req.index = index_ptr or None
        req.dist2 = dist2_ptr or None
        self._check(self._L.nb_knn(self._h, C.byref(req)))

    def knn_shape(self, m, k):
        """{batch, chunks, j_per_chunk}: the launch shape nb_knn gives an m-point request for k neighbours (the answers do not depend
        on it)."""
        _need("nb_knn", "knn_shape()")
        return self._shape(self._L.nb_knn_shape, ("batch", "chunks", "j_per_chunk"), int(m), int(k))

    def local_density(self, k=6):
        """The Casertano-Hut density at every body, (n,) float64: one knn(bodies=(0, n), k=k) call and density_from_knn() on its
        result (``nan`` for every body when n - 1 < k)."""
        return self._local_density(k)[1]

    def _local_density(self, k):
        index, d2 = self.knn(bodies=(0, self.n), k=k)
        b = self.read(vel=False, accel=False)[0]
        return b, density_from_knn(b, index, d2)

    def density_center(self, k=6):
        """The density centre of the system, (3,) float64: sum(rho x) / sum(rho) over the bodies with a density (local_density(k))."""
        b, rho = self._local_density(k)
        ok = np.isfinite(rho)
        return (rho[ok, None] * b[ok, :3].astype(np.float64)).sum(axis=0) / rho[ok].sum()

    def all_close_pairs(self, radius, cap=64):
        """EVERY unordered pair i < j of bodies with d2 < radius^2 (close_pairs() gives the mutual-nearest ones only), as ``(k, 2)
        uint32`` sorted by i, then j -- one neighbor_lists(bodies=(0, n)) call and host code on its result.  Raises ValueError if a
        body has more than ``cap`` neighbours inside the radius."""
        lists, count = self.neighbor_lists(bodies=(0, self.n), radius=radius, cap=cap)
        return pairs_from_lists(lists, count)

    def close_pairs(self, radius):
        """The close pairs of the system: the MUTUAL nearest neighbours (i < j, each the other's nearest body) closer than ``radius``,
        as ``(pairs (k, 2) uint32 sorted by i, d2 (k,))`` -- one neighbors(bodies=(0, n)) call and host code on its result."""
        index, dist2, _ = self.neighbors(bodies=(0, self.n))
        return mutual_pairs(index, dist2, radius)

    def body_energies(self):
        """Per-body energies as two float64 arrays ``(kinetic, potential)``: ``0.5 m_i |v_i|^2`` and ``m_i phi_i``, phi_i the potential
        of all OTHER bodies at body i (one field(bodies=(0, n)) call plus read()).  A body is bound when the two add up to less
        than 0; the potential energy of the system is HALF the sum of the second array (every pair appears in two of its
        entries).  Time pairing: the stored velocities lag the positions by one step, so after a step the two
        arrays belong to different times -- read right after init() they pair exactly."""
        b, v, _ = self.read(accel=False)
        _, p = self.field(bodies=(0, self.n), accel=False, phi=True)
        m = b[:, 3].astype(np.float64)
        v = v[:, :3].astype(np.float64)
        return 0.5 * m * (v * v).sum(1), m * p.astype(np.float64)

    def energy_drift(self, steps, every):
        """Runs ``steps`` steps (parameters as set) and samples the total energy every ``every`` steps with the bookkeeping of
        SURVEY.md §8(c): the stored velocity lags the positions by one call (nbody3d.js:278-283), so KE(vel after call n) pairs
        with PE(positions BEFORE call n); E0 pairs the uploaded state.  Returns [|E_n - E0| / |E0|] at the sampled steps."""
        ke0, pe0, _ = self.diagnostics()
        e0 = ke0 + pe0
        out, done = [], 0
        while done < steps:
            k = min(int(every), steps - done)
            if k > 1:
                self.simulate(k - 1)
            _, pe_prev, _ = self.diagnostics()
            self.step()
            ke, _, _ = self.diagnostics()
            done += k
            out.append(abs((ke + pe_prev - e0) / e0))
        return out


class MultiSimulation:
    """Single-process multi-device handle (nb_multi_*): n_shards i-shards, one per
    entry of ``devices`` (default: round-robin over the visible GPUs; several
    shards may share a GPU), peer-copy all-gather after every step.  Same
    host-side surface as Simulation; arrays hold the unpadded n rows."""

    def __init__(self, n, n_shards, devices=None, precision="f32", eps2=None, force_variant=0, jsplit=0,
                 collective="peer"):
        L = load_library()
        self._L = L
        self.n, self.n_shards = int(n), int(n_shards)
        self.dtype = np.float64 if precision in ("f64", NB_F64, np.float64) else np.float32
        cfg = nb_config()
        cfg.struct_size = C.sizeof(nb_config)
        cfg.n = self.n
        cfg.precision = NB_F64 if self.dtype == np.float64 else NB_F32
        cfg.eps2 = 0.0 if eps2 is None else float(eps2)
        cfg.device = -1
        cfg.force_variant, cfg.jsplit = force_variant, jsplit
        dev = None
        if devices is not None:
            assert len(devices) == self.n_shards
            dev = (C.c_int32 * self.n_shards)(*devices)
        h = C.c_void_p()
        rc = L.nb_multi_create(C.byref(cfg), self.n_shards, dev, C.byref(h))
        if rc != 0:
            raise NBodyError(rc, L.nb_multi_last_error(None).decode())
        self._h = h
        self.dt = self.G = 0.0
        if collective != "peer":
            try:
                self.set_collective(collective)
            except Exception:
                self.close()
                raise

    def set_collective(self, mode):
        """'peer' (event-ordered device-to-device copies) or 'rccl' (ncclCommInitAll + grouped
        in-place ncclAllGather); bit-identical results."""
        self._check(self._L.nb_multi_set_collective(self._h, {"peer": NB_MULTI_PEER, "rccl": NB_MULTI_RCCL, "peer_overlap": NB_MULTI_PEER_OVERLAP}[mode]))

    def collective_info(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.nb_multi_collective_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"mode": {NB_MULTI_RCCL: "rccl", NB_MULTI_PEER_OVERLAP: "peer_overlap"}.get(a.value, "peer"), "nranks": b.value, "rccl_version": c.value}

    def close(self):
        if getattr(self, "_h", None):
            self._L.nb_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise NBodyError(rc, self._L.nb_multi_last_error(self._h).decode())

    def _arr(self, a, name):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.size != 4 * self.n:
            raise ValueError("%s must hold 4*n = %d elements, got %d" % (name, 4 * self.n, a.size))
        return a

    def init(self, bodies, vel, accel=None):
        b, v = self._arr(bodies, "bodies"), self._arr(vel, "vel")
        a = None if accel is None else self._arr(accel, "accel")
        self._check(self._L.nb_multi_upload(self._h, _ptr(b), _ptr(v), _ptr(a)))
        return self

    restore = init

    def set_params(self, dt, G):
        self.dt, self.G = float(dt), float(G)
        self._check(self._L.nb_multi_set_params(self._h, self.dt, self.G))

    def step(self, dt=None, G=None):
        self.simulate(1, dt, G)

    def simulate(self, nsteps, dt=None, G=None):
        if dt is not None or G is not None:
            self.set_params(self.dt if dt is None else dt, self.G if G is None else G)
        self._check(self._L.nb_multi_step(self._h, int(nsteps)))

    def sync(self):
        self._check(self._L.nb_multi_sync(self._h))

    def read(self, bodies=True, vel=True, accel=True):
        out = [np.zeros((self.n, 4), self.dtype) if f else None for f in (bodies, vel, accel)]
        self._check(self._L.nb_multi_download(self._h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def diagnostics(self):
        out = (C.c_double * 5)()
        self._check(self._L.nb_multi_diagnostics(self._h, out))
        return out[0], out[1], np.array(out[2:5])

    def field(self, points=None, *, bodies=None, accel=True, phi=True, f64=False):
        """nb_multi_field_eval: Simulation.field() on the whole system (evaluated on shard 0, which holds every row);
        ``bodies=(first, count)`` counts the caller's unpadded rows."""
        req, pts, a, f = _field_request(self.n, self.dtype, points, bodies, accel, phi, f64)
        self._check(self._L.nb_multi_field_eval(self._h, C.byref(req)))
        return a, f

    def neighbors(self, points=None, *, bodies=None, radius=None, radii=None):
        """nb_multi_neighbors: Simulation.neighbors() on the whole system (evaluated on shard 0 against the caller's unpadded rows);
        ``bodies=(first, count)`` counts the caller's unpadded rows."""
        req, keep, index, dist2, count = _neighbor_request(self.dtype, points, bodies, radius, radii)
        self._check(self._L.nb_multi_neighbors(self._h, C.byref(req)))
        return index, dist2, count

    def neighbor_lists(self, points=None, *, bodies=None, radius=None, radii=None, cap=64, nearest=False):
        """nb_multi_neighbor_lists: Simulation.neighbor_lists() on the whole system (evaluated on shard 0 against the caller's
        unpadded rows: a padding row is never listed); ``bodies=(first, count)`` counts the caller's unpadded rows."""
        req, keep, lists, count, index, dist2 = _neighbor_list_request(self.dtype, points, bodies, radius, radii, cap, nearest)
        self._check(self._L.nb_multi_neighbor_lists(self._h, C.byref(req)))
        return (lists, count, index, dist2) if nearest else (lists, count)

    def list_force(self, lists, *, bodies=None, points=None, point_vel=None, count=None, accel=True, jerk=False, phi=False):
        """nb_multi_list_force: Simulation.list_force() on the whole system (evaluated on shard 0 against the caller's unpadded
        rows); ``jerk`` is refused (NB_ERR_INVALID): the shards are leapfrog handles."""
        req, keep, a, j, f = _list_force_request(self.dtype, lists, bodies, points, point_vel, count, accel, jerk, phi)
        self._check(self._L.nb_multi_list_force(self._h, C.byref(req)))
        return a, j, f

    def split_lists(self, points=None, *, bodies=None, point_vel=None, radius=None, radii=None, jerk=False, cap=64):
        """nb_multi_split_lists: Simulation.split_lists() on the whole system (evaluated on shard 0 against the caller's unpadded
        rows; ``jerk`` must stay False: the shards are leapfrog handles)."""
        req, keep, out = _split_lists_request(self.dtype, points, bodies, point_vel, radius, radii, jerk, cap)
        self._check(self._L.nb_multi_split_lists(self._h, C.byref(req)))
        return out

    def split_force(self, points=None, *, bodies=None, point_vel=None, radius=None, radii=None, jerk=False):
        """nb_multi_split_force: Simulation.split_force() on the whole system (evaluated on shard 0 against the caller's unpadded
        rows); ``jerk`` is refused (NB_ERR_INVALID): the shards are leapfrog handles."""
        req, keep, out = _split_force_request(self.dtype, points, bodies, point_vel, radius, radii, jerk)
        self._check(self._L.nb_multi_split_force(self._h, C.byref(req)))
        return out

    def knn(self, points=None, *, bodies=None, k=6, dist2=True):
        """nb_multi_knn: Simulation.knn() on the whole system (evaluated on shard 0 against the caller's unpadded rows: a padding
        row is never returned); ``bodies=(first, count)`` counts the caller's unpadded rows."""
        req, keep, index, d2 = _knn_request(self.dtype, points, bodies, k, dist2)
        self._check(self._L.nb_multi_knn(self._h, C.byref(req)))
        return index, d2

    @property
    def variant(self):
        return self._L.nb_multi_variant_name(self._h).decode()
