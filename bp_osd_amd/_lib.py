"""ctypes loader for libbposd_mi355x.so (the C-ABI in include/bposd_mi355x.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``bp_osd_amd.build.build_library()`` with hipcc for gfx950.  There is no fallback:
if the library is missing, importing the decoder raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BPOSD_LIB") or os.path.join(_HERE, "libbposd_mi355x.so")

BPOSD_OK = 0
BPOSD_ERR_INVALID = -1
BPOSD_ERR_UNSUPPORTED = -2
BPOSD_ERR_HIP = -3
BPOSD_ERR_NO_DEVICE = -4

# every symbol include/bposd_mi355x.h declares
EXPORTED_SYMBOLS = (
    "bposd_device_count",
    "bposd_version",
    "bposd_create",
    "bposd_update_channel_probs",
    "bposd_decode_batch",
    "bposd_decode_batch_packed",
    "bposd_decode_batch_async",
    "bposd_decode_batch_packed_async",
    "bposd_decode_batch_device",
    "bposd_decode_batch_device_packed",
    "bposd_decode_batch_select",
    "bposd_decode_batch_select_device",
    "bposd_channel_tables",
    "bposd_decode_batch_rows",
    "bposd_decode_batch_rows_device",
    "bposd_pack_rows_device",
    "bposd_pack_rows_device_lane",
    "bposd_observable_table",
    "bposd_set_observables",
    "bposd_observables_device_lane",
    "bposd_decode_batch_observables_device",
    "bposd_decode_batch_observables",
    "bposd_decode_batch_observables_packed",
    "bposd_decode_batch_observables_async",
    "bposd_decode_batch_observables_packed_async",
    "bposd_synchronize",
    "bposd_num_lanes",
    "bposd_last_lane",
    "bposd_synchronize_lane",
    "bposd_lane_timing",
    "bposd_host_alloc",
    "bposd_host_free",
    "bposd_last_timing",
    "bposd_info",
    "bposd_posterior_llr",
    "bposd_set_bp_variant",
    "bposd_set_relay",
    "bposd_relay_stats",
    "bposd_set_lsd",
    "bposd_lsd_stats",
    "bposd_set_lsd_order",
    "bposd_lsd_order_stats",
    "bposd_set_osd_variant",
    "bposd_last_osd_kernel",
    "bposd_mc_create",
    "bposd_mc_run",
    "bposd_mc_fetch",
    "bposd_mc_device_bytes",
    "bposd_mc_last_error",
    "bposd_mc_destroy",
    "bposd_dem_tables",
    "bposd_dem_create",
    "bposd_dem_set_sampling",
    "bposd_dem_set_subset",
    "bposd_dem_set_harvest",
    "bposd_dem_harvest_info",
    "bposd_dem_fault_sums",
    "bposd_dem_sample",
    "bposd_dem_run",
    "bposd_dem_fetch",
    "bposd_dem_device_bytes",
    "bposd_dem_last_error",
    "bposd_dem_destroy",
    "bposd_window_create",
    "bposd_window_decode_device",
    "bposd_window_synchronize",
    "bposd_window_decode",
    "bposd_window_run",
    "bposd_window_set_harvest",
    "bposd_window_harvest_info",
    "bposd_window_fetch",
    "bposd_window_device_bytes",
    "bposd_window_last_error",
    "bposd_window_destroy",
    "bposd_frame_create",
    "bposd_frame_columns",
    "bposd_frame_fetch",
    "bposd_frame_device_bytes",
    "bposd_frame_last_error",
    "bposd_frame_destroy",
    "bposd_last_error",
    "bposd_destroy",
)

# include/bposd_mi355x_debug.h: diagnostics (which kernel ran, LDS layout models and tables)
DEBUG_SYMBOLS = (
    "bposd_layout_info",
    "bposd_bp_kernel_info",
    "bposd_debug_local_layout",
    "bposd_debug_host_chunks",
    "bposd_debug_local_keys",
    "bposd_debug_local_waves",
    "bposd_debug_last_pair_key",
    "bposd_debug_set_park",
    "bposd_debug_last_parked",
    "bposd_debug_lsd_launches",
    "bposd_debug_obs_timing",
    "bposd_debug_dem_timing",
    "bposd_debug_dem_harvest",
    "bposd_debug_dem_harvest_timing",
    "bposd_debug_dem_fault_sums",
    "bposd_debug_dem_fault_sums_timing",
    "bposd_debug_window_step",
    "bposd_debug_window_timing",
    "bposd_debug_frame_timing",
    "bposd_debug_class_layout",
    "bposd_debug_last_instance",
    "bposd_debug_portable_math",
)


class BposdConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("bp_method", C.c_int32),
        ("ms_scaling_factor", C.c_double),
        ("max_iter", C.c_int32),
        ("osd_method", C.c_int32),
        ("osd_order", C.c_int32),
        ("sort_tie_policy", C.c_int32),
        ("weight_fn", C.c_int32),
        ("schedule", C.c_int32),
        ("ps_clip", C.c_double),
        ("osd_e_bit_order", C.c_int32),
        ("ps_math_form", C.c_int32),
    ]


class BposdMcConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("channel_update", C.c_int32),
        ("seed", C.c_uint64),
        ("capacity", C.c_int64),
    ]


class BposdDemConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("seed", C.c_uint64),
        ("capacity", C.c_int64),
    ]


class BposdWindowConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("capacity", C.c_int64),
    ]


class BposdFrameConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("layered", C.c_int32),
        ("max_words", C.c_int64),
        ("workspace_bytes", C.c_int64),
    ]


class BposdWindowStep(C.Structure):
    """bposd_window_step_args of include/bposd_mi355x_debug.h (every pointer a host pointer)."""
    _fields_ = [
        ("device", C.c_int32),
        ("M", C.c_int32),
        ("N", C.c_int32),
        ("k", C.c_int32),
        ("h_indptr", C.c_void_p),
        ("h_indices", C.c_void_p),
        ("l_indptr", C.c_void_p),
        ("l_indices", C.c_void_p),
        ("B", C.c_int64),
        ("n_commit", C.c_int32),
        ("commit_pos", C.c_void_p),
        ("commit_fault", C.c_void_p),
        ("decoded_cols", C.c_int32),
        ("decoded_packed", C.c_int32),
        ("decoded", C.c_void_p),
        ("prev_converged", C.c_void_p),
        ("prev_iters", C.c_void_p),
        ("n_gather", C.c_int32),
        ("gather_det", C.c_void_p),
        ("syndrome_packed", C.c_int32),
        ("syndrome", C.c_void_p),
        ("running", C.c_void_p),
        ("observables", C.c_void_p),
        ("correction", C.c_void_p),
        ("conv_all", C.c_void_p),
        ("iters", C.c_void_p),
        ("word_range", C.c_int32 * 2),
    ]


# bposd_window_fetch(what): item -> (number, dtype, columns) in the notation of DEM_ITEMS
WINDOW_ITEMS = {"obs_osdw": (0, "<u8", "k"), "observables": (1, "<u8", "k"), "correction": (2, "<u8", "N"), "residual": (3, "<u8", "M"),
                "flags": (4, "u1", None), "converged": (5, "u1", None), "iters": (6, "<i4", None), "obs_fail": (7, "<i4", "k32"),
                "fail_rows": (8, "<i4", "F"), "fail_weight": (9, "<i4", "F"), "fail_residual": (10, "<u8", "FN"),
                "fail_faults": (11, "<u8", "FN"), "min_residual": (12, "<u8", "1N")}


# bposd_dem_fetch(what): item -> (number, dtype, columns: "N" / "M" / "k" packed into words, "k32" = k int32 in one row, None = [B];
# of a harvest: "F" = one per failing shot, "FN" = packed fault-space rows of the first min(F, K) failing shots, "1N" = one such row)
DEM_ITEMS = {"faults": (0, "<u8", "N"), "detectors": (1, "<u8", "M"), "observables": (2, "<u8", "k"), "obs_bp": (3, "<u8", "k"),
             "obs_osd0": (4, "<u8", "k"), "obs_osdw": (5, "<u8", "k"), "flags": (6, "u1", None), "converged": (7, "u1", None),
             "iters": (8, "<i4", None), "obs_fail": (9, "<i4", "k32"), "logw": (10, "<i8", None),
             "fail_rows": (11, "<i4", "F"), "fail_weight": (12, "<i4", "F"), "fail_residual": (13, "<u8", "FN"),
             "fail_faults": (14, "<u8", "FN"), "min_residual": (15, "<u8", "1N")}


# bposd_frame_config.layered
FRAME_LAYERED = {None: 0, False: 1, True: 2}

# bposd_dem_fault_sums(select)
DEM_SELECT = {"all": 0, "failing": 1}

# bposd_dem_set_subset(mode)
DEM_SUBSET = {None: 0, "enumerate": 1, "random": 2}

# bposd_mc_config.channel_update / bposd_mc_fetch(what)
MC_UPDATE = {None: 0, "x->z": 1, "z->x": 2}
MC_ITEMS = {"error_x": 0, "error_z": 1, "syndrome_x": 2, "syndrome_z": 3, "flags": 4, "syndrome_x_packed": 5, "syndrome_z_packed": 6}


_lib = None


def load():
    """Load the HIP library; raises RuntimeError (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  bp_osd_amd has no CPU fallback."
        )
    # A handle's lanes are HIP streams that should run side by side; the runtime multiplexes a process's streams onto
    # GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share one take turns.  Read when the runtime starts, so this
    # only helps a process that has not touched the GPU yet; never overrides the caller's own setting.  (Measured, DESIGN.md
    # section 1: one synchronous host-to-host call of 131072 syndromes 30.7 -> 27.5 ms, BASELINE configs[4] as the fifth handle of
    # a process 10.0-10.4 k -> 12.1 k syndromes/s.)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.bposd_device_count.restype = C.c_int
    lib.bposd_version.restype = C.c_char_p
    lib.bposd_create.argtypes = [C.POINTER(BposdConfig), vp, vp, C.c_int32, C.c_int32, vp, C.POINTER(vp)]
    lib.bposd_create.restype = C.c_int
    lib.bposd_update_channel_probs.argtypes = [vp, vp]
    lib.bposd_update_channel_probs.restype = C.c_int
    lib.bposd_decode_batch.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch.restype = C.c_int
    lib.bposd_decode_batch_packed.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_packed.restype = C.c_int
    lib.bposd_decode_batch_async.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_async.restype = C.c_int
    lib.bposd_decode_batch_packed_async.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_packed_async.restype = C.c_int
    lib.bposd_decode_batch_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_device.restype = C.c_int
    lib.bposd_decode_batch_device_packed.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_device_packed.restype = C.c_int
    lib.bposd_decode_batch_select.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_select.restype = C.c_int
    lib.bposd_decode_batch_select_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_select_device.restype = C.c_int
    lib.bposd_channel_tables.argtypes = [vp, C.c_int64, vp, vp]
    lib.bposd_channel_tables.restype = C.c_int
    lib.bposd_decode_batch_rows.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_rows.restype = C.c_int
    lib.bposd_decode_batch_rows_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_rows_device.restype = C.c_int
    lib.bposd_pack_rows_device.argtypes = [vp, vp, C.c_int64, C.c_int32, vp]
    lib.bposd_pack_rows_device.restype = C.c_int
    lib.bposd_observable_table.argtypes = [vp, vp, C.c_int32, C.c_int32, vp]
    lib.bposd_observable_table.restype = C.c_int
    lib.bposd_set_observables.argtypes = [vp, vp, C.c_int32]
    lib.bposd_set_observables.restype = C.c_int
    lib.bposd_observables_device_lane.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_int64, vp]
    lib.bposd_observables_device_lane.restype = C.c_int
    lib.bposd_decode_batch_observables_device.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_decode_batch_observables_device.restype = C.c_int
    for name in ("bposd_decode_batch_observables", "bposd_decode_batch_observables_packed", "bposd_decode_batch_observables_async",
                 "bposd_decode_batch_observables_packed_async"):
        getattr(lib, name).argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
        getattr(lib, name).restype = C.c_int
    lib.bposd_synchronize.argtypes = [vp]
    lib.bposd_synchronize.restype = C.c_int
    lib.bposd_num_lanes.argtypes = [vp]
    lib.bposd_num_lanes.restype = C.c_int
    lib.bposd_last_lane.argtypes = [vp]
    lib.bposd_last_lane.restype = C.c_int
    lib.bposd_synchronize_lane.argtypes = [vp, C.c_int32]
    lib.bposd_synchronize_lane.restype = C.c_int
    lib.bposd_lane_timing.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.bposd_lane_timing.restype = C.c_int
    lib.bposd_host_alloc.argtypes = [C.c_size_t]
    lib.bposd_host_alloc.restype = vp
    lib.bposd_host_free.argtypes = [vp]
    lib.bposd_host_free.restype = None
    lib.bposd_last_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.bposd_last_timing.restype = C.c_int
    lib.bposd_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32)]
    lib.bposd_info.restype = C.c_int
    lib.bposd_layout_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.bposd_layout_info.restype = C.c_int
    lib.bposd_pack_rows_device_lane.argtypes = [vp, C.c_int32, vp, C.c_int64, C.c_int32, vp]
    lib.bposd_pack_rows_device_lane.restype = C.c_int
    lib.bposd_posterior_llr.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp]
    lib.bposd_posterior_llr.restype = C.c_int
    lib.bposd_bp_kernel_info.argtypes = [vp, C.POINTER(C.c_int32), vp]
    lib.bposd_bp_kernel_info.restype = C.c_int
    lib.bposd_debug_local_layout.argtypes = [vp, vp, C.c_int32, C.c_int32, vp]
    lib.bposd_debug_local_layout.restype = C.c_int
    lib.bposd_debug_host_chunks.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    lib.bposd_debug_host_chunks.restype = C.c_int
    lib.bposd_debug_local_keys.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    lib.bposd_debug_local_keys.restype = C.c_int
    lib.bposd_debug_local_waves.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp]
    lib.bposd_debug_local_waves.restype = C.c_int
    lib.bposd_debug_last_pair_key.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.bposd_debug_last_pair_key.restype = C.c_int
    lib.bposd_debug_set_park.argtypes = [vp, C.c_int32]
    lib.bposd_debug_set_park.restype = C.c_int
    lib.bposd_debug_last_parked.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.bposd_debug_last_parked.restype = C.c_int
    lib.bposd_debug_obs_timing.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    lib.bposd_debug_obs_timing.restype = C.c_int
    lib.bposd_debug_class_layout.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    lib.bposd_debug_class_layout.restype = C.c_int
    lib.bposd_debug_last_instance.argtypes = [vp, vp, vp]
    lib.bposd_debug_last_instance.restype = C.c_int
    lib.bposd_debug_portable_math.argtypes = [C.c_int32, vp, vp, vp, C.c_int64]
    lib.bposd_debug_portable_math.restype = C.c_int
    lib.bposd_set_osd_variant.argtypes = [vp, C.c_int32]
    lib.bposd_set_osd_variant.restype = C.c_int
    lib.bposd_last_osd_kernel.argtypes = [vp]
    lib.bposd_last_osd_kernel.restype = C.c_int
    lib.bposd_set_bp_variant.argtypes = [vp, C.c_int32]
    lib.bposd_set_bp_variant.restype = C.c_int
    lib.bposd_set_relay.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32]
    lib.bposd_set_relay.restype = C.c_int
    lib.bposd_relay_stats.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int64]
    lib.bposd_relay_stats.restype = C.c_int
    lib.bposd_set_lsd.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    lib.bposd_set_lsd.restype = C.c_int
    lib.bposd_lsd_stats.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int64]
    lib.bposd_lsd_stats.restype = C.c_int
    lib.bposd_set_lsd_order.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.bposd_set_lsd_order.restype = C.c_int
    lib.bposd_lsd_order_stats.argtypes = [vp, C.c_int32, vp, vp, C.c_int64]
    lib.bposd_lsd_order_stats.restype = C.c_int
    lib.bposd_debug_lsd_launches.argtypes = [vp, vp]
    lib.bposd_debug_lsd_launches.restype = C.c_int
    lib.bposd_last_error.argtypes = [vp]
    lib.bposd_last_error.restype = C.c_char_p
    lib.bposd_destroy.argtypes = [vp]
    lib.bposd_destroy.restype = None
    lib.bposd_mc_create.argtypes = [C.POINTER(BposdMcConfig), vp, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32,
                                    vp, vp, vp, vp, C.POINTER(vp)]
    lib.bposd_mc_create.restype = C.c_int
    lib.bposd_mc_run.argtypes = [vp, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]
    lib.bposd_mc_run.restype = C.c_int
    lib.bposd_mc_fetch.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.bposd_mc_fetch.restype = C.c_int
    lib.bposd_mc_device_bytes.argtypes = [vp]
    lib.bposd_mc_device_bytes.restype = C.c_int64
    lib.bposd_mc_last_error.argtypes = [vp]
    lib.bposd_mc_last_error.restype = C.c_char_p
    lib.bposd_mc_destroy.argtypes = [vp]
    lib.bposd_mc_destroy.restype = None
    lib.bposd_dem_tables.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp]
    lib.bposd_dem_tables.restype = C.c_int
    lib.bposd_dem_create.argtypes = [C.POINTER(BposdDemConfig), vp, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, C.POINTER(vp)]
    lib.bposd_dem_create.restype = C.c_int
    lib.bposd_dem_set_sampling.argtypes = [vp, vp, vp]
    lib.bposd_dem_set_sampling.restype = C.c_int
    lib.bposd_dem_set_subset.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    lib.bposd_dem_set_subset.restype = C.c_int
    lib.bposd_dem_set_harvest.argtypes = [vp, C.c_int64]
    lib.bposd_dem_set_harvest.restype = C.c_int
    lib.bposd_dem_harvest_info.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.bposd_dem_harvest_info.restype = C.c_int
    lib.bposd_debug_dem_harvest.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int64]
    lib.bposd_debug_dem_harvest.restype = C.c_int
    lib.bposd_debug_dem_harvest_timing.argtypes = [vp, C.POINTER(C.c_double)]
    lib.bposd_debug_dem_harvest_timing.restype = C.c_int
    lib.bposd_dem_fault_sums.argtypes = [vp, C.c_int32, vp, C.c_int64, vp, vp]
    lib.bposd_dem_fault_sums.restype = C.c_int
    lib.bposd_debug_dem_fault_sums.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp]
    lib.bposd_debug_dem_fault_sums.restype = C.c_int
    lib.bposd_debug_dem_fault_sums_timing.argtypes = [vp, C.POINTER(C.c_double)]
    lib.bposd_debug_dem_fault_sums_timing.restype = C.c_int
    lib.bposd_window_set_harvest.argtypes = [vp, C.c_int64]
    lib.bposd_window_set_harvest.restype = C.c_int
    lib.bposd_window_harvest_info.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.bposd_window_harvest_info.restype = C.c_int
    lib.bposd_dem_sample.argtypes = [vp, C.c_uint64, C.c_int64]
    lib.bposd_dem_sample.restype = C.c_int
    lib.bposd_dem_run.argtypes = [vp, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]
    lib.bposd_dem_run.restype = C.c_int
    lib.bposd_dem_fetch.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.bposd_dem_fetch.restype = C.c_int
    lib.bposd_dem_device_bytes.argtypes = [vp]
    lib.bposd_dem_device_bytes.restype = C.c_int64
    lib.bposd_dem_last_error.argtypes = [vp]
    lib.bposd_dem_last_error.restype = C.c_char_p
    lib.bposd_dem_destroy.argtypes = [vp]
    lib.bposd_dem_destroy.restype = None
    lib.bposd_debug_dem_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.bposd_debug_dem_timing.restype = C.c_int
    lib.bposd_window_create.argtypes = [C.POINTER(BposdWindowConfig), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32,
                                        C.POINTER(vp), vp, vp, vp, vp, vp, C.POINTER(vp)]
    lib.bposd_window_create.restype = C.c_int
    lib.bposd_window_decode_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_window_decode_device.restype = C.c_int
    lib.bposd_window_synchronize.argtypes = [vp]
    lib.bposd_window_synchronize.restype = C.c_int
    lib.bposd_window_decode.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.bposd_window_decode.restype = C.c_int
    lib.bposd_window_run.argtypes = [vp, vp, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]
    lib.bposd_window_run.restype = C.c_int
    lib.bposd_window_fetch.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.bposd_window_fetch.restype = C.c_int
    lib.bposd_window_device_bytes.argtypes = [vp]
    lib.bposd_window_device_bytes.restype = C.c_int64
    lib.bposd_window_last_error.argtypes = [vp]
    lib.bposd_window_last_error.restype = C.c_char_p
    lib.bposd_window_destroy.argtypes = [vp]
    lib.bposd_window_destroy.restype = None
    lib.bposd_debug_window_step.argtypes = [C.POINTER(BposdWindowStep)]
    lib.bposd_debug_window_step.restype = C.c_int
    lib.bposd_debug_window_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.bposd_debug_window_timing.restype = C.c_int
    lib.bposd_frame_create.argtypes = [C.POINTER(BposdFrameConfig), vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_int32,
                                       C.POINTER(vp)]
    lib.bposd_frame_create.restype = C.c_int
    lib.bposd_frame_columns.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp]
    lib.bposd_frame_columns.restype = C.c_int
    lib.bposd_frame_fetch.argtypes = [vp, vp, vp, vp, vp]
    lib.bposd_frame_fetch.restype = C.c_int
    lib.bposd_frame_device_bytes.argtypes = [vp]
    lib.bposd_frame_device_bytes.restype = C.c_int64
    lib.bposd_frame_last_error.argtypes = [vp]
    lib.bposd_frame_last_error.restype = C.c_char_p
    lib.bposd_frame_destroy.argtypes = [vp]
    lib.bposd_frame_destroy.restype = None
    lib.bposd_debug_frame_timing.argtypes = [vp, vp, vp]
    lib.bposd_debug_frame_timing.restype = C.c_int
    _lib = lib
    return lib


def _raise(last_error_fn, obj, rc):
    """Map a C-ABI return code to the exception the reference's users would expect (obj None: a failed create)."""
    if rc == BPOSD_OK:
        return
    msg = last_error_fn(obj)
    msg = msg.decode() if msg else f"error {rc}"
    if rc in (BPOSD_ERR_INVALID, BPOSD_ERR_UNSUPPORTED):
        raise ValueError(msg)
    raise RuntimeError(msg)


def check_dem(lib, dem, rc):
    """check() for the detector-error-model engine's calls (dem None: a failed bposd_dem_create / bposd_dem_tables)."""
    _raise(lib.bposd_dem_last_error, dem, rc)


def check_window(lib, win, rc):
    """check() for the sliding-window engine's calls (win None: a failed bposd_window_create / bposd_debug_window_step)."""
    _raise(lib.bposd_window_last_error, win, rc)


def check_frame(lib, fr, rc):
    """check() for the frame-propagation handle's calls (fr None: a failed bposd_frame_create)."""
    _raise(lib.bposd_frame_last_error, fr, rc)


def check_mc(lib, mc, rc):
    """check() for the Monte-Carlo engine's calls (mc None: a failed bposd_mc_create)."""
    _raise(lib.bposd_mc_last_error, mc, rc)


def check(lib, handle, rc):
    """check() for a decoder handle's calls (handle None: a failed bposd_create)."""
    _raise(lib.bposd_last_error, handle, rc)
