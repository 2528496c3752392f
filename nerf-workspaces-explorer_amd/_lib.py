"""ctypes binding of libnwe_hip.so (include/nwe.h).  There is no fallback: if the library is missing
or a symbol is absent, importing the render path fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NWE_LIB") or os.path.join(_HERE, "libnwe_hip.so")   # NWE_LIB: timing experiments with variant builds

NWE_OK, NWE_ERR_INVALID, NWE_ERR_UNSUPPORTED, NWE_ERR_HIP, NWE_ERR_STATE = 0, 1, 2, 3, 4
NET_COARSE, NET_FINE = 0, 1
PREC_F16X3, PREC_F16X1, PREC_F32 = 0, 1, 2
PRECISIONS = {"f16x3": PREC_F16X3, "f16x1": PREC_F16X1, "f32": PREC_F32}

OUTPUT_FIELDS = ("rgb", "depth", "acc", "disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "disp_coarse",
                 "raw_coarse", "raw_fine", "z_fine", "weights_coarse", "sample_cond", "sample_amp", "sample_switch", "feat_map", "flags")

# every symbol include/nwe.h declares (tests/test_abi.py checks the library exports all of them)
SYMBOLS = ("nwe_create", "nwe_destroy", "nwe_last_error", "nwe_set_network", "nwe_set_sampling", "nwe_render", "nwe_render_tiled",
           "nwe_create_rays", "nwe_render_rays", "nwe_to8b", "nwe_flops_per_eval", "nwe_last_kernel_ms", "nwe_packed_bytes",
           "nwe_packed_copy", "nwe_packed_bias_count", "nwe_packed_bias_copy", "nwe_packed_scale",
           "nwe_debug_set_fine_depths", "nwe_debug_set_raw", "nwe_debug_set_coarse_weights", "nwe_debug_set_fold", "nwe_set_train_tables", "nwe_set_white_background", "nwe_debug_set_decomposition", "nwe_debug_last_plan", "nwe_debug_set_stamps", "nwe_selftest",
           "nwe_last_warning", "nwe_debug_peer_access", "nwe_set_network_no_view_dirs", "nwe_last_launch_parts",
           "nwe_set_early_termination", "nwe_get_early_termination", "nwe_last_ray_evaluations",
           "nwe_set_shared_coarse", "nwe_get_shared_coarse", "nwe_last_coarse_launch",
           "nwe_set_separate_passes", "nwe_get_separate_passes",
           "nwe_debug_set_work_queue", "nwe_debug_get_work_queue", "nwe_debug_get_work_queue_backfill", "nwe_debug_queue_grid", "nwe_debug_last_queue",
           "nwe_debug_get_work_queue_tail", "nwe_debug_last_tail", "nwe_debug_last_tail_rest",
           "nwe_query_points", "nwe_last_query_ms", "nwe_debug_set_query_steps",
           "nwe_packed_colour_finite", "nwe_debug_set_colour_skip", "nwe_debug_get_colour_skip", "nwe_debug_plan",
           "nwe_set_occupancy", "nwe_clear_occupancy", "nwe_get_occupancy", "nwe_occupancy_copy", "nwe_build_occupancy",
           "nwe_set_coarse_grid", "nwe_clear_coarse_grid", "nwe_get_coarse_grid", "nwe_coarse_grid_copy", "nwe_bake_coarse_grid",
           "nwe_coarse_grid_weights",
           "nwe_set_radiance_grid", "nwe_clear_radiance_grid", "nwe_get_radiance_grid", "nwe_radiance_grid_copy", "nwe_bake_radiance_grid",
           "nwe_render_grid", "nwe_last_grid_ms",
           "nwe_render_sparse", "nwe_debug_set_sparse_chunk", "nwe_last_sparse_ms", "nwe_last_sparse_samples",
           "nwe_render_sparse_async", "nwe_debug_last_sparse_host_waits", "nwe_debug_query_counted_grid",
           "nwe_debug_set_packet_blocks", "nwe_debug_last_packet_blocks", "nwe_debug_packet_pixels",
           "nwe_render_adaptive", "nwe_last_adaptive", "nwe_debug_adaptive_lattice",
           "nwe_set_adaptive_pixel_lists", "nwe_get_adaptive_pixel_lists", "nwe_render_pixels", "nwe_last_pixels", "nwe_debug_pixels_path",
           "nwe_render_adaptive_levels", "nwe_last_adaptive_levels", "nwe_debug_adaptive_levels_lattice", "nwe_debug_adaptive_levels_plan")


class Outputs(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(Outputs), **kw)


POINT_OUTPUT_FIELDS = ("raw", "sigma", "flags")
NWE_FLAG_RAW = 1 << 8


class PointOutputs(C.Structure):
    """nwe_point_outputs of nwe_query_points."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in POINT_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(PointOutputs), **kw)


GRID_OUTPUT_FIELDS = ("rgb", "depth", "acc", "weights_coarse", "z_fine", "raw_fine", "flags")


class GridOutputs(C.Structure):
    """nwe_grid_outputs of nwe_render_grid."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in GRID_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(GridOutputs), **kw)


SPARSE_OUTPUT_FIELDS = ("rgb", "depth", "acc", "weights_coarse", "z_fine", "weights_grid", "selected", "raw_fine", "flags")


class SparseOutputs(C.Structure):
    """nwe_sparse_outputs of nwe_render_sparse."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in SPARSE_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(SparseOutputs), **kw)


ADAPTIVE_OUTPUT_FIELDS = ("rgb", "depth", "acc", "kind", "flags")
ADAPTIVE_MAX_K = 64


class AdaptiveOutputs(C.Structure):
    """nwe_adaptive_outputs of nwe_render_adaptive."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in ADAPTIVE_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(AdaptiveOutputs), **kw)


ADAPTIVE_LEVELS_OUTPUT_FIELDS = ADAPTIVE_OUTPUT_FIELDS + ("level",)
ADAPTIVE_MAX_LEVELS = 4


class AdaptiveLevelsOutputs(C.Structure):
    """nwe_adaptive_levels_outputs of nwe_render_adaptive_levels."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in ADAPTIVE_LEVELS_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(AdaptiveLevelsOutputs), **kw)


PIXEL_OUTPUT_FIELDS = ("rgb", "depth", "acc", "flags")
FLAG_RGB, FLAG_DEPTH, FLAG_ACC = 1, 2, 4


class PixelOutputs(C.Structure):
    """nwe_pixel_outputs of nwe_render_pixels."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in PIXEL_OUTPUT_FIELDS]

    def __init__(self, **kw):
        super().__init__(struct_bytes=C.sizeof(PixelOutputs), **kw)


PLAN_HOOK_COARSE_WEIGHTS, PLAN_HOOK_OTHER = 1, 2


class PlanStage(C.Structure):
    """nwe_plan_stage of nwe_debug_plan."""
    _fields_ = [("active", C.c_int32), ("role", C.c_int32), ("n_rays", C.c_int64), ("n_importance", C.c_int32), ("net", C.c_int32),
                ("variant", C.c_int32), ("plan", C.c_int32), ("n_launches", C.c_int32), ("fork", C.c_int32),
                ("ray_first", C.c_int64 * 2), ("rays", C.c_int64 * 2), ("split", C.c_int32 * 2), ("items", C.c_uint32 * 2),
                ("grid", C.c_uint32 * 2), ("tail", C.c_int32), ("tail_items", C.c_uint32)]


class PlanReport(C.Structure):
    """nwe_plan_report of nwe_debug_plan."""
    _fields_ = [("struct_bytes", C.c_uint64)] + [(name, C.c_int32) for name in (
        "separate", "share", "full", "coarse_launch", "may_queue", "need_side", "need_evals", "coarse_flags", "share_k", "reserved")] + [
        (name, C.c_int64) for name in ("table_elems", "evals_full", "evals_run", "share_rays")] + [("coarse", PlanStage), ("main", PlanStage)]

    def __init__(self):
        super().__init__(struct_bytes=C.sizeof(PlanReport))


_lib = None


def build_hint() -> str:
    return ("build it with `make -C nerf-workspaces-explorer_amd/csrc` (or `python -c 'import __graft_entry__ as g; "
            "g.build()'`); the render path has no CPU or torch fallback")


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP extension {LIB_PATH} is missing: {build_hint()}")
    lib = C.CDLL(LIB_PATH)
    P, I, F, I64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
    sig = {
        "nwe_create": (I, [C.POINTER(P), I]),
        "nwe_destroy": (None, [P]),
        "nwe_last_error": (C.c_char_p, [P]),
        "nwe_set_network": (I, [P, I, I, I, I, I, I, C.POINTER(P), C.POINTER(P)]),
        "nwe_set_network_no_view_dirs": (I, [P, I, I, I, I, I, I, C.POINTER(P), C.POINTER(P)]),
        "nwe_set_sampling": (I, [P, P, P, I, P, I]),
        "nwe_render": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, I, C.POINTER(Outputs), P]),
        "nwe_render_tiled": (I, [C.POINTER(P), I, P, I, I, I, F, F, F, F, F, F, I, P, P, P, P, P]),
        "nwe_create_rays": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, P, P]),
        "nwe_render_rays": (I, [P, P, I64, I, C.POINTER(Outputs), P]),
        "nwe_to8b": (I, [P, P, P, I64, P]),
        "nwe_flops_per_eval": (I64, [P, I]),
        "nwe_last_kernel_ms": (F, [P]),
        "nwe_last_launch_parts": (I, [P, C.POINTER(F), C.POINTER(I64)]),
        "nwe_packed_bytes": (I64, [P, I]),
        "nwe_packed_copy": (I, [P, I, P, I64]),
        "nwe_packed_bias_count": (I64, [P, I]),
        "nwe_packed_bias_copy": (I, [P, I, P, I64]),
        "nwe_packed_scale": (F, [P, I]),
        "nwe_debug_set_fine_depths": (I, [P, P]),
        "nwe_debug_set_raw": (I, [P, P, P]),
        "nwe_debug_set_coarse_weights": (I, [P, P]),
        "nwe_debug_set_fold": (I, [P, I]),
        "nwe_set_train_tables": (I, [P, P, P, P, P]),
        "nwe_set_white_background": (I, [P, I]),
        "nwe_debug_set_decomposition": (I, [P, I]),
        "nwe_debug_last_plan": (I, [P]),
        "nwe_debug_set_stamps": (I, [P, P]),
        "nwe_selftest": (I, [P, C.POINTER(C.c_int32)]),
        "nwe_last_warning": (C.c_char_p, [P]),
        "nwe_debug_peer_access": (I, [P, P]),
        "nwe_set_early_termination": (I, [P, F]),
        "nwe_get_early_termination": (F, [P]),
        "nwe_last_ray_evaluations": (I, [P, C.POINTER(I64)]),
        "nwe_set_shared_coarse": (I, [P, I]),
        "nwe_get_shared_coarse": (I, [P]),
        "nwe_last_coarse_launch": (I, [P, C.POINTER(F), C.POINTER(I64)]),
        "nwe_set_separate_passes": (I, [P, I]),
        "nwe_get_separate_passes": (I, [P]),
        "nwe_debug_set_work_queue": (I, [P, I]),
        "nwe_debug_get_work_queue": (I, [P]),
        "nwe_debug_get_work_queue_backfill": (I, [P]),
        "nwe_debug_queue_grid": (C.c_uint, [C.c_uint]),
        "nwe_debug_last_queue": (I, [P, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(I)]),
        "nwe_debug_get_work_queue_tail": (I, [P]),
        "nwe_debug_last_tail": (I, [P, C.POINTER(C.c_uint)]),
        "nwe_debug_last_tail_rest": (I, [P, C.POINTER(C.c_uint)]),
        "nwe_query_points": (I, [P, I, P, I64, P, I64, I, C.POINTER(PointOutputs), P]),
        "nwe_last_query_ms": (F, [P]),
        "nwe_debug_set_query_steps": (I, [P, I]),
        "nwe_packed_colour_finite": (I, [P, I]),
        "nwe_debug_set_colour_skip": (I, [P, I]),
        "nwe_debug_get_colour_skip": (I, [P]),
        "nwe_debug_set_packet_blocks": (I, [P, I]),
        "nwe_debug_last_packet_blocks": (I, [P]),
        "nwe_debug_packet_pixels": (I, [I64, I64, I, P]),
        "nwe_debug_plan": (I, [P, I, I, I, I, I, I64, C.POINTER(Outputs), C.c_uint, I, I, C.POINTER(PlanReport)]),
        "nwe_set_occupancy": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), P, I]),
        "nwe_clear_occupancy": (I, [P]),
        "nwe_get_occupancy": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), C.POINTER(F), C.POINTER(I64)]),
        "nwe_occupancy_copy": (I, [P, P, I64]),
        "nwe_build_occupancy": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), I, F, I, I, P]),
        "nwe_set_coarse_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), P, I]),
        "nwe_clear_coarse_grid": (I, [P]),
        "nwe_get_coarse_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), C.POINTER(F)]),
        "nwe_coarse_grid_copy": (I, [P, P, I64]),
        "nwe_bake_coarse_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), I, P]),
        "nwe_coarse_grid_weights": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, P, P, P]),
        "nwe_set_radiance_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), P, I]),
        "nwe_clear_radiance_grid": (I, [P]),
        "nwe_get_radiance_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), C.POINTER(F)]),
        "nwe_radiance_grid_copy": (I, [P, P, I64]),
        "nwe_bake_radiance_grid": (I, [P, C.POINTER(F), C.POINTER(F), C.POINTER(I), I, C.POINTER(F), I, P]),
        "nwe_render_grid": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, C.POINTER(GridOutputs), P]),
        "nwe_last_grid_ms": (F, [P]),
        "nwe_render_sparse": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, I, I, F, I, C.POINTER(SparseOutputs), P]),
        "nwe_debug_set_sparse_chunk": (I, [P, I]),
        "nwe_last_sparse_ms": (F, [P]),
        "nwe_last_sparse_samples": (I, [P, C.POINTER(I64)]),
        "nwe_render_sparse_async": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, I, I, F, I, C.POINTER(SparseOutputs), P]),
        "nwe_debug_last_sparse_host_waits": (I, [P]),
        "nwe_debug_query_counted_grid": (C.c_uint, [I64, I, I, I]),
        "nwe_render_adaptive": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, I, I, F, F, C.POINTER(AdaptiveOutputs), P]),
        "nwe_last_adaptive": (I, [P, C.POINTER(I64), C.POINTER(F)]),
        "nwe_debug_adaptive_lattice": (I, [I, I, I, C.POINTER(C.c_int32), I]),
        "nwe_set_adaptive_pixel_lists": (I, [P, I]),
        "nwe_get_adaptive_pixel_lists": (I, [P]),
        "nwe_render_pixels": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, P, I64, I, C.POINTER(PixelOutputs), P]),
        "nwe_last_pixels": (I, [P, C.POINTER(I64), C.POINTER(I)]),
        "nwe_debug_pixels_path": (I, [P, I]),
        "nwe_render_adaptive_levels": (I, [P, P, I, I, I, F, F, F, F, F, F, I, I, I, I, I, F, F, C.POINTER(AdaptiveLevelsOutputs), P]),
        "nwe_last_adaptive_levels": (I, [P, C.POINTER(I64), I, C.POINTER(F)]),
        "nwe_debug_adaptive_levels_lattice": (I, [I, I, I, I, I, C.POINTER(C.c_int32), I]),
        "nwe_debug_adaptive_levels_plan": (I, [I, I, I, I, I, I, C.POINTER(I64), I]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing: loud by design
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib
