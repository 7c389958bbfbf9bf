"""
ctypes binding of ``libbspy_amd.so`` (C ABI: ``include/bspy_amd.h``).

This is the only way the package computes anything: there is no CPU fallback.
If the shared library is missing or cannot be loaded, every compute entry point
raises ``NativeLibraryError`` with build instructions.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BSPY_AMD_LIB: alternative build of the same library (e.g. the -DBSK_ABLATE timing build)
LIB_PATH = os.environ.get("BSPY_AMD_LIB") or os.path.join(_HERE, "csrc", "libbspy_amd.so")

BSK_F32, BSK_F64 = 0, 1
BSK_HOST, BSK_DEVICE = 0, 1
BSK_OK, BSK_ERR_INVALID, BSK_ERR_DOMAIN, BSK_ERR_HIP, BSK_ERR_NO_DEVICE, BSK_ERR_UNSUPPORTED = range(6)
BSK_MAX_NIND, BSK_MAX_ORDER = 8, 16
BSK_INTEGRAL_MEASURE, BSK_INTEGRAL_NODES = 0, 1

# every symbol of the product ABI in include/bspy_amd.h (tests check the library exports them all) ...
PRODUCT_SYMBOLS = (
    "bsk_version", "bsk_last_error", "bsk_device_count",
    "bsk_spline_create", "bsk_spline_update", "bsk_spline_destroy",
    "bsk_evaluate", "bsk_jacobian", "bsk_normal", "bsk_curvature", "bsk_evaluate_grid", "bsk_tessellate",
    "bsk_domain_status", "bsk_bspline_values", "bsk_last_kernel",
    "bsk_multi_create", "bsk_multi_destroy", "bsk_multi_shard_plan", "bsk_multi_stream", "bsk_multi_evaluate",
    "bsk_multi_jacobian", "bsk_integral",
    "bsk_fit_create", "bsk_fit_destroy", "bsk_fit_info", "bsk_fit_solve_host", "bsk_fit_sweep", "bsk_fit_residual",
    "bsk_fit_last_kernel",
    "bsk_band_create", "bsk_band_destroy", "bsk_band_apply_host", "bsk_band_apply", "bsk_band_last_kernel",
    "bsk_band_absmax", "bsk_band_absmax_host", "bsk_band_apply_fma_host",
    "bsk_product_create", "bsk_product_destroy", "bsk_product_apply_host", "bsk_product_apply", "bsk_product_last_kernel",
    "bsk_scan_create", "bsk_scan_destroy", "bsk_scan_apply_host", "bsk_scan_apply", "bsk_scan_last_kernel",
    "bsk_sum_apply_host", "bsk_sum_apply", "bsk_sum_last_kernel",
    "bsk_roots_extract_host", "bsk_roots_flag_host", "bsk_roots_flag", "bsk_roots_isolate_host", "bsk_roots_isolate", "bsk_roots_last_kernel",
    "bsk_project_seed_host", "bsk_project_seed", "bsk_project_newton_host", "bsk_project_newton", "bsk_project_last_kernel",
    "bsk_contour_flag_host", "bsk_contour_flag", "bsk_contour_march_host", "bsk_contour_march", "bsk_contour_last_kernel",
    "bsk_iso_flag_host", "bsk_iso_flag", "bsk_iso_walk_host", "bsk_iso_walk", "bsk_iso_leaf_host", "bsk_iso_leaf", "bsk_iso_vertex_host",
    "bsk_iso_vertex", "bsk_iso_last_kernel",
    "bsk_mesh_bound_host", "bsk_mesh_bound", "bsk_mesh_count_host", "bsk_mesh_count", "bsk_mesh_emit_host", "bsk_mesh_emit",
    "bsk_mesh_vertex_host", "bsk_mesh_vertex", "bsk_mesh_last_kernel",
    "bsk_rays_boxes_host", "bsk_rays_boxes", "bsk_rays_count_host", "bsk_rays_count", "bsk_rays_emit_host", "bsk_rays_emit",
    "bsk_rays_isolate_host", "bsk_rays_isolate", "bsk_rays_reduce_host", "bsk_rays_reduce", "bsk_rays_last_kernel",
    "bsk_ssx_count_host", "bsk_ssx_count", "bsk_ssx_emit_host", "bsk_ssx_emit", "bsk_ssx_isolate_host", "bsk_ssx_isolate",
    "bsk_ssx_merge_host", "bsk_ssx_merge", "bsk_ssx_last_kernel",
    "bsk_scatter_key_host", "bsk_scatter_key", "bsk_scatter_gram_host", "bsk_scatter_gram", "bsk_scatter_cell_host", "bsk_scatter_cell",
    "bsk_scatter_fold_host", "bsk_scatter_fold", "bsk_scatter_residual_host", "bsk_scatter_residual", "bsk_scatter_solve_host",
    "bsk_scatter_solve_work", "bsk_scatter_solve", "bsk_scatter_reweight_host", "bsk_scatter_reweight", "bsk_scatter_last_kernel",
)
# ... and the measurement hooks of its BSK_INTERNAL section (bench.py, tools/: not used by the product path)
INTERNAL_SYMBOLS = ("bsk_debug_probe", "bsk_debug_stage_times", "bsk_debug_fill_lds", "bsk_debug_scatter_solve")
SYMBOLS = PRODUCT_SYMBOLS + INTERNAL_SYMBOLS
# ... and the family of Spline.zeros2, also product ABI.  Listed apart because of the digit in the names: the header scan of
# tests/test_host_logic.py reads names of [a-z_] only and compares them with the tuples above; tests/test_roots2_host.py
# compares these with the header, and build() checks that the library exports them
ROOTS2_SYMBOLS = ("bsk_roots2_flag_host", "bsk_roots2_flag", "bsk_roots2_isolate_host", "bsk_roots2_isolate", "bsk_roots2_merge_host",
                  "bsk_roots2_merge", "bsk_roots2_last_kernel")
# ... and the family of Spline.zeros3, listed apart for the same reason; tests/test_roots3_host.py compares it with the header
ROOTS3_SYMBOLS = ("bsk_roots3_flag_host", "bsk_roots3_flag", "bsk_roots3_isolate_host", "bsk_roots3_isolate", "bsk_roots3_merge_host",
                  "bsk_roots3_merge", "bsk_roots3_last_kernel", "bsk_roots3_walk_bound")


class NativeLibraryError(RuntimeError):
    """libbspy_amd.so is missing or failed to load."""


class BskError(RuntimeError):
    """A libbspy_amd call failed (status + library message)."""

    def __init__(self, status, message):
        super().__init__(f"libbspy_amd status {status}: {message}")
        self.status = status


class DomainError(Exception):
    """A parameter lies outside the spline's domain; ``index`` = flat index of the first offender."""

    def __init__(self, index):
        super().__init__(f"parameter outside domain at flat index {index}")
        self.index = int(index)


_lib = None

_vp = ctypes.c_void_p
_vpp = ctypes.POINTER(ctypes.c_void_p)
_ip = ctypes.POINTER(ctypes.c_int)
_i64 = ctypes.c_int64
_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)


def lib():
    """Load the shared library once; fail loudly when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found. Build it with `make -C {os.path.dirname(LIB_PATH)}` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). bspy_amd has no CPU fallback.")
    if not os.environ.get("BSPY_AMD_NO_TORCH"):
        # PyTorch-ROCm ships its own libamdhip64; if it is going to be used in this process it
        # must be the first HIP runtime loaded (a second copy finds "no HIP GPUs"), so let it
        # load before libbspy_amd.so resolves the same SONAME.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    L.bsk_version.restype = ctypes.c_int
    L.bsk_last_error.restype = ctypes.c_char_p
    L.bsk_device_count.argtypes = [_ip]
    L.bsk_spline_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, _ip, _vpp, _vp,
                                    ctypes.POINTER(_vp)]
    L.bsk_spline_update.argtypes = [_vp, _vpp, _vp]
    L.bsk_spline_destroy.argtypes = [_vp]
    L.bsk_evaluate.argtypes = [_vp, _ip, _vpp, _i64, ctypes.c_int, _vp, _vp, _i64p]
    L.bsk_jacobian.argtypes = [_vp, _vpp, _i64, ctypes.c_int, _vp, _vp, _i64p]
    L.bsk_normal.argtypes = [_vp, _vpp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _i64p]
    L.bsk_curvature.argtypes = [_vp, _vpp, _i64, ctypes.c_int, _vp, _vp, _i64p]
    L.bsk_evaluate_grid.argtypes = [_vp, _ip, _vpp, _i64p, ctypes.c_int, _vp, _vp, _i64p]
    L.bsk_tessellate.argtypes = [_vpp, ctypes.c_int, _vpp, _i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                 _i64p]
    L.bsk_domain_status.argtypes = [_vp, _vp, _i64p]
    L.bsk_bspline_values.argtypes = [ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _i64,
                                     ctypes.c_int, ctypes.c_int, _i32p, _i32p, _vp]
    L.bsk_multi_create.argtypes = [ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, _ip, _ip, _vpp, _vp,
                                   ctypes.POINTER(_vp)]
    L.bsk_multi_destroy.argtypes = [_vp]
    L.bsk_multi_shard_plan.argtypes = [_vp, _i64, _i64p]
    L.bsk_multi_stream.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(_vp)]
    L.bsk_multi_evaluate.argtypes = [_vp, _ip, _vpp, _i64, ctypes.c_int, _vpp, ctypes.c_int, _i64p]
    L.bsk_multi_jacobian.argtypes = [_vp, _vpp, _i64, ctypes.c_int, _vpp, ctypes.c_int, _i64p]
    L.bsk_integral.argtypes = [_vp, ctypes.c_int, _vp, _i32p, _i64, _vp, _vp]
    L.bsk_fit_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, _vp, ctypes.POINTER(_vp)]
    L.bsk_fit_destroy.argtypes = [_vp]
    L.bsk_fit_info.argtypes = [_vp, _ip, ctypes.POINTER(ctypes.c_double), _vp]
    L.bsk_fit_solve_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp]
    L.bsk_fit_sweep.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp, _vp]
    L.bsk_fit_residual.argtypes = [_vp, ctypes.c_int, _vp, _vp, _i64, _i64, _vp, _vp]
    L.bsk_fit_last_kernel.argtypes = [_vp]
    L.bsk_fit_last_kernel.restype = ctypes.c_char_p
    L.bsk_band_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, _vp, ctypes.POINTER(_vp)]
    L.bsk_band_destroy.argtypes = [_vp]
    L.bsk_band_apply_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp]
    L.bsk_band_apply.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp, _vp]
    L.bsk_band_absmax.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp]
    L.bsk_band_absmax_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp]
    L.bsk_band_apply_fma_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp]
    L.bsk_band_last_kernel.argtypes = [_vp]
    L.bsk_band_last_kernel.restype = ctypes.c_char_p
    L.bsk_product_create.argtypes = [ctypes.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, ctypes.POINTER(_i32p), ctypes.POINTER(_i32p),
                                     _vpp, ctypes.POINTER(_vp)]
    L.bsk_product_destroy.argtypes = [_vp]
    L.bsk_product_apply_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _vp, _i64, _i32p, _i64, ctypes.c_int, _vp]
    L.bsk_product_apply.argtypes = [_vp, ctypes.c_int, _vp, _i64, _vp, _i64, _i32p, _i64, ctypes.c_int, _vp, _vp]
    L.bsk_product_last_kernel.argtypes = [_vp]
    L.bsk_product_last_kernel.restype = ctypes.c_char_p
    L.bsk_scan_create.argtypes = [ctypes.c_int, _vp, ctypes.POINTER(_vp)]
    L.bsk_scan_destroy.argtypes = [_vp]
    L.bsk_scan_apply_host.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp]
    L.bsk_scan_apply.argtypes = [_vp, ctypes.c_int, _vp, _i64, _i64, _vp, ctypes.c_int, _vp]
    L.bsk_scan_last_kernel.argtypes = [_vp]
    L.bsk_scan_last_kernel.restype = ctypes.c_char_p
    L.bsk_sum_apply_host.argtypes = [ctypes.c_int, ctypes.c_int, _i64p, _vp, _i64p, _vp, _i64p, ctypes.c_int, _vp]
    L.bsk_sum_apply.argtypes = [ctypes.c_int, ctypes.c_int, _i64p, _vp, _i64p, _vp, _i64p, ctypes.c_int, _vp, _vp]
    L.bsk_sum_last_kernel.argtypes = []
    L.bsk_sum_last_kernel.restype = ctypes.c_char_p
    L.bsk_roots_extract_host.argtypes = [ctypes.c_int, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
    L.bsk_roots_flag_host.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp]
    L.bsk_roots_flag.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]
    L.bsk_roots_isolate_host.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_double,
                                         _vp, _i64, _vp, _vp]
    L.bsk_roots_isolate.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_double, _vp,
                                    _i64, _vp, _vp, _vp]
    L.bsk_roots_last_kernel.argtypes = []
    L.bsk_roots_last_kernel.restype = ctypes.c_char_p
    grid2 = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp]
    L.bsk_roots2_flag_host.argtypes = grid2 + [_vp, _vp]
    L.bsk_roots2_flag.argtypes = grid2 + [_vp, _vp, _vp]
    L.bsk_roots2_isolate_host.argtypes = grid2 + [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
    L.bsk_roots2_isolate.argtypes = grid2 + [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]
    L.bsk_roots2_merge_host.argtypes = [ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]
    L.bsk_roots2_merge.argtypes = [ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]
    L.bsk_roots2_last_kernel.argtypes = []
    L.bsk_roots2_last_kernel.restype = ctypes.c_char_p
    grid3 = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]
    merge3 = [ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]
    L.bsk_roots3_flag_host.argtypes = grid3 + [_vp, _vp]
    L.bsk_roots3_flag.argtypes = grid3 + [_vp, _vp, _vp]
    L.bsk_roots3_isolate_host.argtypes = grid3 + [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
    L.bsk_roots3_isolate.argtypes = grid3 + [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]
    L.bsk_roots3_merge_host.argtypes = merge3
    L.bsk_roots3_merge.argtypes = merge3 + [_vp]
    L.bsk_roots3_last_kernel.argtypes = []
    L.bsk_roots3_last_kernel.restype = ctypes.c_char_p
    L.bsk_roots3_walk_bound.argtypes = []
    newton = [ctypes.c_int] * 4 + [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp, _i64,
                                   _vp, _vp, _vp, _vp, _vp]
    L.bsk_project_seed_host.argtypes = [ctypes.c_int, _vp, _i64, _vp, _i64, _i64, _vp, _vp]
    L.bsk_project_seed.argtypes = [ctypes.c_int, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]
    L.bsk_project_newton_host.argtypes = newton
    L.bsk_project_newton.argtypes = newton + [_vp]
    L.bsk_project_last_kernel.argtypes = []
    L.bsk_project_last_kernel.restype = ctypes.c_char_p
    grid_c = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp]
    march_c = grid_c + [_vp, _vp, _vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp, _vp, _vp]
    L.bsk_contour_flag_host.argtypes = grid_c + [_vp, _vp]
    L.bsk_contour_flag.argtypes = grid_c + [_vp, _vp, _vp]
    L.bsk_contour_march_host.argtypes = march_c
    L.bsk_contour_march.argtypes = march_c + [_vp]
    L.bsk_contour_last_kernel.argtypes = []
    L.bsk_contour_last_kernel.restype = ctypes.c_char_p
    grid_i = [ctypes.c_int] * 3 + [_vp] + [_i64] * 7 + [_vp, _vp, _vp, _vp, _i64, _vp]
    walk_i = grid_i + [_vp, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp]
    leaf_i = grid_i + [_vp, _i64, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _vp, _vp]
    vertex_i = grid_i + [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_int, _vp]
    L.bsk_iso_flag_host.argtypes = grid_i + [_vp, _vp]
    L.bsk_iso_flag.argtypes = grid_i + [_vp, _vp, _vp]
    L.bsk_iso_walk_host.argtypes = walk_i
    L.bsk_iso_walk.argtypes = walk_i + [_vp]
    L.bsk_iso_leaf_host.argtypes = leaf_i
    L.bsk_iso_leaf.argtypes = leaf_i + [_vp]
    L.bsk_iso_vertex_host.argtypes = vertex_i
    L.bsk_iso_vertex.argtypes = vertex_i + [_vp]
    L.bsk_iso_last_kernel.argtypes = []
    L.bsk_iso_last_kernel.restype = ctypes.c_char_p
    net_m = [ctypes.c_int, ctypes.c_int, _vp, _i64, ctypes.c_int] + [_i64] * 4 + [_vp, _vp]
    quad_m = [_vp, _i64, _i64, _i64, _vp, ctypes.c_int, ctypes.c_int, _i64, _i64, _i64]
    L.bsk_mesh_bound_host.argtypes = net_m + [ctypes.c_double, ctypes.c_int, _vp, _vp, _vp]
    L.bsk_mesh_bound.argtypes = net_m + [ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp]
    L.bsk_mesh_count_host.argtypes = quad_m + [_vp]
    L.bsk_mesh_count.argtypes = quad_m + [_vp, _vp]
    L.bsk_mesh_emit_host.argtypes = quad_m + [_vp, _i64, _vp]
    L.bsk_mesh_emit.argtypes = quad_m + [_vp, _i64, _vp, _vp]
    L.bsk_mesh_vertex_host.argtypes = net_m + [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]
    L.bsk_mesh_vertex.argtypes = net_m + [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]
    L.bsk_mesh_last_kernel.argtypes = []
    L.bsk_mesh_last_kernel.restype = ctypes.c_char_p
    surface = [ctypes.c_int, ctypes.c_int, _vp, _i64, _i64, _i64, _i64, _vp, _vp]
    rays = [_vp, _vp, _vp, _i64]
    search = surface + rays + [ctypes.c_double, ctypes.c_double, _i64, ctypes.c_int, _vp]
    isolate_r = surface + [_vp, _vp] + rays + [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
    reduce_r = surface + [_vp, _vp] + rays + [ctypes.c_double, ctypes.c_double, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                              _vp, _i64, _vp, _vp, _vp, _vp, _vp]
    L.bsk_rays_boxes_host.argtypes = surface + [_vp]
    L.bsk_rays_boxes.argtypes = surface + [_vp, _vp]
    L.bsk_rays_count_host.argtypes = search + [_vp, _vp]
    L.bsk_rays_count.argtypes = search + [_vp, _vp, _vp]
    L.bsk_rays_emit_host.argtypes = search + [_vp, _vp, _vp, _i64]
    L.bsk_rays_emit.argtypes = search + [_vp, _vp, _vp, _i64, _vp]
    L.bsk_rays_isolate_host.argtypes = isolate_r
    L.bsk_rays_isolate.argtypes = isolate_r + [_vp]
    L.bsk_rays_reduce_host.argtypes = reduce_r
    L.bsk_rays_reduce.argtypes = reduce_r + [_vp]
    L.bsk_rays_last_kernel.argtypes = []
    L.bsk_rays_last_kernel.restype = ctypes.c_char_p
    side = surface + surface + [ctypes.c_int, _i64]
    search_s = side + [_i64, _i64, _i64, ctypes.c_int, _vp, _vp]
    isolate_s = side + [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]
    merge_s = [ctypes.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]
    L.bsk_ssx_count_host.argtypes = search_s + [_vp]
    L.bsk_ssx_count.argtypes = search_s + [_vp, _vp]
    L.bsk_ssx_emit_host.argtypes = search_s + [_vp, _vp, _vp, _i64]
    L.bsk_ssx_emit.argtypes = search_s + [_vp, _vp, _vp, _i64, _vp]
    L.bsk_ssx_isolate_host.argtypes = isolate_s
    L.bsk_ssx_isolate.argtypes = isolate_s + [_vp]
    L.bsk_ssx_merge_host.argtypes = merge_s
    L.bsk_ssx_merge.argtypes = merge_s + [_vp]
    L.bsk_ssx_last_kernel.argtypes = []
    L.bsk_ssx_last_kernel.restype = ctypes.c_char_p
    shape_s = [ctypes.c_int] * 3 + [_i64, _i64, _vp, _vp, _i64, _i64, ctypes.c_int]
    key_s = shape_s + [_vp, _vp, _vp, _i64, _vp, _vp]
    gram_s = shape_s + [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
    cell_s = [_i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
    fold_s = [ctypes.c_int] * 3 + [_i64, _i64, ctypes.c_int, _vp, _vp, _vp]
    residual_s = shape_s + [_vp, _vp, _vp, _vp, _i64, _vp]
    L.bsk_scatter_key_host.argtypes = key_s
    L.bsk_scatter_key.argtypes = key_s + [_vp]
    L.bsk_scatter_gram_host.argtypes = gram_s
    L.bsk_scatter_gram.argtypes = gram_s + [_vp]
    L.bsk_scatter_cell_host.argtypes = cell_s
    L.bsk_scatter_cell.argtypes = cell_s + [_vp]
    L.bsk_scatter_fold_host.argtypes = fold_s
    L.bsk_scatter_fold.argtypes = fold_s + [_vp]
    L.bsk_scatter_residual_host.argtypes = residual_s
    L.bsk_scatter_residual.argtypes = residual_s + [_vp]
    L.bsk_scatter_solve_host.argtypes = fold_s + [_i64p]
    reweight_s = [ctypes.c_int, ctypes.c_double, _vp, _vp, _vp, _i64, _vp]
    L.bsk_scatter_solve_work.argtypes = [ctypes.c_int] * 3 + [_i64, _i64, ctypes.c_int, _i64p]
    L.bsk_scatter_solve.argtypes = fold_s + [_vp, _i64, _vp, _vp]
    L.bsk_debug_scatter_solve.argtypes = fold_s + [_vp, _i64, _vp, ctypes.c_int, _vp]
    L.bsk_scatter_reweight_host.argtypes = reweight_s
    L.bsk_scatter_reweight.argtypes = reweight_s + [_vp]
    L.bsk_scatter_last_kernel.argtypes = []
    L.bsk_scatter_last_kernel.restype = ctypes.c_char_p
    L.bsk_last_kernel.argtypes = [_vp]
    L.bsk_last_kernel.restype = ctypes.c_char_p
    L.bsk_debug_probe.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _i64, _vp, _vp]
    L.bsk_debug_stage_times.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.c_int, _ip]
    L.bsk_debug_fill_lds.argtypes = [_vp, ctypes.c_uint32, ctypes.c_int, _i64p, _vp]
    for name in SYMBOLS + ROOTS2_SYMBOLS + ROOTS3_SYMBOLS:
        if name not in ("bsk_version", "bsk_last_error", "bsk_last_kernel", "bsk_fit_last_kernel", "bsk_band_last_kernel",
                        "bsk_product_last_kernel", "bsk_scan_last_kernel", "bsk_sum_last_kernel", "bsk_roots_last_kernel",
                        "bsk_roots2_last_kernel", "bsk_roots3_last_kernel", "bsk_project_last_kernel", "bsk_contour_last_kernel", "bsk_iso_last_kernel", "bsk_mesh_last_kernel", "bsk_rays_last_kernel",
                        "bsk_ssx_last_kernel", "bsk_scatter_last_kernel"):
            getattr(L, name).restype = ctypes.c_int
    _lib = L
    return L


def check(status, first_bad=None):
    if status == BSK_OK:
        return
    if status == BSK_ERR_DOMAIN:
        raise DomainError(first_bad.value if first_bad is not None else -1)
    raise BskError(status, lib().bsk_last_error().decode("utf-8", "replace"))


def device_count():
    n = ctypes.c_int(0)
    st = lib().bsk_device_count(ctypes.byref(n))
    if st != BSK_OK:
        return 0
    return n.value


def dtype_code(dtype):
    return BSK_F32 if np.dtype(dtype) == np.float32 else BSK_F64


def ptr_array(pointers):
    arr = (ctypes.c_void_p * max(len(pointers), 1))()
    for i, p in enumerate(pointers):
        arr[i] = p
    return arr


def int_array(values):
    return (ctypes.c_int * max(len(values), 1))(*[int(v) for v in values])
