"""ceres_raytracer_amd -- MI355X-native CERES hot path, Python host mirror over the C ABI.

This module mirrors the reference's render interface (include/render.hpp of
iracigt/ceres-raytracer) for Python callers, tests and bench.py:

    Camera(eye, dir, up, fov)                 render.hpp:16-22
    load_obj(path) -> Mesh                    obj_norms.hpp:120-127 (triangles + tri_norms)
    rotate_triangles(mesh, axis, degrees)     render.hpp:24-44
    build_bvh(mesh) -> Bvh                    binned_sah_builder.hpp:39-234 (static.cpp:100-107)
    build_bvh_gpu(mesh) -> Bvh                the same BVH, built by gfx950 kernels
    Scene(mesh, bvh, device)                  the (bvh, triangles, tri_norms) arguments, on the GPU
    render(camera, sun, scene, W, H) -> (pixels, rays, hits)   render.hpp:86-156
    Scene.trace(rays) / CpuScene.trace(rays)  traverser.traverse(ray, intersector) for the caller's
                                              own rays (single_ray_traverser.hpp:68-126, ray.hpp:10-22),
                                              float or double scenes (ray32 / ray64 records)
    Scene.trace_all(rays, max_hits) / CpuScene.trace_all   every hit in each ray's window, in order: the
                                              traversal under an intersector that never narrows the ray
    Scene.trace_lists(rays) / CpuScene.trace_lists         every hit of every ray without a cap, as offsets + records
    Scene.shade(rays, sun) / CpuScene.shade   render()'s pixel (render.hpp:114-150) for the caller's own rays

Everything runs through libceres_hip.so (include/ceres_render.h): host scene preparation in
C++, the hot path in hand-written gfx950 HIP kernels.  There is no CPU fallback: rendering
without the library or without a gfx950 device raises CeresError.
"""
import ctypes
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# CERES_LIB: an A/B build of the same library (tools/ab.py, `make variant`); default the in-tree one
LIB_PATH = os.environ.get("CERES_LIB") or os.path.join(_PKG, "libceres_hip.so")
CLI_PATH = os.path.join(_PKG, "render")

if _PKG not in sys.path:
    sys.path.insert(0, _PKG)
import configs  # noqa: E402,F401  (re-exported)

MODE_FULL, MODE_PRIMARY = 0, 1
MODE_ROBUST = 0x10          # OR-ed: RobustNodeIntersector traversal (node_intersectors.hpp:54-79)
MODE_QBVH4 = 0x20           # OR-ed: compressed shadow BVH4 (8-bit child bounds; budget-gated, not exact)
MODE_FMA = 0x40             # OR-ed: the reference CMake build's arithmetic (GCC FMA contraction)
# Arithmetic of the host scene prep (CERES_ARITH_*): the reference without contraction, or as its
# own CMake build (g++ -O3 -mavx2 -mfma) compiles it; pair ARITH_FMA scenes with MODE_FMA renders
ARITH_EXACT, ARITH_FMA = 0, 1


def cfg_mode(cfg, arith=ARITH_EXACT):
    """The C-ABI mode of a configs.CONFIGS entry (| MODE_FMA for the reference-flag arithmetic)."""
    return ((MODE_PRIMARY if cfg["mode"] == "primary" else MODE_FULL) | (MODE_ROBUST if cfg.get("robust") else 0)
            | (MODE_FMA if arith else 0))
SCENE_STATS = 1
SCENE_FIRST_ORDER = 2

EXPORTED_SYMBOLS = (
    "ceres_obj_load", "ceres_proc_mesh", "ceres_rotate_triangles", "ceres_bvh_build", "ceres_bvh_build_gpu",
    "ceres_bvh_build_device", "ceres_obj_load_gpu", "ceres_obj_parse_device", "ceres_rotate_triangles_device",
    "ceres_device_free", "ceres_camera_basis", "ceres_obj_load_f64", "ceres_proc_mesh_f64", "ceres_rotate_triangles_f64",
    "ceres_bvh_build_f64", "ceres_camera_basis_f64", "ceres_orbit_cameras_f64", "ceres_scene_create_f64",
    "ceres_render_f64", "ceres_render_records_f64", "ceres_obj_load_f64_arith", "ceres_proc_mesh_f64_arith",
    "ceres_rotate_triangles_f64_arith", "ceres_bvh_build_f64_arith", "ceres_camera_basis_f64_arith",
    "ceres_orbit_cameras_f64_arith",
    "ceres_free", "ceres_scene_create", "ceres_scene_create_device", "ceres_scene_destroy", "ceres_scene_info", "ceres_scene_shadow_stacks", "ceres_scene_stack_width", "ceres_render_f32",
    "ceres_render_device", "ceres_render_batch_device", "ceres_render_multi_f32", "ceres_device_count", "ceres_assemble_rgb8_packed", "ceres_render_records", "ceres_tiling_local_rows",
    "ceres_scene_set_timing", "ceres_scene_read_timing", "ceres_scene_wave_log", "ceres_fetch_counters",
    "ceres_debug_compact_order", "ceres_debug_kept_tiles",
    "ceres_entry_cut_words", "ceres_entry_cut_build", "ceres_entry_relayout", "ceres_entry_rects", "ceres_entry_tiles",
    "ceres_debug_entry_record", "ceres_debug_entry_nodes", "ceres_debug_retire",
    "ceres_cpu_scene_create", "ceres_cpu_scene_destroy", "ceres_render_cpu_f32", "ceres_cpu_scene_create_f64",
    "ceres_render_cpu_f64",
    "ceres_orbit_cameras", "ceres_assemble_rgb8",
    "ceres_kernel_names", "ceres_last_error", "ceres_version",
    "ceres_obj_load_arith", "ceres_proc_mesh_arith", "ceres_rotate_triangles_arith", "ceres_bvh_build_arith",
    "ceres_camera_basis_arith", "ceres_orbit_cameras_arith", "ceres_content_hash",
    "ceres_bvh_build_gpu_arith", "ceres_bvh_build_device_arith", "ceres_obj_load_gpu_arith",
    "ceres_obj_parse_device_arith", "ceres_rotate_triangles_device_arith",
    "ceres_trace_rays", "ceres_trace_rays_device", "ceres_trace_rays_cpu",
    "ceres_trace_rays_f64", "ceres_trace_rays_f64_device", "ceres_trace_rays_cpu_f64",
    "ceres_shade_rays", "ceres_shade_rays_device", "ceres_shade_rays_cpu", "ceres_camera_rays",
    "ceres_shade_rays_f64", "ceres_shade_rays_f64_device", "ceres_shade_rays_cpu_f64", "ceres_camera_rays_f64",
    "ceres_scene_refit", "ceres_scene_refit_device", "ceres_scene_refit_f64", "ceres_scene_refit_f64_device",
    "ceres_cpu_scene_refit", "ceres_cpu_scene_refit_f64", "ceres_scene_read_boxes",
    "ceres_scene_sah_cost", "ceres_scene_rebuild", "ceres_scene_rebuild_device", "ceres_scene_update",
    "ceres_scene_update_device", "ceres_cpu_scene_sah_cost", "ceres_cpu_scene_rebuild", "ceres_cpu_scene_rebuild_f64",
    "ceres_cpu_scene_update", "ceres_cpu_scene_update_f64",
    "ceres_bvh_build_f64_gpu", "ceres_bvh_build_f64_gpu_arith", "ceres_bvh_build_f64_device",
    "ceres_bvh_build_f64_device_arith", "ceres_scene_create_f64_device",
    "ceres_trace_rays_all", "ceres_trace_rays_all_device", "ceres_trace_rays_all_cpu",
    "ceres_hit_offsets_scratch_bytes", "ceres_hit_offsets_device", "ceres_trace_rays_lists_device", "ceres_trace_rays_lists",
    "ceres_trace_rays_lists_cpu",
    "ceres_trace_rays_all_f64", "ceres_trace_rays_all_f64_device", "ceres_trace_rays_all_cpu_f64",
    "ceres_trace_rays_lists_f64_device", "ceres_trace_rays_lists_f64", "ceres_trace_rays_lists_cpu_f64",
    "ceres_trace_rays_indexed_device", "ceres_trace_rays_all_indexed_device", "ceres_trace_rays_lists_indexed_device",
    "ceres_shade_rays_indexed_device", "ceres_trace_rays_f64_indexed_device", "ceres_trace_rays_all_f64_indexed_device",
    "ceres_trace_rays_lists_f64_indexed_device", "ceres_shade_rays_f64_indexed_device",
    "ceres_ray_order_scratch_bytes", "ceres_ray_order_device", "ceres_ray_order_f64_device", "ceres_ray_order_cpu",
    "ceres_ray_order_cpu_f64", "ceres_cpu_scene_order_box", "ceres_trace_rays_coherent", "ceres_trace_rays_coherent_f64",
    "ceres_closest_points", "ceres_closest_points_device", "ceres_closest_points_indexed_device", "ceres_closest_points_cpu",
    "ceres_closest_points_f64", "ceres_closest_points_f64_device", "ceres_closest_points_f64_indexed_device",
    "ceres_closest_points_cpu_f64",
)

# ray queries (Scene.trace / CpuScene.trace): ray32 = bvh::Ray<float>, hit16 = {prim, t, u, v}
HIT_DTYPE = np.dtype([("prim", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
FLT_MAX = np.float32(np.finfo(np.float32).max)
# ... on double scenes: ray64 = bvh::Ray<double>, hit32 = {prim, reserved 0, t, u, v}
HIT64_DTYPE = np.dtype([("prim", np.int32), ("pad", np.uint32), ("t", np.float64), ("u", np.float64), ("v", np.float64)])
DBL_MAX = np.float64(np.finfo(np.float64).max)
# closest-point queries (Scene.closest_points / CpuScene.closest_points): point16 = {x, y, z, r2max} in,
# near16 = {prim, d2, u, v} out (u, v: the weights of p1() and p2(), the hit records' convention)
NEAR_DTYPE = np.dtype([("prim", np.int32), ("d2", np.float32), ("u", np.float32), ("v", np.float32)])
# ... on double scenes (Scene.closest_points_f64 / CpuScene.closest_points_f64): point32 = four doubles in,
# near32 = {prim, reserved 0, d2, u, v} out -- the hit32 shape
NEAR64_DTYPE = np.dtype([("prim", np.int32), ("pad", np.int32), ("d2", np.float64), ("u", np.float64), ("v", np.float64)])
MAX_HITS = 32               # CERES_MAX_HITS: the longest row of an all-hits query (Scene.trace_all)


class CeresError(RuntimeError):
    pass


class _Stats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("primary_rays", ctypes.c_uint64),
                ("shadow_rays", ctypes.c_uint64), ("node_pairs", ctypes.c_uint64), ("tri_tests", ctypes.c_uint64),
                ("ms", ctypes.c_double)]


class _UpdateInfo(ctypes.Structure):
    """ceres_update_info (Scene.update / CpuScene.update return its fields as a dict)."""
    _fields_ = [("cost", ctypes.c_double), ("built_cost", ctypes.c_double), ("new_cost", ctypes.c_double),
                ("rebuilt", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return dict(cost=self.cost, built_cost=self.built_cost, new_cost=self.new_cost, rebuilt=int(self.rebuilt))


class Tiling(ctypes.Structure):
    """ceres_tiling: bands = 0 -- row blocks dealt round-robin; bands = 1 -- frame f of a call renders
    the contiguous band (rank + f) mod world of row_block rows (distributed.FrameBands)."""
    _fields_ = [("row_block", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
                ("bands", ctypes.c_uint32)]


_lib = None
_fp = ctypes.POINTER(ctypes.c_float)
_dp = ctypes.POINTER(ctypes.c_double)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_sz = ctypes.c_size_t
_vp = ctypes.c_void_p


def build(verbose=False):
    """Compile libceres_hip.so and ./render for gfx950 (hipcc), in-tree."""
    import subprocess
    r = subprocess.run(["make", "-C", os.path.join(_PKG, "csrc"), "-j4", "all"], capture_output=True, text=True)
    if verbose or r.returncode:
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
    if r.returncode:
        raise CeresError("build of libceres_hip.so failed")


def _all_hits_argtypes(L):
    L.ceres_trace_rays_all.argtypes = [_vp, _vp, _sz, ctypes.c_int, ctypes.c_uint32, _vp, _vp, ctypes.POINTER(_Stats)]
    L.ceres_trace_rays_all_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp, _vp]
    L.ceres_trace_rays_all_cpu.argtypes = [_vp, _vp, _sz, ctypes.c_int, ctypes.c_uint32, _vp, _vp, ctypes.POINTER(_Stats),
                                           ctypes.c_int]
    if hasattr(L, "ceres_trace_rays_all_f64"):      # (an older revision's build lacks the double all-hits calls)
        L.ceres_trace_rays_all_f64.argtypes = L.ceres_trace_rays_all.argtypes
        L.ceres_trace_rays_all_f64_device.argtypes = L.ceres_trace_rays_all_device.argtypes
        L.ceres_trace_rays_all_cpu_f64.argtypes = L.ceres_trace_rays_all_cpu.argtypes


def _hit_lists_argtypes(L):
    L.ceres_hit_offsets_scratch_bytes.argtypes = [_sz]
    L.ceres_hit_offsets_scratch_bytes.restype = _sz
    L.ceres_hit_offsets_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _sz, _vp]
    L.ceres_trace_rays_lists_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, ctypes.c_uint64, _vp, _vp]
    L.ceres_trace_rays_lists.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, ctypes.c_uint64, _u64p, ctypes.POINTER(_Stats)]
    L.ceres_trace_rays_lists_cpu.argtypes = L.ceres_trace_rays_lists.argtypes + [ctypes.c_int]
    if hasattr(L, "ceres_trace_rays_lists_f64"):
        L.ceres_trace_rays_lists_f64_device.argtypes = L.ceres_trace_rays_lists_device.argtypes
        L.ceres_trace_rays_lists_f64.argtypes = L.ceres_trace_rays_lists.argtypes
        L.ceres_trace_rays_lists_cpu_f64.argtypes = L.ceres_trace_rays_lists_cpu.argtypes


def lib():
    """Load libceres_hip.so (import torch first when present so one HIP runtime is shared)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CeresError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    L.ceres_last_error.restype = ctypes.c_char_p
    L.ceres_version.restype = ctypes.c_char_p
    L.ceres_kernel_names.restype = ctypes.c_char_p
    L.ceres_obj_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(_fp), ctypes.POINTER(_fp), ctypes.POINTER(_sz)]
    L.ceres_proc_mesh.argtypes = [ctypes.c_int, ctypes.POINTER(_fp), ctypes.POINTER(_fp), ctypes.POINTER(_sz)]
    L.ceres_rotate_triangles.argtypes = [_fp, _sz, ctypes.c_int, ctypes.c_float]
    L.ceres_bvh_build.argtypes = [_fp, _sz, ctypes.POINTER(_u32p), ctypes.POINTER(_sz), ctypes.POINTER(_u64p)]
    L.ceres_bvh_build_gpu.argtypes = [_fp, _sz, ctypes.POINTER(_u32p), ctypes.POINTER(_sz), ctypes.POINTER(_u64p),
                                      ctypes.c_int]
    L.ceres_bvh_build_device.argtypes = [_vp, _sz, _vp, _vp, ctypes.POINTER(_sz), _vp]
    L.ceres_obj_load_gpu.argtypes = [ctypes.c_char_p, ctypes.POINTER(_fp), ctypes.POINTER(_fp), ctypes.POINTER(_sz),
                                     ctypes.c_int]
    L.ceres_obj_parse_device.argtypes = [_vp, _sz, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz), _vp]
    L.ceres_rotate_triangles_device.argtypes = [_vp, _sz, ctypes.c_int, ctypes.c_float, _vp]
    L.ceres_device_free.argtypes = [_vp]
    L.ceres_device_free.restype = None
    L.ceres_camera_basis.argtypes = [_fp, _fp, _fp, ctypes.c_float, _sz, _sz, _fp]
    L.ceres_obj_load_f64.argtypes = [ctypes.c_char_p, ctypes.POINTER(_dp), ctypes.POINTER(_dp), ctypes.POINTER(_sz)]
    L.ceres_proc_mesh_f64.argtypes = [ctypes.c_int, ctypes.POINTER(_dp), ctypes.POINTER(_dp), ctypes.POINTER(_sz)]
    L.ceres_rotate_triangles_f64.argtypes = [_dp, _sz, ctypes.c_int, ctypes.c_double]
    L.ceres_bvh_build_f64.argtypes = [_dp, _sz, ctypes.POINTER(_u64p), ctypes.POINTER(_sz), ctypes.POINTER(_u64p)]
    L.ceres_camera_basis_f64.argtypes = [_dp, _dp, _dp, ctypes.c_double, _sz, _sz, _dp]
    L.ceres_orbit_cameras_f64.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_double, _sz, _sz, _dp, ctypes.c_double,
                                          ctypes.c_uint32, ctypes.c_int, _dp, _dp, _dp]
    L.ceres_obj_load_f64_arith.argtypes = [ctypes.c_char_p, ctypes.POINTER(_dp), ctypes.POINTER(_dp), ctypes.POINTER(_sz),
                                           ctypes.c_int]
    L.ceres_proc_mesh_f64_arith.argtypes = [ctypes.c_int, ctypes.POINTER(_dp), ctypes.POINTER(_dp), ctypes.POINTER(_sz),
                                            ctypes.c_int]
    L.ceres_rotate_triangles_f64_arith.argtypes = [_dp, _sz, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    L.ceres_bvh_build_f64_arith.argtypes = [_dp, _sz, ctypes.POINTER(_u64p), ctypes.POINTER(_sz), ctypes.POINTER(_u64p),
                                            ctypes.c_int]
    L.ceres_camera_basis_f64_arith.argtypes = [_dp, _dp, _dp, ctypes.c_double, _sz, _sz, _dp, ctypes.c_int]
    L.ceres_orbit_cameras_f64_arith.argtypes = [_dp, _dp, _dp, _dp, ctypes.c_double, _sz, _sz, _dp, ctypes.c_double,
                                                ctypes.c_uint32, ctypes.c_int, _dp, _dp, _dp, ctypes.c_int]
    L.ceres_scene_create_f64.argtypes = [_dp, _sz, _dp, _vp, _sz, _u64p, ctypes.c_int, ctypes.c_uint32]
    L.ceres_scene_create_f64.restype = _vp
    L.ceres_bvh_build_f64_gpu.argtypes = [_dp, _sz, ctypes.POINTER(_u64p), ctypes.POINTER(_sz), ctypes.POINTER(_u64p),
                                          ctypes.c_int]
    L.ceres_bvh_build_f64_gpu_arith.argtypes = L.ceres_bvh_build_f64_gpu.argtypes + [ctypes.c_int]
    L.ceres_bvh_build_f64_device.argtypes = [_vp, _sz, _vp, _vp, ctypes.POINTER(_sz), _vp]
    L.ceres_bvh_build_f64_device_arith.argtypes = L.ceres_bvh_build_f64_device.argtypes + [ctypes.c_int]
    L.ceres_scene_create_f64_device.argtypes = [_vp, _sz, _vp, _vp, _sz, _vp, ctypes.c_int, ctypes.c_uint32, _vp]
    L.ceres_scene_create_f64_device.restype = _vp
    L.ceres_render_f64.argtypes = [_vp, _dp, _dp, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_uint8), _sz, _sz,
                                   ctypes.POINTER(_Stats)]
    L.ceres_render_records_f64.argtypes = [_vp, _dp, _dp, ctypes.c_int, _sz, _sz, ctypes.POINTER(ctypes.c_int32), _dp,
                                           ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(_Stats)]
    L.ceres_orbit_cameras.argtypes = [_fp, _fp, _fp, _fp, ctypes.c_float, _sz, _sz, _fp, ctypes.c_float,
                                      ctypes.c_uint32, ctypes.c_int, _fp, _fp, _fp]
    L.ceres_free.argtypes = [_vp]
    L.ceres_free.restype = None
    L.ceres_scene_create.argtypes = [_fp, _sz, _fp, _vp, _sz, _u64p, ctypes.c_int, ctypes.c_uint32]
    L.ceres_scene_create.restype = _vp
    L.ceres_scene_create_device.argtypes = [_vp, _sz, _vp, _vp, _sz, _vp, ctypes.c_int, ctypes.c_uint32, _vp]
    L.ceres_scene_create_device.restype = _vp
    L.ceres_scene_destroy.argtypes = [_vp]
    L.ceres_scene_destroy.restype = None
    L.ceres_scene_info.argtypes = [_vp, _u32p, _u32p, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    L.ceres_scene_shadow_stacks.argtypes = [_vp, _u32p, _u32p]
    L.ceres_scene_stack_width.argtypes = [_vp]
    L.ceres_render_f32.argtypes = [_vp, _fp, _fp, ctypes.c_int, _fp, ctypes.POINTER(ctypes.c_uint8), _sz, _sz,
                                   ctypes.POINTER(_Stats)]
    L.ceres_render_device.argtypes = [_vp, _fp, _fp, ctypes.c_int, _sz, _sz, ctypes.POINTER(Tiling), _vp, _vp, _vp, _vp]
    L.ceres_render_batch_device.argtypes = [_vp, ctypes.c_uint32, _fp, _fp, ctypes.c_int, _sz, _sz,
                                            ctypes.POINTER(Tiling), _vp, _vp, _vp, _vp]
    L.ceres_render_multi_f32.argtypes = [ctypes.POINTER(_vp), ctypes.c_uint32, ctypes.c_uint32, _fp, _fp, ctypes.c_int, _fp,
                                         ctypes.POINTER(ctypes.c_uint8), _sz, _sz, ctypes.POINTER(_Stats)]
    L.ceres_assemble_rgb8_packed.argtypes = [_vp, _vp, ctypes.c_uint32, _sz, _sz, ctypes.c_uint32, ctypes.c_uint32, _vp]
    L.ceres_assemble_rgb8.argtypes = [_vp, _sz, _vp, ctypes.c_uint32, _sz, _sz, ctypes.c_uint32, ctypes.c_uint32, _vp]
    L.ceres_render_records.argtypes = [_vp, _fp, _fp, ctypes.c_int, _sz, _sz, ctypes.POINTER(ctypes.c_int32), _fp,
                                       ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(_Stats)]
    L.ceres_tiling_local_rows.argtypes = [_sz, ctypes.POINTER(Tiling)]
    L.ceres_tiling_local_rows.restype = _sz
    L.ceres_scene_set_timing.argtypes = [_vp, ctypes.c_int]
    L.ceres_scene_read_timing.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                          _u64p]
    L.ceres_scene_wave_log.argtypes = [_vp, _u64p, _sz, ctypes.POINTER(_sz)]
    L.ceres_fetch_counters.argtypes = [ctypes.c_int, _u64p, ctypes.c_int]
    if hasattr(L, "ceres_debug_compact_order"):     # (tools/ab.py also loads builds of earlier revisions)
        L.ceres_debug_compact_order.argtypes = [_vp, _u32p, _u32p, _u32p, _sz]
        L.ceres_debug_kept_tiles.argtypes = [_sz, _sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint16), _u32p,
                                             _u32p, _sz]
    if hasattr(L, "ceres_entry_cut_build"):
        _u16p = ctypes.POINTER(ctypes.c_uint16)
        L.ceres_entry_cut_words.restype = _sz
        L.ceres_entry_cut_build.argtypes = [_vp, _sz, ctypes.c_uint32, _fp, _u32p]
        L.ceres_entry_relayout.argtypes = [_fp, _sz, _vp, _sz, _u64p, _vp, ctypes.POINTER(_sz), _u32p, _u32p]
        L.ceres_entry_rects.argtypes = [_u32p, _fp, _sz, _sz, _u16p]
        L.ceres_entry_tiles.argtypes = [_u32p, _u16p, _sz, _sz, _u32p]
        L.ceres_debug_entry_record.argtypes = [_vp, ctypes.c_int]
        L.ceres_debug_entry_nodes.argtypes = [_vp, _u32p, _u32p, _u16p, _u32p, _sz]
    if hasattr(L, "ceres_debug_retire"):
        L.ceres_debug_retire.argtypes = [_vp, _u32p, _u32p, ctypes.POINTER(ctypes.c_uint8), _sz]
    L.ceres_cpu_scene_create.argtypes = [_fp, _sz, _fp, _vp, _sz, _u64p]
    L.ceres_cpu_scene_create.restype = _vp
    L.ceres_cpu_scene_destroy.argtypes = [_vp]
    L.ceres_cpu_scene_destroy.restype = None
    L.ceres_render_cpu_f32.argtypes = [_vp, _fp, _fp, ctypes.c_int, _fp, ctypes.POINTER(ctypes.c_uint8), _sz, _sz,
                                       ctypes.POINTER(_Stats), ctypes.c_int]
    L.ceres_cpu_scene_create_f64.argtypes = [_dp, _sz, _dp, _vp, _sz, _u64p]
    L.ceres_cpu_scene_create_f64.restype = _vp
    L.ceres_render_cpu_f64.argtypes = [_vp, _dp, _dp, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_uint8), _sz, _sz,
                                       ctypes.POINTER(_Stats), ctypes.c_int]
    L.ceres_trace_rays.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, ctypes.POINTER(_Stats)]
    L.ceres_trace_rays_device.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, _vp, _vp]
    L.ceres_trace_rays_cpu.argtypes = [_vp, _vp, _sz, ctypes.c_int, _vp, _vp, ctypes.POINTER(_Stats), ctypes.c_int]
    if hasattr(L, "ceres_trace_rays_all"):      # (CERES_LIB may name a build of an older revision: tools/trace_bench.py --closest-only)
        _all_hits_argtypes(L)
    if hasattr(L, "ceres_trace_rays_lists"):    # (likewise: tools/trace_bench.py --lists measures the parent's library beside)
        _hit_lists_argtypes(L)
    L.ceres_trace_rays_f64.argtypes = L.ceres_trace_rays.argtypes
    L.ceres_trace_rays_f64_device.argtypes = L.ceres_trace_rays_device.argtypes
    L.ceres_trace_rays_cpu_f64.argtypes = L.ceres_trace_rays_cpu.argtypes
    L.ceres_shade_rays.argtypes = [_vp, _vp, _sz, _fp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.POINTER(_Stats)]
    L.ceres_shade_rays_device.argtypes = [_vp, _vp, _sz, _fp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    L.ceres_shade_rays_cpu.argtypes = L.ceres_shade_rays.argtypes + [ctypes.c_int]
    L.ceres_camera_rays.argtypes = [_fp, _sz, _sz, ctypes.c_int, _vp]
    L.ceres_shade_rays_f64.argtypes = [_vp, _vp, _sz, _dp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.POINTER(_Stats)]
    L.ceres_shade_rays_f64_device.argtypes = [_vp, _vp, _sz, _dp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    L.ceres_shade_rays_cpu_f64.argtypes = L.ceres_shade_rays_f64.argtypes + [ctypes.c_int]
    L.ceres_camera_rays_f64.argtypes = [_dp, _sz, _sz, ctypes.c_int, _vp]
    if hasattr(L, "ceres_ray_order_device"):    # (CERES_LIB may name a build of an older revision: tools/trace_bench.py)
        _indexed_argtypes(L)
    if hasattr(L, "ceres_closest_points"):      # (likewise)
        L.ceres_closest_points.argtypes = [_vp, _vp, _sz, _vp, ctypes.POINTER(_Stats)]
        L.ceres_closest_points_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp]
        L.ceres_closest_points_indexed_device.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]
        L.ceres_closest_points_cpu.argtypes = [_vp, _vp, _sz, _vp, ctypes.POINTER(_Stats), ctypes.c_int]
    if hasattr(L, "ceres_closest_points_f64"):  # (likewise)
        L.ceres_closest_points_f64.argtypes = [_vp, _vp, _sz, _vp, ctypes.POINTER(_Stats)]
        L.ceres_closest_points_f64_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp]
        L.ceres_closest_points_f64_indexed_device.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]
        L.ceres_closest_points_cpu_f64.argtypes = [_vp, _vp, _sz, _vp, ctypes.POINTER(_Stats), ctypes.c_int]
    L.ceres_scene_refit.argtypes = [_vp, _fp, _sz, _fp]
    L.ceres_scene_refit_f64.argtypes = [_vp, _dp, _sz, _dp]
    L.ceres_scene_refit_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.ceres_scene_refit_f64_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.ceres_cpu_scene_refit.argtypes = [_vp, _fp, _sz, _fp]
    L.ceres_cpu_scene_refit_f64.argtypes = [_vp, _dp, _sz, _dp]
    L.ceres_scene_read_boxes.argtypes = [_vp, _vp, ctypes.POINTER(_sz), _fp, ctypes.POINTER(_sz)]
    _ui = ctypes.POINTER(_UpdateInfo)
    L.ceres_scene_sah_cost.argtypes = [_vp, _dp, _vp]
    L.ceres_scene_rebuild.argtypes = [_vp, _fp, _sz, _fp, ctypes.c_int]
    L.ceres_scene_rebuild_device.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_int, _vp]
    L.ceres_scene_update.argtypes = [_vp, _fp, _sz, _fp, ctypes.c_int, ctypes.c_double, _ui]
    L.ceres_scene_update_device.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_int, ctypes.c_double, _ui, _vp]
    L.ceres_cpu_scene_sah_cost.argtypes = [_vp, _dp]
    L.ceres_cpu_scene_rebuild.argtypes = [_vp, _fp, _sz, _fp, ctypes.c_int]
    L.ceres_cpu_scene_rebuild_f64.argtypes = [_vp, _dp, _sz, _dp, ctypes.c_int]
    L.ceres_cpu_scene_update.argtypes = [_vp, _fp, _sz, _fp, ctypes.c_int, ctypes.c_double, _ui]
    L.ceres_cpu_scene_update_f64.argtypes = [_vp, _dp, _sz, _dp, ctypes.c_int, ctypes.c_double, _ui]
    L.ceres_content_hash.argtypes = [_vp, _sz]
    L.ceres_content_hash.restype = ctypes.c_uint64
    L.ceres_obj_load_arith.argtypes = L.ceres_obj_load.argtypes + [ctypes.c_int]
    L.ceres_proc_mesh_arith.argtypes = L.ceres_proc_mesh.argtypes + [ctypes.c_int]
    L.ceres_rotate_triangles_arith.argtypes = L.ceres_rotate_triangles.argtypes + [ctypes.c_int]
    L.ceres_bvh_build_arith.argtypes = L.ceres_bvh_build.argtypes + [ctypes.c_int]
    L.ceres_camera_basis_arith.argtypes = L.ceres_camera_basis.argtypes + [ctypes.c_int]
    L.ceres_orbit_cameras_arith.argtypes = L.ceres_orbit_cameras.argtypes + [ctypes.c_int]
    L.ceres_bvh_build_gpu_arith.argtypes = L.ceres_bvh_build_gpu.argtypes + [ctypes.c_int]
    L.ceres_bvh_build_device_arith.argtypes = L.ceres_bvh_build_device.argtypes + [ctypes.c_int]
    L.ceres_obj_load_gpu_arith.argtypes = L.ceres_obj_load_gpu.argtypes + [ctypes.c_int]
    L.ceres_obj_parse_device_arith.argtypes = L.ceres_obj_parse_device.argtypes + [ctypes.c_int]
    L.ceres_rotate_triangles_device_arith.argtypes = L.ceres_rotate_triangles_device.argtypes + [ctypes.c_int]
    _lib = L
    return L


def _indexed_argtypes(L):
    """The indexed ray queries and the coherent order: each indexed call is its plain sibling with
    (d_index, n_index) after n_rays."""
    for plain in ("ceres_trace_rays_device", "ceres_trace_rays_all_device", "ceres_trace_rays_lists_device",
                  "ceres_shade_rays_device", "ceres_trace_rays_f64_device", "ceres_trace_rays_all_f64_device",
                  "ceres_trace_rays_lists_f64_device", "ceres_shade_rays_f64_device"):
        a = list(getattr(L, plain).argtypes)
        getattr(L, plain.replace("_device", "_indexed_device")).argtypes = a[:3] + [_vp, _sz] + a[3:]
    L.ceres_ray_order_scratch_bytes.argtypes = [_sz]
    L.ceres_ray_order_scratch_bytes.restype = _sz
    L.ceres_ray_order_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _sz, _vp]
    L.ceres_ray_order_f64_device.argtypes = L.ceres_ray_order_device.argtypes
    L.ceres_ray_order_cpu.argtypes = [_vp, _vp, _sz, _vp]
    L.ceres_ray_order_cpu_f64.argtypes = L.ceres_ray_order_cpu.argtypes
    L.ceres_cpu_scene_order_box.argtypes = [_vp, _dp, ctypes.POINTER(ctypes.c_int)]
    L.ceres_trace_rays_coherent.argtypes = L.ceres_trace_rays.argtypes
    L.ceres_trace_rays_coherent_f64.argtypes = L.ceres_trace_rays.argtypes


def _check(rc):
    if rc != 0:
        raise CeresError(f"ceres error {rc}: {lib().ceres_last_error().decode()}")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def _take(ptr, count, dtype):
    if count == 0:
        lib().ceres_free(ctypes.cast(ptr, _vp))
        return np.zeros(0, dtype)
    a = np.ctypeslib.as_array(ptr, shape=(count,)).copy().view(dtype)
    lib().ceres_free(ctypes.cast(ptr, _vp))
    return a


class Camera:
    """render.hpp:16-22 -- eye, dir, up, fov (degrees); Camera<float> or, with dtype=np.float64,
    Camera<double> (anim.cpp -d)."""

    def __init__(self, eye, dir, up, fov, dtype=np.float32, arith=ARITH_EXACT):
        self.dtype = np.dtype(dtype)
        self.eye = np.asarray(eye, self.dtype)
        self.dir = np.asarray(dir, self.dtype)
        self.up = np.asarray(up, self.dtype)
        self.fov = float(fov)
        self.arith = int(arith)                      # float cameras: CERES_ARITH_* of the basis

    def basis(self, W, H):
        """render.hpp:91-97 on the host (libm stays on the host): {eye, dir, image_u, image_v}."""
        if self.dtype == np.float64:
            out = np.zeros(9, np.float64)
            _check(lib().ceres_camera_basis_f64_arith(_p(self.eye, ctypes.c_double), _p(self.dir, ctypes.c_double),
                                                      _p(self.up, ctypes.c_double), self.fov, W, H,
                                                      _p(out, ctypes.c_double), self.arith))
            return np.concatenate([self.eye, out])
        out = np.zeros(9, np.float32)
        _check(lib().ceres_camera_basis_arith(_p(self.eye, ctypes.c_float), _p(self.dir, ctypes.c_float),
                                              _p(self.up, ctypes.c_float), self.fov, W, H, _p(out, ctypes.c_float),
                                              self.arith))
        return np.concatenate([self.eye, out]).astype(np.float32)


class Mesh:
    """Triangles (n x 12 = bvh::Triangle<S>) and per-triangle vertex normals (n x 9); S = float
    (f32 arrays) or double (f64 arrays, render<double>)."""

    def __init__(self, tri, norm):
        dt = np.float64 if np.asarray(tri).dtype == np.float64 else np.float32
        self.tri = np.ascontiguousarray(tri, dt).reshape(-1, 12)
        self.norm = np.ascontiguousarray(norm, dt).reshape(-1, 9)

    @property
    def f64(self):
        return self.tri.dtype == np.float64

    def __len__(self):
        return self.tri.shape[0]


class Bvh:
    """bvh::Bvh<S>: nodes (m x 8 u32 = Node<float>, or m x 8 u64 = Node<double>: 6 doubles +
    2 u64) and primitive_indices (u64)."""

    def __init__(self, nodes, prim):
        dt = np.uint64 if np.asarray(nodes).dtype == np.uint64 else np.uint32
        self.nodes = np.ascontiguousarray(nodes, dt).reshape(-1, 8)
        self.prim = np.ascontiguousarray(prim, np.uint64)


def load_obj(path, arith=ARITH_EXACT):
    t, n, cnt = _fp(), _fp(), _sz()
    _check(lib().ceres_obj_load_arith(os.fsencode(path), ctypes.byref(t), ctypes.byref(n), ctypes.byref(cnt), int(arith)))
    c = cnt.value
    return Mesh(_take(t, c * 12, np.float32).reshape(c, 12), _take(n, c * 9, np.float32).reshape(c, 9))


def load_obj_f64(path, arith=ARITH_EXACT):
    """obj::load_from_file<double> (anim.cpp -d): strtof coordinates widened to double."""
    t, n, cnt = _dp(), _dp(), _sz()
    _check(lib().ceres_obj_load_f64_arith(os.fsencode(path), ctypes.byref(t), ctypes.byref(n), ctypes.byref(cnt),
                                          int(arith)))
    c = cnt.value
    return Mesh(_take(t, c * 12, np.float64).reshape(c, 12), _take(n, c * 9, np.float64).reshape(c, 9))


def proc_mesh_f64(n, arith=ARITH_EXACT):
    t, nn, cnt = _dp(), _dp(), _sz()
    _check(lib().ceres_proc_mesh_f64_arith(int(n), ctypes.byref(t), ctypes.byref(nn), ctypes.byref(cnt), int(arith)))
    c = cnt.value
    return Mesh(_take(t, c * 12, np.float64).reshape(c, 12), _take(nn, c * 9, np.float64).reshape(c, 9))


def load_obj_gpu(path, device=0, arith=ARITH_EXACT):
    """load_obj with the text parsed on the GPU (ceres_obj_load_gpu): the same bits."""
    t, n, cnt = _fp(), _fp(), _sz()
    _check(lib().ceres_obj_load_gpu_arith(os.fsencode(path), ctypes.byref(t), ctypes.byref(n), ctypes.byref(cnt),
                                          int(device), int(arith)))
    c = cnt.value
    return Mesh(_take(t, c * 12, np.float32).reshape(c, 12), _take(n, c * 9, np.float32).reshape(c, 9))


def parse_obj_device(d_text, length, stream=0, arith=ARITH_EXACT):
    """ceres_obj_parse_device on a device text buffer (int pointer): returns (d_tri48, d_norm36, n_tri)
    device pointers (free with device_free)."""
    t, n, cnt = _vp(), _vp(), _sz()
    _check(lib().ceres_obj_parse_device_arith(d_text, length, ctypes.byref(t), ctypes.byref(n), ctypes.byref(cnt),
                                              stream or None, int(arith)))
    return t.value or 0, n.value or 0, cnt.value


def rotate_triangles_device(d_tri48, n_tri, axis, degrees, stream=0, arith=ARITH_EXACT):
    ax = {"x": 0, "y": 1, "z": 2}[axis] if isinstance(axis, str) else int(axis)
    _check(lib().ceres_rotate_triangles_device_arith(d_tri48, n_tri, ax, float(degrees), stream or None, int(arith)))


def device_free(d_ptr):
    lib().ceres_device_free(d_ptr or None)


def proc_mesh(n, arith=ARITH_EXACT):
    t, nn, cnt = _fp(), _fp(), _sz()
    _check(lib().ceres_proc_mesh_arith(int(n), ctypes.byref(t), ctypes.byref(nn), ctypes.byref(cnt), int(arith)))
    c = cnt.value
    return Mesh(_take(t, c * 12, np.float32).reshape(c, 12), _take(nn, c * 9, np.float32).reshape(c, 9))


def rotate_triangles(mesh, axis, degrees, arith=ARITH_EXACT):
    ax = {"x": 0, "y": 1, "z": 2}[axis] if isinstance(axis, str) else int(axis)
    if mesh.f64:
        _check(lib().ceres_rotate_triangles_f64_arith(_p(mesh.tri, ctypes.c_double), len(mesh), ax, float(degrees),
                                                      int(arith)))
    else:
        _check(lib().ceres_rotate_triangles_arith(_p(mesh.tri, ctypes.c_float), len(mesh), ax, float(degrees),
                                                  int(arith)))
    return mesh


def build_bvh(mesh, arith=ARITH_EXACT):
    if mesh.f64:
        nodes, prim, m = _u64p(), _u64p(), _sz()
        _check(lib().ceres_bvh_build_f64_arith(_p(mesh.tri, ctypes.c_double), len(mesh), ctypes.byref(nodes),
                                               ctypes.byref(m), ctypes.byref(prim), int(arith)))
        return Bvh(_take(nodes, m.value * 8, np.uint64).reshape(-1, 8), _take(prim, len(mesh), np.uint64))
    nodes, prim, m = _u32p(), _u64p(), _sz()
    _check(lib().ceres_bvh_build_arith(_p(mesh.tri, ctypes.c_float), len(mesh), ctypes.byref(nodes), ctypes.byref(m),
                                       ctypes.byref(prim), int(arith)))
    return Bvh(_take(nodes, m.value * 8, np.uint32).reshape(-1, 8), _take(prim, len(mesh), np.uint64))


def build_bvh_gpu(mesh, device=0, arith=ARITH_EXACT):
    """The same binned-SAH BVH as build_bvh, built on the GPU (ceres_bvh_build_gpu; a double mesh:
    ceres_bvh_build_f64_gpu, 64-B nodes)."""
    if mesh.f64:
        nodes, prim, m = _u64p(), _u64p(), _sz()
        _check(lib().ceres_bvh_build_f64_gpu_arith(_p(mesh.tri, ctypes.c_double), len(mesh), ctypes.byref(nodes),
                                                   ctypes.byref(m), ctypes.byref(prim), int(device), int(arith)))
        return Bvh(_take(nodes, m.value * 8, np.uint64).reshape(-1, 8), _take(prim, len(mesh), np.uint64))
    nodes, prim, m = _u32p(), _u64p(), _sz()
    _check(lib().ceres_bvh_build_gpu_arith(_p(mesh.tri, ctypes.c_float), len(mesh), ctypes.byref(nodes),
                                           ctypes.byref(m), ctypes.byref(prim), int(device), int(arith)))
    return Bvh(_take(nodes, m.value * 8, np.uint32).reshape(-1, 8), _take(prim, len(mesh), np.uint64))


def build_bvh_device(d_tri48, n_tri, d_nodes32, d_prim32, stream=0, arith=ARITH_EXACT):
    """ceres_bvh_build_device on device pointers (ints); returns the node count."""
    m = _sz()
    _check(lib().ceres_bvh_build_device_arith(d_tri48, n_tri, d_nodes32, d_prim32, ctypes.byref(m), stream or None,
                                              int(arith)))
    return m.value


def build_bvh_device_f64(d_tri96, n_tri, d_nodes64, d_prim32, stream=0, arith=ARITH_EXACT):
    """ceres_bvh_build_f64_device on device pointers (ints, 16-byte aligned): Triangle<double> records in,
    64-B nodes and u32 primitive_indices out; returns the node count."""
    m = _sz()
    _check(lib().ceres_bvh_build_f64_device_arith(d_tri96 or None, n_tri, d_nodes64 or None, d_prim32 or None, ctypes.byref(m),
                                                  stream or None, int(arith)))
    return m.value


def ray_order_scratch_bytes(n_rays):
    """ceres_ray_order_scratch_bytes: the scratch Scene.ray_order_device needs for n_rays rays (host
    arithmetic: no device is touched)."""
    return int(lib().ceres_ray_order_scratch_bytes(int(n_rays)))


def hit_offsets_scratch_bytes(n_rays):
    """ceres_hit_offsets_scratch_bytes: the scratch Scene.hit_offsets_device needs for n_rays counts."""
    return int(lib().ceres_hit_offsets_scratch_bytes(int(n_rays)))


def _rays32(rays, f64=False):
    r = np.ascontiguousarray(rays, np.float64 if f64 else np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise CeresError("rays: an [n, 8] %s array {origin[3], direction[3], tmin, tmax}" % ("float64" if f64 else "float32"))
    return r


def _trace_host(call, rays, mode, closest, occluded, f64=False):
    """Shared body of Scene.trace / CpuScene.trace: call(rays_ptr, n, mode, hits_ptr, occ_ptr, stats_ref);
    f64: ray64 records in, hit32 records (HIT64_DTYPE) out."""
    r = _rays32(rays, f64)
    n = r.shape[0]
    hits = np.zeros(n, HIT64_DTYPE if f64 else HIT_DTYPE) if closest else None
    occ = np.zeros(n, np.uint8) if occluded else None
    st = _Stats()
    vp = lambda a: None if a is None else a.ctypes.data_as(_vp)     # noqa: E731
    _check(call(vp(r), n, int(mode), vp(hits), vp(occ), ctypes.byref(st)))
    return hits, occ, dict(rays=st.rays, hits=st.hits, node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


def _points16(points):
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] not in (3, 4):
        raise CeresError("points: an [n, 4] float32 array {x, y, z, r2max}, or [n, 3] (r2max = +inf)")
    if p.shape[1] == 3:
        p = np.concatenate([p, np.full((p.shape[0], 1), np.inf, np.float32)], axis=1)
    return p


def _points32(points):
    p = np.ascontiguousarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] not in (3, 4):
        raise CeresError("points: an [n, 4] float64 array {x, y, z, r2max}, or [n, 3] (r2max = +inf)")
    if p.shape[1] == 3:
        p = np.concatenate([p, np.full((p.shape[0], 1), np.inf, np.float64)], axis=1)
    return p


def _closest_host(call, points, f64=False):
    """Shared body of Scene.closest_points / CpuScene.closest_points: call(points_ptr, n, near_ptr, stats_ref);
    f64: point32 records in, near32 records (NEAR64_DTYPE) out."""
    p = _points32(points) if f64 else _points16(points)
    n = p.shape[0]
    near = np.zeros(n, NEAR64_DTYPE if f64 else NEAR_DTYPE)
    st = _Stats()
    _check(call(p.ctypes.data_as(_vp), n, near.ctypes.data_as(_vp), ctypes.byref(st)))
    return near, dict(rays=st.rays, hits=st.hits, node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


def _trace_all_host(call, rays, max_hits, mode, hits, f64=False):
    """Shared body of Scene.trace_all / CpuScene.trace_all: call(rays_ptr, n, mode, max_hits, counts_ptr,
    hits_ptr, stats_ref) -> (counts [n] u32, hits [n, max_hits] HIT_DTYPE | None, stats); f64: ray64 records
    in, hit32 records (HIT64_DTYPE) out."""
    r = _rays32(rays, f64)
    n = r.shape[0]
    if hits and not 1 <= int(max_hits) <= MAX_HITS:
        raise CeresError("max_hits: 1 .. %d with hits (hits=False: the count-only query)" % MAX_HITS)
    counts = np.zeros(n, np.uint32)
    rows = np.zeros((n, int(max_hits)), HIT64_DTYPE if f64 else HIT_DTYPE) if hits else None
    st = _Stats()
    vp = lambda a: None if a is None else a.ctypes.data_as(_vp)     # noqa: E731
    _check(call(vp(r), n, int(mode), int(max_hits), vp(counts), vp(rows), ctypes.byref(st)))
    return counts, rows, dict(rays=st.rays, hits=st.hits, node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


ENOMEM = -3                 # CERES_ENOMEM: what a complete-hit-list call returns while `capacity` is below the total


def _trace_lists_host(call, rays, mode, f64=False):
    """Shared body of Scene.trace_lists / CpuScene.trace_lists: call(rays_ptr, n, mode, offsets_ptr, hits_ptr,
    capacity, total_ref, stats_ref), asked first without a buffer (offsets and the total come back with
    CERES_ENOMEM), then with one of `total` records -> (offsets [n + 1] u64, hits [total] HIT_DTYPE, stats);
    f64: ray64 records in, hit32 records (HIT64_DTYPE) out."""
    r = _rays32(rays, f64)
    n = r.shape[0]
    offsets = np.zeros(n + 1, np.uint64)
    total = ctypes.c_uint64(0)
    st = _Stats()
    vp = lambda a: None if a is None else a.ctypes.data_as(_vp)     # noqa: E731
    rc = call(vp(r), n, int(mode), vp(offsets), None, 0, ctypes.byref(total), ctypes.byref(st))
    if rc != ENOMEM:
        _check(rc)                                                  # no hit at all: done; or a refusal
    hits = np.zeros(int(total.value), HIT64_DTYPE if f64 else HIT_DTYPE)
    if rc == ENOMEM:
        _check(call(vp(r), n, int(mode), vp(offsets), vp(hits), hits.shape[0], ctypes.byref(total), ctypes.byref(st)))
    return offsets, hits, dict(rays=st.rays, hits=st.hits, node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


def _shade_host(call, rays, sun, mode, pixels, rgb8, hits, status, f64=False):
    """Shared body of Scene.shade / CpuScene.shade: call(rays_ptr, n, sun_ptr, mode, pixels_ptr, rgb8_ptr,
    hits_ptr, status_ptr, stats_ref); f64: ray64 records and a float64 sun in, float64 pixels and hit32
    records (HIT64_DTYPE) out."""
    dt, ct = (np.float64, ctypes.c_double) if f64 else (np.float32, ctypes.c_float)
    r = _rays32(rays, f64)
    n = r.shape[0]
    s = np.ascontiguousarray(sun, dt).reshape(3)
    px = np.zeros((n, 3), dt) if pixels else None
    q = np.zeros((n, 3), np.uint8) if rgb8 else None
    h = np.zeros(n, HIT64_DTYPE if f64 else HIT_DTYPE) if hits else None
    stt = np.zeros(n, np.uint8) if status else None
    st = _Stats()
    vp = lambda a: None if a is None else a.ctypes.data_as(_vp)     # noqa: E731
    _check(call(vp(r), n, _p(s, ct), int(mode), vp(px), vp(q), vp(h), vp(stt), ctypes.byref(st)))
    return px, q, h, stt, dict(rays=st.rays, hits=st.hits, primary_rays=st.primary_rays, shadow_rays=st.shadow_rays,
                               node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


def camera_rays(basis12, W, H, arith=ARITH_EXACT):
    """The [W*H, 8] ray32 records of a view's primary rays (render.hpp:105-113), ray j*W + i for
    pixel (i, j), built on the host in float32 in the contraction-free arithmetic -- bit for bit the
    rays the exact (non-FMA) render kernels trace: u = 2(i + 0.5)/W - 1, v = 2(j + 0.5)/H - 1,
    a = iu u + iv v + dir, d = a * (1 / sqrt(a.a)), origin = eye, window [0, FLT_MAX].
    arith = ARITH_FMA: ceres_camera_rays in the reference CMake build's arithmetic (the rays the
    MODE_FMA render kernels trace)."""
    f = np.float32
    if arith != ARITH_EXACT:
        return camera_rays_native(basis12, W, H, arith)
    b = np.asarray(basis12, f).reshape(12)
    eye, dir_, iu, iv = b[0:3], b[3:6], b[6:9], b[9:12]
    u = f(2) * (np.arange(W, dtype=f) + f(0.5)) / f(W) - f(1)
    v = f(2) * (np.arange(H, dtype=f) + f(0.5)) / f(H) - f(1)
    uu = np.tile(u, H)[:, None]
    vv = np.repeat(v, W)[:, None]
    a = (iu[None, :] * uu + iv[None, :] * vv) + dir_[None, :]
    s = a[:, 0] * a[:, 0]
    s = s + a[:, 1] * a[:, 1]
    s = s + a[:, 2] * a[:, 2]
    inv = f(1) / np.sqrt(s)
    rays = np.empty((W * H, 8), f)
    rays[:, 0:3] = eye
    rays[:, 3:6] = a * inv[:, None]
    rays[:, 6] = 0
    rays[:, 7] = FLT_MAX
    return rays


def camera_rays_native(basis12, W, H, arith=ARITH_EXACT):
    """ceres_camera_rays: camera_rays by the library's own ray generator (render_rows' expressions), in
    either arithmetic."""
    b = np.ascontiguousarray(basis12, np.float32).reshape(12)
    rays = np.empty((int(W) * int(H), 8), np.float32)
    _check(lib().ceres_camera_rays(_p(b, ctypes.c_float), int(W), int(H), int(arith), rays.ctypes.data_as(_vp)))
    return rays


def shadow_rays(mesh, hits, sun):
    """render()'s shadow rays (render.hpp:127-136) of closest hits, as ray32 records in the same
    float32 contraction-free arithmetic: for a hit (prim, u, v) on triangle {p0, e1, e2, n},
    p = p0 u + (p0 - e1) v + (p0 + e2)(1 - u - v), origin = p + normalize(n) * -0.00001f, direction =
    normalize(sun - origin), window [0, FLT_MAX].  Returns (rays [k, 8], the indices of the k hits)."""
    f = np.float32
    idx = np.nonzero(hits["prim"] >= 0)[0]
    tr = mesh.tri[hits["prim"][idx]]
    p0, e1, e2, n = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9], tr[:, 9:12]
    hu, hv = hits["u"][idx][:, None], hits["v"][idx][:, None]
    w = f(1) - hu - hv

    def normalize(x):
        s = x[:, 0] * x[:, 0]
        s = s + x[:, 1] * x[:, 1]
        s = s + x[:, 2] * x[:, 2]
        return x * (f(1) / np.sqrt(s))[:, None]

    p = (p0 * hu + (p0 - e1) * hv) + (p0 + e2) * w
    o = p + normalize(n) * f(-0.00001)
    out = np.empty((len(idx), 8), f)
    out[:, 0:3] = o
    out[:, 3:6] = normalize(np.asarray(sun, f)[None, :] - o)
    out[:, 6] = 0
    out[:, 7] = FLT_MAX
    return out, idx


def _dot3(a, b):
    s = a[:, 0] * b[:, 0]
    s = s + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def camera_rays64(basis12, W, H, arith=ARITH_EXACT):
    """camera_rays for render<double>: the [W*H, 8] ray64 records of a view's primary rays
    (render.hpp:105-113), in contraction-free float64 -- bit for bit the rays the exact ceres_render_f64
    kernel traces; window [0, DBL_MAX].  arith = ARITH_FMA: ceres_camera_rays_f64 in the reference CMake
    build's arithmetic (the rays the MODE_FMA double kernel traces)."""
    f = np.float64
    if arith != ARITH_EXACT:
        return camera_rays64_native(basis12, W, H, arith)
    b = np.asarray(basis12, f).reshape(12)
    eye, dir_, iu, iv = b[0:3], b[3:6], b[6:9], b[9:12]
    u = f(2) * (np.arange(W, dtype=f) + f(0.5)) / f(W) - f(1)
    v = f(2) * (np.arange(H, dtype=f) + f(0.5)) / f(H) - f(1)
    uu = np.tile(u, H)[:, None]
    vv = np.repeat(v, W)[:, None]
    a = (iu[None, :] * uu + iv[None, :] * vv) + dir_[None, :]
    inv = f(1) / np.sqrt(_dot3(a, a))
    rays = np.empty((W * H, 8), f)
    rays[:, 0:3] = eye
    rays[:, 3:6] = a * inv[:, None]
    rays[:, 6] = 0
    rays[:, 7] = DBL_MAX
    return rays


def camera_rays64_native(basis12, W, H, arith=ARITH_EXACT):
    """ceres_camera_rays_f64: camera_rays64 by the library's own ray generator, in either arithmetic."""
    b = np.ascontiguousarray(basis12, np.float64).reshape(12)
    rays = np.empty((int(W) * int(H), 8), np.float64)
    _check(lib().ceres_camera_rays_f64(_p(b, ctypes.c_double), int(W), int(H), int(arith), rays.ctypes.data_as(_vp)))
    return rays


def shadow_rays64(mesh, hits, sun):
    """shadow_rays for render<double> (render.hpp:127-136) in contraction-free float64: a double mesh,
    hits as HIT64_DTYPE (or any record array with prim, u, v); returns (ray64 records [k, 8], the
    indices of the k hits)."""
    f = np.float64
    idx = np.nonzero(hits["prim"] >= 0)[0]
    tr = np.asarray(mesh.tri, f)[hits["prim"][idx]]
    p0, e1, e2, n = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9], tr[:, 9:12]
    hu, hv = np.asarray(hits["u"][idx], f)[:, None], np.asarray(hits["v"][idx], f)[:, None]
    w = f(1) - hu - hv

    def normalize(x):
        return x * (f(1) / np.sqrt(_dot3(x, x)))[:, None]

    p = (p0 * hu + (p0 - e1) * hv) + (p0 + e2) * w
    o = p + f(-0.00001) * normalize(n)
    out = np.empty((len(idx), 8), f)
    out[:, 0:3] = o
    out[:, 3:6] = normalize(np.asarray(sun, f)[None, :] - o)
    out[:, 6] = 0
    out[:, 7] = DBL_MAX
    return out, idx


class CpuScene:
    """The CPU path's scene (ceres_cpu_scene_create): render<float>() on host cores, chosen
    explicitly (./render --cpu); the GPU classes never fall back to it."""

    def __init__(self, mesh, bvh):
        L = lib()
        self.f64 = mesh.f64
        if self.f64:
            self._h = L.ceres_cpu_scene_create_f64(_p(mesh.tri, ctypes.c_double), len(mesh), _p(mesh.norm, ctypes.c_double),
                                                   bvh.nodes.ctypes.data_as(_vp), bvh.nodes.shape[0],
                                                   _p(bvh.prim, ctypes.c_uint64))
        else:
            self._h = L.ceres_cpu_scene_create(_p(mesh.tri, ctypes.c_float), len(mesh), _p(mesh.norm, ctypes.c_float),
                                               bvh.nodes.ctypes.data_as(_vp), bvh.nodes.shape[0],
                                               _p(bvh.prim, ctypes.c_uint64))
        if not self._h:
            raise CeresError("ceres_cpu_scene_create: " + L.ceres_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().ceres_cpu_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def refit(self, mesh):
        """ceres_cpu_scene_refit(_f64): the same scene after its triangles moved -- mesh.tri / mesh.norm in
        ORIGINAL order, same count and scalar type; topology kept, every box recomputed (min / max only)."""
        if mesh.f64 != self.f64:
            raise CeresError("refit: a %s mesh for a %s scene" % (("float", "double")[mesh.f64], ("float", "double")[self.f64]))
        fn, ct = (lib().ceres_cpu_scene_refit_f64, ctypes.c_double) if self.f64 else (lib().ceres_cpu_scene_refit, ctypes.c_float)
        _check(fn(self._h, _p(mesh.tri, ct), len(mesh), _p(mesh.norm, ct)))

    def sah_cost(self):
        """ceres_cpu_scene_sah_cost: the SAH cost of the scene's tree (compute_cost, traversal_cost = 1)."""
        c = ctypes.c_double()
        _check(lib().ceres_cpu_scene_sah_cost(self._h, ctypes.byref(c)))
        return c.value

    def rebuild(self, mesh, arith=ARITH_EXACT):
        """ceres_cpu_scene_rebuild(_f64): a new BVH for the moved triangles behind the same handle -- the scene
        CpuScene(mesh, build_bvh(mesh, arith)) would be; mesh.norm None keeps the normals."""
        if mesh.f64 != self.f64:
            raise CeresError("rebuild: a %s mesh for a %s scene" % (("float", "double")[mesh.f64], ("float", "double")[self.f64]))
        fn, ct = (lib().ceres_cpu_scene_rebuild_f64, ctypes.c_double) if self.f64 else (lib().ceres_cpu_scene_rebuild, ctypes.c_float)
        _check(fn(self._h, _p(mesh.tri, ct), len(mesh), _p(mesh.norm, ct), int(arith)))

    def update(self, mesh, max_ratio, arith=ARITH_EXACT):
        """ceres_cpu_scene_update(_f64): refit, measure, rebuild iff cost > max_ratio * built_cost; returns the
        ceres_update_info fields {cost, built_cost, new_cost, rebuilt}."""
        if mesh.f64 != self.f64:
            raise CeresError("update: a %s mesh for a %s scene" % (("float", "double")[mesh.f64], ("float", "double")[self.f64]))
        fn, ct = (lib().ceres_cpu_scene_update_f64, ctypes.c_double) if self.f64 else (lib().ceres_cpu_scene_update, ctypes.c_float)
        u = _UpdateInfo()
        _check(fn(self._h, _p(mesh.tri, ct), len(mesh), _p(mesh.norm, ct), int(arith), float(max_ratio), ctypes.byref(u)))
        return u.as_dict()

    def render(self, basis12, sun, W, H, mode=MODE_FULL, threads=0, want_pixels=True, want_rgb8=True):
        """ceres_render_cpu_f32 / _f64: (pixels [H*W*3] f32|f64 | None, rgb8 | None, stats dict)."""
        dt, ct = (np.float64, ctypes.c_double) if self.f64 else (np.float32, ctypes.c_float)
        b = np.ascontiguousarray(basis12, dt)
        s = np.ascontiguousarray(sun, dt)
        px = np.empty(3 * W * H, dt) if want_pixels else None
        rgb = np.empty(3 * W * H, np.uint8) if want_rgb8 else None
        st = _Stats()
        fn = lib().ceres_render_cpu_f64 if self.f64 else lib().ceres_render_cpu_f32
        _check(fn(self._h, _p(b, ct), _p(s, ct), int(mode), _p(px, ct), _p(rgb, ctypes.c_uint8), W, H, ctypes.byref(st),
                  int(threads)))
        return px, rgb, dict(rays=st.rays, hits=st.hits, primary_rays=st.primary_rays, shadow_rays=st.shadow_rays,
                             node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)

    def trace(self, rays, mode=0, closest=True, occluded=False, threads=0):
        """ceres_trace_rays_cpu: rays [n, 8] float32 -> (hits [n] HIT_DTYPE | None, occluded [n] u8 | None, stats);
        a double scene: ceres_trace_rays_cpu_f64, rays [n, 8] float64 -> hits [n] HIT64_DTYPE."""
        fn = lib().ceres_trace_rays_cpu_f64 if self.f64 else lib().ceres_trace_rays_cpu
        return _trace_host(lambda r, n, m, h, o, st: fn(self._h, r, n, m, h, o, st, int(threads)),
                           rays, mode, closest, occluded, self.f64)

    def closest_points(self, points, threads=0):
        """ceres_closest_points_cpu: Scene.closest_points on host cores -- the same bytes.  Float scenes."""
        return _closest_host(lambda p, n, o, st: lib().ceres_closest_points_cpu(self._h, p, n, o, st, int(threads)), points)

    def closest_points_f64(self, points, threads=0):
        """ceres_closest_points_cpu_f64: Scene.closest_points_f64 on host cores -- the same bytes.  Double scenes."""
        return _closest_host(lambda p, n, o, st: lib().ceres_closest_points_cpu_f64(self._h, p, n, o, st, int(threads)), points, f64=True)

    def ray_order(self, rays):
        """ceres_ray_order_cpu(_f64): the coherent order of rays [n, 8] (float32; a double scene: float64) ->
        order [n] uint32, the permutation Scene.ray_order_device writes."""
        dt = np.float64 if self.f64 else np.float32
        r = np.ascontiguousarray(rays, dt).reshape(-1, 8)
        order = np.empty(len(r), np.uint32)
        fn = lib().ceres_ray_order_cpu_f64 if self.f64 else lib().ceres_ray_order_cpu
        _check(fn(self._h, r.ctypes.data_as(_vp), len(r), order.ctypes.data_as(_vp)))
        return order

    def order_box(self):
        """ceres_cpu_scene_order_box: (lo [3], hi [3], usable) -- the box the order's key is computed in."""
        b = np.zeros(6, np.float64)
        ok = ctypes.c_int()
        _check(lib().ceres_cpu_scene_order_box(self._h, _p(b, ctypes.c_double), ctypes.byref(ok)))
        return b[:3].copy(), b[3:].copy(), bool(ok.value)

    def trace_lists(self, rays, mode=0, threads=0):
        """ceres_trace_rays_lists_cpu / ceres_trace_rays_lists_cpu_f64 (double scenes): Scene.trace_lists on
        host cores."""
        fn = lib().ceres_trace_rays_lists_cpu_f64 if self.f64 else lib().ceres_trace_rays_lists_cpu
        return _trace_lists_host(lambda r, n, m, o, h, cap, tot, st: fn(self._h, r, n, m, o, h, cap, tot, st, int(threads)),
                                 rays, mode, self.f64)

    def trace_all(self, rays, max_hits=8, mode=0, hits=True, threads=0):
        """ceres_trace_rays_all_cpu / ceres_trace_rays_all_cpu_f64 (double scenes): Scene.trace_all on host
        cores."""
        fn = lib().ceres_trace_rays_all_cpu_f64 if self.f64 else lib().ceres_trace_rays_all_cpu
        return _trace_all_host(lambda r, n, m, k, c, h, st: fn(self._h, r, n, m, k, c, h, st, int(threads)),
                               rays, max_hits, mode, hits, self.f64)

    def shade(self, rays, sun, mode=0, pixels=True, rgb8=False, hits=False, status=False, threads=0):
        """ceres_shade_rays_cpu / ceres_shade_rays_cpu_f64 (double scenes): Scene.shade on host cores."""
        fn = lib().ceres_shade_rays_cpu_f64 if self.f64 else lib().ceres_shade_rays_cpu
        return _shade_host(lambda r, n, s, m, px, q, h, stt, st: fn(self._h, r, n, s, m, px, q, h, stt, st, int(threads)),
                           rays, sun, mode, pixels, rgb8, hits, status, self.f64)


class Scene:
    """A scene resident in HBM of one device (ceres_scene_create)."""

    def __init__(self, mesh, bvh, device=0, stats=False, first_order=False, _handle=None):
        L = lib()
        if _handle is not None:                      # Scene.from_device
            self._h, self.device, self.n_tri = _handle[:3]
            self.f64 = len(_handle) > 3 and bool(_handle[3])
            return
        self.f64 = mesh.f64
        flags = (SCENE_STATS if stats else 0) | (SCENE_FIRST_ORDER if first_order else 0)
        if self.f64:
            self._h = L.ceres_scene_create_f64(_p(mesh.tri, ctypes.c_double), len(mesh), _p(mesh.norm, ctypes.c_double),
                                               bvh.nodes.ctypes.data_as(_vp), bvh.nodes.shape[0],
                                               _p(bvh.prim, ctypes.c_uint64), int(device), flags)
        else:
            self._h = L.ceres_scene_create(_p(mesh.tri, ctypes.c_float), len(mesh), _p(mesh.norm, ctypes.c_float),
                                           bvh.nodes.ctypes.data_as(_vp), bvh.nodes.shape[0],
                                           _p(bvh.prim, ctypes.c_uint64), int(device), flags)
        if not self._h:
            raise CeresError("ceres_scene_create: " + L.ceres_last_error().decode())
        self.device = device
        self.n_tri = len(mesh)

    @classmethod
    def from_device(cls, d_tri48, n_tri, d_norm36, d_nodes32, n_nodes, d_prim32, device=0, stats=False, stream=0):
        """ceres_scene_create_device: a scene from arrays already in HBM (int device pointers)."""
        L = lib()
        h = L.ceres_scene_create_device(d_tri48, n_tri, d_norm36, d_nodes32, n_nodes, d_prim32, int(device),
                                        SCENE_STATS if stats else 0, stream or None)
        if not h:
            raise CeresError("ceres_scene_create_device: " + L.ceres_last_error().decode())
        return cls(None, None, _handle=(h, device, n_tri))

    @classmethod
    def from_device_f64(cls, d_tri96, n_tri, d_norm72, d_nodes64, n_nodes, d_prim32, device=0, stats=False, stream=0):
        """ceres_scene_create_f64_device: a double scene from arrays already in HBM (int device pointers):
        Triangle<double> records, 72-B normals, 64-B nodes and u32 primitive_indices, e.g. from
        build_bvh_device_f64.  To every call it is the scene Scene(mesh, bvh) makes from the same arrays."""
        L = lib()
        h = L.ceres_scene_create_f64_device(d_tri96 or None, n_tri, d_norm72 or None, d_nodes64 or None, n_nodes,
                                            d_prim32 or None, int(device), SCENE_STATS if stats else 0, stream or None)
        if not h:
            raise CeresError("ceres_scene_create_f64_device: " + L.ceres_last_error().decode())
        return cls(None, None, _handle=(h, device, n_tri, True))

    def info(self):
        d, s, n, b = ctypes.c_uint32(), ctypes.c_uint32(), _sz(), _sz()
        _check(lib().ceres_scene_info(self._h, ctypes.byref(d), ctypes.byref(s), ctypes.byref(n), ctypes.byref(b)))
        near, first = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().ceres_scene_shadow_stacks(self._h, ctypes.byref(near), ctypes.byref(first)))
        return dict(depth=d.value, stack_entries=s.value, n_pairs=n.value, device_bytes=b.value,
                    shadow_stack_nearest=near.value, shadow_stack_first=first.value)

    def stack_width(self):
        """ceres_scene_stack_width: bytes per LDS traversal-stack entry of the scene's kernels -- 2, 3 or 4,
        by its record count, or wider when CERES_DEBUG_STACK_WIDTH=3|4 was set as it was created."""
        w = lib().ceres_scene_stack_width(self._h)
        if w < 0:
            _check(w)
        return int(w)

    def refit(self, mesh):
        """ceres_scene_refit(_f64): the same scene after its triangles moved, from host arrays -- mesh.tri /
        mesh.norm in ORIGINAL order, same count and scalar type as at creation.  Topology, leaf assignment and
        record numbering are kept; every pair box, BVH4 child box and the root box are recomputed exactly."""
        if mesh.f64 != self.f64:
            raise CeresError("refit: a %s mesh for a %s scene" % (("float", "double")[mesh.f64], ("float", "double")[self.f64]))
        fn, ct = (lib().ceres_scene_refit_f64, ctypes.c_double) if self.f64 else (lib().ceres_scene_refit, ctypes.c_float)
        _check(fn(self._h, _p(mesh.tri, ct), len(mesh), _p(mesh.norm, ct)))

    def refit_device(self, d_tri, d_norm=0, stream=0, n_tri=None):
        """ceres_scene_refit_device / _f64_device: device pointers (ints) to the moved triangles (16-byte
        aligned) and optionally normals (0: kept), enqueued on `stream` (0: the default stream), which is
        synchronised once at the end."""
        fn = lib().ceres_scene_refit_f64_device if self.f64 else lib().ceres_scene_refit_device
        _check(fn(self._h, d_tri or None, int(self.n_tri if n_tri is None else n_tri), d_norm or None, stream or None))

    def sah_cost(self, stream=0):
        """ceres_scene_sah_cost: the SAH cost of the scene's tree (compute_cost, traversal_cost = 1), float and
        double scenes; enqueued on `stream` (0: the default stream), which is synchronised once."""
        c = ctypes.c_double()
        _check(lib().ceres_scene_sah_cost(self._h, ctypes.byref(c), stream or None))
        return c.value

    def _float_mesh(self, what, mesh):
        if mesh.f64:                                  # a double GPU scene: the library's refusal (CERES_EUNSUPPORTED)
            if self.f64:
                return _p(mesh.tri, ctypes.c_double), _p(mesh.norm, ctypes.c_double)
            raise CeresError("%s: a double mesh for a float scene" % what)
        return _p(mesh.tri, ctypes.c_float), _p(mesh.norm, ctypes.c_float)

    def rebuild(self, mesh, arith=ARITH_EXACT):
        """ceres_scene_rebuild: a new GPU-built BVH for the moved triangles (host arrays, ORIGINAL order, same
        count) behind the same handle -- afterwards the scene Scene.from_device would make from them; a
        double scene: CERES_EUNSUPPORTED.  mesh.norm None keeps the normals."""
        t, n = self._float_mesh("rebuild", mesh)
        _check(lib().ceres_scene_rebuild(self._h, ctypes.cast(t, _fp), len(mesh), ctypes.cast(n, _fp), int(arith)))

    def rebuild_device(self, d_tri, d_norm=0, stream=0, n_tri=None, arith=ARITH_EXACT):
        """ceres_scene_rebuild_device: device pointers (ints) to the moved triangles (16-byte aligned) and
        optionally normals (0: kept); enqueued on `stream`, synchronised at the end."""
        _check(lib().ceres_scene_rebuild_device(self._h, d_tri or None, int(self.n_tri if n_tri is None else n_tri),
                                                d_norm or None, int(arith), stream or None))

    def update(self, mesh, max_ratio, arith=ARITH_EXACT):
        """ceres_scene_update: refit, measure, rebuild iff cost > max_ratio * built_cost (host arrays); returns
        the ceres_update_info fields {cost, built_cost, new_cost, rebuilt}."""
        t, n = self._float_mesh("update", mesh)
        u = _UpdateInfo()
        _check(lib().ceres_scene_update(self._h, ctypes.cast(t, _fp), len(mesh), ctypes.cast(n, _fp), int(arith),
                                        float(max_ratio), ctypes.byref(u)))
        return u.as_dict()

    def update_device(self, d_tri, max_ratio, d_norm=0, stream=0, n_tri=None, arith=ARITH_EXACT):
        """ceres_scene_update_device: the same from device pointers (see rebuild_device)."""
        u = _UpdateInfo()
        _check(lib().ceres_scene_update_device(self._h, d_tri or None, int(self.n_tri if n_tri is None else n_tri),
                                               d_norm or None, int(arith), float(max_ratio), ctypes.byref(u), stream or None))
        return u.as_dict()

    def read_boxes(self):
        """ceres_scene_read_boxes (diagnostic): (pairs [n, 12] f32|f64 = lb[6], rb[6] per sibling pair,
        nodes4 [m, 24] f32 in Node4 row order (lo_x[4], hi_x[4], lo_y[4], hi_y[4], lo_z[4], hi_z[4]) or None
        when the scene has no BVH4: a double scene, or a root leaf (then n = 0 too)."""
        n, m = _sz(), _sz()
        _check(lib().ceres_scene_read_boxes(self._h, None, ctypes.byref(n), None, ctypes.byref(m)))
        pairs = np.zeros((n.value, 12), np.float64 if self.f64 else np.float32)
        nodes4 = np.zeros((m.value, 24), np.float32) if m.value else None
        _check(lib().ceres_scene_read_boxes(self._h, pairs.ctypes.data_as(_vp), ctypes.byref(n),
                                            _p(nodes4, ctypes.c_float), ctypes.byref(m)))
        return pairs, nodes4

    def close(self):
        if getattr(self, "_h", None):
            lib().ceres_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, basis12, sun, W, H, mode=MODE_FULL, want_pixels=True, want_rgb8=True):
        """ceres_render_f32 / ceres_render_f64 (double scenes): host buffers out; returns
        (pixels [H*W*3] f32|f64 | None, rgb8 | None, stats dict)."""
        dt, ct = (np.float64, ctypes.c_double) if self.f64 else (np.float32, ctypes.c_float)
        b = np.ascontiguousarray(basis12, dt)
        s = np.ascontiguousarray(sun, dt)
        px = np.empty(3 * W * H, dt) if want_pixels else None
        rgb = np.empty(3 * W * H, np.uint8) if want_rgb8 else None
        st = _Stats()
        fn = lib().ceres_render_f64 if self.f64 else lib().ceres_render_f32
        _check(fn(self._h, _p(b, ct), _p(s, ct), int(mode), _p(px, ct), _p(rgb, ctypes.c_uint8), W, H, ctypes.byref(st)))
        return px, rgb, dict(rays=st.rays, hits=st.hits, primary_rays=st.primary_rays, shadow_rays=st.shadow_rays,
                             node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)

    def records(self, basis12, sun, W, H, mode=MODE_FULL):
        """ceres_render_records(_f64): per-pixel (prim [W*H] i32, tuv [W*H,3] f32|f64, shadow [W*H] i8, stats)."""
        dt, ct = (np.float64, ctypes.c_double) if self.f64 else (np.float32, ctypes.c_float)
        b = np.ascontiguousarray(basis12, dt)
        s = np.ascontiguousarray(sun, dt)
        prim = np.empty(W * H, np.int32)
        tuv = np.empty(3 * W * H, dt)
        sh = np.empty(W * H, np.int8)
        st = _Stats()
        fn = lib().ceres_render_records_f64 if self.f64 else lib().ceres_render_records
        _check(fn(self._h, _p(b, ct), _p(s, ct), int(mode), W, H, _p(prim, ctypes.c_int32), _p(tuv, ct),
                  _p(sh, ctypes.c_int8), ctypes.byref(st)))
        return prim, tuv.reshape(-1, 3), sh, dict(rays=st.rays, hits=st.hits, node_pairs=st.node_pairs,
                                                  tri_tests=st.tri_tests)

    def render_device(self, basis12, sun, W, H, mode=MODE_FULL, tiling=None, d_pixels=0, d_rgb8=0, d_counters=0,
                      stream=0):
        """ceres_render_device: device pointers (ints, e.g. torch data_ptr()), async on `stream`."""
        b = np.ascontiguousarray(basis12, np.float32)
        s = np.ascontiguousarray(sun, np.float32)
        t = ctypes.byref(tiling) if tiling is not None else None
        _check(lib().ceres_render_device(self._h, _p(b, ctypes.c_float), _p(s, ctypes.c_float), int(mode), W, H, t,
                                         d_pixels or None, d_rgb8 or None, d_counters or None, stream or None))

    def render_batch_device(self, basis12, sun3, W, H, mode=MODE_FULL, tiling=None, d_pixels=0, d_rgb8=0,
                            d_counters=0, stream=0):
        """ceres_render_batch_device: F frames (basis12 [F,12], sun3 [F,3]) in one launch pair.
        Frame f's rows are at offset f*3*W*local_rows of d_pixels / d_rgb8."""
        b = np.ascontiguousarray(basis12, np.float32).reshape(-1, 12)
        s = np.ascontiguousarray(sun3, np.float32).reshape(-1, 3)
        if b.shape[0] != s.shape[0]:
            raise CeresError("render_batch_device: %d cameras but %d suns" % (b.shape[0], s.shape[0]))
        t = ctypes.byref(tiling) if tiling is not None else None
        _check(lib().ceres_render_batch_device(self._h, b.shape[0], _p(b, ctypes.c_float), _p(s, ctypes.c_float),
                                               int(mode), W, H, t, d_pixels or None, d_rgb8 or None,
                                               d_counters or None, stream or None))

    def trace(self, rays, mode=0, closest=True, occluded=False, coherent=False):
        """ceres_trace_rays: closest hit and / or occlusion of caller-supplied rays ([n, 8] float32:
        origin, direction (any length), tmin, tmax) -> (hits [n] HIT_DTYPE {prim, t, u, v} | None,
        occluded [n] u8 | None, stats dict); mode: 0, MODE_FMA, MODE_ROBUST or both.  A double scene:
        ceres_trace_rays_f64, rays [n, 8] float64 -> hits [n] HIT64_DTYPE {prim, pad, t, u, v}; mode 0 or MODE_FMA.
        coherent=True: ceres_trace_rays_coherent(_f64) -- the rays are traced in the coherent order
        (ray_order_device); the same bytes come back, stats["ms"] covers order plus trace."""
        if coherent:
            fn = lib().ceres_trace_rays_coherent_f64 if self.f64 else lib().ceres_trace_rays_coherent
        else:
            fn = lib().ceres_trace_rays_f64 if self.f64 else lib().ceres_trace_rays
        return _trace_host(lambda r, n, m, h, o, st: fn(self._h, r, n, m, h, o, st), rays, mode, closest, occluded, self.f64)

    def closest_points(self, points):
        """ceres_closest_points: for each point ([n, 4] float32 {x, y, z, r2max}; [n, 3]: r2max = +inf) the
        nearest point of the surface -> (near [n] NEAR_DTYPE {prim, d2, u, v}, stats dict).  prim: the original
        triangle index, -1 (with zeros) when nothing lies within r2max; d2: the squared distance; u, v: the
        weights of p1() and p2().  The answer is the minimum over all triangles of one float formula
        (ceres_render.h), equal distances to the smallest index -- whatever the tree.  Float scenes."""
        return _closest_host(lambda p, n, o, st: lib().ceres_closest_points(self._h, p, n, o, st), points)

    def closest_points_device(self, d_points16, n_points, d_near16, d_counters=0, stream=0, d_index=0, n_index=None):
        """ceres_closest_points_device: device pointers (ints, 16-byte aligned), enqueued on `stream`, not
        synchronised.  d_index / n_index: the indexed call (see _indexed)."""
        fn = lib().ceres_closest_points_device
        ix = ()
        if d_index or n_index is not None:
            fn, ix = lib().ceres_closest_points_indexed_device, (d_index or None, int(n_index or 0))
        _check(fn(self._h, d_points16 or None, int(n_points), *ix, d_near16 or None, d_counters or None, stream or None))

    def closest_points_f64(self, points):
        """ceres_closest_points_f64: closest_points on a double scene -- points [n, 4] float64 {x, y, z, r2max}
        ([n, 3]: r2max = +inf) -> (near [n] NEAR64_DTYPE {prim, pad, d2, u, v}, stats dict).  The same formula,
        selection and pruning rule in double (ceres_render.h): the minimum over all triangles, whatever the tree."""
        return _closest_host(lambda p, n, o, st: lib().ceres_closest_points_f64(self._h, p, n, o, st), points, f64=True)

    def closest_points_f64_device(self, d_points32, n_points, d_near32, d_counters=0, stream=0, d_index=0, n_index=None):
        """ceres_closest_points_f64_device: device pointers (ints, 16-byte aligned), enqueued on `stream`, not
        synchronised.  d_index / n_index: the indexed call (see _indexed)."""
        fn = lib().ceres_closest_points_f64_device
        ix = ()
        if d_index or n_index is not None:
            fn, ix = lib().ceres_closest_points_f64_indexed_device, (d_index or None, int(n_index or 0))
        _check(fn(self._h, d_points32 or None, int(n_points), *ix, d_near32 or None, d_counters or None, stream or None))

    def _indexed(self, name, d_index, n_index):
        """(C function, its leading arguments after n_rays) of a device query: the plain call, or with
        d_index (a device pointer to n_index u32 ray indices) the indexed one -- lane i takes ray
        d_index[i] and writes that ray's own output slots; entries >= n_rays are skipped."""
        fn = getattr(lib(), name % ("_f64" if self.f64 else ""))
        if not d_index and n_index is None:
            return fn, ()
        fn = getattr(lib(), (name % ("_f64" if self.f64 else "")).replace("_device", "_indexed_device"))
        return fn, (d_index or None, int(n_index or 0))

    def ray_order_device(self, d_rays, n_rays, d_order, d_scratch, scratch_bytes, stream=0):
        """ceres_ray_order_device(_f64_device): d_order [n_rays] u32 = the coherent order of the rays, a
        permutation to pass as d_index (device pointers as ints; d_scratch: ray_order_scratch_bytes(n_rays)
        of the caller's); enqueued on `stream`, not synchronised."""
        fn = lib().ceres_ray_order_f64_device if self.f64 else lib().ceres_ray_order_device
        _check(fn(self._h, d_rays or None, int(n_rays), d_order or None, d_scratch or None, int(scratch_bytes), stream or None))

    def trace_device(self, d_rays32, n_rays, mode=0, d_hits16=0, d_occluded=0, d_counters=0, stream=0, d_index=0,
                     n_index=None):
        """ceres_trace_rays_device: device pointers (ints), enqueued on `stream`, not synchronised.  A double
        scene: ceres_trace_rays_f64_device (d_rays32: ray64 records, d_hits16: hit32 records).  d_index /
        n_index: the indexed call (see _indexed)."""
        fn, ix = self._indexed("ceres_trace_rays%s_device", d_index, n_index)
        _check(fn(self._h, d_rays32 or None, int(n_rays), *ix, int(mode), d_hits16 or None, d_occluded or None,
                  d_counters or None, stream or None))

    def trace_all(self, rays, max_hits=8, mode=0, hits=True):
        """ceres_trace_rays_all: every hit in each ray's window ([n, 8] float32 ray32 records) -> (counts [n] u32,
        the size of each ray's hit set, hits [n, max_hits] HIT_DTYPE | None, stats dict).  A row holds the
        min(count, max_hits) smallest hits by t, equal t by original triangle index, then misses {-1, 0, 0, 0};
        max_hits 1 .. MAX_HITS; hits=False: the count-only query.  mode: 0, MODE_FMA, MODE_ROBUST or both.
        stats["hits"]: rays with at least one hit.  A double scene: ceres_trace_rays_all_f64, rays [n, 8]
        float64 -> hits [n, max_hits] HIT64_DTYPE (misses {-1, 0, 0.0, 0.0, 0.0}), t by double <; mode 0 or
        MODE_FMA."""
        fn = lib().ceres_trace_rays_all_f64 if self.f64 else lib().ceres_trace_rays_all
        return _trace_all_host(lambda r, n, m, k, c, h, st: fn(self._h, r, n, m, k, c, h, st), rays, max_hits, mode, hits,
                               self.f64)

    def trace_lists(self, rays, mode=0):
        """ceres_trace_rays_lists: every hit of every ray ([n, 8] float32 ray32 records), without a cap, as a
        CSR pair -> (offsets [n + 1] u64, hits [offsets[n]] HIT_DTYPE, stats dict): ray r owns
        hits[offsets[r]:offsets[r + 1]], its whole set in trace_all's order; no miss records.  The buffer is
        allocated here (the count pass runs twice: once to size it, once inside the filling call).  A double
        scene: ceres_trace_rays_lists_f64, rays [n, 8] float64 -> hits HIT64_DTYPE; mode 0 or MODE_FMA."""
        fn = lib().ceres_trace_rays_lists_f64 if self.f64 else lib().ceres_trace_rays_lists
        return _trace_lists_host(lambda r, n, m, o, h, cap, tot, st: fn(self._h, r, n, m, o, h, cap, tot, st), rays, mode,
                                 self.f64)

    def hit_offsets_device(self, d_counts, n_rays, d_offsets, d_scratch, scratch_bytes, stream=0):
        """ceres_hit_offsets_device: d_offsets [n_rays + 1] u64 = exclusive prefix sums of d_counts [n_rays] u32
        (device pointers as ints; d_scratch: hit_offsets_scratch_bytes(n_rays) of the caller's); enqueued."""
        _check(lib().ceres_hit_offsets_device(self._h, d_counts or None, int(n_rays), d_offsets or None, d_scratch or None,
                                              int(scratch_bytes), stream or None))

    def trace_lists_device(self, d_rays32, n_rays, d_offsets, d_hits16, capacity, mode=0, d_counters=0, stream=0,
                           d_index=0, n_index=None):
        """ceres_trace_rays_lists_device: fills the segments d_offsets describes (device pointers as ints),
        enqueued on `stream`, not synchronised; d_counters: 8 u64 {rays, rays with a non-empty segment, rays,
        records written, node_pairs, tri_tests, stack-overflow flag, segment-mismatch flag}.  A double scene:
        ceres_trace_rays_lists_f64_device (d_rays32: ray64 records, d_hits16: hit32 records).  d_index /
        n_index: the indexed call (distinct entries; unlisted rays' segments are unspecified afterwards)."""
        fn, ix = self._indexed("ceres_trace_rays_lists%s_device", d_index, n_index)
        _check(fn(self._h, d_rays32 or None, int(n_rays), *ix, int(mode), d_offsets or None,
                  d_hits16 or None, int(capacity), d_counters or None, stream or None))

    def trace_all_device(self, d_rays32, n_rays, max_hits=8, mode=0, d_counts=0, d_hits16=0, d_counters=0, stream=0,
                         d_index=0, n_index=None):
        """ceres_trace_rays_all_device: device pointers (ints), enqueued on `stream`, not synchronised;
        d_hits16: n_rays x max_hits hit16 records, ray-major, or 0 for the count-only query.  A double scene:
        ceres_trace_rays_all_f64_device (d_rays32: ray64 records, d_hits16: hit32 records).  d_index /
        n_index: the indexed call."""
        fn, ix = self._indexed("ceres_trace_rays_all%s_device", d_index, n_index)
        _check(fn(self._h, d_rays32 or None, int(n_rays), *ix, int(mode), int(max_hits),
                  d_counts or None, d_hits16 or None, d_counters or None, stream or None))

    def shade(self, rays, sun, mode=0, pixels=True, rgb8=False, hits=False, status=False):
        """ceres_shade_rays: render()'s pixel for caller-supplied rays ([n, 8] float32 ray32 records) and one
        sun position -> (pixels [n, 3] f32 | None, rgb8 [n, 3] u8 | None, hits [n] HIT_DTYPE | None,
        status [n] u8 (0 miss, 1 lit, 2 in shadow) | None, stats dict); mode: 0, MODE_FMA, MODE_ROBUST or
        both.  The direction is used as given (shading's `view`): unit directions for a meaningful
        specular term.  A double scene: ceres_shade_rays_f64, rays [n, 8] float64 and a float64 sun ->
        pixels [n, 3] f64 (the float colour widened, as Scene.render's), hits [n] HIT64_DTYPE; mode 0 or
        MODE_FMA."""
        fn = lib().ceres_shade_rays_f64 if self.f64 else lib().ceres_shade_rays
        return _shade_host(lambda r, n, s, m, px, q, h, stt, st: fn(self._h, r, n, s, m, px, q, h, stt, st),
                           rays, sun, mode, pixels, rgb8, hits, status, self.f64)

    def shade_device(self, d_rays32, n_rays, sun, mode=0, d_pixels=0, d_rgb8=0, d_hits16=0, d_status=0, d_counters=0,
                     stream=0, d_index=0, n_index=None):
        """ceres_shade_rays_device: device pointers (ints; `sun` stays a host triple), enqueued on
        `stream`, not synchronised.  A double scene: ceres_shade_rays_f64_device (d_rays32: ray64 records,
        d_pixels: 3 doubles per ray, d_hits16: hit32 records).  d_index / n_index: the indexed call."""
        dt, ct = (np.float64, ctypes.c_double) if self.f64 else (np.float32, ctypes.c_float)
        fn, ix = self._indexed("ceres_shade_rays%s_device", d_index, n_index)
        s = np.ascontiguousarray(sun, dt).reshape(3)
        _check(fn(self._h, d_rays32 or None, int(n_rays), *ix, _p(s, ct), int(mode), d_pixels or None, d_rgb8 or None,
                  d_hits16 or None, d_status or None, d_counters or None, stream or None))

    def set_timing(self, on):
        _check(lib().ceres_scene_set_timing(self._h, 1 if on else 0))

    def wave_log(self, max_waves=1 << 16):
        """Diagnostic per-wavefront records of the last full-mode render (stats scenes), one row per
        8x8 tile: start / after primary / end (100-MHz ticks), longest primary chain, shadow-loop
        trips, primary hits, primary and shadow node pairs of the wavefront."""
        out = np.zeros(8 * max_waves, np.uint64)
        n = _sz()
        _check(lib().ceres_scene_wave_log(self._h, _p(out, ctypes.c_uint64), max_waves, ctypes.byref(n)))
        return out[: 8 * n.value].reshape(-1, 8)

    def compact_order(self):
        """ceres_debug_compact_order: None when the latest batch launch took the plain grid, else a dict:
        host_tiles / device_tiles (kept tiles as the host sized the grid and as the device counted),
        groups, tpw, deal (XCD chunk in groups, 0: none), order (the compacted order, zero-padded to a
        multiple of 8) and source (the order it was gathered from).  Synchronises the launch's stream."""
        info = np.zeros(8, np.uint32)
        _check(lib().ceres_debug_compact_order(self._h, _p(info, ctypes.c_uint32), None, None, 0))
        if not info[0]:
            return None
        cap = int(info[6]) + 16
        order, source = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        _check(lib().ceres_debug_compact_order(self._h, _p(info, ctypes.c_uint32), _p(order, ctypes.c_uint32),
                                               _p(source, ctypes.c_uint32), cap))
        return {"host_tiles": int(info[1]), "device_tiles": int(info[2]), "groups": int(info[3]), "tpw": int(info[4]),
                "deal": int(info[5]), "order": order[:(int(info[2]) + 7) // 8 * 8], "source": source[:int(info[6])]}

    def entry_record(self, on=True):
        """ceres_debug_entry_record: later batch launches record the entry record of every order entry."""
        _check(lib().ceres_debug_entry_record(self._h, 1 if on else 0))

    def entry_nodes(self):
        """ceres_debug_entry_nodes: {"cut": CutTable | None (double scenes), "used": whether the latest
        batch launch started its walks at entry nodes, and then "rects" [frames, 64, 4] u16 and
        "entries" (per tile of the batch, [frame][tile row][tile column] flattened: the record its walk
        started at, ENTRY_EMPTY, or ENTRY_CULLED for a tile no wavefront looked up; empty unless
        entry_record was on), "W", "H"}.  Synchronises the device."""
        info = np.zeros(8, np.uint32)
        table = np.zeros(cut_words(), np.uint32)
        _check(lib().ceres_debug_entry_nodes(self._h, _p(info, ctypes.c_uint32), _p(table, ctypes.c_uint32), None, None, 0))
        out = {"cut": CutTable(table) if info[0] else None, "used": bool(info[1])}
        if info[1]:
            rects = np.zeros((int(info[2]), 64, 4), np.uint16)
            entries = np.zeros(max(int(info[3]), 1), np.uint32)
            _check(lib().ceres_debug_entry_nodes(self._h, _p(info, ctypes.c_uint32), None, _p(rects, ctypes.c_uint16), None,
                                                 rects.shape[0] * 64))
            _check(lib().ceres_debug_entry_nodes(self._h, _p(info, ctypes.c_uint32), None, None, _p(entries, ctypes.c_uint32),
                                                 len(entries)))
            out.update(rects=rects, entries=entries[:int(info[3])], W=int(info[4]), H=int(info[5]))
        return out

    def retire(self):
        """ceres_debug_retire: None when the latest batch launch retired no tile beyond the root cull,
        else {"live": bool [frames, tile rows, tile columns] (the tile is neither root-culled nor
        unreached by every cut rectangle), "flags": u8 per group slot of compact_order()'s order (1: no
        tile of the group is live), "W", "H"}.  Synchronises the launch's stream."""
        info = np.zeros(8, np.uint32)
        _check(lib().ceres_debug_retire(self._h, _p(info, ctypes.c_uint32), None, None, 0))
        if not info[0]:
            return None
        frames, rows, mw, W = int(info[1]), int(info[2]), int(info[3]), int(info[6])
        mask = np.zeros(max(int(info[4]), 1), np.uint32)
        flags = np.zeros(max(int(info[5]), 1), np.uint8)
        _check(lib().ceres_debug_retire(self._h, _p(info, ctypes.c_uint32), _p(mask, ctypes.c_uint32), None, len(mask)))
        _check(lib().ceres_debug_retire(self._h, _p(info, ctypes.c_uint32), None, _p(flags, ctypes.c_uint8), len(flags)))
        words = mask[:frames * rows * mw].reshape(frames, rows, mw)
        bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & 1
        live = bits.reshape(frames, rows, mw * 32)[:, :, :(W + 7) // 8].astype(bool)
        return {"live": live, "words": words, "flags": flags[:int(info[5])], "W": W, "H": int(info[7])}

    def read_timing(self):
        """(kernel ms summed over the renders since set_timing, 0.0, renders)."""
        p, q, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        _check(lib().ceres_scene_read_timing(self._h, ctypes.byref(p), ctypes.byref(q), ctypes.byref(n)))
        return p.value, q.value, n.value


# ---- entry nodes (csrc/entry_cut.hpp): host entry points, no device needed
ENTRY_EMPTY, ENTRY_CULLED = 0xffffffff, 0xfefefefe


def cut_words():
    return int(lib().ceres_entry_cut_words())


class CutTable:
    """A scene's cut table (include/ceres_render.h, ceres_entry_cut_words): n cut nodes in depth-first
    order -- src (pair << 1 | side holding the node's box), child (the pair record of its children,
    0xffffffff: a leaf), box [n, 6] -- lca / depth [64, 64] and entry_ok."""

    def __init__(self, words):
        self.words = np.ascontiguousarray(words, np.uint32)
        w = self.words
        self.n, self.entry_ok = int(w[0]), int(w[1])
        self.src, self.child = w[4:4 + self.n], w[68:68 + self.n]
        self.box = w[132:132 + 384].view(np.float32).reshape(64, 6)[:self.n]
        self.lca = w[516:516 + 4096].reshape(64, 64)
        self.depth = w[4868:4868 + 4096].reshape(64, 64)


def entry_relayout(mesh, bvh):
    """ceres_entry_relayout -> (pairs [n, 16] u32 = 64-byte sibling-pair records: lb, rb as float
    bits, lcount, lfirst, rcount, rfirst; orig [n_tri] u32; root_leaf_count)."""
    n, rlc = _sz(0), ctypes.c_uint32(0)
    args = (_p(mesh.tri, ctypes.c_float), len(mesh), bvh.nodes.ctypes.data_as(_vp), bvh.nodes.shape[0], _p(bvh.prim, ctypes.c_uint64))
    _check(lib().ceres_entry_relayout(*args, None, ctypes.byref(n), None, ctypes.byref(rlc)))
    pairs, orig = np.zeros((n.value, 16), np.uint32), np.zeros(len(mesh), np.uint32)
    _check(lib().ceres_entry_relayout(*args, pairs.ctypes.data_as(_vp), ctypes.byref(n), _p(orig, ctypes.c_uint32), ctypes.byref(rlc)))
    return pairs, orig, int(rlc.value)


def entry_cut(pairs, root_leaf_count, root_box):
    """ceres_entry_cut_build: the CutTable of a pair array ([n, 16] u32) under a root box (6 floats)."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 16)
    table = np.zeros(cut_words(), np.uint32)
    rb = np.ascontiguousarray(root_box, np.float32).reshape(6)
    _check(lib().ceres_entry_cut_build(pairs.ctypes.data_as(_vp), pairs.shape[0], int(root_leaf_count), _p(rb, ctypes.c_float),
                                       _p(table, ctypes.c_uint32)))
    return CutTable(table)


def entry_rects(cut, basis12, W, H):
    """ceres_entry_rects: one frame's 64 rectangles {i0, i1, j0, j1} -> [64, 4] u16."""
    b = np.ascontiguousarray(basis12, np.float32).reshape(12)
    out = np.zeros((64, 4), np.uint16)
    _check(lib().ceres_entry_rects(_p(cut.words, ctypes.c_uint32), _p(b, ctypes.c_float), int(W), int(H), _p(out, ctypes.c_uint16)))
    return out


def entry_tiles(cut, rects, W, H):
    """ceres_entry_tiles: the record each 8x8 tile's walk starts at -> [tile rows, tile columns] u32
    (ENTRY_EMPTY: no rectangle reaches the tile)."""
    r = np.ascontiguousarray(rects, np.uint16).reshape(64, 4)
    out = np.zeros(((int(H) + 7) // 8, (int(W) + 7) // 8), np.uint32)
    _check(lib().ceres_entry_tiles(_p(cut.words, ctypes.c_uint32), _p(r, ctypes.c_uint16), int(W), int(H), _p(out, ctypes.c_uint32)))
    return out


def source_sha16(repo=None):
    """sha256 (16 hex digits) of the sources libceres_hip.so is built from, in the Makefile's order
    (build_info.o: include/*.h and include/ceres/*.hpp sorted by path, then csrc/*.cpp *.hip *.hpp
    sorted by name); ceres_version() carries the value the loaded library was built with."""
    import glob
    import hashlib
    repo = repo or os.path.dirname(_PKG)
    inc = sorted(glob.glob(os.path.join(repo, "include", "*.h")) + glob.glob(os.path.join(repo, "include", "ceres", "*.hpp")))
    csrc = os.path.join(_PKG, "csrc")
    names = sorted(n for n in os.listdir(csrc) if n.endswith((".cpp", ".hip", ".hpp")))
    h = hashlib.sha256()
    for f in inc + [os.path.join(csrc, n) for n in names]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def native_provenance():
    """Which native library this process loaded and whether it was built from the sources in this
    tree: {lib, sha256 of the .so, sources_sha16 it was built with, sources_sha16 of the tree, match}."""
    import hashlib
    v = lib().ceres_version().decode()
    built = v.rsplit(" src ", 1)[1] if " src " in v else None
    with open(LIB_PATH, "rb") as fh:
        so_sha = hashlib.sha256(fh.read()).hexdigest()
    now = source_sha16()
    return {"lib": os.path.relpath(LIB_PATH, os.path.dirname(_PKG)), "version": v, "so_sha256": so_sha,
            "built_from_sources_sha16": built, "tree_sources_sha16": now, "built_from_this_tree": built == now}


FETCH_KINDS = ("bvh2_vector", "bvh4_vector", "bvh4_scalar", "tri_vector", "tri_scalar", "shade_vector",
               "store_vector", "order_scalar")
COUNT_LIB_PATH = os.path.join(_PKG, "variants", "libceres_hip_count.so")


def fetch_counters(device=0, reset=True):
    """Bytes moved by the kernels' own fetch sites since the last reset (the counting build only,
    `make count`; the product library raises CeresError EUNSUPPORTED): {kind: bytes}, vector kinds
    per lane, scalar kinds per wavefront (include/ceres_render.h ceres_fetch_counters)."""
    out = np.zeros(8, np.uint64)
    _check(lib().ceres_fetch_counters(int(device), _p(out, ctypes.c_uint64), 1 if reset else 0))
    return {k: int(v) for k, v in zip(FETCH_KINDS, out)}


def render_multi(scenes, basis12, sun, W, H, row_block=8, mode=MODE_FULL, want_pixels=True, want_rgb8=True):
    """ceres_render_multi_f32: one frame split over len(scenes) ranks (one Scene per rank, e.g. one
    per device) in this process; returns (pixels, rgb8, stats) like Scene.render."""
    b = np.ascontiguousarray(basis12, np.float32)
    s = np.ascontiguousarray(sun, np.float32)
    px = np.empty(3 * W * H, np.float32) if want_pixels else None
    rgb = np.empty(3 * W * H, np.uint8) if want_rgb8 else None
    hs = (_vp * len(scenes))(*[sc._h for sc in scenes])
    st = _Stats()
    _check(lib().ceres_render_multi_f32(hs, len(scenes), int(row_block), _p(b, ctypes.c_float), _p(s, ctypes.c_float),
                                        int(mode), _p(px, ctypes.c_float), _p(rgb, ctypes.c_uint8), W, H,
                                        ctypes.byref(st)))
    return px, rgb, dict(rays=st.rays, hits=st.hits, primary_rays=st.primary_rays, shadow_rays=st.shadow_rays,
                         node_pairs=st.node_pairs, tri_tests=st.tri_tests, ms=st.ms)


def orbit_cameras(camera, sun, W, H, n_frames, axis=(0, 1, 0), step_deg=None, rotate_first=True, want_dirs=False):
    """anim.cpp:76-88 orbit: eye, dir and sun rotated by step_deg (default 360/n_frames, as
    anim.cpp) about `axis` per frame.  Returns (basis12 [F,12] f32, sun3 [F,3] f32) and, with
    want_dirs, the rotated camera dirs [F,3] as a third element."""
    n = int(n_frames)
    step = np.float32(360.0) / np.float32(n) if step_deg is None else np.float32(step_deg)
    b = np.zeros((n, 12), np.float32)
    s3 = np.zeros((n, 3), np.float32)
    d3 = np.zeros((n, 3), np.float32)
    ax = np.asarray(axis, np.float32)
    sn = np.asarray(sun, np.float32)
    _check(lib().ceres_orbit_cameras_arith(_p(camera.eye, ctypes.c_float), _p(camera.dir, ctypes.c_float),
                                           _p(camera.up, ctypes.c_float), _p(sn, ctypes.c_float), camera.fov, W, H,
                                           _p(ax, ctypes.c_float), float(step), n, 1 if rotate_first else 0,
                                           _p(b, ctypes.c_float), _p(s3, ctypes.c_float), _p(d3, ctypes.c_float),
                                           camera.arith))
    return (b, s3, d3) if want_dirs else (b, s3)


def bench_views(camera, sun, W, H, F, basis0=None):
    """The F views of one bench.py step: frame f = the camera + sun rotated once by
    configs.orbit_step(f, F) degrees about configs.BENCH_AXIS (anim.cpp:76-88, Transform::rotate
    transform.hpp:67-112); frame 0 unrotated, with `basis0` (the fixture's pinned basis12) when
    given.  Returns (basis12 [F,12] f32, sun3 [F,3] f32, step_deg [F] f32); the reference PPM of
    every such view is pinned in tests/golden/orbit/<cfg>.json by its step bits."""
    F = int(F)
    b12 = np.zeros((F, 12), np.float32)
    s3 = np.zeros((F, 3), np.float32)
    steps = np.asarray([configs.orbit_step(f, F) for f in range(F)], np.float32)
    b12[0] = camera.basis(W, H) if basis0 is None else np.asarray(basis0, np.float32)
    s3[0] = np.asarray(sun, np.float32)
    for f in range(1, F):
        b, s = orbit_cameras(camera, sun, W, H, 2, axis=configs.BENCH_AXIS, step_deg=float(steps[f]),
                             rotate_first=False)
        b12[f], s3[f] = b[1], s[1]
    return b12, s3, steps


def pose(cfg, frame=0, arith=ARITH_EXACT):
    """(Camera, sun) of a config: configs with "orbit": (axis, step_deg, count) are the anim.cpp
    orbit pose after count + frame rotations; otherwise the config's camera rotated `frame`
    times by configs.BENCH_ORBIT."""
    cam = Camera(cfg["eye"], cfg["dir"], cfg["up"], cfg["fov"], arith=arith)
    axis, step = (cfg["orbit"][0], cfg["orbit"][1]) if cfg.get("orbit") else configs.BENCH_ORBIT
    n = (cfg["orbit"][2] if cfg.get("orbit") else 0) + int(frame)
    if n == 0:
        return cam, np.asarray(cfg["sun"], np.float32)
    b, s3, d3 = orbit_cameras(cam, cfg["sun"], cfg["W"], cfg["H"], n + 1, axis=axis, step_deg=step,
                              rotate_first=False, want_dirs=True)
    return Camera(b[n, :3], d3[n], cfg["up"], cfg["fov"], arith=arith), s3[n].copy()


def pose_f64(cfg, arith=ARITH_EXACT):
    """(Camera<double>, sun) of a config: its values as double literals (anim.cpp writes its
    camera as double literals), orbited with Transform<double> when the config has "orbit"."""
    cam = Camera(cfg["eye"], cfg["dir"], cfg["up"], cfg["fov"], dtype=np.float64, arith=arith)
    sun = np.asarray(cfg["sun"], np.float64)
    if not cfg.get("orbit"):
        return cam, sun
    (axis, step, n) = cfg["orbit"]
    b = np.zeros((n + 1, 12), np.float64)
    s3 = np.zeros((n + 1, 3), np.float64)
    d3 = np.zeros((n + 1, 3), np.float64)
    ax = np.asarray(axis, np.float64)
    _check(lib().ceres_orbit_cameras_f64_arith(_p(cam.eye, ctypes.c_double), _p(cam.dir, ctypes.c_double),
                                               _p(cam.up, ctypes.c_double), _p(sun, ctypes.c_double), cam.fov, cfg["W"],
                                               cfg["H"], _p(ax, ctypes.c_double), float(step), n + 1, 0,
                                               _p(b, ctypes.c_double), _p(s3, ctypes.c_double), _p(d3, ctypes.c_double),
                                               int(arith)))
    return Camera(b[n, :3], d3[n], cfg["up"], cfg["fov"], dtype=np.float64, arith=arith), s3[n].copy()


def assemble_rgb8(d_gathered, rank_stride, d_out, frames, W, H, row_block, world, stream=0):
    """ceres_assemble_rgb8 (device pointers): rank-major gathered batch rows -> F PPM bodies."""
    _check(lib().ceres_assemble_rgb8(d_gathered, rank_stride, d_out, int(frames), W, H, int(row_block), int(world),
                                     stream or None))


def assemble_rgb8_packed(d_gathered, d_out, frames, W, H, row_block, world, stream=0):
    """ceres_assemble_rgb8_packed (device pointers): packed rank-major rows -> F PPM bodies."""
    _check(lib().ceres_assemble_rgb8_packed(d_gathered, d_out, int(frames), W, H, int(row_block), int(world),
                                            stream or None))


def local_rows(H, tiling):
    return lib().ceres_tiling_local_rows(H, ctypes.byref(tiling))


def kept_tiles(W, H, frames, tpw, rects):
    """ceres_debug_kept_tiles (no GPU): for a batch of whole W x H frames with cull rectangles rects
    [frames, 4] = {i0, i1, j0, j1} -> dict: tiles (what the host sizes a compacted grid for), deal (XCD
    chunk in groups, 0: none), packed (entries are frame << 26 | tile row << 13 | tile column words, else
    linear ids), count (how the host counts: "walk", "boxes", or None -- no cheap count, such launches keep
    the plain grid and tiles is every tile) and source (the order whose groups of tpw entries are kept or
    dropped)."""
    r = np.ascontiguousarray(rects, np.uint16).reshape(frames, 4)
    info = np.zeros(4, np.uint32)
    n = ((W + 7) // 8) * ((H + 7) // 8) * frames
    src = np.zeros(n, np.uint32)
    _check(lib().ceres_debug_kept_tiles(W, H, frames, tpw, _p(r, ctypes.c_uint16), _p(info, ctypes.c_uint32),
                                        _p(src, ctypes.c_uint32), n))
    assert int(info[1]) == n
    how = "boxes" if info[3] & 4 else "walk" if info[3] & 2 else None
    return {"tiles": int(info[0]), "deal": int(info[2]), "packed": bool(info[3] & 1), "count": how, "source": src}


def row_map(H, row_block, world):
    """For each rank, the global rows j of its local rows k (ceres_tiling)."""
    out = []
    nb = (H + row_block - 1) // row_block
    for r in range(world):
        rows = []
        for b in range(r, nb, world):
            rows.extend(range(b * row_block, min(H, (b + 1) * row_block)))
        out.append(np.asarray(rows, np.int64))
    return out


def prepare(cfg, f64=False, arith=ARITH_EXACT):
    """Scene prep of the reference app for a config (configs.CONFIGS entry): mesh, bvh, camera
    (at the config's orbit pose; pose(cfg) also gives the sun).  f64: the render<double>
    pipeline (anim.cpp -d) -- double mesh / BVH, camera at the config's pose in double.
    arith = ARITH_FMA: every step in the reference CMake build's arithmetic (render with MODE_FMA)."""
    if f64:
        mesh = proc_mesh_f64(cfg["proc"], arith) if cfg.get("proc") else load_obj_f64(configs.obj_path(cfg), arith)
        if len(mesh) == 0:
            raise CeresError("The given scene is empty or cannot be loaded")
        if cfg.get("rotate"):
            rotate_triangles(mesh, cfg["rotate"][0], cfg["rotate"][1], arith)
        return mesh, build_bvh(mesh, arith), pose_f64(cfg, arith)[0]
    mesh = proc_mesh(cfg["proc"], arith) if cfg.get("proc") else load_obj(configs.obj_path(cfg), arith)
    if len(mesh) == 0:
        raise CeresError("The given scene is empty or cannot be loaded")
    if cfg.get("rotate"):
        rotate_triangles(mesh, cfg["rotate"][0], cfg["rotate"][1], arith)
    bvh = build_bvh(mesh, arith)
    cam, _ = pose(cfg, arith=arith)
    return mesh, bvh, cam


def render(camera, sun, scene, W, H, mode=MODE_FULL):
    """render<float>() (render.hpp:86-156): returns (pixels [3*W*H] f32, rays, hits)."""
    px, _, st = scene.render(camera.basis(W, H), sun, W, H, mode=mode, want_rgb8=False)
    return px, st["rays"], st["hits"]


def ppm(W, H, rgb8):
    """P6 file bytes exactly as static.cpp:135-147 writes them."""
    return b"P6 %d %d 255\n" % (W, H) + np.asarray(rgb8, np.uint8).tobytes()
