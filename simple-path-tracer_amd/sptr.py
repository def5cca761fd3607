"""sptr — Python (ctypes) binding of libsptr_hip.so, the MI355X wavefront path-tracing backend.

This is the ctypes form of the binding a reference-side maintainer would add:
every call goes straight to the C ABI in include/sptr_hip.h.  There is no CPU fallback: if the
library is missing or no GPU is present, constructing a Renderer raises.

Reference mapping: Renderer mirrors backends::OptixBackend (include/backends/OptixBackend.h:39-71)
with the CPU wavefront integrator's semantics (src/wavefront/wf_pt_cpu.cpp:61-255).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPTR_LIB") or os.path.join(HERE, "libsptr_hip.so")  # SPTR_LIB: A/B builds

SPTR_ABI_VERSION = 9  # include/sptr_hip.h
SPTR_FRAME_TIMING = 1
SPTR_FRAME_NO_RESOLVE = 2
SPTR_FRAME_COUNT_VISITS = 4
SPTR_FRAME_ASYNC = 8
SPTR_FRAME_TIMING_TRACE = 16
SPTR_FRAME_NO_CULL = 32
SPTR_FRAME_RECULL = 64
SPTR_UPDATE_DEVICE_PTRS = 1
SPTR_DYNAMIC_REFIT = 1
SPTR_DYNAMIC_TRANSFORMS = 2
SPTR_QUERY_ANY_HIT = 1
SPTR_QUERY_DEVICE_PTRS = 2
SPTR_QUERY_SORT = 4
SPTR_QUERY_NO_SORT = 8

SPTR_INTEGRATOR_WAVEFRONT = 0   # WavefrontPathTracerCPU semantics (default)
SPTR_INTEGRATOR_PATHTRACER = 1  # PathTracer (the reference's default CPU integrator) semantics
SPTR_INTEGRATOR_OPTIX = 2       # the reference's OptiX device-program shading (GPU 'G' path)


class SptrError(RuntimeError):
    pass


class Scene(C.Structure):
    _fields_ = [
        ("positions", C.POINTER(C.c_float)), ("num_verts", C.c_uint32),
        ("indices", C.POINTER(C.c_uint32)), ("num_tris", C.c_uint32),
        ("tri_geom_first", C.POINTER(C.c_uint32)), ("num_tri_geoms", C.c_uint32),
        ("spheres", C.POINTER(C.c_float)), ("num_spheres", C.c_uint32),
        ("geom_material", C.POINTER(C.c_uint32)),
    ]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("metallic", C.c_float), ("roughness", C.c_float),
                ("emission", C.c_float * 3), ("ior", C.c_float), ("type", C.c_int32), ("pad", C.c_float * 2)]


class Light(C.Structure):
    _fields_ = [("type", C.c_int32), ("v", C.c_float * 3), ("color", C.c_float * 3), ("intensity", C.c_float)]


class Environment(C.Structure):
    _fields_ = [("faces", C.POINTER(C.c_float)), ("size", C.c_int32), ("intensity", C.c_float),
                ("max_clamp", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3),
                ("up", C.c_float * 3), ("half_width", C.c_float), ("half_height", C.c_float)]

    def as_array(self) -> np.ndarray:
        return np.array(list(self.pos) + list(self.forward) + list(self.right) + list(self.up)
                        + [self.half_width, self.half_height], dtype=np.float32)


class Frame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("camera", Camera), ("frame_begin", C.c_uint32),
                ("spp", C.c_uint32), ("max_depth", C.c_uint32), ("shard_rank", C.c_int32),
                ("shard_count", C.c_int32), ("flags", C.c_uint32), ("integrator", C.c_uint32),
                ("samples_per_frame", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64), ("samples", C.c_uint64),
                ("waves", C.c_uint64), ("ms_total", C.c_double), ("ms_raygen", C.c_double),
                ("ms_trace", C.c_double), ("ms_shade", C.c_double), ("ms_shadow", C.c_double),
                ("ms_accum", C.c_double), ("trace_launches", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("sphere_tests", C.c_uint64), ("shadow_node_visits", C.c_uint64),
                ("shadow_prim_tests", C.c_uint64), ("ms_trace0", C.c_double), ("ms_shade0", C.c_double),
                ("rays_tail", C.c_uint64), ("ms_tail", C.c_double), ("traced_primary", C.c_uint64),
                ("traced_bounce", C.c_uint64), ("node_visits_primary", C.c_uint64),
                ("tri_tests_primary", C.c_uint64), ("sphere_tests_primary", C.c_uint64), ("ms_cull", C.c_double),
                ("cull_launches", C.c_uint64), ("shadow_launches", C.c_uint64),
                ("traced_by_depth", C.c_uint64 * 8), ("nodes_by_depth", C.c_uint64 * 8),
                ("trace_visit_hist", C.c_uint64 * 16), ("shadow_visit_hist", C.c_uint64 * 16),
                ("hits_primary", C.c_uint64), ("hits_bounce", C.c_uint64), ("paths_handed_off", C.c_uint64), ("strag_visits", C.c_uint64 * 3),
                ("ms_trace_busy", C.c_double), ("traced_fused", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: (list(v) if isinstance(v, C.Array) else v) for k, v in ((k, getattr(self, k)) for k, _ in self._fields_)}


class SceneLayout(C.Structure):
    _fields_ = [("num_tris", C.c_uint32), ("num_spheres", C.c_uint32), ("num_nodes", C.c_uint32),
                ("leaf_size", C.c_uint32), ("bvh_depth", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("node_bytes", C.c_uint64), ("tri_bytes", C.c_uint64), ("sphere_bytes", C.c_uint64),
                ("prim_ref_bytes", C.c_uint64), ("bvh_width", C.c_uint32), ("num_prim_refs", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class TreeOrderInfo(C.Structure):
    _fields_ = [("order", C.c_uint32), ("fallback", C.c_uint32), ("depth", C.c_uint32), ("num_leaves", C.c_uint32),
                ("cost_sah", C.c_double), ("cost_morton", C.c_double)]


class ShadowEntriesInfo(C.Structure):  # sptr_shadow_entries_info_t
    _fields_ = [("mode", C.c_uint32), ("cells", C.c_uint32), ("bytes", C.c_uint32), ("builds", C.c_uint32),
                ("cells_below_root", C.c_float), ("cells_unoccluded", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("normal_log2_power", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class HistoryParams(C.Structure):
    """sptr_history_params."""
    _fields_ = [("max_history", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RayQuery(C.Structure):
    """sptr_ray_query: pointers as addresses (host or device, by SPTR_QUERY_DEVICE_PTRS)."""
    _fields_ = [("rays", C.c_void_p), ("n", C.c_uint32), ("flags", C.c_uint32), ("geom", C.c_void_p),
                ("prim", C.c_void_p), ("t", C.c_void_p), ("ng", C.c_void_p), ("uv", C.c_void_p),
                ("occluded", C.c_void_p), ("reserved", C.c_uint64 * 4)]


class MultiHitQuery(C.Structure):
    """sptr_multi_hit_query: pointers as addresses (host or device, by SPTR_QUERY_DEVICE_PTRS)."""
    _fields_ = [("rays", C.c_void_p), ("n", C.c_uint32), ("flags", C.c_uint32), ("max_hits", C.c_uint32),
                ("pad", C.c_uint32), ("count", C.c_void_p), ("geom", C.c_void_p), ("prim", C.c_void_p),
                ("t", C.c_void_p), ("ng", C.c_void_p), ("uv", C.c_void_p), ("reserved", C.c_uint64 * 4)]


SPTR_MULTI_HIT_MAX = 16


class PointQuery(C.Structure):
    """sptr_point_query: pointers as addresses (host or device, by SPTR_QUERY_DEVICE_PTRS)."""
    _fields_ = [("points", C.c_void_p), ("n", C.c_uint32), ("flags", C.c_uint32), ("geom", C.c_void_p),
                ("prim", C.c_void_p), ("dist2", C.c_void_p), ("dist", C.c_void_p), ("point", C.c_void_p),
                ("uv", C.c_void_p), ("ng", C.c_void_p), ("reserved", C.c_uint64 * 4)]


class SignedQuery(C.Structure):
    """sptr_signed_query: a PointQuery and the three outputs of the sign pass."""
    _fields_ = [("q", PointQuery), ("signed_dist", C.c_void_p), ("normal", C.c_void_p), ("feature", C.c_void_p),
                ("reserved", C.c_uint64 * 4)]


class SignedInfo(C.Structure):
    """sptr_signed_info_t"""
    _fields_ = [("welded_vertices", C.c_uint64), ("edges", C.c_uint64), ("open_edges", C.c_uint64),
                ("irregular_edges", C.c_uint64), ("table_bytes", C.c_uint64), ("builds", C.c_uint32),
                ("valid", C.c_uint32), ("num_tris", C.c_uint32), ("pad", C.c_uint32), ("ms_build", C.c_double),
                ("ms_sign", C.c_double)]


SPTR_POINT_COUNT = 16
SPTR_SIGNED_FLIP_TRIANGLES = 32


class RayRender(C.Structure):
    """sptr_ray_render: pointers as addresses (host or device, by SPTR_RAYS_DEVICE_PTRS)."""
    _fields_ = [("rays", C.c_void_p), ("seeds", C.c_void_p), ("n", C.c_uint32), ("samples", C.c_uint32),
                ("frame_index", C.c_uint32), ("max_depth", C.c_uint32), ("flags", C.c_uint32),
                ("radiance", C.c_void_p), ("reserved", C.c_uint32 * 4)]


class AdaptiveParams(C.Structure):
    """sptr_adaptive_params."""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32),
                ("step", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class AdaptiveInfo(C.Structure):
    """sptr_adaptive_info."""
    _fields_ = [("samples", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("passes", C.c_uint32), ("chunks", C.c_uint32), ("active_first", C.c_uint32),
                ("active_last", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("ms", C.c_double), ("reserved", C.c_uint32 * 4)]


SPTR_RAYS_DEVICE_PTRS, SPTR_RAYS_ACCUMULATE, SPTR_RAYS_NORMALIZE = 1, 2, 4
SPTR_ADAPTIVE_CONTINUE = 1
SPTR_AOV_ALBEDO, SPTR_AOV_NORMAL, SPTR_AOV_DEPTH, SPTR_AOV_ID, SPTR_AOV_UV = 0, 1, 2, 3, 4
DEFAULT_MAX_HISTORY = 4  # the cap to ask set_denoise_history for without a number of one's own

_lib = None

# every symbol include/sptr_hip.h declares
EXPORTS = [
    "sptr_abi_version", "sptr_create", "sptr_destroy", "sptr_last_error", "sptr_set_debug_mode",
    "sptr_set_wave_paths", "sptr_set_launch_mode", "sptr_set_pixel_lanes", "sptr_pixel_lanes_info", "sptr_graph_info", "sptr_capture_error", "sptr_overlap_probe", "sptr_set_tail_depth", "sptr_set_bounce_chain", "sptr_set_sky_split", "sptr_sky_split_info", "sptr_set_shadow_entries", "sptr_shadow_entries_info", "sptr_set_leaf_size", "sptr_set_tree_order", "sptr_tree_info", "sptr_set_split_refs", "sptr_set_stragglers", "sptr_set_bvh_width", "sptr_upload_scene", "sptr_set_materials", "sptr_set_lights",
    "sptr_set_environment", "sptr_scene_info", "sptr_scene_layout_info", "sptr_render", "sptr_collect_stats",
    "sptr_read_rgb8", "sptr_read_rgb8_lagged",
    "sptr_read_accum",
    "sptr_tiles_device", "sptr_unpack_tiles", "sptr_intersect", "sptr_occluded", "sptr_primary_rays",
    "sptr_sort_pairs_u64", "sptr_scan_u32", "sptr_eval_math",
    "sptr_set_denoise", "sptr_read_aov", "sptr_read_denoised", "sptr_denoise_info",
    "sptr_set_seed_offset", "sptr_set_denoise_history", "sptr_read_history", "sptr_history_info",
    "sptr_set_history_motion", "sptr_read_motion", "sptr_motion_info",
    "sptr_set_dynamic", "sptr_update_geometry", "sptr_refit_info",
    "sptr_set_rest_positions", "sptr_update_transforms", "sptr_tree_cost",
    "sptr_query_rays", "sptr_query_info", "sptr_query_multi_hit", "sptr_multi_hit_info",
    "sptr_query_points", "sptr_point_query_info", "sptr_host_query_points", "sptr_render_rays", "sptr_ray_render_info",
    "sptr_set_signed_distance", "sptr_query_signed_distance", "sptr_signed_info", "sptr_read_pseudonormals",
    "sptr_host_pseudonormals", "sptr_host_query_signed_distance",
    "sptr_render_adaptive", "sptr_read_sample_counts",
    "sptr_host_builtin_scene", "sptr_host_scene_view", "sptr_host_scene_free", "sptr_host_camera_lookat",
    "sptr_host_preset_materials", "sptr_host_default_lights", "sptr_host_equirect_to_faces",
    "sptr_host_pack_tiles", "sptr_host_unpack_tiles", "sptr_host_load_hdr", "sptr_host_free",
]


def lib() -> C.CDLL:
    """Load libsptr_hip.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SptrError(f"{LIB_PATH} not built (run make in simple-path-tracer_amd/)")
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    sig = {
        "sptr_abi_version": (C.c_int, []),
        "sptr_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "sptr_destroy": (C.c_int, [vp]),
        "sptr_last_error": (C.c_char_p, [vp]),
        "sptr_set_debug_mode": (C.c_int, [vp, C.c_int]),
        "sptr_set_wave_paths": (C.c_int, [vp, u64]),
        "sptr_set_launch_mode": (C.c_int, [vp, u32]),
        "sptr_set_pixel_lanes": (C.c_int, [vp, u32]),
        "sptr_pixel_lanes_info": (C.c_int, [vp, C.POINTER(u32), C.POINTER(u32)]),
        "sptr_graph_info": (C.c_int, [vp, up, up, up, up, up, C.POINTER(C.c_int32)]),
        "sptr_capture_error": (C.c_char_p, [vp]),
        "sptr_overlap_probe": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sptr_set_tail_depth": (C.c_int, [vp, u32]),
        "sptr_set_bounce_chain": (C.c_int, [vp, u32]),
        "sptr_set_sky_split": (C.c_int, [vp, u32, u32]),
        "sptr_sky_split_info": (C.c_int, [vp, C.POINTER(u32)]),
        "sptr_set_shadow_entries": (C.c_int, [vp, u32]),
        "sptr_shadow_entries_info": (C.c_int, [vp, C.POINTER(ShadowEntriesInfo)]),
        "sptr_set_leaf_size": (C.c_int, [vp, u32]),
        "sptr_set_tree_order": (C.c_int, [vp, u32]),
        "sptr_tree_info": (C.c_int, [vp, C.POINTER(TreeOrderInfo)]),
        "sptr_set_split_refs": (C.c_int, [vp, u32]),
        "sptr_set_stragglers": (C.c_int, [vp, u32]),
        "sptr_set_bvh_width": (C.c_int, [vp, u32]),
        "sptr_upload_scene": (C.c_int, [vp, C.POINTER(Scene)]),
        "sptr_set_materials": (C.c_int, [vp, C.POINTER(Material), u32]),
        "sptr_set_lights": (C.c_int, [vp, C.POINTER(Light), u32]),
        "sptr_set_environment": (C.c_int, [vp, C.POINTER(Environment)]),
        "sptr_scene_info": (C.c_int, [vp, up, up, up, C.POINTER(C.c_double)]),
        "sptr_scene_layout_info": (C.c_int, [vp, C.POINTER(SceneLayout)]),
        "sptr_render": (C.c_int, [vp, C.POINTER(Frame), vp, C.POINTER(Stats)]),
        "sptr_collect_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "sptr_read_rgb8": (C.c_int, [vp, bp]),
        "sptr_read_rgb8_lagged": (C.c_int, [vp, bp, C.POINTER(u32)]),
        "sptr_read_accum": (C.c_int, [vp, fp]),
        "sptr_tiles_device": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "sptr_unpack_tiles": (C.c_int, [vp, vp, i32, u32, i32, i32, vp, vp]),
        "sptr_intersect": (C.c_int, [vp, fp, u32, up, up, fp, fp]),
        "sptr_occluded": (C.c_int, [vp, fp, u32, bp]),
        "sptr_primary_rays": (C.c_int, [vp, C.POINTER(Camera), i32, i32, u32, fp, up]),
        "sptr_sort_pairs_u64": (C.c_int, [vp, C.POINTER(C.c_uint64), up, u32, C.POINTER(C.c_uint64), up]),
        "sptr_scan_u32": (C.c_int, [vp, up, u32, up]),
        "sptr_eval_math": (C.c_int, [vp, C.c_int, fp, u32, fp]),
        "sptr_set_denoise": (C.c_int, [vp, C.POINTER(DenoiseParams)]),
        "sptr_read_aov": (C.c_int, [vp, C.c_int, vp]),
        "sptr_read_denoised": (C.c_int, [vp, fp]),
        "sptr_denoise_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), up]),
        "sptr_set_seed_offset": (C.c_int, [vp, u32]),
        "sptr_set_denoise_history": (C.c_int, [vp, C.POINTER(HistoryParams)]),
        "sptr_read_history": (C.c_int, [vp, fp]),
        "sptr_history_info": (C.c_int, [vp, up, C.POINTER(C.c_double), up]),
        "sptr_set_history_motion": (C.c_int, [vp, u32]),
        "sptr_read_motion": (C.c_int, [vp, fp]),
        "sptr_motion_info": (C.c_int, [vp, up, C.POINTER(C.c_double), up]),
        "sptr_set_dynamic": (C.c_int, [vp, u32]),
        "sptr_update_geometry": (C.c_int, [vp, vp, u32, vp, u32, u32]),
        "sptr_refit_info": (C.c_int, [vp, up, C.POINTER(C.c_double), C.POINTER(C.c_double), up]),
        "sptr_set_rest_positions": (C.c_int, [vp, vp, u32, u32]),
        "sptr_update_transforms": (C.c_int, [vp, vp, u32, vp, u32, u32]),
        "sptr_tree_cost": (C.c_int, [vp] + [C.POINTER(C.c_double)] * 4),
        "sptr_query_rays": (C.c_int, [vp, C.POINTER(RayQuery), vp]),
        "sptr_query_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), up, up]),
        "sptr_query_multi_hit": (C.c_int, [vp, C.POINTER(MultiHitQuery), vp]),
        "sptr_multi_hit_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), up, up, up, up]),
        "sptr_query_points": (C.c_int, [vp, C.POINTER(PointQuery), vp]),
        "sptr_point_query_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), up, up, C.POINTER(u64),
                                            C.POINTER(u64)]),
        "sptr_host_query_points": (C.c_int, [C.POINTER(Scene), C.POINTER(PointQuery)]),
        "sptr_set_signed_distance": (C.c_int, [vp, u32]),
        "sptr_query_signed_distance": (C.c_int, [vp, C.POINTER(SignedQuery), vp]),
        "sptr_signed_info": (C.c_int, [vp, C.POINTER(SignedInfo)]),
        "sptr_read_pseudonormals": (C.c_int, [vp, fp, fp]),
        "sptr_host_pseudonormals": (C.c_int, [C.POINTER(Scene), fp, fp, C.POINTER(u64)]),
        "sptr_host_query_signed_distance": (C.c_int, [C.POINTER(Scene), C.POINTER(SignedQuery)]),
        "sptr_render_rays": (C.c_int, [vp, C.POINTER(RayRender), vp]),
        "sptr_ray_render_info": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64), up]),
        "sptr_render_adaptive": (C.c_int, [vp, C.POINTER(Frame), C.POINTER(AdaptiveParams), C.POINTER(AdaptiveInfo)]),
        "sptr_read_sample_counts": (C.c_int, [vp, up]),
        "sptr_host_builtin_scene": (C.c_int, [C.c_char_p, u32, u32, C.POINTER(vp)]),
        "sptr_host_scene_view": (C.c_int, [vp, C.POINTER(Scene)]),
        "sptr_host_scene_free": (None, [vp]),
        "sptr_host_camera_lookat": (C.c_int, [fp, fp, C.c_float, C.c_float, C.POINTER(Camera)]),
        "sptr_host_preset_materials": (C.c_int, [C.c_int, C.POINTER(Material), C.c_int]),
        "sptr_host_default_lights": (C.c_int, [C.POINTER(Light), C.c_int]),
        "sptr_host_equirect_to_faces": (C.c_int, [fp, i32, i32, i32, fp]),
        "sptr_host_pack_tiles": (C.c_int, [bp, i32, i32, i32, i32, up]),
        "sptr_host_unpack_tiles": (C.c_int, [up, i32, u32, i32, i32, bp]),
        "sptr_host_load_hdr": (C.c_int, [C.c_char_p, C.POINTER(fp), C.POINTER(i32), C.POINTER(i32)]),
        "sptr_host_free": (None, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.sptr_abi_version() != SPTR_ABI_VERSION:  # a stale build would misread the structs below
        raise SptrError(f"{LIB_PATH}: ABI {L.sptr_abi_version()}, this binding expects {SPTR_ABI_VERSION} (rebuild)")
    _lib = L
    return L


def _f(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _b(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


# --------------------------------------------------------------------------------- host scene layer
@dataclass
class FlatScene:
    """World-space flattened scene in EmbreeBackend::build geomID order (numpy-owned copies)."""
    positions: np.ndarray       # (V,3) float32
    indices: np.ndarray         # (T,3) uint32
    tri_geom_first: np.ndarray  # (G+1,) uint32
    spheres: np.ndarray         # (S,4) float32
    geom_material: np.ndarray   # (G+S,) uint32

    def to_c(self) -> Scene:
        self._keep = [np.ascontiguousarray(self.positions, np.float32), np.ascontiguousarray(self.indices, np.uint32),
                      np.ascontiguousarray(self.tri_geom_first, np.uint32),
                      np.ascontiguousarray(self.spheres, np.float32),
                      np.ascontiguousarray(self.geom_material, np.uint32)]
        p, i, g, s, m = self._keep
        return Scene(_f(p), len(p), _u(i), len(i), _u(g), len(g) - 1, _f(s), len(s), _u(m))


def builtin_scene(name: str, p0: int = 0, p1: int = 0) -> FlatScene:
    """Scenes built by the C++ host layer: default, default_emitter, test_triangle,
    sphere_mesh (p0 stacks, p1 slices), gltf:<path> (p0 = material)."""
    L = lib()
    h = C.c_void_p()
    rc = L.sptr_host_builtin_scene(name.encode(), p0, p1, C.byref(h))
    if rc != 0:
        raise SptrError(f"builtin scene {name!r} failed ({rc})")
    try:
        v = Scene()
        L.sptr_host_scene_view(h, C.byref(v))

        def arr(ptr, n, dt, cols):
            if n == 0:
                return np.zeros((0, cols) if cols > 1 else (0,), dt)
            a = np.ctypeslib.as_array(ptr, shape=(n * cols,)).copy().astype(dt)
            return a.reshape(n, cols) if cols > 1 else a

        return FlatScene(
            positions=arr(v.positions, v.num_verts, np.float32, 3),
            indices=arr(v.indices, v.num_tris, np.uint32, 3),
            tri_geom_first=arr(v.tri_geom_first, v.num_tri_geoms + 1, np.uint32, 1),
            spheres=arr(v.spheres, v.num_spheres, np.float32, 4),
            geom_material=arr(v.geom_material, v.num_tri_geoms + v.num_spheres, np.uint32, 1),
        )
    finally:
        L.sptr_host_scene_free(h)


_POINT_FIELDS = (("geom", 1, np.uint32), ("prim", 1, np.uint32), ("dist2", 1, np.float32), ("dist", 1, np.float32),
                 ("point", 3, np.float32), ("uv", 2, np.float32), ("ng", 3, np.float32))


def host_query_points(scene: FlatScene, points, fields=None) -> dict:
    """sptr_host_query_points: the host twin of Renderer.query_points, brute force over every primitive of a flat
    scene with the device's arithmetic (csrc/closest_point.h).  points: (n, 4) float32 (p.xyz, max_dist)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    n = len(pts)
    known = [f for f, _, _ in _POINT_FIELDS]
    names = known if fields is None else list(fields)
    if any(f not in known for f in names):
        raise SptrError(f"host_query_points: fields must name some of {known} (got {names})")
    res = {f: np.zeros((n, cols) if cols > 1 else (n,), dt) for f, cols, dt in _POINT_FIELDS if f in names}
    q = PointQuery()
    q.points = pts.ctypes.data if n else None
    q.n = n
    for name, a in res.items():
        setattr(q, name, a.ctypes.data if n else None)
    cs = scene.to_c()
    rc = lib().sptr_host_query_points(C.byref(cs), C.byref(q))
    if rc != 0:
        raise SptrError(f"host_query_points failed ({rc})")
    return res


_SIGNED_FIELDS = (("signed_dist", 1, np.float32), ("normal", 3, np.float32), ("feature", 1, np.uint32))
_SIGNED_COUNTS = ("welded_vertices", "edges", "open_edges", "irregular_edges")


def _signed_query_set(q: SignedQuery, name: str, value) -> None:
    setattr(q if name in [f for f, _, _ in _SIGNED_FIELDS] else q.q, name, value)


def host_pseudonormals(scene: FlatScene) -> dict:
    """sptr_host_pseudonormals: the host twin of the device's table build (csrc/pseudonormal.h): nv, ne as
    (num_tris, 3, 3) float32 (corner k, edge k of each uploaded triangle) and the four counts."""
    cs = scene.to_c()
    nt = int(cs.num_tris)
    nv, ne = np.zeros((nt, 3, 3), np.float32), np.zeros((nt, 3, 3), np.float32)
    cnt = (C.c_uint64 * 4)()
    fp = C.POINTER(C.c_float)
    rc = lib().sptr_host_pseudonormals(C.byref(cs), nv.ctypes.data_as(fp), ne.ctypes.data_as(fp), cnt)
    if rc != 0:
        raise SptrError(f"host_pseudonormals failed ({rc})")
    res = {"nv": nv, "ne": ne}
    res.update({k: int(cnt[i]) for i, k in enumerate(_SIGNED_COUNTS)})
    return res


def host_query_signed_distance(scene: FlatScene, points, fields=None, flip_triangles: bool = False) -> dict:
    """sptr_host_query_signed_distance: the host twin of Renderer.query_signed_distance: host_query_points' fields
    and signed_dist (n), normal (n, 3), feature (n, uint32)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    n = len(pts)
    table = _POINT_FIELDS + _SIGNED_FIELDS
    known = [f for f, _, _ in table]
    names = known if fields is None else list(fields)
    if any(f not in known for f in names):
        raise SptrError(f"host_query_signed_distance: fields must name some of {known} (got {names})")
    res = {f: np.zeros((n, cols) if cols > 1 else (n,), dt) for f, cols, dt in table if f in names}
    q = SignedQuery()
    q.q.points = pts.ctypes.data if n else None
    q.q.n = n
    q.q.flags = SPTR_SIGNED_FLIP_TRIANGLES if flip_triangles else 0
    for name, a in res.items():
        _signed_query_set(q, name, a.ctypes.data if n else None)
    cs = scene.to_c()
    rc = lib().sptr_host_query_signed_distance(C.byref(cs), C.byref(q))
    if rc != 0:
        raise SptrError(f"host_query_signed_distance failed ({rc})")
    return res


_QUERY_FIELDS = (("geom", 1, np.uint32), ("prim", 1, np.uint32), ("t", 1, np.float32), ("ng", 3, np.float32),
                 ("uv", 2, np.float32))
_QUERY_EMPTY = C.c_uint64(0)
_QUERY_INPUT = {8: ("rays", ", ".join), 4: ("points", str)}  # by row width: the noun and how a message lists the fields


def _query_flags(sort, device: bool) -> int:
    return ((SPTR_QUERY_DEVICE_PTRS if device else 0)
            | (0 if sort is None else SPTR_QUERY_SORT if sort else SPTR_QUERY_NO_SORT))


def _query_arrays(x, width: int, who: str, table, fields, out, stream, per_row=None, always=()):
    """What Renderer.query_rays, query_multi_hit, query_points and query_signed_distance (who) do before the call: x
    is a numpy (n, width) array (host path) or a contiguous float32 device tensor of n x width (device path).  table:
    (name, cols, dtype) of the outputs that fields (None: all) chooses from; always: such rows that every result
    holds, before the chosen ones.  An output is out[name], checked, or a new array: numpy or torch, like x, of
    (n,) or (n, cols), with per_row = K of (n, K) or (n, K, cols) (the rows of `always` stay (n,)).
    Returns x as the call takes it, n, whether the device path is taken, {name: array} and the address function."""
    noun, listing = _QUERY_INPUT[width]
    device = hasattr(x, "data_ptr")
    if device:
        import torch

        if x.element_size() != 4 or not x.is_floating_point() or not x.is_contiguous() or x.numel() % width:
            raise SptrError(f"{who}: device {noun} must be a contiguous float32 tensor of n x {width}")
        n = x.numel() // width
        tdt = {np.uint32: torch.uint32, np.float32: torch.float32, np.uint8: torch.uint8}

        def alloc(shape, dt):
            return torch.empty(shape, dtype=tdt[dt], device=x.device)

        def addr(a):
            return a.data_ptr()

        def ok(a, size, dt):
            return a.is_contiguous() and a.numel() == size and a.dtype == tdt[dt] and a.device == x.device
    else:
        if stream is not None:
            raise SptrError(f"{who}: a stream needs device tensors")
        x = np.ascontiguousarray(x, np.float32).reshape(-1, width)
        n = len(x)

        def alloc(shape, dt):
            return np.zeros(shape, dt)

        def addr(a):
            return a.ctypes.data

        def ok(a, size, dt):
            return isinstance(a, np.ndarray) and a.flags.c_contiguous and a.size == size and a.dtype == dt
    known = [f for f, _, _ in table]
    names = known if fields is None else list(fields)
    if any(f not in known for f in names):
        raise SptrError(f"{who}: fields must name some of {listing(known)} (got {names})")
    rows = (n,) if per_row is None else (n, per_row)
    res = {}
    for lead, (name, cols, dt) in [((n,), f) for f in always] + [(rows, f) for f in table if f[0] in names]:
        shape = lead + ((cols,) if cols > 1 else ())
        a = (out or {}).get(name)
        if a is None:
            a = alloc(shape, dt)
        elif not ok(a, int(np.prod(shape)), dt):
            of = f"{n} x {cols}" if per_row is None else f"{shape}"
            raise SptrError(f"{who}: out[{name!r}] must be contiguous, of {of} {np.dtype(dt).name}")
        res[name] = a
    return x, n, device, res, addr


def camera_lookat(pos=(0.0, 3.0, 8.0), target=(0.0, 1.0, 0.0), fov=60.0, aspect=800 / 600) -> Camera:
    """Camera(pos, target, +Y, fov, aspect) as src/main.cpp:97-103 sets it up."""
    L = lib()
    c = Camera()
    p = np.array(pos, np.float32)
    t = np.array(target, np.float32)
    rc = L.sptr_host_camera_lookat(_f(p), _f(t), C.c_float(fov), C.c_float(aspect), C.byref(c))
    if rc != 0:
        raise SptrError("camera_lookat failed")
    return c


def preset_materials(with_light: bool = False) -> list:
    L = lib()
    arr = (Material * 16)()
    n = L.sptr_host_preset_materials(1 if with_light else 0, arr, 16)
    return [arr[i] for i in range(n)]


def materials_as_array(mats) -> np.ndarray:
    """(n,12) float32: albedo3 metallic roughness emission3 ior type pad pad (oracle layout)."""
    out = np.zeros((len(mats), 12), np.float32)
    for i, m in enumerate(mats):
        out[i, 0:3] = list(m.albedo)
        out[i, 3] = m.metallic
        out[i, 4] = m.roughness
        out[i, 5:8] = list(m.emission)
        out[i, 8] = m.ior
        out[i, 9] = m.type
    return out


def default_lights() -> list:
    L = lib()
    arr = (Light * 8)()
    n = L.sptr_host_default_lights(arr, 8)
    return [arr[i] for i in range(n)]


def lights_as_array(lights) -> np.ndarray:
    out = np.zeros((len(lights), 8), np.float32)
    for i, l in enumerate(lights):
        out[i, 0] = l.type
        out[i, 1:4] = list(l.v)
        out[i, 4:7] = list(l.color)
        out[i, 7] = l.intensity
    return out


def equirect_to_faces(rgb: np.ndarray, size: int = 512) -> np.ndarray:
    L = lib()
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    faces = np.zeros((6, size, size, 3), np.float32)
    if L.sptr_host_equirect_to_faces(_f(rgb), w, h, size, _f(faces)) != 0:
        raise SptrError("equirect_to_faces failed")
    return faces


def tiles_per_rank(width: int, height: int, shard_count: int) -> int:
    ntiles = ((width + 31) // 32) * ((height + 31) // 32)
    return (ntiles + shard_count - 1) // shard_count


def pack_tiles(rgb: np.ndarray, shard_count: int, shard_rank: int) -> np.ndarray:
    """Host twin of the device tile packing: this shard's pixels as RGBA8 words, tile-packed and
    padded to tiles_per_rank tiles (the send buffer of the gather to rank 0)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    out = np.zeros(tiles_per_rank(w, h, shard_count) * 1024, np.uint32)
    if lib().sptr_host_pack_tiles(_b(rgb), w, h, shard_count, shard_rank, _u(out)) != 0:
        raise SptrError("pack_tiles failed")
    return out


def unpack_tiles(gathered: np.ndarray, shard_count: int, width: int, height: int) -> np.ndarray:
    g = np.ascontiguousarray(gathered, np.uint32)
    out = np.zeros((height, width, 3), np.uint8)
    if lib().sptr_host_unpack_tiles(_u(g), shard_count, tiles_per_rank(width, height, shard_count), width, height,
                                    _b(out)) != 0:
        raise SptrError("unpack_tiles failed")
    return out


def load_hdr(path: str) -> np.ndarray:
    L = lib()
    p = C.POINTER(C.c_float)()
    w, h = C.c_int32(), C.c_int32()
    if L.sptr_host_load_hdr(path.encode(), C.byref(p), C.byref(w), C.byref(h)) != 0:
        raise SptrError(f"cannot read {path}")
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        L.sptr_host_free(p)


# --------------------------------------------------------------------------------- device renderer
class Renderer:
    """One sptr context (one GPU).  Raises SptrError on any failure; never falls back to the CPU."""

    def __init__(self, device: int = 0):
        L = lib()
        self._L = L
        h = C.c_void_p()
        rc = L.sptr_create(device, C.byref(h))
        if rc != 0:
            raise SptrError(f"sptr_create(device={device}) failed ({rc}); a HIP GPU is required")
        self._h = h
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.sptr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._L.sptr_last_error(self._h)
            raise SptrError(f"{what}: rc={rc}: {msg.decode() if msg else ''}")

    def upload_scene(self, s: FlatScene):
        cs = s.to_c()
        self._check(self._L.sptr_upload_scene(self._h, C.byref(cs)), "upload_scene")

    def set_dynamic(self, on: bool = True, transforms: bool = False):
        """sptr_set_dynamic: the next upload_scene keeps what update_geometry's refit needs; with transforms
        (SPTR_DYNAMIC_TRANSFORMS) also the rest pose update_transforms moves, and it records its tree cost."""
        v = (SPTR_DYNAMIC_REFIT if on or transforms else 0) | (SPTR_DYNAMIC_TRANSFORMS if transforms else 0)
        self._check(self._L.sptr_set_dynamic(self._h, v), "set_dynamic")

    @staticmethod
    def _coord_args(what, arrays, device):
        """[(array or None, columns)] -> addresses, row counts and the host copies to keep alive."""
        ptr, cnt, keep = [None] * len(arrays), [0] * len(arrays), []
        for k, (a, cols) in enumerate(arrays):
            if a is None:
                continue
            if device:
                if a.numel() % cols or not a.is_contiguous() or a.element_size() != 4:
                    raise SptrError(f"{what}: device arrays must be contiguous float32")
                ptr[k], cnt[k] = C.c_void_p(a.data_ptr()), a.numel() // cols
            else:
                h = np.ascontiguousarray(a, np.float32).reshape(-1, cols)
                keep.append(h)
                ptr[k], cnt[k] = C.c_void_p(h.ctypes.data), len(h)
        return ptr, cnt, keep

    def update_geometry(self, positions=None, spheres=None, device: bool = False):
        """sptr_update_geometry: new coordinates for the uploaded topology, refitted in place.  positions
        (V, 3) and spheres (S, 4) float32, or None for unchanged; with device=True they are contiguous
        float32 tensors on this context's GPU (anything with data_ptr() and numel()).  Restart the
        accumulation (frame_begin=1) afterwards."""
        ptr, cnt, keep = self._coord_args("update_geometry", ((positions, 3), (spheres, 4)), device)
        self._check(self._L.sptr_update_geometry(self._h, ptr[0], cnt[0], ptr[1], cnt[1],
                                                 SPTR_UPDATE_DEVICE_PTRS if device else 0), "update_geometry")

    def set_rest_positions(self, positions, device: bool = False):
        """sptr_set_rest_positions: the vertices update_transforms moves, (V, 3) float32 (object space, in the
        upload's vertex order), instead of the uploaded positions."""
        ptr, cnt, keep = self._coord_args("set_rest_positions", ((positions, 3),), device)
        self._check(self._L.sptr_set_rest_positions(self._h, ptr[0], cnt[0], SPTR_UPDATE_DEVICE_PTRS if device else 0),
                    "set_rest_positions")

    def update_transforms(self, xforms=None, spheres=None, device: bool = False):
        """sptr_update_transforms: one glm-layout mat4 per triangle geometry, (G, 4, 4) float32 with
        xforms[g][col][row], applied to the rest pose on the device, and / or new spheres (S, 4); None for
        unchanged.  Needs set_dynamic(transforms=True) before the upload.  Restart the accumulation afterwards."""
        ptr, cnt, keep = self._coord_args("update_transforms", ((xforms, 16), (spheres, 4)), device)
        self._check(self._L.sptr_update_transforms(self._h, ptr[0], cnt[0], ptr[1], cnt[1],
                                                   SPTR_UPDATE_DEVICE_PTRS if device else 0), "update_transforms")

    def tree_cost(self) -> dict:
        """sptr_tree_cost: the BVH2's cost (sum of weight x child box area) and root area now, and as the upload
        recorded them (0 without set_dynamic(transforms=True))."""
        v = [C.c_double() for _ in range(4)]
        self._check(self._L.sptr_tree_cost(self._h, *[C.byref(d) for d in v]), "tree_cost")
        return dict(zip(("cost", "root_area", "cost_at_upload", "root_area_at_upload"), (d.value for d in v)))

    def refit_info(self) -> dict:
        """Refits since the upload, wall / device ms of the last one, and the triangles left out of the tree
        because they were exactly degenerate at upload."""
        n, ex = C.c_uint32(), C.c_uint32()
        w, d = C.c_double(), C.c_double()
        self._check(self._L.sptr_refit_info(self._h, C.byref(n), C.byref(w), C.byref(d), C.byref(ex)), "refit_info")
        return {"refits": n.value, "ms_wall": w.value, "ms_device": d.value, "excluded_prims": ex.value}

    def scene_info(self) -> dict:
        n, nn, dep = C.c_uint32(), C.c_uint32(), C.c_uint32()
        ms = C.c_double()
        self._check(self._L.sptr_scene_info(self._h, C.byref(n), C.byref(nn), C.byref(dep), C.byref(ms)), "info")
        return {"prims": n.value, "nodes": nn.value, "depth": dep.value, "build_ms": ms.value}

    def scene_layout(self) -> dict:
        lay = SceneLayout()
        self._check(self._L.sptr_scene_layout_info(self._h, C.byref(lay)), "scene_layout")
        return lay.as_dict()

    def set_materials(self, mats):
        arr = (Material * len(mats))(*mats)
        self._check(self._L.sptr_set_materials(self._h, arr, len(mats)), "set_materials")

    def set_lights(self, lights):
        arr = (Light * max(1, len(lights)))(*lights)
        self._check(self._L.sptr_set_lights(self._h, arr, len(lights)), "set_lights")

    def set_environment(self, faces: np.ndarray | None = None, intensity: float = 0.8, max_clamp: float = 5.0):
        e = Environment()
        if faces is not None:
            self._env_keep = np.ascontiguousarray(faces, np.float32)
            e.faces = _f(self._env_keep)
            e.size = self._env_keep.shape[1]
        e.intensity = intensity
        e.max_clamp = max_clamp
        self._check(self._L.sptr_set_environment(self._h, C.byref(e)), "set_environment")

    def set_wave_paths(self, n: int):
        self._check(self._L.sptr_set_wave_paths(self._h, n), "set_wave_paths")

    def graph_info(self) -> dict:
        """sptr_graph_info: the held launch graph (valid, nodes, edges, longest-path depth)."""
        v = [C.c_uint32() for _ in range(5)] + [C.c_int32()]
        self._check(self._L.sptr_graph_info(self._h, *[C.byref(x) for x in v]), "graph_info")
        d = dict(zip(("valid", "nodes", "edges", "depth", "captures", "capture_status"), (int(x.value) for x in v)))
        d["capture_error"] = self._L.sptr_capture_error(self._h).decode()
        return d

    def overlap_probe(self) -> dict:
        """sptr_overlap_probe: ms of two 200-us spins serial, and beside each side stream."""
        ms = (C.c_double * 3)()
        self._check(self._L.sptr_overlap_probe(self._h, ms), "overlap_probe")
        return {"serial_ms": round(ms[0], 4), "side_ms": round(ms[1], 4), "sky_side_ms": round(ms[2], 4),
                "side_has_own_queue": bool(ms[1] < 0.75 * ms[0]), "sky_side_has_own_queue": bool(ms[2] < 0.75 * ms[0])}

    def set_launch_mode(self, mode: int):
        """0: replay captured launch graphs for large repeated call shapes that fork nothing (default);
        1: direct launches; 2: direct launches, all on the render stream (no overlap); 3: launch graphs
        for every repeated shape."""
        self._check(self._L.sptr_set_launch_mode(self._h, mode), "set_launch_mode")

    def set_pixel_lanes(self, lanes: int):
        """0: automatic (two lanes for large calls on LDS-staged scenes); 1: one launch chain; 2: the
        shard's even and odd tiles as two concurrent launch chains (include/sptr_hip.h)."""
        self._check(self._L.sptr_set_pixel_lanes(self._h, lanes), "set_pixel_lanes")

    def pixel_lanes_info(self) -> dict:
        """{"requested": 0/1/2, "active": whether the current accumulation runs in two lanes}."""
        r, a = C.c_uint32(), C.c_uint32()
        self._check(self._L.sptr_pixel_lanes_info(self._h, C.byref(r), C.byref(a)), "pixel_lanes_info")
        return {"requested": r.value, "active": bool(a.value)}

    def set_tail_depth(self, n: int):
        self._check(self._L.sptr_set_tail_depth(self._h, n), "set_tail_depth")

    def set_bounce_chain(self, mode: int):
        """0 automatic, 1 off (one launch per bounce), 2 on wherever applicable (sptr_set_bounce_chain)."""
        self._check(self._L.sptr_set_bounce_chain(self._h, mode), "set_bounce_chain")

    def set_sky_split(self, mode: int, bulk_threads: int = 0):
        """0 automatic, 1 off, 2 on wherever a lane-group bounce 0 has a cull mask; bulk_threads 0 = automatic
        (sptr_set_sky_split)."""
        self._check(self._L.sptr_set_sky_split(self._h, mode, bulk_threads), "set_sky_split")

    def sky_split_info(self) -> dict:
        """{"bulk_threads": of the last wavefront call's first batch, 0 if it did not split}."""
        t = C.c_uint32()
        self._check(self._L.sptr_sky_split_info(self._h, C.byref(t)), "sky_split_info")
        return {"bulk_threads": t.value}

    def set_shadow_entries(self, mode: int):
        """0 off, 1 automatic (the first table after an upload built by a call of at least 2^23 samples, a rebuild
        after a refit, transform update or light change by one of at least 2^27; a cached table always used), 2
        built by any wavefront call (sptr_set_shadow_entries)."""
        self._check(self._L.sptr_set_shadow_entries(self._h, mode), "set_shadow_entries")

    def shadow_entries_info(self) -> dict:
        """{"mode", "cells" per side, "bytes", "builds", "cells_below_root", "cells_unoccluded"}; cells 0: no
        current table (sptr_shadow_entries_info)."""
        i = ShadowEntriesInfo()
        self._check(self._L.sptr_shadow_entries_info(self._h, C.byref(i)), "shadow_entries_info")
        return {k: getattr(i, k) for k, _ in ShadowEntriesInfo._fields_}

    def set_leaf_size(self, n: int):
        self._check(self._L.sptr_set_leaf_size(self._h, n), "set_leaf_size")

    def set_tree_order(self, mode: int):
        """sptr_set_tree_order: 0 automatic (SAH order for LDS-staged scenes), 1 Morton; next upload."""
        self._check(self._L.sptr_set_tree_order(self._h, mode), "set_tree_order")

    def tree_info(self) -> dict:
        """sptr_tree_info: {"order": 0 SAH / 1 Morton, "fallback": why Morton (0: SAH in use), "depth",
        "num_leaves", "cost_sah", "cost_morton"} of the last upload."""
        t = TreeOrderInfo()
        self._check(self._L.sptr_tree_info(self._h, C.byref(t)), "tree_info")
        return {k: getattr(t, k) for k, _ in TreeOrderInfo._fields_}

    def set_split_refs(self, max_pieces: int):
        """sptr_set_split_refs: most references per split triangle (0 = default 1: none); next upload."""
        self._check(self._L.sptr_set_split_refs(self._h, max_pieces), "set_split_refs")

    def set_stragglers(self, lanes: int):
        """sptr_set_stragglers: hand a drained wave's rays off once at most `lanes` lanes still trace
        (0 = off, default 12); HBM-resident scenes only."""
        self._check(self._L.sptr_set_stragglers(self._h, lanes), "set_stragglers")

    def set_bvh_width(self, n: int):
        self._check(self._L.sptr_set_bvh_width(self._h, n), "set_bvh_width")

    def set_debug_mode(self, m: int):
        self._check(self._L.sptr_set_debug_mode(self._h, m), "set_debug_mode")

    def render(self, cam: Camera, width: int, height: int, spp: int = 1, frame_begin: int = 1,
               max_depth: int = 6, shard_rank: int = 0, shard_count: int = 1, flags: int = 0,
               stream: int | None = None, integrator: int = SPTR_INTEGRATOR_WAVEFRONT,
               samples_per_frame: int = 0) -> Stats:
        """spp = progressive frames; integrator / samples_per_frame as in include/sptr_hip.h."""
        f = Frame(width, height, cam, frame_begin, spp, max_depth, shard_rank, shard_count, flags, integrator,
                  samples_per_frame)
        st = Stats()
        self._check(self._L.sptr_render(self._h, C.byref(f), C.c_void_p(stream) if stream else None, C.byref(st)),
                    "render")
        self.width, self.height = width, height
        return st

    def collect_stats(self) -> Stats:
        """Wait for the SPTR_FRAME_ASYNC renders and return their summed stats."""
        st = Stats()
        self._check(self._L.sptr_collect_stats(self._h, C.byref(st)), "collect_stats")
        return st

    def read_rgb8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(self._L.sptr_read_rgb8(self._h, _b(out)), "read_rgb8")
        return out

    def read_rgb8_lagged(self, out: np.ndarray) -> bool:
        """After an asynchronous render: out <- the image of the previous such call (True), or False
        (out untouched) when there is none of this size yet.  out stays page-locked while in use."""
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == self.width * self.height * 3
        got = C.c_uint32()
        self._check(self._L.sptr_read_rgb8_lagged(self._h, _b(out), C.byref(got)), "read_rgb8_lagged")
        return bool(got.value)

    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 3), np.float32)
        self._check(self._L.sptr_read_accum(self._h, _f(out)), "read_accum")
        return out

    def set_denoise(self, iterations: int = 0, sigma_color: float = 0.0, sigma_depth: float = 0.0,
                    sigma_albedo: float = 0.0, normal_log2_power: int = 0):
        """sptr_set_denoise: iterations 0 = off, 1..5 = an edge-avoiding a-trous pass after every wavefront
        render call (read_rgb8 / read_rgb8_lagged then return the filtered image); a zero parameter takes
        its default (0.5, 0.05, 0.2, 6)."""
        p = DenoiseParams(iterations, sigma_color, sigma_depth, sigma_albedo, normal_log2_power)
        self._check(self._L.sptr_set_denoise(self._h, C.byref(p) if iterations else None), "set_denoise")

    def read_aov(self, kind: int) -> np.ndarray:
        """First-hit feature buffer of the last render call's camera and size: SPTR_AOV_ALBEDO / _NORMAL
        (H, W, 3) float32, SPTR_AOV_DEPTH (H, W) float32 (-1 on a miss), SPTR_AOV_ID (H, W, 2) uint32
        (geomID, primID; 0xFFFFFFFF on a miss), SPTR_AOV_UV (H, W, 2) float32 (query_rays' barycentrics; 0 on
        a sphere or a miss)."""
        shape, dt = {SPTR_AOV_ALBEDO: ((3,), np.float32), SPTR_AOV_NORMAL: ((3,), np.float32),
                     SPTR_AOV_DEPTH: ((), np.float32), SPTR_AOV_ID: ((2,), np.uint32),
                     SPTR_AOV_UV: ((2,), np.float32)}[kind]
        out = np.zeros((self.height, self.width) + shape, dt)
        self._check(self._L.sptr_read_aov(self._h, kind, out.ctypes.data_as(C.c_void_p)), "read_aov")
        return out

    def read_denoised(self) -> np.ndarray:
        """The filter's output of the last render call, before the resolve: (H, W, 3) linear radiance."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        self._check(self._L.sptr_read_denoised(self._h, _f(out)), "read_denoised")
        return out

    def denoise_info(self) -> dict:
        """Device ms of the last denoise pass's AOV launch (0: cached) and filter launches; AOV passes so far."""
        a, f, n = C.c_double(), C.c_double(), C.c_uint32()
        self._check(self._L.sptr_denoise_info(self._h, C.byref(a), C.byref(f), C.byref(n)), "denoise_info")
        return {"ms_aov": a.value, "ms_filter": f.value, "aov_passes": n.value}

    def set_seed_offset(self, offset: int = 0):
        """sptr_set_seed_offset: wavefront calls seed their frames as accumulation index frame_begin + offset."""
        self._check(self._L.sptr_set_seed_offset(self._h, offset), "set_seed_offset")

    def set_denoise_history(self, max_history: int = 0, reserved=(0, 0, 0)):
        """sptr_set_denoise_history: 0 = off, else the cap on a pixel's history length in frames (at most
        1024); while the denoiser is on, its passes carry the integrated image across restarts of the
        accumulation (camera moves).  Any call drops the history held."""
        p = HistoryParams(max_history, (C.c_uint32 * 3)(*reserved))
        self._check(self._L.sptr_set_denoise_history(self._h, C.byref(p) if (max_history or any(reserved)) else None),
                    "set_denoise_history")

    def read_history(self) -> np.ndarray:
        """The last pass's integrated colour t_0 and history length m': (H, W, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.sptr_read_history(self._h, _f(out)), "read_history")
        return out

    def history_info(self) -> dict:
        """Of the last pass: pixels that took history, device ms of the reprojection launch, whether it had a carry."""
        n, ms, k = C.c_uint32(), C.c_double(), C.c_uint32()
        self._check(self._L.sptr_history_info(self._h, C.byref(n), C.byref(ms), C.byref(k)), "history_info")
        return {"reprojected": n.value, "ms_reproject": ms.value, "carried": bool(k.value)}

    def set_history_motion(self, on: bool = True):
        """sptr_set_history_motion: update_geometry keeps the denoiser's history, which the next pass reads
        through a snapshot of the geometry it saw (motion vectors).  Any call drops the history held."""
        self._check(self._L.sptr_set_history_motion(self._h, 1 if on else 0), "set_history_motion")

    def read_motion(self) -> np.ndarray:
        """The last motion pass's vectors: (H, W, 2) float32, where the pixel's surface point was in the carry's
        image relative to the pixel; NaN where the projection is not reached (a miss)."""
        out = np.zeros((self.height, self.width, 2), np.float32)
        self._check(self._L.sptr_read_motion(self._h, _f(out)), "read_motion")
        return out

    def motion_info(self) -> dict:
        """Snapshots since the upload, device ms of the last one, whether the last pass took the motion path."""
        n, ms, k = C.c_uint32(), C.c_double(), C.c_uint32()
        self._check(self._L.sptr_motion_info(self._h, C.byref(n), C.byref(ms), C.byref(k)), "motion_info")
        return {"snapshots": n.value, "ms_snapshot": ms.value, "used": bool(k.value)}

    def tiles_device(self) -> tuple[int, int]:
        p = C.c_void_p()
        n = C.c_size_t()
        self._check(self._L.sptr_tiles_device(self._h, C.byref(p), C.byref(n)), "tiles_device")
        return p.value, n.value

    def unpack_tiles(self, gathered_ptr: int, shard_count: int, tiles_per_rank: int, width: int, height: int,
                     out_ptr: int, stream: int | None = None):
        self._check(self._L.sptr_unpack_tiles(self._h, C.c_void_p(gathered_ptr), shard_count, tiles_per_rank, width,
                                              height, C.c_void_p(out_ptr),
                                              C.c_void_p(stream) if stream else None), "unpack_tiles")

    def intersect(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        geom = np.zeros(n, np.uint32)
        prim = np.zeros(n, np.uint32)
        t = np.zeros(n, np.float32)
        ng = np.zeros((n, 3), np.float32)
        self._check(self._L.sptr_intersect(self._h, _f(rays), n, _u(geom), _u(prim), _f(t), _f(ng)), "intersect")
        return geom, prim, t, ng

    def occluded(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(len(rays), np.uint8)
        self._check(self._L.sptr_occluded(self._h, _f(rays), len(rays), _b(out)), "occluded")
        return out

    def _query_call(self, who: str, q, flags: int, sort, stream, x, n: int, device: bool, res: dict, addr) -> dict:
        """The call of a query method after _query_arrays: the input, n and the flags go into q (a SignedQuery holds
        them in its PointQuery), the outputs' addresses into the members of their names."""
        head = q.q if isinstance(q, SignedQuery) else q
        put = _signed_query_set if isinstance(q, SignedQuery) else setattr
        setattr(head, "points" if isinstance(head, PointQuery) else "rays", addr(x) if n else None)
        head.n = n
        head.flags = flags | _query_flags(sort, device)
        for name, a in res.items():  # (an empty tensor has no address: n == 0 writes nothing, any non-NULL will do)
            put(q, name, addr(a) or (C.addressof(_QUERY_EMPTY) if n == 0 else None))
        if device and stream is None and n:
            import torch

            torch.cuda.current_stream(x.device).synchronize()  # the input's (and the outputs') producers
        self._check(getattr(self._L, "sptr_" + who)(self._h, C.byref(q), C.c_void_p(stream) if stream else None), who)
        return res

    def query_rays(self, rays, any_hit: bool = False, sort: bool | None = None, uv: bool = True,
                   stream: int | None = None, fields=None, out: dict | None = None) -> dict:
        """sptr_query_rays: closest-hit (or, with any_hit, occlusion) queries for n rays of 8 floats (o3, d3,
        tnear, tfar), walked by the render kernels' traversal.

        A numpy (n, 8) array takes the host path and returns numpy arrays.  A contiguous float32 tensor on
        this context's GPU (anything with data_ptr() and numel(); 16-byte aligned) takes the device path and
        returns torch tensors allocated on that device; nothing crosses the host.  The result is a dict with
        geom, prim (n, uint32; 0xFFFFFFFF on a miss), t (n; +inf on a miss), ng (n, 3) and uv (n, 2; the
        barycentrics of a triangle hit, include/sptr_hip.h), or with occluded (n, uint8).
        sort: None lets the library decide, True / False force SPTR_QUERY_SORT / SPTR_QUERY_NO_SORT (the
        results do not depend on it).  uv=False leaves the barycentrics out; fields names the outputs wanted
        (a subset of geom, prim, t, ng, uv), the others are not computed.  out: preallocated contiguous arrays
        (host path) or tensors (device path) to write into, by name.
        stream: a hipStream_t handle (device path only): the query is only enqueued there and the returned
        tensors are valid once that stream is synchronised; the caller orders the stream after the rays'
        producer.  Without it a device-path call waits for torch's current stream first, runs on the
        context's stream and returns when the results are written."""
        if any_hit:
            table, fields = (("occluded", 1, np.uint8),), None
        else:
            table = _QUERY_FIELDS
            fields = [f for f, _, _ in table if uv or f != "uv"] if fields is None else list(fields)
        arrays = _query_arrays(rays, 8, "query_rays", table, fields, out, stream)
        if not arrays[3]:
            raise SptrError(f"query_rays: fields must name some of geom, prim, t, ng, uv (got {fields})")
        return self._query_call("query_rays", RayQuery(), SPTR_QUERY_ANY_HIT if any_hit else 0, sort, stream, *arrays)

    def query_info(self) -> dict:
        """sptr_query_info: waits for the last query; device ms of its sort phase (0 when unsorted) and of its
        trace launch, whether it was sorted (0 / 1), and the queries launched so far."""
        s, t = C.c_double(), C.c_double()
        so, n = C.c_uint32(), C.c_uint32()
        self._check(self._L.sptr_query_info(self._h, C.byref(s), C.byref(t), C.byref(so), C.byref(n)), "query_info")
        return {"ms_sort": s.value, "ms_trace": t.value, "sorted": so.value, "queries": n.value}

    def query_multi_hit(self, rays, max_hits: int, sort: bool | None = None, fields=None, out: dict | None = None,
                        stream: int | None = None) -> dict:
        """sptr_query_multi_hit: per ray the max_hits = K nearest hits in ascending (t, geomID, primID)
        (include/sptr_hip.h states which hits a primitive gives).  rays, sort, out and stream are query_rays'.

        The result is a dict with count (n, uint32: the hits found, at most K) and the per-hit arrays named by
        fields (default: all of geom, prim, t, ng, uv), shaped (n, K), (n, K, 3) for ng and (n, K, 2) for uv;
        slots at and beyond a ray's count hold 0xFFFFFFFF ids, t = +inf and zeros.  numpy in, numpy out; device
        tensors in, torch tensors out."""
        K = int(max_hits)
        arrays = _query_arrays(rays, 8, "query_multi_hit", _QUERY_FIELDS, fields, out, stream, per_row=max(K, 0),
                               always=(("count", 1, np.uint32),))
        q = MultiHitQuery()
        q.max_hits = K if 0 <= K < 2 ** 32 else 0
        return self._query_call("query_multi_hit", q, 0, sort, stream, *arrays)

    def multi_hit_info(self) -> dict:
        """sptr_multi_hit_info: waits for the last multi-hit query; query_info's values for it, and the list
        capacity and LDS bytes per block of the kernel instantiation it launched."""
        s, t = C.c_double(), C.c_double()
        so, n, cap, lds = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._L.sptr_multi_hit_info(self._h, C.byref(s), C.byref(t), C.byref(so), C.byref(n), C.byref(cap),
                                                C.byref(lds)), "multi_hit_info")
        return {"ms_sort": s.value, "ms_trace": t.value, "sorted": so.value, "queries": n.value,
                "list_capacity": cap.value, "lds_bytes": lds.value}

    def query_points(self, points, sort: bool | None = None, fields=None, out: dict | None = None,
                     stream: int | None = None, count: bool = False) -> dict:
        """sptr_query_points: per point (p.xyz, max_dist) the nearest surface point within max_dist
        (include/sptr_hip.h states the definition).  points, sort, out and stream follow query_rays' conventions
        with n x 4 floats per point.

        The result is a dict with the arrays named by fields (default: all of geom, prim, dist2, dist, point, uv,
        ng): geom, prim (n, uint32; 0xFFFFFFFF on a miss), dist2, dist (n; +inf on a miss), point (n, 3), uv (n, 2),
        ng (n, 3).  numpy in, numpy out; device tensors in, torch tensors out.  count=True (SPTR_POINT_COUNT) makes
        the kernel count node visits and primitive tests for point_query_info()."""
        arrays = _query_arrays(points, 4, "query_points", _POINT_FIELDS, fields, out, stream)
        return self._query_call("query_points", PointQuery(), SPTR_POINT_COUNT if count else 0, sort, stream, *arrays)

    def set_signed_distance(self, on: bool = True) -> None:
        """sptr_set_signed_distance: the next upload keeps the triangles' corners and builds the pseudonormal tables
        query_signed_distance needs; update_geometry and update_transforms rebuild them."""
        self._check(self._L.sptr_set_signed_distance(self._h, 1 if on else 0), "set_signed_distance")

    def query_signed_distance(self, points, sort: bool | None = None, fields=None, out: dict | None = None,
                              stream: int | None = None, count: bool = False, flip_triangles: bool = False) -> dict:
        """sptr_query_signed_distance: query_points (same conventions, same fields) and, per point, signed_dist (n;
        negative on the side the normals point away from, +inf on a miss), normal (n, 3: the pseudonormal N of the
        closest feature, unnormalised) and feature (n, uint32: 0 face, 1-3 edge, 4-6 vertex, 7 sphere, 0xFFFFFFFF
        miss).  flip_triangles (SPTR_SIGNED_FLIP_TRIANGLES) negates the sign of triangle results, for meshes whose
        stored normals point inward.  The scene must have been uploaded after set_signed_distance()."""
        arrays = _query_arrays(points, 4, "query_signed_distance", _POINT_FIELDS + _SIGNED_FIELDS, fields, out, stream)
        flags = (SPTR_POINT_COUNT if count else 0) | (SPTR_SIGNED_FLIP_TRIANGLES if flip_triangles else 0)
        return self._query_call("query_signed_distance", SignedQuery(), flags, sort, stream, *arrays)

    def signed_info(self) -> dict:
        """sptr_signed_info: the table's counts (welded vertices, edges, open and irregular edges), its bytes, the
        builds so far, whether the current scene has tables, and the device ms of the last build and of the last
        sign pass (waits for it)."""
        s = SignedInfo()
        self._check(self._L.sptr_signed_info(self._h, C.byref(s)), "signed_info")
        return {k: getattr(s, k) for k, _ in SignedInfo._fields_ if k != "pad"}

    def read_pseudonormals(self) -> dict:
        """sptr_read_pseudonormals: N_v and N_e of the uploaded scene's triangles, (num_tris, 3, 3) float32 each
        (corner k, edge k)."""
        num_tris = self.signed_info()["num_tris"]
        nv, ne = np.zeros((num_tris, 3, 3), np.float32), np.zeros((num_tris, 3, 3), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._L.sptr_read_pseudonormals(self._h, nv.ctypes.data_as(fp), ne.ctypes.data_as(fp)),
                    "read_pseudonormals")
        return {"nv": nv, "ne": ne}

    def point_query_info(self) -> dict:
        """sptr_point_query_info: waits for the last point query; device ms of its sort phase and walk, whether it
        was sorted, the point queries so far, and the node visits and primitive tests of a count=True query."""
        s, t = C.c_double(), C.c_double()
        so, n = C.c_uint32(), C.c_uint32()
        nv, nt = C.c_uint64(), C.c_uint64()
        self._check(self._L.sptr_point_query_info(self._h, C.byref(s), C.byref(t), C.byref(so), C.byref(n), C.byref(nv),
                                                  C.byref(nt)), "point_query_info")
        return {"ms_sort": s.value, "ms_walk": t.value, "sorted": so.value, "queries": n.value,
                "node_visits": nv.value, "prim_tests": nt.value}

    def render_rays(self, rays, seeds=None, samples: int = 1, frame_index: int = 1, max_depth: int = 6,
                    accumulate: bool = False, normalize: bool = False, out=None, stream: int | None = None):
        """sptr_render_rays: the wavefront integrator's radiance along n caller-supplied rays of 8 floats (o3, unit
        d3, two ignored words): (n, 3) float32, per ray the sum of `samples` paths (divide for the mean).

        A numpy (n, 8) array takes the host path and returns a numpy array.  A contiguous float32 tensor on this
        context's GPU (16-byte aligned) takes the device path and returns a torch tensor on that device; seeds and
        out are then tensors there too.  seeds: n uint32 (numpy) or a 4-byte integer tensor, or None; the rng
        state of sample s of ray i is seeds[i] itself when samples == 1, else the wavefront raygen's state for
        pixel seed seeds[i] (or i without seeds) in frame frame_index + s (include/sptr_hip.h).
        accumulate adds to out (which must then be given) instead of storing; normalize applies the shading's
        safe_normalize to the directions first.  out: a preallocated contiguous (n, 3) float32 array / tensor.
        stream: a hipStream_t handle (device path only): the context's stream waits for that stream, and that
        stream for the result; nothing waits on the host.  Without it a device-path call waits for torch's
        current stream first and returns when the result is written."""
        device = hasattr(rays, "data_ptr")
        if device:
            import torch

            if rays.element_size() != 4 or not rays.is_floating_point() or not rays.is_contiguous() or rays.numel() % 8:
                raise SptrError("render_rays: device rays must be a contiguous float32 tensor of n x 8")
            n = rays.numel() // 8
            if seeds is not None and (not hasattr(seeds, "data_ptr") or seeds.element_size() != 4 or seeds.is_floating_point()
                                      or not seeds.is_contiguous() or seeds.numel() != n or seeds.device != rays.device):
                raise SptrError(f"render_rays: device seeds must be a contiguous 4-byte integer tensor of {n} on the rays' device")
            if out is None:
                out = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
            elif not (hasattr(out, "data_ptr") and out.is_contiguous() and out.numel() == n * 3
                      and out.dtype == torch.float32 and out.device == rays.device):
                raise SptrError(f"render_rays: out must be a contiguous float32 tensor of {n} x 3 on the rays' device")

            def addr(a):
                return a.data_ptr()
        else:
            if stream is not None:
                raise SptrError("render_rays: a stream needs device tensors")
            rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
            n = len(rays)
            if seeds is not None:
                seeds = np.ascontiguousarray(seeds, np.uint32).ravel()
                if len(seeds) != n:
                    raise SptrError(f"render_rays: seeds must hold {n} words")
            if out is None:
                out = np.zeros((n, 3), np.float32)
            elif not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.size == n * 3 and out.dtype == np.float32):
                raise SptrError(f"render_rays: out must be a contiguous float32 array of {n} x 3")

            def addr(a):
                return a.ctypes.data
        q = RayRender()
        q.rays = addr(rays) if n else None
        q.seeds = addr(seeds) if (seeds is not None and n) else None
        q.n = n
        q.samples = samples
        q.frame_index = frame_index
        q.max_depth = max_depth
        q.flags = ((SPTR_RAYS_DEVICE_PTRS if device else 0) | (SPTR_RAYS_ACCUMULATE if accumulate else 0)
                   | (SPTR_RAYS_NORMALIZE if normalize else 0))
        q.radiance = addr(out) if n else None
        if device and stream is None and n:
            torch.cuda.current_stream(rays.device).synchronize()  # the rays' (and the output's) producers
        self._check(self._L.sptr_render_rays(self._h, C.byref(q), C.c_void_p(stream) if stream else None), "render_rays")
        return out

    def ray_render_info(self) -> dict:
        """sptr_ray_render_info: waits for the last render_rays call; its device ms, its closest-hit and any-hit
        query counts and the chunks it ran in."""
        ms, c, s, k = C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self._L.sptr_ray_render_info(self._h, C.byref(ms), C.byref(c), C.byref(s), C.byref(k)), "ray_render_info")
        return {"ms": ms.value, "closest": c.value, "shadow": s.value, "chunks": k.value}

    def render_adaptive(self, cam: Camera, width: int, height: int, threshold: float, min_samples: int,
                        max_samples: int, step: int, max_depth: int = 6, cont: bool = False, shard=(0, 1),
                        frame_flags: int = 0, flags: int | None = None, reserved=(0, 0, 0),
                        integrator: int = SPTR_INTEGRATOR_WAVEFRONT, frame_begin: int = 1) -> dict:
        """sptr_render_adaptive: sample every pixel until its half-buffer error falls below threshold (at least
        min_samples, at most max_samples, step more per pass); cont goes on from the last adaptive call's state.
        Returns sptr_adaptive_info's fields.  The image, accumulation and counts are read with read_rgb8,
        read_accum and read_sample_counts.  (flags, reserved, integrator, frame_begin: as the C structs take
        them, for the error cases.)"""
        f = Frame(width, height, cam, frame_begin, 1, max_depth, shard[0], shard[1], frame_flags, integrator, 0)
        p = AdaptiveParams(threshold, min_samples, max_samples, step,
                           (SPTR_ADAPTIVE_CONTINUE if cont else 0) if flags is None else flags,
                           (C.c_uint32 * 3)(*reserved))
        info = AdaptiveInfo()
        self._check(self._L.sptr_render_adaptive(self._h, C.byref(f), C.byref(p), C.byref(info)), "render_adaptive")
        self.width, self.height = width, height
        return {k: getattr(info, k) for k, _ in AdaptiveInfo._fields_ if k != "reserved"}

    def read_sample_counts(self) -> np.ndarray:
        """(H, W) uint32: the samples every pixel of the last adaptive call's image holds (other shards' 0)."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.sptr_read_sample_counts(self._h, _u(out)), "read_sample_counts")
        return out

    def primary_rays(self, cam: Camera, width: int, height: int, acc: int):
        dirs = np.zeros((height, width, 3), np.float32)
        rng = np.zeros((height, width), np.uint32)
        self._check(self._L.sptr_primary_rays(self._h, C.byref(cam), width, height, acc, _f(dirs), _u(rng)),
                    "primary_rays")
        return dirs, rng

    def sort_pairs_u64(self, keys: np.ndarray, vals: np.ndarray):
        """The LBVH build's stable device radix sort (kernels_sort.hip): (keys, vals) sorted by key."""
        k = np.ascontiguousarray(keys, np.uint64)
        v = np.ascontiguousarray(vals, np.uint32)
        assert k.shape == v.shape and k.ndim == 1
        ko, vo = np.empty_like(k), np.empty_like(v)
        u64p = C.POINTER(C.c_uint64)
        self._check(self._L.sptr_sort_pairs_u64(self._h, k.ctypes.data_as(u64p), _u(v), len(k),
                                                ko.ctypes.data_as(u64p), _u(vo)), "sort_pairs_u64")
        return ko, vo

    def cosine_sincos_table(self) -> np.ndarray:
        """(sin, cos) of the cosine sample's phi for every r1 = k / 2^24, as the device computes them:
        (2^24, 2) float32 (sptr_eval_math, fn 0)."""
        out = np.empty((1 << 24, 2), np.float32)
        self._check(self._L.sptr_eval_math(self._h, 0, None, 0, _f(out)), "eval_math")
        return out

    def gamma_pow(self, x: np.ndarray) -> np.ndarray:
        """powf(x, 1/2.2) as the device's resolve computes it (sptr_eval_math, fn 1)."""
        a = np.ascontiguousarray(x, np.float32).ravel()
        out = np.empty_like(a)
        self._check(self._L.sptr_eval_math(self._h, 1, _f(a), len(a), _f(out)), "eval_math")
        return out.reshape(np.shape(x))

    def scan_u32(self, counts: np.ndarray) -> np.ndarray:
        """The LBVH build's device exclusive prefix sum of u32 counts (mod 2^32)."""
        a = np.ascontiguousarray(counts, np.uint32)
        out = np.empty_like(a)
        self._check(self._L.sptr_scan_u32(self._h, _u(a), len(a), _u(out)), "scan_u32")
        return out


def setup_default(r: Renderer, scene: str = "default", p0: int = 0, p1: int = 0, env_faces=None) -> FlatScene:
    """Upload a builtin scene with the reference's default state (presets, one sun, sky)."""
    s = builtin_scene(scene, p0, p1)
    r.upload_scene(s)
    r.set_materials(preset_materials(with_light=(scene == "default_emitter")))
    r.set_lights(default_lights())
    r.set_environment(env_faces)
    return s
