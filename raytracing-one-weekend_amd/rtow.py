"""ctypes view of the C-ABI in include/rtow.h (librtow.so).

Plumbing only: it mirrors the structs, loads the in-tree shared library and adds
thin helpers for device buffers (torch is used for device memory, streams and
torch.distributed — not for any of the rendering arithmetic).

There is no CPU fallback here by design: if librtow.so is missing or no HIP
device is usable the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
LIB_PATH = Path(os.environ.get("RTOW_LIB", PKG_DIR / "librtow.so"))  # RTOW_LIB: A/B against another build

RTOW_ABI_VERSION = 9
RTOW_OK, RTOW_EINVAL, RTOW_ENODEV, RTOW_EHIP, RTOW_ENOSCENE, RTOW_EEMPTY, RTOW_ENOMEM = 0, -1, -2, -3, -4, -5, -6
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2
PRIM_SPHERE, PRIM_MOVING_SPHERE, PRIM_TRIANGLE = 0, 1, 2
F64_STRICT, F64_FAST, F32 = 0, 1, 2
KERNEL_AUTO, KERNEL_BRUTE, KERNEL_BVH, KERNEL_GRID, KERNEL_BVH4, KERNEL_REFTREE = 0, 1, 2, 3, 4, 5
MAX_HITS = 8  # RTOW_MAX_HITS: the most entries rtow_first_hits keeps per ray
MAX_NEAREST = 8  # RTOW_MAX_NEAREST: the most entries rtow_nearest keeps per point
SPEC_GENERIC, SPEC_STATIC_SPHERES, SPEC_MOVING_SPHERES, SPEC_FLAT_Y = 0, 1, 2, 4  # Context.last_spec()
MODEL_OO, MODEL_VARIANT, MODEL_WORLD = 0, 1, 2  # scene models of the host scene scripts (include/rtow.h)
BUILDER_HOST_SAH, BUILDER_DEVICE_LBVH, BUILDER_AUTO = 0, 1, 2

d3 = C.c_double * 3
_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)


class Camera(C.Structure):
    _fields_ = [
        ("origin", d3), ("u", d3), ("v", d3), ("w", d3),
        ("horizontal", d3), ("vertical", d3), ("lower_left_corner", d3),
        ("lens_radius", C.c_double), ("t0", C.c_double), ("t1", C.c_double),
    ]


class Material(C.Structure):
    _fields_ = [
        ("albedo", d3), ("fuzz", C.c_double), ("ir", C.c_double),
        ("kind", C.c_int32), ("pad_", C.c_int32),
    ]


class Scene(C.Structure):
    _fields_ = [
        ("camera", Camera),
        ("n_spheres", C.c_int32), ("sphere_geom", _pd), ("sphere_mat", _pi),
        ("n_moving", C.c_int32), ("moving_geom", _pd), ("moving_mat", _pi),
        ("n_triangles", C.c_int32), ("triangle_geom", _pd), ("triangle_mat", _pi),
        ("n_materials", C.c_int32), ("materials", C.POINTER(Material)),
        ("n_prims", C.c_int32), ("prim_kind", _pi), ("prim_index", _pi),
    ]


class Config(C.Structure):
    _fields_ = [
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("samples_per_pixel", C.c_int32), ("nstreams", C.c_int32),
        ("max_child_rays", C.c_int32), ("precision", C.c_int32), ("kernel", C.c_int32),
        ("rank", C.c_int32), ("nranks", C.c_int32), ("tile_rows", C.c_int32),
        ("seed", C.c_uint64),
        ("stream_first", C.c_int32), ("stream_count", C.c_int32), ("accumulate", C.c_int32),
        ("pad_", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64), ("segments", C.c_uint64),
        ("prim_tests", C.c_uint64), ("node_tests", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double),
        ("local_rows", C.c_int32), ("kernel_used", C.c_int32),
    ]


class BuildInfo(C.Structure):
    _fields_ = [
        ("builder", C.c_int32), ("bvh_nodes", C.c_int32),
        ("bvh_image_bytes", C.c_int32), ("grid_image_bytes", C.c_int32),
        ("bvh_build_ms", C.c_double), ("grid_build_ms", C.c_double), ("upload_ms", C.c_double),
        ("bvh4_nodes", C.c_int32), ("bvh4_image_bytes", C.c_int32),
        ("ref_tree_nodes", C.c_int32), ("bvh4_node_bytes", C.c_int32),
        ("ref_tree_stupid_volume", C.c_double), ("ref_tree_build_ms", C.c_double),
    ]


class RefitInfo(C.Structure):
    """rtow_refit_info_t: the refits since the last upload."""
    _fields_ = [
        ("refits", C.c_int32), ("grid_resident", C.c_int32),
        ("refit_ms", C.c_double), ("device_ms", C.c_double), ("bvh_area_ratio", C.c_double),
    ]


class HostConfig(C.Structure):
    _fields_ = [
        ("number_of_balls_sqrt", C.c_int32), ("aspect_ratio", C.c_double),
        ("moving_spheres", C.c_int32),
    ]


class Ray(C.Structure):
    """rtow_ray_t (64 B): the closest hit in [0.001, tmax] is reported."""
    _fields_ = [("origin", d3), ("time", C.c_double), ("direction", d3), ("tmax", C.c_double)]


class Hit(C.Structure):
    """rtow_hit_t (72 B): t = inf and prim = kind = material = -1 on a miss."""
    _fields_ = [
        ("t", C.c_double), ("point", d3), ("normal", d3),
        ("prim", C.c_int32), ("kind", C.c_int32), ("material", C.c_int32), ("front_face", C.c_int32),
    ]


class PointQuery(C.Structure):
    """rtow_point_query_t (48 B): the nearest primitive is reported if its distance <= max_dist."""
    _fields_ = [("point", d3), ("time", C.c_double), ("max_dist", C.c_double), ("pad_", C.c_double)]


class PointHit(C.Structure):
    """rtow_point_hit_t (48 B): dist = inf and prim = kind = material = -1 on a miss."""
    _fields_ = [
        ("dist", C.c_double), ("point", d3),
        ("prim", C.c_int32), ("kind", C.c_int32), ("material", C.c_int32), ("pad_", C.c_int32),
    ]


class Guide(C.Structure):
    """rtow_guide_t (64 B): per-pixel SUMS over the pixel's samples of first-hit albedo, unit normal, distance, hits."""
    _fields_ = [("albedo", d3), ("normal", d3), ("depth", C.c_double), ("hits", C.c_double)]


class RadianceParams(C.Structure):
    """rtow_radiance_params_t (24 B): Philox key, samples per ray, depth, offset of every ray's first sample index."""
    _fields_ = [("seed", C.c_uint64), ("samples_per_ray", C.c_int32), ("max_child_rays", C.c_int32),
                ("sample_first", C.c_uint32), ("pad_", C.c_int32)]


class StepParams(C.Structure):
    """rtow_step_params_t (16 B): Philox key, the segment's index on its path, offset of every ray's sample index."""
    _fields_ = [("seed", C.c_uint64), ("bounce", C.c_int32), ("sample_first", C.c_uint32)]


# rtow_path_step*: what became of each ray (RTOW_STEP_* of include/rtow.h)
STEP_MISS, STEP_SCATTERED, STEP_ABSORBED, STEP_SKIPPED = 0, 1, 2, 3


class SurfacePoint(C.Structure):
    """rtow_surface_point_t (64 B, the layout of rtow_ray_t): occluders count within [0.001, max_dist] of the point."""
    _fields_ = [("point", d3), ("time", C.c_double), ("normal", d3), ("max_dist", C.c_double)]


class AmbientParams(C.Structure):
    """rtow_ambient_params_t (16 B): Philox key, samples per point, offset of every point's first sample index."""
    _fields_ = [("seed", C.c_uint64), ("samples", C.c_int32), ("sample_first", C.c_uint32)]


class Ambient(C.Structure):
    """rtow_ambient_t (64 B): SUMS over a point's unoccluded samples (count, directions, sky colour) and the samples taken."""
    _fields_ = [("open", C.c_double), ("bent", d3), ("sky", d3), ("samples", C.c_double)]


class SweepQuery(C.Structure):
    """rtow_sweep_t (80 B): a sphere of `radius` whose centre travels origin + direction * t, t in [0, tmax]."""
    _fields_ = [("origin", d3), ("time", C.c_double), ("direction", d3), ("tmax", C.c_double),
                ("radius", C.c_double), ("pad_", C.c_double)]


class SweepHit(C.Structure):
    """rtow_sweep_hit_t (80 B): t = dist = inf, centre = point = 0 and prim = kind = material = -1 on a miss."""
    _fields_ = [
        ("t", C.c_double), ("dist", C.c_double), ("centre", d3), ("point", d3),
        ("prim", C.c_int32), ("kind", C.c_int32), ("material", C.c_int32), ("start_overlap", C.c_int32),
    ]


MAX_OVERLAP_IDS = 8  # RTOW_MAX_OVERLAP_IDS: the most ids rtow_overlap returns per box and call
MAX_AMBIENT_SAMPLES = 65536  # RTOW_MAX_AMBIENT_SAMPLES: the most samples rtow_ambient takes per point


# numpy views of the same layouts (arrays of rays / hits for rtow_intersect*)
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("time", "<f8"), ("direction", "<f8", (3,)), ("tmax", "<f8")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("prim", "<i4"), ("kind", "<i4"),
                      ("material", "<i4"), ("front_face", "<i4")])

# rtow_guide_t (rtow_guides*): per-pixel SUMS over the pixel's samples
GUIDE_DTYPE = np.dtype([("albedo", "<f8", (3,)), ("normal", "<f8", (3,)), ("depth", "<f8"), ("hits", "<f8")])


# rtow_point_query_t / rtow_point_hit_t (rtow_closest_point*)
POINT_QUERY_DTYPE = np.dtype([("point", "<f8", (3,)), ("time", "<f8"), ("max_dist", "<f8"), ("pad_", "<f8")])
POINT_HIT_DTYPE = np.dtype([("dist", "<f8"), ("point", "<f8", (3,)), ("prim", "<i4"), ("kind", "<i4"),
                            ("material", "<i4"), ("pad_", "<i4")])


# rtow_surface_point_t / rtow_ambient_t (rtow_ambient*)
SURFACE_POINT_DTYPE = np.dtype([("point", "<f8", (3,)), ("time", "<f8"), ("normal", "<f8", (3,)), ("max_dist", "<f8")])
AMBIENT_DTYPE = np.dtype([("open", "<f8"), ("bent", "<f8", (3,)), ("sky", "<f8", (3,)), ("samples", "<f8")])


# rtow_sweep_t / rtow_sweep_hit_t (rtow_sweep*)
SWEEP_QUERY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("time", "<f8"), ("direction", "<f8", (3,)), ("tmax", "<f8"),
                              ("radius", "<f8"), ("pad_", "<f8")])
SWEEP_HIT_DTYPE = np.dtype([("t", "<f8"), ("dist", "<f8"), ("centre", "<f8", (3,)), ("point", "<f8", (3,)),
                            ("prim", "<i4"), ("kind", "<i4"), ("material", "<i4"), ("start_overlap", "<i4")])


def make_sweeps(origins, directions, radius, time=0.0, tmax=float("inf")):
    """A SWEEP_QUERY_DTYPE array from [n, 3] origins and directions (radius, time and tmax: scalars or [n])."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    q = np.empty(len(o), dtype=SWEEP_QUERY_DTYPE)
    q["origin"] = o
    q["direction"] = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    q["time"] = time
    q["tmax"] = tmax
    q["radius"] = radius
    q["pad_"] = 0.0
    return q


# rtow_box_query_t (rtow_overlap*)
BOX_QUERY_DTYPE = np.dtype([("lo", "<f8", (3,)), ("hi", "<f8", (3,)), ("time", "<f8"), ("min_prim", "<i4"), ("pad_", "<i4")])


def make_boxes(lo, hi, time=0.0, min_prim=0):
    """A BOX_QUERY_DTYPE array from [n, 3] lower and upper corners (time and min_prim: scalars or [n])."""
    l = np.asarray(lo, dtype=np.float64).reshape(-1, 3)
    q = np.empty(len(l), dtype=BOX_QUERY_DTYPE)
    q["lo"] = l
    q["hi"] = np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    q["time"] = time
    q["min_prim"] = min_prim
    q["pad_"] = 0
    return q


def make_surface_points(points, normals, time=0.0, max_dist=float("inf")):
    """A SURFACE_POINT_DTYPE array from [n, 3] points and normals (time and max_dist: scalars or [n])."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    q = np.empty(len(p), dtype=SURFACE_POINT_DTYPE)
    q["point"] = p
    q["normal"] = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    q["time"] = time
    q["max_dist"] = max_dist
    return q


def make_point_queries(points, time=0.0, max_dist=float("inf")):
    """A POINT_QUERY_DTYPE array from [n, 3] points (time and max_dist: scalars or [n])."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    q = np.empty(len(p), dtype=POINT_QUERY_DTYPE)
    q["point"] = p
    q["time"] = time
    q["max_dist"] = max_dist
    q["pad_"] = 0.0
    return q


def make_rays(origins, directions, time=0.0, tmax=float("inf")):
    """A RAY_DTYPE array from [n, 3] origins and directions (time and tmax: scalars or [n])."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    r = np.empty(len(o), dtype=RAY_DTYPE)
    r["origin"] = o
    r["direction"] = d
    r["time"] = time
    r["tmax"] = tmax
    return r


# every symbol include/rtow.h declares
EXPORTS = [
    "rtow_abi_version", "rtow_last_error", "rtow_ctx_create", "rtow_ctx_destroy",
    "rtow_scene_upload", "rtow_local_rows", "rtow_local_row_list", "rtow_render_device",
    "rtow_render", "rtow_host_scene_cover", "rtow_host_scene_obj", "rtow_host_scene_free",
    "rtow_host_rng_reset", "rtow_host_ppm", "rtow_host_free", "rtow_tonemap_device",
    "rtow_profile_collect", "rtow_debug_counters", "rtow_render_rgb8",
    "rtow_ctx_set_builder", "rtow_build_info", "rtow_debug_image", "rtow_render_multi",
    "rtow_debug_schedule", "rtow_host_scene_cover_model", "rtow_host_scene_obj_model",
    "rtow_multi_create", "rtow_multi_set_builder", "rtow_multi_upload", "rtow_multi_build_info",
    "rtow_multi_render", "rtow_multi_destroy", "rtow_host_reftree_info",
    "rtow_render_device_rgb8", "rtow_multi_render_rgb8", "rtow_multi_frame_breakdown",
    "rtow_intersect_device", "rtow_intersect", "rtow_occluded_device", "rtow_occluded",
    "rtow_scene_refit", "rtow_refit_info", "rtow_closest_point_device", "rtow_closest_point",
    "rtow_debug_tile_order", "rtow_radiance_device", "rtow_radiance",
    "rtow_camera_rays_device", "rtow_camera_rays", "rtow_camera_ray_count", "rtow_guides_device", "rtow_guides",
    "rtow_debug_last_spec", "rtow_first_hits_device", "rtow_first_hits", "rtow_nearest_device", "rtow_nearest",
    "rtow_debug_last_counted", "rtow_debug_walk_consts", "rtow_path_step_device", "rtow_path_step",
    "rtow_ambient_device", "rtow_ambient", "rtow_sweep_device", "rtow_sweep", "rtow_overlap_device", "rtow_overlap",
]
MULTI_BREAKDOWN = ("total", "handoff_enqueue", "place_enqueue", "wait_and_copy", "wait_only", "dev_trace", "dev_gather",
                   "dev_place_copy")  # RTOW_MB_* of include/rtow.h, milliseconds


class RtowError(RuntimeError):
    pass


_lib = None


def lib():
    """Load librtow.so (built in-tree by __graft_entry__.build / make)."""
    global _lib
    if _lib is not None:
        return _lib
    # Load-order guard: torch bundles its own copy of the HIP runtime, librtow.so links /opt/rocm's.  Both
    # live in one process whenever torch supplies device memory and streams (bench.py, some tests); that is
    # reliable when torch's libraries are mapped FIRST (bench.py's order) and was not the other way round
    # ("No HIP GPUs are available" / "no ROCm-capable device" from whichever runtime came second).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise RtowError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                        " (there is no CPU fallback)")
    L = C.CDLL(str(LIB_PATH))
    L.rtow_abi_version.restype = C.c_int
    L.rtow_last_error.restype = C.c_char_p
    L.rtow_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.rtow_ctx_destroy.argtypes = [C.c_void_p]
    L.rtow_ctx_destroy.restype = None
    L.rtow_scene_upload.argtypes = [C.c_void_p, C.POINTER(Scene)]
    L.rtow_local_rows.argtypes = [C.POINTER(Config)]
    L.rtow_local_row_list.argtypes = [C.POINTER(Config), _pi, C.c_int32]
    L.rtow_render_device.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.c_void_p,
                                     C.POINTER(Stats)]
    L.rtow_render.argtypes = [C.c_void_p, C.POINTER(Scene), C.POINTER(Config), _pd,
                              C.POINTER(Stats)]
    L.rtow_host_scene_cover.argtypes = [C.POINTER(HostConfig), C.POINTER(C.POINTER(Scene))]
    L.rtow_host_scene_obj.argtypes = [C.POINTER(HostConfig), C.c_char_p,
                                      C.POINTER(C.POINTER(Scene))]
    if hasattr(L, "rtow_host_scene_cover_model"):
        L.rtow_host_scene_cover_model.argtypes = [C.POINTER(HostConfig), C.c_int32, C.POINTER(C.POINTER(Scene))]
        L.rtow_host_scene_obj_model.argtypes = [C.POINTER(HostConfig), C.c_char_p, C.c_int32,
                                                C.POINTER(C.POINTER(Scene))]
    L.rtow_host_scene_free.argtypes = [C.POINTER(Scene)]
    L.rtow_host_scene_free.restype = None
    L.rtow_host_rng_reset.restype = None
    L.rtow_host_ppm.argtypes = [_pd, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p),
                                C.POINTER(C.c_uint64)]
    L.rtow_host_free.argtypes = [C.c_void_p]
    L.rtow_host_free.restype = None
    L.rtow_tonemap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.rtow_ctx_set_builder.argtypes = [C.c_void_p, C.c_int32]
    L.rtow_build_info.argtypes = [C.c_void_p, C.POINTER(BuildInfo)]
    L.rtow_render_multi.argtypes = [C.c_int32, _pi, C.POINTER(Scene), C.POINTER(Config), _pd, C.POINTER(Stats),
                                    C.c_int32]
    L.rtow_debug_image.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    if hasattr(L, "rtow_host_reftree_info"):
        L.rtow_host_reftree_info.argtypes = [C.POINTER(Scene), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double)]
    if hasattr(L, "rtow_multi_create"):
        L.rtow_multi_create.argtypes = [C.c_int32, _pi, C.c_int32, C.POINTER(C.c_void_p)]
        L.rtow_multi_set_builder.argtypes = [C.c_void_p, C.c_int32]
        L.rtow_multi_upload.argtypes = [C.c_void_p, C.POINTER(Scene)]
        L.rtow_multi_build_info.argtypes = [C.c_void_p, C.POINTER(BuildInfo)]
        L.rtow_multi_render.argtypes = [C.c_void_p, C.POINTER(Config), _pd, C.POINTER(Stats)]
        L.rtow_multi_destroy.argtypes = [C.c_void_p]
        L.rtow_multi_destroy.restype = None
    if hasattr(L, "rtow_multi_render_rgb8"):
        L.rtow_multi_render_rgb8.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.POINTER(Stats)]
        L.rtow_render_device_rgb8.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.rtow_render_rgb8.argtypes = [C.c_void_p, C.POINTER(Scene), C.POINTER(Config), C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_intersect"):
        L.rtow_intersect_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.POINTER(Stats)]
        L.rtow_intersect.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.POINTER(Stats)]
    if hasattr(L, "rtow_occluded"):
        L.rtow_occluded_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.POINTER(Stats)]
        L.rtow_occluded.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.POINTER(Stats)]
    if hasattr(L, "rtow_first_hits"):
        L.rtow_first_hits_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_first_hits.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_closest_point"):
        L.rtow_closest_point_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.POINTER(Stats)]
        L.rtow_closest_point.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.POINTER(Stats)]
    if hasattr(L, "rtow_nearest"):
        L.rtow_nearest_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_nearest.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_radiance"):
        L.rtow_radiance_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RadianceParams), C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_radiance.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RadianceParams), C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_path_step"):
        L.rtow_path_step_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(StepParams), C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(Stats)]
        L.rtow_path_step.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(StepParams), C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_ambient"):
        L.rtow_ambient_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AmbientParams), C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_ambient.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AmbientParams), C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_sweep"):
        L.rtow_sweep_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.POINTER(Stats)]
        L.rtow_sweep.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_overlap"):
        L.rtow_overlap_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_overlap.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_guides"):
        L.rtow_camera_rays_device.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtow_camera_rays.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.c_void_p]
        L.rtow_camera_ray_count.argtypes = [C.POINTER(Config)]
        L.rtow_camera_ray_count.restype = C.c_int64
        L.rtow_guides_device.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.rtow_guides.argtypes = [C.c_void_p, C.POINTER(Config), C.c_void_p, C.POINTER(Stats)]
    if hasattr(L, "rtow_scene_refit"):
        L.rtow_scene_refit.argtypes = [C.c_void_p, C.POINTER(Scene)]
        L.rtow_refit_info.argtypes = [C.c_void_p, C.POINTER(RefitInfo)]
    L.rtow_profile_collect.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    if hasattr(L, "rtow_debug_schedule"):  # (absent from older builds loaded through RTOW_LIB for A/B runs)
        L.rtow_debug_schedule.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(C.c_uint32), C.c_int32]
    if hasattr(L, "rtow_debug_tile_order"):
        L.rtow_debug_tile_order.argtypes = [C.POINTER(Scene), C.POINTER(Config), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_ubyte), C.c_int32, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(L, "rtow_debug_last_spec"):
        L.rtow_debug_last_spec.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "rtow_debug_last_counted"):
        L.rtow_debug_last_counted.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "rtow_debug_walk_consts"):
        L.rtow_debug_walk_consts.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    ver = L.rtow_abi_version()
    if ver != RTOW_ABI_VERSION and not ("RTOW_LIB" in os.environ and ver >= 4):  # (older builds: A/B runs only)
        raise RtowError("librtow.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int, what: str = "rtow"):
    if rc != 0:
        msg = lib().rtow_last_error()
        raise RtowError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def image_height(width: int, aspect_ratio: float) -> int:
    """int(image_width / aspect_ratio) — reference src/render.cpp:137."""
    return int(width / aspect_ratio)


def make_config(width, height, spp, nstreams=1, max_child_rays=50, seed=1, precision=F64_FAST,
                kernel=KERNEL_AUTO, rank=0, nranks=1, tile_rows=8, stream_first=0, stream_count=0,
                accumulate=0) -> Config:
    return Config(width, height, spp, nstreams, max_child_rays, precision, kernel, rank, nranks,
                  tile_rows, seed, stream_first, stream_count, accumulate, 0)


def spp_effective(cfg: Config) -> int:
    """samples_per_pixel / nthreads * nthreads — reference src/render.cpp:185."""
    return cfg.samples_per_pixel // cfg.nstreams * cfg.nstreams


def local_rows(cfg: Config):
    L = lib()
    n = L.rtow_local_rows(C.byref(cfg))
    if n < 0:
        check(n, "rtow_local_rows")
    buf = (C.c_int32 * max(n, 1))()
    got = L.rtow_local_row_list(C.byref(cfg), buf, n)
    if got < 0:
        check(got, "rtow_local_row_list")
    return list(buf[:n])


class HostScene:
    """A flattened scene built by the product's host-side scene scripts."""

    def __init__(self, ptr):
        self.ptr = ptr

    @property
    def c(self) -> Scene:
        return self.ptr.contents

    @classmethod
    def cover(cls, nsqrt=11, aspect=1.5, moving=False, reset_rng=True, model=MODEL_OO):
        """`model`: which of the reference's scene models the script builds (MODEL_OO / _VARIANT / _WORLD)."""
        L = lib()
        if reset_rng:
            L.rtow_host_rng_reset()
        hc = HostConfig(nsqrt, aspect, int(moving))
        out = C.POINTER(Scene)()
        if model == MODEL_OO:
            check(L.rtow_host_scene_cover(C.byref(hc), C.byref(out)), "rtow_host_scene_cover")
        else:
            check(L.rtow_host_scene_cover_model(C.byref(hc), model, C.byref(out)), "rtow_host_scene_cover_model")
        return cls(out)

    @classmethod
    def obj(cls, path, aspect=16.0 / 9.0, reset_rng=True, model=MODEL_OO):
        L = lib()
        if reset_rng:
            L.rtow_host_rng_reset()
        hc = HostConfig(0, aspect, 0)
        out = C.POINTER(Scene)()
        if model == MODEL_OO:
            check(L.rtow_host_scene_obj(C.byref(hc), str(path).encode(), C.byref(out)), "rtow_host_scene_obj")
        else:
            check(L.rtow_host_scene_obj_model(C.byref(hc), str(path).encode(), model, C.byref(out)),
                  "rtow_host_scene_obj_model")
        return cls(out)

    def close(self):
        if self.ptr:
            lib().rtow_host_scene_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ppm_text(rgb_sums, width, height, spp_eff) -> bytes:
    """write_color + P3 framing (reference src/render.cpp:11-20,182-186)."""
    import numpy as np

    a = np.ascontiguousarray(rgb_sums, dtype=np.float64)
    assert a.size == width * height * 3
    txt = C.c_char_p()
    n = C.c_uint64()
    L = lib()
    check(L.rtow_host_ppm(a.ctypes.data_as(_pd), width, height, spp_eff, C.byref(txt), C.byref(n)),
          "rtow_host_ppm")
    try:
        return C.string_at(txt, n.value)
    finally:
        L.rtow_host_free(txt)


class Context:
    """One HIP device (one process per GPU)."""

    def __init__(self, device_id: int = 0):
        self._h = C.c_void_p()
        check(lib().rtow_ctx_create(device_id, C.byref(self._h)), "rtow_ctx_create")
        self.device_id = device_id

    def upload(self, scene):
        s = scene.c if isinstance(scene, HostScene) else scene
        check(lib().rtow_scene_upload(self._h, C.byref(s)), "rtow_scene_upload")

    def refit(self, scene):
        """Replace the resident scene's geometry, materials and camera in place, keeping its trees' topology
        (rtow_scene_refit): same counts and insertion order as the uploaded scene."""
        s = scene.c if isinstance(scene, HostScene) else scene
        check(lib().rtow_scene_refit(self._h, C.byref(s)), "rtow_scene_refit")

    def refit_info(self) -> RefitInfo:
        """Refits since the last upload, the last one's host and device times, and the binary BVH's area ratio
        (rtow_refit_info; synchronises)."""
        ri = RefitInfo()
        check(lib().rtow_refit_info(self._h, C.byref(ri)), "rtow_refit_info")
        return ri

    def set_builder(self, builder: int):
        """BUILDER_AUTO (default of a new context), BUILDER_HOST_SAH or BUILDER_DEVICE_LBVH; applies from the next upload."""
        check(lib().rtow_ctx_set_builder(self._h, builder), "rtow_ctx_set_builder")

    def debug_image(self, which: int) -> bytes:
        """A resident scene image, for tests: 0 BVH, 1 grid, 2/3 the f32 build's, 4 the 4-wide BVH, 5 the 4-wide
        walk's 48-byte frame record (double c[3], float is[3], uint32 half, uint32 lds_limit, pad).  b"" when that
        image is not resident."""
        n = C.c_int64()
        check(lib().rtow_debug_image(self._h, which, None, 0, C.byref(n)), "rtow_debug_image")
        buf = (C.c_ubyte * max(n.value, 1))()
        check(lib().rtow_debug_image(self._h, which, buf, n.value, C.byref(n)), "rtow_debug_image")
        return bytes(buf[:n.value])

    def last_spec(self) -> int:
        """Specialisation of the GRID trace kernel the last trace launch took (rtow_debug_last_spec): 0 generic, 1 static
        spheres, 2 static + moving spheres, | SPEC_FLAT_Y for the two-axis walk of a grid with one layer in y."""
        v = C.c_uint32()
        check(lib().rtow_debug_last_spec(self._h, C.byref(v)), "rtow_debug_last_spec")
        return int(v.value)

    def last_counted(self) -> bool:
        """Whether the last trace launch ran a kernel that counts statistics (rtow_debug_last_counted): False for the
        instantiation a render without statistics launches where the kernel has one."""
        v = C.c_uint32()
        check(lib().rtow_debug_last_counted(self._h, C.byref(v)), "rtow_debug_last_counted")
        return bool(v.value)

    def walk_consts(self):
        """The GRID walk's constants block of the resident grid image (rtow_debug_walk_consts) as 32-bit words
        (csrc/rtow_walk_consts.h: words 16 n_large, 32-35 large_rec, 36-39 large_id, 40 n_large_fast)."""
        n = C.c_int32()
        check(lib().rtow_debug_walk_consts(self._h, None, 0, C.byref(n)), "rtow_debug_walk_consts")
        buf = (C.c_uint32 * (n.value // 4))()
        check(lib().rtow_debug_walk_consts(self._h, buf, n.value, C.byref(n)), "rtow_debug_walk_consts")
        return np.frombuffer(bytes(buf), dtype=np.uint32)

    def build_info(self) -> BuildInfo:
        bi = BuildInfo()
        check(lib().rtow_build_info(self._h, C.byref(bi)), "rtow_build_info")
        return bi

    def render_device(self, cfg: Config, d_ptr: int, stream: int = 0, want_stats=False):
        st = Stats() if want_stats else None
        check(lib().rtow_render_device(self._h, C.byref(cfg), C.c_void_p(d_ptr),
                                       C.c_void_p(stream), C.byref(st) if st is not None else None),
              "rtow_render_device")
        return st

    def tonemap_device(self, d_sums: int, n_values: int, spp_eff: int, d_rgb8: int, stream: int = 0):
        """write_color on the device: 8-bit RGB from radiance sums (both device pointers)."""
        check(lib().rtow_tonemap_device(self._h, C.c_void_p(d_sums), n_values, spp_eff,
                                        C.c_void_p(d_rgb8), C.c_void_p(stream)), "rtow_tonemap_device")

    def render(self, scene, cfg: Config, into=None):
        """Upload + render + D2H: returns (numpy [rows, W, 3] float64 sums, Stats).  `into`: an
        existing sums array to accumulate onto (cfg.accumulate)."""
        import numpy as np

        s = scene.c if isinstance(scene, HostScene) else scene
        rows = lib().rtow_local_rows(C.byref(cfg))
        if rows < 0:
            check(rows, "rtow_local_rows")
        out = np.zeros((rows, cfg.image_width, 3), dtype=np.float64) if into is None else into
        st = Stats()
        check(lib().rtow_render(self._h, C.byref(s), C.byref(cfg), out.ctypes.data_as(_pd),
                                C.byref(st)), "rtow_render")
        return out, st

    def render_rgb8(self, scene, cfg: Config, want_stats=True):
        """Upload + render + write_color on the device + D2H of the bytes: (numpy [rows, W, 3] uint8, Stats | None)."""
        import numpy as np

        s = scene.c if isinstance(scene, HostScene) else scene
        rows = lib().rtow_local_rows(C.byref(cfg))
        if rows < 0:
            check(rows, "rtow_local_rows")
        out = np.zeros((rows, cfg.image_width, 3), dtype=np.uint8)
        st = Stats() if want_stats else None
        check(lib().rtow_render_rgb8(self._h, C.byref(s), C.byref(cfg), out.ctypes.data_as(C.c_void_p),
                                     C.byref(st) if st is not None else None), "rtow_render_rgb8")
        return out, st

    def render_device_rgb8(self, cfg: Config, d_ptr: int, stream: int = 0, want_stats=False):
        """This rank's rows as bytes on the device (write_color fused into the reduce kernel)."""
        st = Stats() if want_stats else None
        check(lib().rtow_render_device_rgb8(self._h, C.byref(cfg), C.c_void_p(d_ptr), C.c_void_p(stream),
                                            C.byref(st) if st is not None else None), "rtow_render_device_rgb8")
        return st

    def intersect(self, rays, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """Closest hit of every ray (a RAY_DTYPE array, host memory) against the resident scene: a HIT_DTYPE array,
        and Stats with `want_stats` (rtow_intersect)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        hits = np.empty(len(r), dtype=HIT_DTYPE)
        st = Stats() if want_stats else None
        check(lib().rtow_intersect(self._h, precision, kernel, r.ctypes.data_as(C.c_void_p), len(r),
                                   hits.ctypes.data_as(C.c_void_p), C.byref(st) if st is not None else None),
              "rtow_intersect")
        return (hits, st) if want_stats else hits

    def intersect_device(self, d_rays: int, n: int, d_hits: int, precision=F64_FAST, kernel=KERNEL_AUTO,
                         stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte rays, n x 72-byte hits), enqueued on `stream`
        (rtow_intersect_device); returns Stats with `want_stats` (then synchronised), else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_intersect_device(self._h, precision, kernel, C.c_void_p(d_rays), n, C.c_void_p(d_hits),
                                          C.c_void_p(stream), C.byref(st) if st is not None else None),
              "rtow_intersect_device")
        return st

    def occluded(self, rays, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """Any-hit test of every ray (a RAY_DTYPE array, host memory) over [0.001, tmax]: a numpy bool array, and Stats
        with `want_stats` (rtow_occluded)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        out = np.empty(len(r), dtype=np.uint8)
        st = Stats() if want_stats else None
        check(lib().rtow_occluded(self._h, precision, kernel, r.ctypes.data_as(C.c_void_p), len(r),
                                  out.ctypes.data_as(C.c_void_p), C.byref(st) if st is not None else None),
              "rtow_occluded")
        occ = out.view(np.bool_)
        return (occ, st) if want_stats else occ

    def occluded_device(self, d_rays: int, n: int, d_occluded: int, precision=F64_FAST, kernel=KERNEL_AUTO,
                        stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte rays, n bytes of results — a torch.bool tensor),
        enqueued on `stream` (rtow_occluded_device); returns Stats with `want_stats` (then synchronised), else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_occluded_device(self._h, precision, kernel, C.c_void_p(d_rays), n, C.c_void_p(d_occluded),
                                         C.c_void_p(stream), C.byref(st) if st is not None else None),
              "rtow_occluded_device")
        return st

    def first_hits(self, rays, max_hits, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """The first `max_hits` (1 .. MAX_HITS) primitives every ray (a RAY_DTYPE array, host memory) passes through
        within [0.001, tmax], ordered by (t, insertion index): (hits, counts) — an [n, max_hits] HIT_DTYPE array whose
        unused slots hold the miss record, and int32 [n] — plus Stats with `want_stats` (rtow_first_hits)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        hits = np.empty((len(r), max(int(max_hits), 0)), dtype=HIT_DTYPE)
        counts = np.empty(len(r), dtype=np.int32)
        st = Stats() if want_stats else None
        check(lib().rtow_first_hits(self._h, precision, kernel, r.ctypes.data_as(C.c_void_p), len(r), int(max_hits),
                                    hits.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                    C.byref(st) if st is not None else None), "rtow_first_hits")
        return (hits, counts, st) if want_stats else (hits, counts)

    def first_hits_device(self, d_rays: int, n: int, max_hits: int, d_hits: int, d_counts: int = 0, precision=F64_FAST,
                          kernel=KERNEL_AUTO, stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte rays, n x max_hits x 72-byte hits, n int32 counts or 0
        for none), enqueued on `stream` (rtow_first_hits_device); returns Stats with `want_stats` (then synchronised),
        else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_first_hits_device(self._h, precision, kernel, C.c_void_p(d_rays), n, int(max_hits),
                                           C.c_void_p(d_hits), C.c_void_p(d_counts) if d_counts else None,
                                           C.c_void_p(stream), C.byref(st) if st is not None else None),
              "rtow_first_hits_device")
        return st

    def closest_point(self, queries, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """Nearest primitive to every point (a POINT_QUERY_DTYPE array, host memory) within its max_dist: a
        POINT_HIT_DTYPE array, and Stats with `want_stats` (rtow_closest_point)."""
        q = np.ascontiguousarray(queries, dtype=POINT_QUERY_DTYPE).reshape(-1)
        hits = np.empty(len(q), dtype=POINT_HIT_DTYPE)
        st = Stats() if want_stats else None
        check(lib().rtow_closest_point(self._h, precision, kernel, q.ctypes.data_as(C.c_void_p), len(q),
                                       hits.ctypes.data_as(C.c_void_p), C.byref(st) if st is not None else None),
              "rtow_closest_point")
        return (hits, st) if want_stats else hits

    def closest_point_device(self, d_q: int, n: int, d_hits: int, precision=F64_FAST, kernel=KERNEL_AUTO,
                             stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers, both 16-byte aligned: n x 48-byte queries, n x 48-byte hits),
        enqueued on `stream` (rtow_closest_point_device); returns Stats with `want_stats` (then synchronised), else
        None."""
        st = Stats() if want_stats else None
        check(lib().rtow_closest_point_device(self._h, precision, kernel, C.c_void_p(d_q), n, C.c_void_p(d_hits),
                                              C.c_void_p(stream), C.byref(st) if st is not None else None),
              "rtow_closest_point_device")
        return st

    def nearest(self, queries, k, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """The `k` (1 .. MAX_NEAREST) primitives nearest to every point (a POINT_QUERY_DTYPE array, host memory) within
        its max_dist, ordered by (dist, insertion index): (hits, counts) — an [n, k] POINT_HIT_DTYPE array whose unused
        slots hold the miss record, and int32 [n] — plus Stats with `want_stats` (rtow_nearest)."""
        q = np.ascontiguousarray(queries, dtype=POINT_QUERY_DTYPE).reshape(-1)
        hits = np.empty((len(q), max(int(k), 0)), dtype=POINT_HIT_DTYPE)
        counts = np.empty(len(q), dtype=np.int32)
        st = Stats() if want_stats else None
        check(lib().rtow_nearest(self._h, precision, kernel, q.ctypes.data_as(C.c_void_p), len(q), int(k),
                                 hits.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                 C.byref(st) if st is not None else None), "rtow_nearest")
        return (hits, counts, st) if want_stats else (hits, counts)

    def nearest_device(self, d_q: int, n: int, k: int, d_hits: int, d_counts: int = 0, precision=F64_FAST,
                       kernel=KERNEL_AUTO, stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 48-byte queries and n x k x 48-byte hits, both 16-byte aligned,
        n int32 counts or 0 for none), enqueued on `stream` (rtow_nearest_device); returns Stats with `want_stats` (then
        synchronised), else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_nearest_device(self._h, precision, kernel, C.c_void_p(d_q), n, int(k), C.c_void_p(d_hits),
                                        C.c_void_p(d_counts) if d_counts else None, C.c_void_p(stream),
                                        C.byref(st) if st is not None else None), "rtow_nearest_device")
        return st

    def radiance(self, rays, samples_per_ray=1, max_child_rays=50, seed=1, ids=None, sample_first=0, precision=F64_FAST,
                 kernel=KERNEL_AUTO, want_stats=False):
        """Path-traced radiance along every ray (a RAY_DTYPE array, host memory; tmax is not read): an [n, 3] float64
        array of SUMS over `samples_per_ray` paths of depth `max_child_rays`, and Stats with `want_stats`
        (rtow_radiance).  `ids`: [n, 2] uint32 (pixel, first sample) Philox identities; None: (i, 0)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        out = np.empty((len(r), 3), dtype=np.float64)
        idp = None
        if ids is not None:
            ida = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1, 2)
            if len(ida) != len(r):
                raise ValueError("ids must be [n, 2]")
            idp = ida.ctypes.data_as(C.c_void_p)
        prm = RadianceParams(seed, samples_per_ray, max_child_rays, sample_first, 0)
        st = Stats() if want_stats else None
        check(lib().rtow_radiance(self._h, precision, kernel, C.byref(prm), r.ctypes.data_as(C.c_void_p), len(r), idp,
                                  out.ctypes.data_as(C.c_void_p), C.byref(st) if st is not None else None),
              "rtow_radiance")
        return (out, st) if want_stats else out

    def radiance_device(self, d_rays: int, n: int, d_ids: int, d_rgb: int, samples_per_ray=1, max_child_rays=50, seed=1,
                        sample_first=0, precision=F64_FAST, kernel=KERNEL_AUTO, stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte rays, n x 2 uint32 ids or 0, n x 3 float64 sums),
        enqueued on `stream` (rtow_radiance_device); returns Stats with `want_stats` (then synchronised), else None."""
        prm = RadianceParams(seed, samples_per_ray, max_child_rays, sample_first, 0)
        st = Stats() if want_stats else None
        check(lib().rtow_radiance_device(self._h, precision, kernel, C.byref(prm), C.c_void_p(d_rays), n,
                                         C.c_void_p(d_ids) if d_ids else None, C.c_void_p(d_rgb), C.c_void_p(stream),
                                         C.byref(st) if st is not None else None),
              "rtow_radiance_device")
        return st

    def path_step(self, rays, bounce, seed=1, ids=None, sample_first=0, precision=F64_FAST, kernel=KERNEL_AUTO,
                  want_stats=False, want_hits=True):
        """One path segment per ray (a RAY_DTYPE array, host memory): the closest hit in [0.001, tmax], then the
        reference's scatter drawn from request 1 + `bounce` of the ray's Philox identity.  Returns (status, next_rays,
        atten, hits) — int32 [n] STEP_*, a RAY_DTYPE array (the dead ray, tmax = -1, where the path ended), [n, 3] float64
        and a HIT_DTYPE array (None without `want_hits`) — plus Stats with `want_stats` (rtow_path_step).  `ids`: [n, 2]
        uint32 (pixel, sample) identities; None: (i, 0)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        n = len(r)
        idp = None
        if ids is not None:
            ida = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1, 2)
            if len(ida) != n:
                raise ValueError("ids must be [n, 2]")
            idp = ida.ctypes.data_as(C.c_void_p)
        status = np.empty(n, dtype=np.int32)
        nxt = np.empty(n, dtype=RAY_DTYPE)
        atten = np.empty((n, 3), dtype=np.float64)
        hits = np.empty(n, dtype=HIT_DTYPE) if want_hits else None
        prm = StepParams(seed, bounce, sample_first)
        st = Stats() if want_stats else None
        check(lib().rtow_path_step(self._h, precision, kernel, C.byref(prm), r.ctypes.data_as(C.c_void_p), n, idp,
                                   nxt.ctypes.data_as(C.c_void_p), atten.ctypes.data_as(C.c_void_p),
                                   status.ctypes.data_as(C.c_void_p),
                                   hits.ctypes.data_as(C.c_void_p) if hits is not None else None,
                                   C.byref(st) if st is not None else None), "rtow_path_step")
        return (status, nxt, atten, hits, st) if want_stats else (status, nxt, atten, hits)

    def path_step_device(self, d_rays: int, n: int, d_ids: int, d_next: int, d_atten: int, d_status: int, d_hits: int = 0,
                         bounce=0, seed=1, sample_first=0, precision=F64_FAST, kernel=KERNEL_AUTO, stream: int = 0,
                         want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte rays, n x 2 uint32 ids or 0, n x 64-byte next rays —
        which may be the rays themselves —, n x 3 float64 attenuations, n int32 status words, n x 72-byte hits or 0 for
        none), enqueued on `stream` (rtow_path_step_device); returns Stats with `want_stats` (then synchronised), else
        None."""
        prm = StepParams(seed, bounce, sample_first)
        st = Stats() if want_stats else None
        check(lib().rtow_path_step_device(self._h, precision, kernel, C.byref(prm), C.c_void_p(d_rays), n,
                                          C.c_void_p(d_ids) if d_ids else None, C.c_void_p(d_next), C.c_void_p(d_atten),
                                          C.c_void_p(d_status), C.c_void_p(d_hits) if d_hits else None, C.c_void_p(stream),
                                          C.byref(st) if st is not None else None), "rtow_path_step_device")
        return st

    def ambient(self, points, samples, seed=1, ids=None, sample_first=0, precision=F64_FAST, kernel=KERNEL_AUTO,
                want_rays=False, want_stats=False):
        """Hemisphere visibility at every surface point (a SURFACE_POINT_DTYPE array, host memory): `samples`
        cosine-weighted directions per point drawn from its Philox identity, and over those that reach max_dist
        unoccluded their count, the sum of the directions and the sum of the sky colour — an AMBIENT_DTYPE array
        (rtow_ambient).  `ids`: [n, 2] uint32 (pixel, first sample) identities; None: (i, 0).  With `want_rays` also the
        [n, samples] RAY_DTYPE array of the rays the walks took, and Stats with `want_stats`: out[, rays][, stats]."""
        p = np.ascontiguousarray(points, dtype=SURFACE_POINT_DTYPE).reshape(-1)
        n = len(p)
        idp = None
        if ids is not None:
            ida = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1, 2)
            if len(ida) != n:
                raise ValueError("ids must be [n, 2]")
            idp = ida.ctypes.data_as(C.c_void_p)
        out = np.empty(n, dtype=AMBIENT_DTYPE)
        rays = np.empty((n, min(max(int(samples), 0), MAX_AMBIENT_SAMPLES)), dtype=RAY_DTYPE) if want_rays else None
        prm = AmbientParams(seed, int(samples), sample_first)
        st = Stats() if want_stats else None
        check(lib().rtow_ambient(self._h, precision, kernel, C.byref(prm), p.ctypes.data_as(C.c_void_p), n, idp,
                                 out.ctypes.data_as(C.c_void_p),
                                 rays.ctypes.data_as(C.c_void_p) if rays is not None else None,
                                 C.byref(st) if st is not None else None), "rtow_ambient")
        res = (out,) + ((rays,) if want_rays else ()) + ((st,) if want_stats else ())
        return res if len(res) > 1 else out

    def ambient_device(self, d_points: int, n: int, d_ids: int, d_out: int, samples: int, d_rays_out: int = 0, seed=1,
                       sample_first=0, precision=F64_FAST, kernel=KERNEL_AUTO, stream: int = 0, want_stats=False):
        """The same on device buffers (raw pointers: n x 64-byte points, n x 2 uint32 ids or 0, n x 64-byte records,
        n x samples x 64-byte rays or 0 for none), enqueued on `stream` (rtow_ambient_device); returns Stats with
        `want_stats` (then synchronised), else None."""
        prm = AmbientParams(seed, int(samples), sample_first)
        st = Stats() if want_stats else None
        check(lib().rtow_ambient_device(self._h, precision, kernel, C.byref(prm), C.c_void_p(d_points), n,
                                        C.c_void_p(d_ids) if d_ids else None, C.c_void_p(d_out),
                                        C.c_void_p(d_rays_out) if d_rays_out else None, C.c_void_p(stream),
                                        C.byref(st) if st is not None else None), "rtow_ambient_device")
        return st

    def sweep(self, queries, precision=F64_FAST, kernel=KERNEL_AUTO, want_stats=False):
        """The first primitive a travelling sphere touches, for every sweep (rtow_sweep / rtow_sweep_device).  `queries`
        is a SWEEP_QUERY_DTYPE array in host memory — the answer is a SWEEP_HIT_DTYPE array — or a torch device tensor
        holding n 80-byte records (any dtype, contiguous, 16-byte aligned): the answer is then a uint8 [n, 80] tensor on
        the same device, enqueued on torch's current stream (view it through SWEEP_HIT_DTYPE after .cpu().numpy()).
        With `want_stats` also Stats."""
        st = Stats() if want_stats else None
        if hasattr(queries, "data_ptr"):  # a torch device tensor
            import torch
            if not queries.is_cuda or not queries.is_contiguous():
                raise ValueError("a sweep tensor must be a contiguous device tensor")
            nbytes = queries.numel() * queries.element_size()
            if nbytes % SWEEP_QUERY_DTYPE.itemsize:
                raise ValueError("a sweep tensor must hold whole 80-byte records")
            n = nbytes // SWEEP_QUERY_DTYPE.itemsize
            hits = torch.empty((n, SWEEP_HIT_DTYPE.itemsize), dtype=torch.uint8, device=queries.device)
            stream = torch.cuda.current_stream(queries.device).cuda_stream
            check(lib().rtow_sweep_device(self._h, precision, kernel, C.c_void_p(queries.data_ptr()), n,
                                          C.c_void_p(hits.data_ptr()), C.c_void_p(stream),
                                          C.byref(st) if st is not None else None), "rtow_sweep_device")
            return (hits, st) if want_stats else hits
        q = np.ascontiguousarray(queries, dtype=SWEEP_QUERY_DTYPE).reshape(-1)
        hits = np.empty(len(q), dtype=SWEEP_HIT_DTYPE)
        check(lib().rtow_sweep(self._h, precision, kernel, q.ctypes.data_as(C.c_void_p), len(q),
                               hits.ctypes.data_as(C.c_void_p), C.byref(st) if st is not None else None), "rtow_sweep")
        return (hits, st) if want_stats else hits

    def sweep_device(self, d_q: int, n: int, d_hits: int, precision=F64_FAST, kernel=KERNEL_AUTO, stream: int = 0,
                     want_stats=False):
        """The same on raw device pointers (both 16-byte aligned: n x 80-byte queries, n x 80-byte hits), enqueued on
        `stream` (rtow_sweep_device); returns Stats with `want_stats` (then synchronised), else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_sweep_device(self._h, precision, kernel, C.c_void_p(d_q), n, C.c_void_p(d_hits),
                                      C.c_void_p(stream), C.byref(st) if st is not None else None), "rtow_sweep_device")
        return st

    def overlap(self, queries, max_ids=MAX_OVERLAP_IDS, precision=F64_FAST, kernel=KERNEL_AUTO, want_ids=True,
                want_stats=False):
        """The primitives whose geometry overlaps every box (rtow_overlap / rtow_overlap_device): (counts, ids) — int32
        [n], the uncapped size of each box's set, and int32 [n, max_ids], its lowest insertion indices ascending with -1
        in the unused slots (None without `want_ids`: counts only).  `queries` is a BOX_QUERY_DTYPE array in host memory
        (make_boxes) — the answers are numpy arrays — or a torch device tensor holding n 64-byte records (any dtype,
        contiguous, 16-byte aligned): the answers are then int32 tensors on the same device, enqueued on torch's current
        stream.  With `want_stats` also Stats."""
        st = Stats() if want_stats else None
        if hasattr(queries, "data_ptr"):  # a torch device tensor
            import torch
            if not queries.is_cuda or not queries.is_contiguous():
                raise ValueError("a box tensor must be a contiguous device tensor")
            nbytes = queries.numel() * queries.element_size()
            if nbytes % BOX_QUERY_DTYPE.itemsize:
                raise ValueError("a box tensor must hold whole 64-byte records")
            n = nbytes // BOX_QUERY_DTYPE.itemsize
            counts = torch.empty((n,), dtype=torch.int32, device=queries.device)
            ids = torch.empty((n, max(int(max_ids), 0)), dtype=torch.int32, device=queries.device) if want_ids else None
            stream = torch.cuda.current_stream(queries.device).cuda_stream
            check(lib().rtow_overlap_device(self._h, precision, kernel, C.c_void_p(queries.data_ptr()), n, int(max_ids),
                                            C.c_void_p(counts.data_ptr()),
                                            C.c_void_p(ids.data_ptr()) if want_ids else None, C.c_void_p(stream),
                                            C.byref(st) if st is not None else None), "rtow_overlap_device")
            return (counts, ids, st) if want_stats else (counts, ids)
        q = np.ascontiguousarray(queries, dtype=BOX_QUERY_DTYPE).reshape(-1)
        counts = np.empty(len(q), dtype=np.int32)
        ids = np.empty((len(q), max(int(max_ids), 0)), dtype=np.int32) if want_ids else None
        check(lib().rtow_overlap(self._h, precision, kernel, q.ctypes.data_as(C.c_void_p), len(q), int(max_ids),
                                 counts.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p) if want_ids else None,
                                 C.byref(st) if st is not None else None), "rtow_overlap")
        return (counts, ids, st) if want_stats else (counts, ids)

    def overlap_device(self, d_q: int, n: int, d_counts: int, d_ids: int = 0, max_ids=MAX_OVERLAP_IDS, precision=F64_FAST,
                       kernel=KERNEL_AUTO, stream: int = 0, want_stats=False):
        """The same on raw device pointers (n x 64-byte queries, 16-byte aligned; n int32 counts; n x max_ids int32 ids
        or 0 for none), enqueued on `stream` (rtow_overlap_device); returns Stats with `want_stats` (then synchronised),
        else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_overlap_device(self._h, precision, kernel, C.c_void_p(d_q), n, int(max_ids), C.c_void_p(d_counts),
                                        C.c_void_p(d_ids) if d_ids else None, C.c_void_p(stream),
                                        C.byref(st) if st is not None else None), "rtow_overlap_device")
        return st

    def overlap_all(self, queries, precision=F64_FAST, kernel=KERNEL_AUTO, max_ids=MAX_OVERLAP_IDS):
        """Every primitive that overlaps every box (a BOX_QUERY_DTYPE array, host memory): a list of n int32 arrays, each
        ascending from the box's own min_prim.  Pages through rtow_overlap: a box whose count exceeds max_ids is asked
        again with min_prim = its last id + 1, all such boxes in one call per round."""
        q = np.ascontiguousarray(queries, dtype=BOX_QUERY_DTYPE).reshape(-1).copy()
        pages = [[] for _ in range(len(q))]
        todo = np.arange(len(q))
        while len(todo):
            counts, ids = self.overlap(q[todo], max_ids, precision, kernel)
            for row, i in enumerate(todo):
                pages[i].append(ids[row, :min(int(counts[row]), max_ids)])
            more = counts > max_ids
            todo = todo[more]
            q["min_prim"][todo] = ids[more, max_ids - 1] + 1
        return [np.concatenate(p).astype(np.int32) for p in pages]

    def camera_rays(self, cfg: Config):
        """The primaries a render of `cfg` generates on this rank, from the resident camera: (rays, ids) — a RAY_DTYPE
        array of rows x W x samples rays, pixel-major with a pixel's samples ascending, and the [n, 2] uint32 (global
        pixel, sample) Philox identities `radiance` takes (rtow_camera_rays)."""
        n = lib().rtow_camera_ray_count(C.byref(cfg))
        if n < 0:
            check(int(n), "rtow_camera_ray_count")
        rays = np.empty(n, dtype=RAY_DTYPE)
        ids = np.empty((n, 2), dtype=np.uint32)
        check(lib().rtow_camera_rays(self._h, C.byref(cfg), rays.ctypes.data_as(C.c_void_p),
                                     ids.ctypes.data_as(C.c_void_p)), "rtow_camera_rays")
        return rays, ids

    def camera_rays_device(self, cfg: Config, d_rays: int, d_ids: int = 0, stream: int = 0):
        """The same into device buffers (raw pointers: n x 64-byte rays, n x 2 uint32 ids or 0), enqueued on `stream`
        (rtow_camera_rays_device)."""
        check(lib().rtow_camera_rays_device(self._h, C.byref(cfg), C.c_void_p(d_rays), C.c_void_p(d_ids) if d_ids else None,
                                            C.c_void_p(stream)), "rtow_camera_rays_device")

    def guides(self, cfg: Config, want_stats=False):
        """First-hit guide buffers of this rank's rows for a denoiser: a [rows, W] GUIDE_DTYPE array of SUMS over the
        samples a render of `cfg` traces (albedo, unit normal, distance, hit count), and Stats with `want_stats`
        (rtow_guides)."""
        rows = lib().rtow_local_rows(C.byref(cfg))
        if rows < 0:
            check(rows, "rtow_local_rows")
        out = np.empty((rows, cfg.image_width), dtype=GUIDE_DTYPE)
        st = Stats() if want_stats else None
        check(lib().rtow_guides(self._h, C.byref(cfg), out.ctypes.data_as(C.c_void_p),
                                C.byref(st) if st is not None else None), "rtow_guides")
        return (out, st) if want_stats else out

    def guides_device(self, cfg: Config, d_guides: int, stream: int = 0, want_stats=False):
        """The same into a device buffer (raw pointer: rows x W x 64 bytes, 16-byte aligned), enqueued on `stream`
        (rtow_guides_device); returns Stats with `want_stats` (then synchronised), else None."""
        st = Stats() if want_stats else None
        check(lib().rtow_guides_device(self._h, C.byref(cfg), C.c_void_p(d_guides), C.c_void_p(stream),
                                       C.byref(st) if st is not None else None), "rtow_guides_device")
        return st

    def profile_collect(self):
        """(trace-kernel ms since the last collect, launches); raises if a launch dropped samples."""
        ms, n = C.c_double(), C.c_int32()
        check(lib().rtow_profile_collect(self._h, C.byref(ms), C.byref(n)), "rtow_profile_collect")
        return ms.value, n.value

    def close(self):
        if self._h:
            lib().rtow_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_multi(device_ids, scene, cfg: Config, use_rccl=True):
    """One frame over several devices from this process (rtow_render_multi): returns ([H, W, 3] sums, Stats)."""
    import numpy as np

    s = scene.c if isinstance(scene, HostScene) else scene
    ids = (C.c_int32 * len(device_ids))(*device_ids)
    out = np.zeros((cfg.image_height, cfg.image_width, 3), dtype=np.float64)
    st = Stats()
    check(lib().rtow_render_multi(len(device_ids), ids, C.byref(s), C.byref(cfg), out.ctypes.data_as(_pd), C.byref(st),
                                  int(bool(use_rccl))), "rtow_render_multi")
    return out, st


class MultiContext:
    """Persistent multi-device handle (rtow_multi_*): contexts, streams, buffers, worker threads and the RCCL
    communicator live as long as the object; upload once, render many frames."""

    def __init__(self, device_ids, use_rccl=True):
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        self._h = C.c_void_p()
        check(lib().rtow_multi_create(len(device_ids), ids, int(bool(use_rccl)), C.byref(self._h)), "rtow_multi_create")
        self.n = len(device_ids)

    def upload(self, scene):
        s = scene.c if isinstance(scene, HostScene) else scene
        check(lib().rtow_multi_upload(self._h, C.byref(s)), "rtow_multi_upload")

    def build_info(self) -> BuildInfo:
        bi = BuildInfo()
        check(lib().rtow_multi_build_info(self._h, C.byref(bi)), "rtow_multi_build_info")
        return bi

    def render(self, cfg: Config, want_stats=True):
        import numpy as np

        out = np.zeros((cfg.image_height, cfg.image_width, 3), dtype=np.float64)
        st = Stats() if want_stats else None
        check(lib().rtow_multi_render(self._h, C.byref(cfg), out.ctypes.data_as(_pd),
                                      C.byref(st) if st is not None else None), "rtow_multi_render")
        return out, st

    def render_rgb8(self, cfg: Config, want_stats=True):
        """The frame as the PPM's bytes: write_color by the owning rank, bytes gathered, rows placed on the first
        device, one copy.  ([H, W, 3] uint8, Stats | None)"""
        import numpy as np

        out = np.zeros((cfg.image_height, cfg.image_width, 3), dtype=np.uint8)
        st = Stats() if want_stats else None
        check(lib().rtow_multi_render_rgb8(self._h, C.byref(cfg), out.ctypes.data_as(C.c_void_p),
                                           C.byref(st) if st is not None else None), "rtow_multi_render_rgb8")
        return out, st

    def frame_breakdown(self) -> dict:
        """Where the last frame's time went (rtow_multi_frame_breakdown), milliseconds by name."""
        v = (C.c_double * len(MULTI_BREAKDOWN))()
        L = lib()
        L.rtow_multi_frame_breakdown.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
        n = L.rtow_multi_frame_breakdown(self._h, v, len(MULTI_BREAKDOWN))
        if n < 0:
            check(n, "rtow_multi_frame_breakdown")
        return {k: float(v[i]) for i, k in enumerate(MULTI_BREAKDOWN[:n])}

    def close(self):
        if self._h:
            lib().rtow_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def have_gpu() -> bool:
    """True when a HIP device can be bound (used by tests to choose markers only)."""
    try:
        c = Context(0)
        c.close()
        return True
    except Exception:
        return False
