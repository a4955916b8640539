"""Helpers of test_gpu_guides.py: the oracle's ray log, bit comparison, the row partition, and the numpy statement of the
guide fold (csrc/rtow_guides.h) — IEEE binary64, the written operand order, samples added in order from zero."""
import ctypes as C

import numpy as np

import orc
import rtow
from conftest import GOLDEN

_pd = C.POINTER(C.c_double)


def logged_render(scene, cfg, cap=200_000):
    """(sums [pixels, 3], log [n, 12]) of a single-threaded oracle render; a log row is (pixel, sample, segment, o xyz,
    d xyz, time, t_hit or inf, class index or -1)."""
    buf = np.zeros((cap, 12))
    L = orc.lib()
    L.orc_set_raylog.argtypes = [_pd, C.c_uint64]
    L.orc_set_raylog.restype = None
    L.orc_raylog_count.restype = C.c_uint64
    L.orc_set_raylog(buf.ctypes.data_as(_pd), cap)
    try:
        img, _ = orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=1)
        n = L.orc_raylog_count()
    finally:
        L.orc_set_raylog(None, 0)
    assert 0 < n < cap
    return img.reshape(-1, 3).copy(), buf[:n].copy()


def primaries(log):
    """(rays, ids) of the log's segment-0 rows: the render's primaries and their Philox identities (pixel, sample)."""
    p = log[log[:, 2] == 0]
    r = np.empty(len(p), dtype=rtow.RAY_DTYPE)
    r["origin"] = p[:, 3:6]
    r["direction"] = p[:, 6:9]
    r["time"] = p[:, 9]
    r["tmax"] = np.inf
    return r, p[:, 0:2].astype(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def sum_in_order(per_sample, spp):
    """[pixels * spp, ...] -> [pixels, ...]: ((0 + c_0) + c_1) + ... over a pixel's samples."""
    c = per_sample.reshape((-1, spp) + per_sample.shape[1:])
    s = np.zeros((c.shape[0],) + per_sample.shape[1:])
    for j in range(spp):
        s = s + c[:, j]
    return s


def row_list(cfg):
    """This rank's global rows, ascending (rtow_local_row_list)."""
    L = rtow.lib()
    n = L.rtow_local_rows(C.byref(cfg))
    rows = np.zeros(max(n, 1), dtype=np.int32)
    assert L.rtow_local_row_list(C.byref(cfg), rows.ctypes.data_as(C.POINTER(C.c_int32)), n) == n
    return rows[:n]


def cover():
    return rtow.HostScene.cover(11, 1.5, False)


def cover_moving():
    return rtow.HostScene.cover(11, 1.5, True)


def suzanne():
    return rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)


def expected_kernel(scene, kernel):
    """The render's fallbacks: BVH4 walks triangle meshes only; GRID falls back to BVH where there is no grid."""
    mesh = scene.c.n_triangles == scene.c.n_prims
    if kernel == rtow.KERNEL_BVH4 and not mesh:
        return rtow.KERNEL_BVH
    if kernel == rtow.KERNEL_GRID and mesh:
        return None  # (a small mesh may or may not get a grid: either is the render's rule)
    return kernel


def attenuations(scene):
    """[n_materials, 3]: what the reference's scatter returns as attenuation — albedo, or (1, 1, 1) for a Dielectric."""
    m = orc.scene_arrays(scene.c)["materials"]
    att = m[:, 0:3].copy()
    att[m[:, 5] == rtow.MAT_DIELECTRIC] = 1.0
    return att


def fold_guides(rays, hits, sky, att, spp):
    """The guide sums of csrc/rtow_guides.h from pinned pieces: `hits` the strict closest hits of `rays` (HIT_DTYPE), `sky`
    [n, 3] the strict radiance of the rays at depth 0 (the sky on a miss, black on a hit), `att` attenuations().  Returns a
    GUIDE_DTYPE array [pixels].  A miss adds +0.0 where the kernel adds nothing: the same bits (no sum is ever -0.0)."""
    hit = np.isfinite(hits["t"])
    mat = np.where(hit, hits["material"], 0)
    albedo = np.where(hit[:, None], att[mat], sky)
    n = hits["normal"]
    tri = hits["kind"] == rtow.PRIM_TRIANGLE
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        unit = np.where(tri[:, None], n / s[:, None], n)
        d = rays["direction"]
        depth = hits["t"] * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    unit = np.where(hit[:, None], unit, 0.0)
    depth = np.where(hit, depth, 0.0)
    out = np.zeros(len(rays) // spp, dtype=rtow.GUIDE_DTYPE)
    out["albedo"] = sum_in_order(albedo, spp)
    out["normal"] = sum_in_order(unit, spp)
    out["depth"] = sum_in_order(depth, spp)
    out["hits"] = sum_in_order(hit.astype(np.float64), spp)
    return out


def guide_values(g):
    """[..., 8] float64 view of a GUIDE_DTYPE array: albedo, normal, depth, hits."""
    g = np.ascontiguousarray(g)
    return g.view(np.float64).reshape(g.shape + (8,))
