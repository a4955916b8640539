"""Oracle ray logs and the comparisons more than one test module makes: the log capture and what is read off a log, the
brute force over the oracle's hit tests, bit and record comparisons, the in-order sum, image reductions, and the LOGGED
table of the three small logged renders.

Importing this module loads no library: liboracle.so and librtow.so are loaded by the functions that call them.
"""
import ctypes as C
import math

import numpy as np

import orc
import rtow
from support_scenes import cover, cover_moving, suzanne
from support_tables import WALKS

_pd = C.POINTER(C.c_double)

LOGGED = {
    # name: (scene, width, height, spp, max_child_rays, seed)
    "cover_static": (cover, 120, 80, 4, 50, 21),
    "cover_moving": (cover_moving, 120, 80, 4, 50, 22),
    "suzanne": (suzanne, 96, 54, 4, 20, 23),
}
# (scene, walk) of the fast-against-strict comparisons: the logged renders and the 96,800-triangle mesh of the `big_mesh`
# fixture (not under the brute-force walk: 96,800 triangle tests per ray)
FAST_CASES = [(n, k) for n in list(LOGGED) + ["mesh96k"] for k in WALKS if (n, k) != ("mesh96k", "brute")]


# --------------------------------------------------------------------------------------------------- ray logs ---
def logged_render(scene, cfg, accel=False, cap=1_500_000):
    """(sums [pixels, 3], log [n, 12]) of a single-threaded oracle render (orc_set_raylog); a log row is (pixel, sample,
    segment, o xyz, d xyz, time, t_hit or inf, class index or -1).  `accel`: the checker's tree instead of the
    reference's (the same hits, much faster on a large mesh)."""
    buf = np.zeros((cap, 12))
    L = orc.lib()
    L.orc_set_raylog.argtypes = [_pd, C.c_uint64]
    L.orc_set_raylog.restype = None
    L.orc_raylog_count.restype = C.c_uint64
    L.orc_set_raylog(buf.ctypes.data_as(_pd), cap)
    try:
        img, _ = orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=1, accel=accel)
        n = L.orc_raylog_count()
    finally:
        L.orc_set_raylog(None, 0)
    assert 0 < n < cap
    return img.reshape(-1, 3).copy(), buf[:n].copy()


def log_rays(scene, cfg, accel=False, cap=1_500_000):
    """The log of logged_render alone: every segment of the render."""
    return logged_render(scene, cfg, accel, cap)[1]


def rays_of(log, tmax=math.inf):
    r = np.empty(len(log), dtype=rtow.RAY_DTYPE)
    r["origin"] = log[:, 3:6]
    r["direction"] = log[:, 6:9]
    r["time"] = log[:, 9]
    r["tmax"] = tmax
    return r


def primaries(log):
    """(rays, ids) of the log's segment-0 rows: the render's primaries and their Philox identities (pixel, sample)."""
    p = log[log[:, 2] == 0]
    return rays_of(p), p[:, 0:2].astype(np.uint32)


def seeded_finite_tmax(rays, seed=11):
    g = np.random.default_rng(seed)
    finite = rays.copy()
    finite["tmax"] = g.choice([0.0005, 0.3, 1.0, 2.5, 6.0, 50.0], size=len(rays)) * g.random(len(rays)) * 2.0
    finite["tmax"][:3] = [math.nan, 0.000999, 0.001]  # (the empty interval, both ways, and its edge)
    return finite


def brute_force(view, rays):
    """The reference's hittable list: every primitive in insertion order, the interval shrinking to the closest hit."""
    out = np.zeros(len(rays), dtype=rtow.HIT_DTYPE)
    out["t"], out["prim"], out["kind"], out["material"] = math.inf, -1, -1, -1
    for j, r in enumerate(rays):
        best, tmax = None, math.inf
        for p in range(len(view.kind)):
            h = view.oracle_hit(p, r["origin"], r["direction"], r["time"], tmax=tmax)
            if h is not None:
                best, tmax = (p, h), h[0]
        if best is not None:
            p, (t, pt, n, front) = best
            out[j] = (t, pt, n, p, view.kind[p], view.prim_mat[p], front)
    return out


# ------------------------------------------------------------------------------------------------ comparisons ---
def same_bits(a, b):
    """The same shape, the same dtype and the same bits.  What is not an array (a number, a ctypes or Python sequence)
    is taken as binary64; arrays keep their dtype, structured ones included."""
    a, b = (x if isinstance(x, np.ndarray) else np.asarray(x, dtype=np.float64) for x in (a, b))
    return (a.shape == b.shape and a.dtype == b.dtype
            and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)))


def assert_hits_equal(a, b, what):
    for f in ("t", "point", "normal", "prim", "kind", "material", "front_face"):
        x, y = a[f], b[f]
        same = (x == y) | (np.isnan(x) & np.isnan(y)) if x.dtype.kind == "f" else x == y
        bad = np.nonzero(~same.reshape(len(a), -1).all(axis=1))[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:5])


def sum_in_order(per_sample, spp):
    """[pixels * spp, ...] -> [pixels, ...]: ((0 + c_0) + c_1) + ... over a pixel's samples, as the oracle adds them."""
    c = per_sample.reshape((-1, spp) + per_sample.shape[1:])
    s = np.zeros((c.shape[0],) + per_sample.shape[1:])
    for j in range(spp):
        s = s + c[:, j]
    return s


def sky_of_strict(d):
    """The reference's background for directions d [n, 3], operation by operation in binary64 (ray_color's last lines)."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    dot = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    t = 0.5 * (d[:, 1] * (1.0 / np.sqrt(dot)) + 1.0)
    return np.stack([(1.0 - t) * 1.0 + t * k for k in (0.5, 0.7, 1.0)], axis=1)


def expected_kernel(scene, kernel):
    """The render's fallbacks, for a host scene or a SceneView: BVH4 walks triangle meshes only; GRID falls back to BVH
    where there is no grid."""
    if hasattr(scene, "kind"):
        mesh = bool(np.all(scene.kind == rtow.PRIM_TRIANGLE))
    else:
        mesh = scene.c.n_triangles == scene.c.n_prims
    if kernel == rtow.KERNEL_BVH4 and not mesh:
        return rtow.KERNEL_BVH
    if kernel == rtow.KERNEL_GRID and mesh:
        return None  # (a small mesh may or may not get a grid: either is the render's rule)
    return kernel


# ----------------------------------------------------------------------------------------------------- images ---
def to8(img, spp):
    """The 8-bit levels write_color gives the sums of `spp` samples."""
    return (256 * np.clip(np.sqrt(img / spp), 0.0, 0.999)).astype(np.int32)


def block_means(a, b=16):
    h, w, _ = a.shape
    h, w = h // b * b, w // b * b
    return a[:h, :w].reshape(h // b, b, w // b, b, 3).mean(axis=(1, 3))


def tile_order(scene, cfg):
    """rtow_debug_tile_order: (table, empty flags, number of empty tiles, tile width, tile height)."""
    L = rtow.lib()
    cap = 1 << 16
    table, empty = (C.c_uint32 * cap)(), (C.c_ubyte * cap)()
    ne, tw, th = C.c_int32(), C.c_int32(), C.c_int32()
    n = L.rtow_debug_tile_order(C.byref(scene.c), C.byref(cfg), table, empty, cap, C.byref(ne), C.byref(tw), C.byref(th))
    if n < 0:
        rtow.check(n, "rtow_debug_tile_order")
    return np.array(table[:n], dtype=np.int64), np.array(empty[:n], dtype=bool), ne.value, tw.value, th.value
