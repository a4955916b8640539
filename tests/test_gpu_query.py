"""Closest-hit ray queries (rtow_intersect / rtow_intersect_device) on the GPU.

The strict build is checked RAY BY RAY against the oracle: every segment an oracle render traces is logged
(orc_set_raylog: origin, direction, time, t_hit, class index of the hit primitive) and queried again under every
strategy; t must equal the logged t_hit bit for bit, and point / normal / front_face must equal the oracle's own hit
test (orc_sphere_hit / orc_triangle_hit) on the returned primitive.  The fast build is checked against the strict one
by tolerance; hand-made rays cover the corner cases; the contracts (ordering, residency, errors, no side effect on the
render) close the file.
"""
import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest

import orc
import rtow
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

STRICT_KERNELS = {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID,
                  "bvh4": rtow.KERNEL_BVH4, "reftree": rtow.KERNEL_REFTREE}
_pd = C.POINTER(C.c_double)


# ---------------------------------------------------------------------------------------------------- helpers ---
def log_rays(scene, cfg, accel=False, cap=1_500_000):
    """Every segment of a single-threaded oracle render: [n, 12] (pixel, sample, segment, o xyz, d xyz, time, t_hit or
    inf, class index or -1)."""
    buf = np.zeros((cap, 12))
    L = orc.lib()
    L.orc_set_raylog.argtypes = [_pd, C.c_uint64]
    L.orc_set_raylog.restype = None
    L.orc_raylog_count.restype = C.c_uint64
    L.orc_set_raylog(buf.ctypes.data_as(_pd), cap)
    try:
        orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=1, accel=accel)
        n = L.orc_raylog_count()
    finally:
        L.orc_set_raylog(None, 0)
    assert 0 < n < cap
    return buf[:n].copy()


def rays_of(log, tmax=math.inf):
    r = np.empty(len(log), dtype=rtow.RAY_DTYPE)
    r["origin"] = log[:, 3:6]
    r["direction"] = log[:, 6:9]
    r["time"] = log[:, 9]
    r["tmax"] = tmax
    return r


class SceneView:
    """numpy copy of a flattened scene: geometry per class, insertion order, material per inserted primitive."""

    def __init__(self, scene):
        a = orc.scene_arrays(scene.c)
        self.sph = a["sphere_geom"].reshape(-1, 4)
        self.mov = a["moving_geom"].reshape(-1, 8)
        self.tri = a["triangle_geom"].reshape(-1, 9)
        self.kind = a["prim_kind"]
        self.index = a["prim_index"]
        mats = {rtow.PRIM_SPHERE: a["sphere_mat"], rtow.PRIM_MOVING_SPHERE: a["moving_mat"],
                rtow.PRIM_TRIANGLE: a["triangle_mat"]}
        self.prim_mat = np.array([mats[k][i] for k, i in zip(self.kind, self.index)], dtype=np.int32)

    def oracle_hit(self, prim, o, d, time, tmin=0.001, tmax=math.inf):
        """The oracle's hit test of inserted primitive `prim`: (t, point, normal, front) or None."""
        L = orc.lib()
        t = C.c_double()
        p, n = (C.c_double * 3)(), (C.c_double * 3)()
        ro, rd = (C.c_double * 3)(*o), (C.c_double * 3)(*d)
        k, i = int(self.kind[prim]), int(self.index[prim])
        if k == rtow.PRIM_TRIANGLE:
            g = self.tri[i]
            ok = L.orc_triangle_hit((C.c_double * 3)(*g[0:3]), (C.c_double * 3)(*g[3:6]), (C.c_double * 3)(*g[6:9]), ro,
                                    rd, tmin, tmax, C.byref(t), p, n)
            front = 1
        else:
            if k == rtow.PRIM_SPHERE:
                c, r = self.sph[i, 0:3], self.sph[i, 3]
            else:  # the oracle's moving_center, in numpy (binary64, no contraction)
                g = self.mov[i]
                c, r = g[0:3] + time * (g[3:6] - g[0:3]), g[6]
            f = C.c_int()
            ok = L.orc_sphere_hit((C.c_double * 3)(*c), r, ro, rd, tmin, tmax, C.byref(t), p, n, C.byref(f))
            front = f.value
        if not ok:
            return None
        return t.value, np.array(p[:]), np.array(n[:]), front


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_strict_against_log(view, log, hits, what):
    """t bitwise = the log's t_hit, class index = the log's, hit record = the oracle's hit test on that primitive."""
    t_log = log[:, 10]
    assert same_bits(hits["t"], t_log), (what, int((hits["t"].view(np.uint64) != t_log.view(np.uint64)).sum()))
    miss = ~np.isfinite(t_log)
    assert np.all(hits["prim"][miss] == -1) and np.all(hits["kind"][miss] == -1)
    assert np.all(hits["material"][miss] == -1) and np.all(hits["front_face"][miss] == 0)
    hit = ~miss
    prim = hits["prim"][hit]
    assert np.all(prim >= 0)
    assert np.array_equal(view.index[prim], log[hit, 11].astype(np.int32)), what
    assert np.array_equal(view.kind[prim], hits["kind"][hit]), what
    assert np.array_equal(view.prim_mat[prim], hits["material"][hit]), what
    # the hit record: one oracle call per distinct (primitive, ray) — the records of the other kernels must be equal
    for j in np.nonzero(hit)[0]:
        h = view.oracle_hit(int(hits["prim"][j]), log[j, 3:6], log[j, 6:9], log[j, 9])
        assert h is not None, (what, j)
        t, p, n, front = h
        assert same_bits(t, hits["t"][j]) and same_bits(p, hits["point"][j]) and same_bits(n, hits["normal"][j]), (what, j)
        assert front == hits["front_face"][j], (what, j)


def expected_kernel(view, kernel):
    """The render's fallbacks: BVH4 walks triangle meshes only; GRID falls back to BVH where there is no grid."""
    mesh = bool(np.all(view.kind == rtow.PRIM_TRIANGLE))
    if kernel == rtow.KERNEL_BVH4 and not mesh:
        return rtow.KERNEL_BVH
    if kernel == rtow.KERNEL_GRID and mesh:
        return None  # (a small mesh may or may not get a grid: either is the render's rule)
    return kernel


# ------------------------------------------------------------------------------------------------- fixtures ---
LOGGED = {
    # name: (scene, width, height, spp, max_child_rays, seed)
    "cover_static": (lambda: rtow.HostScene.cover(11, 1.5, False), 120, 80, 4, 50, 21),
    "cover_moving": (lambda: rtow.HostScene.cover(11, 1.5, True), 120, 80, 4, 50, 22),
    "suzanne": (lambda: rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9), 96, 54, 4, 20, 23),
}


@pytest.fixture(scope="module")
def logged():
    """name -> (scene, view, log) of the three small renders."""
    out = {}
    for name, (mk, w, h, spp, depth, seed) in LOGGED.items():
        scene = mk()
        cfg = rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        out[name] = (scene, SceneView(scene), log_rays(scene, cfg))
    return out


@pytest.fixture(scope="module")
def qctx():
    c = rtow.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_mesh(tmp_path_factory):
    """The 96,800-triangle mesh (scripts/make_mesh.py) and a 64x36x2 spp raylog of it (the checker's tree: the same
    hits as the reference's tree, ~100x faster)."""
    obj = tmp_path_factory.mktemp("mesh") / "m10.obj"
    subprocess.run([sys.executable, str(REPO / "scripts" / "make_mesh.py"), str(obj), "10"], check=True,
                   capture_output=True)
    scene = rtow.HostScene.obj(obj, 16 / 9)
    assert scene.c.n_triangles == 96800
    cfg = rtow.make_config(64, 36, 2, 1, 20, seed=24, precision=rtow.F64_STRICT)
    return scene, SceneView(scene), log_rays(scene, cfg, accel=True)


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("kernel", list(STRICT_KERNELS))
@pytest.mark.parametrize("name", list(LOGGED))
def test_logged_rays_strict_every_kernel(qctx, logged, name, kernel):
    """Every segment of an oracle render, queried in the strict build: t bit for bit, the same primitive, the oracle's
    point / normal / front_face bit for bit, the scene's material — under every strategy (REFTREE included)."""
    scene, view, log = logged[name]
    qctx.upload(scene)
    hits, st = qctx.intersect(rays_of(log), rtow.F64_STRICT, STRICT_KERNELS[kernel], want_stats=True)
    want = expected_kernel(view, STRICT_KERNELS[kernel])
    if want is not None:
        assert st.kernel_used == want
    assert st.segments == len(log) and st.samples == 0
    check_strict_against_log(view, log, hits, (name, kernel))


@pytest.mark.parametrize("builder", [rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH])
@pytest.mark.parametrize("kernel", ["bvh4", "bvh"])
def test_big_mesh_strict(qctx, big_mesh, builder, kernel):
    """96,800 triangles (image not staged whole, leaf-ordered records): both builders, the 4-wide and the binary walk."""
    scene, view, log = big_mesh
    qctx.set_builder(builder)
    try:
        qctx.upload(scene)
        assert qctx.build_info().builder == builder
        hits, st = qctx.intersect(rays_of(log), rtow.F64_STRICT, STRICT_KERNELS[kernel], want_stats=True)
        assert st.kernel_used == STRICT_KERNELS[kernel]
        assert st.node_tests > 0 and st.prim_tests > 0
        check_strict_against_log(view, log, hits, (builder, kernel))
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


FAST_KERNELS = {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID, "bvh4": rtow.KERNEL_BVH4}


FAST_CASES = [(n, k) for n in list(LOGGED) + ["mesh96k"] for k in FAST_KERNELS if (n, k) != ("mesh96k", "brute")]


@pytest.mark.parametrize("name,kernel", FAST_CASES)
def test_fast_agrees_with_strict(qctx, logged, big_mesh, name, kernel):
    """The fast build against the strict one on the same logged rays: hit / miss agree on >= 99.99 % of the rays; where
    both hit the same primitive |t_fast - t_strict| <= 1e-9 t_strict; a different primitive only at such a near-tie.
    Observed on the MI355X: every ray of every case agrees on hit / miss and on the primitive; the worst relative
    difference in t is 1.8e-10 (cover_moving, GRID: the fast grid walk's unit-direction sphere test), 1.6e-10 on the
    static cover scene, 4.8e-14 on suzanne, 2.8e-15 on the 96.8k mesh (printed per case)."""
    if name == "mesh96k":  # (not the brute-force walk: 96,800 triangle tests per ray)
        scene, view, log = big_mesh
    else:
        scene, view, log = logged[name]
    qctx.upload(scene)
    rays = rays_of(log)
    s = qctx.intersect(rays, rtow.F64_STRICT, FAST_KERNELS[kernel])
    f = qctx.intersect(rays, rtow.F64_FAST, FAST_KERNELS[kernel])
    hs, hf = np.isfinite(s["t"]), np.isfinite(f["t"])
    agree = float(np.mean(hs == hf))
    assert agree >= 0.9999, agree
    both = hs & hf
    rel = np.abs(f["t"][both] - s["t"][both]) / s["t"][both]
    same = f["prim"][both] == s["prim"][both]
    assert np.all(rel <= 1e-9), float(rel.max())
    worst = float(rel.max()) if rel.size else 0.0
    print(f"\n{name}/{kernel}: hit/miss agree {agree:.6f}, other primitive {int((~same).sum())}, worst rel dt {worst:.3e}")


@pytest.mark.parametrize("kernel", list(STRICT_KERNELS))
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_tmax_is_an_inclusive_bound(qctx, logged, name, kernel):
    """tmax = t_hit gives the same hit (inclusive), tmax = nextafter(t_hit, 0) a miss, tmax < 0.001 always a miss."""
    scene, view, log = logged[name]
    qctx.upload(scene)
    log = log[:20000]
    hit = np.isfinite(log[:, 10])
    full = qctx.intersect(rays_of(log), rtow.F64_STRICT, STRICT_KERNELS[kernel])
    rays = rays_of(log[hit], tmax=log[hit, 10])
    at = qctx.intersect(rays, rtow.F64_STRICT, STRICT_KERNELS[kernel])
    assert at.tobytes() == full[hit].tobytes()
    rays["tmax"] = np.nextafter(log[hit, 10], 0.0)
    below = qctx.intersect(rays, rtow.F64_STRICT, STRICT_KERNELS[kernel])
    assert np.all(np.isinf(below["t"])) and np.all(below["prim"] == -1)
    short = qctx.intersect(rays_of(log, tmax=0.000999), rtow.F64_STRICT, STRICT_KERNELS[kernel])
    assert np.all(np.isinf(short["t"])) and np.all(short["prim"] == -1) and np.all(short["front_face"] == 0)


# ---- hand-made scene and rays, against a brute force over the oracle's hit tests ----
def handmade_scene():
    """Ground, a glass sphere with a negative-radius inner sphere (hollow glass), a moving sphere, two triangles —
    inserted triangles first, so insertion order and class-major order differ."""
    sph = np.array([[0, -1000, 0, 1000], [0, 1, 0, 1.0], [0, 1, 0, -0.8], [-3, 1, 0.5, 0.7]], dtype=np.float64)
    mov = np.array([[3, 0.5, 0, 3, 1.5, 0, 0.5, 0]], dtype=np.float64)
    tri = np.array([[-1, 0, -2, 1, 0, -2, 0, 2, -2], [2, 0, -3, 4, 0, -3, 3, 2.5, -3]], dtype=np.float64)
    sph_mat = np.array([0, 1, 1, 2], dtype=np.int32)
    mov_mat = np.array([0], dtype=np.int32)
    tri_mat = np.array([2, 0], dtype=np.int32)
    kind = np.array([2, 0, 1, 0, 2, 0, 0], dtype=np.int32)
    index = np.array([1, 2, 0, 0, 0, 3, 1], dtype=np.int32)
    mats = (rtow.Material * 3)()
    mats[0].albedo[:] = [0.5, 0.5, 0.5]
    mats[1].kind, mats[1].ir = rtow.MAT_DIELECTRIC, 1.5
    mats[2].kind, mats[2].fuzz = rtow.MAT_METAL, 0.1
    mats[2].albedo[:] = [0.7, 0.6, 0.5]
    keep = [sph, mov, tri, sph_mat, mov_mat, tri_mat, kind, index, mats]
    s = rtow.Scene()
    base = rtow.HostScene.cover(11, 1.5, False)  # (its camera: the queries do not use one)
    s.camera = base.c.camera
    pd = lambda a: a.ctypes.data_as(_pd)  # noqa: E731
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    s.n_spheres, s.sphere_geom, s.sphere_mat = len(sph), pd(sph), pi(sph_mat)
    s.n_moving, s.moving_geom, s.moving_mat = len(mov), pd(mov), pi(mov_mat)
    s.n_triangles, s.triangle_geom, s.triangle_mat = len(tri), pd(tri), pi(tri_mat)
    s.n_materials, s.materials = 3, mats
    s.n_prims, s.prim_kind, s.prim_index = len(kind), pi(kind), pi(index)

    class Held:
        c = s

    h = Held()
    h.keep = keep
    base.close()
    return h


def handmade_rays():
    rng = np.random.default_rng(5)
    o, d, tm = [], [], []
    axes = [np.array(v, dtype=np.float64) for v in np.vstack([np.eye(3), -np.eye(3)])]
    for origin in ([0, 1, 5], [0, 1, -5], [5, 1, 0], [-5, 1, 0], [0, 5, 0], [0.3, 0.9, 0.2], [3, 1, 4], [0, 1, 0],
                   [0, 0.5, -1], [3.2, 4, -3]):
        for ax in axes:  # axis-parallel directions: zero components, both signs
            o.append(origin), d.append(ax), tm.append(0.5)
    for _ in range(200):  # inside the glass shell (0.8 < r < 1): the far root of the outer sphere, front_face 0
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o.append(np.array([0, 1, 0]) + 0.9 * u), d.append(u + 0.3 * rng.normal(size=3)), tm.append(0.0)
    for _ in range(200):  # inside the negative-radius sphere, and from outside through the hollow glass
        u = rng.normal(size=3)
        o.append(np.array([0, 1, 0]) + 0.5 * u / np.linalg.norm(u)), d.append(rng.normal(size=3)), tm.append(0.0)
        o.append(np.array([0, 1, 4.0]) + 0.3 * rng.normal(size=3)), d.append([0, 0, -1] + 0.2 * rng.normal(size=3))
        tm.append(1.0)
    for x in np.linspace(-2, 2, 21):  # in the plane of a triangle, parallel to it
        o.append([x, 0.7, -2.0]), d.append([1, 0.1 * x, 0]), tm.append(0.5)
        o.append([x, 0.5, -3.0]), d.append([0, 1, 0]), tm.append(0.5)
    for t in (0.0, 0.5, 1.0):  # the moving sphere at three shutter times
        for y in np.linspace(0.0, 2.2, 23):
            o.append([3, y, 3]), d.append([0, 0, -1]), tm.append(t)
            o.append([0, y, 0.01]), d.append([1, 0, 0]), tm.append(t)
    for _ in range(100):  # rays that miss everything: up and away from above
        o.append([0, 3000, 0] + rng.normal(size=3)), d.append([rng.normal(), 1.0, rng.normal()]), tm.append(0.3)
    for _ in range(400):  # and a random cloud
        o.append(rng.uniform(-5, 5, 3) + [0, 2, 0]), d.append(rng.normal(size=3)), tm.append(rng.uniform(0, 1))
    r = np.empty(len(o), dtype=rtow.RAY_DTYPE)
    r["origin"], r["direction"], r["time"], r["tmax"] = np.array(o), np.array(d), np.array(tm), math.inf
    return r


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


@pytest.mark.parametrize("kernel", list(FAST_KERNELS))
def test_handmade_rays_strict_equal_brute_force(qctx, kernel):
    """Axis-parallel rays, rays from inside the glass shell and the hollow, rays in a triangle's plane, the moving
    sphere at three shutter times, rays that miss: every field bit for bit equal to the hittable-list brute force.
    (REFTREE is left out here: it reproduces the reference's TREE, which misses negative-radius spheres and grazing
    hits of flat leaf boxes by design; the logged rays check it against the oracle's tree.)"""
    scene = handmade_scene()
    view = SceneView(scene)
    qctx.upload(scene.c)
    rays = handmade_rays()
    want = brute_force(view, rays)
    got = qctx.intersect(rays, rtow.F64_STRICT, STRICT_KERNELS[kernel])
    assert np.sum(want["front_face"][np.isfinite(want["t"])] == 0) > 50  # the shell rays leave through the far root
    assert np.sum(~np.isfinite(want["t"])) > 100
    assert set(np.unique(want["kind"])) == {-1, 0, 1, 2}
    for f in rtow.HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]) if got[f].dtype.kind == "i" else same_bits(got[f], want[f]), \
            (kernel, f, np.nonzero(np.any((got[f] != want[f]).reshape(len(got), -1), axis=1))[0][:5])


def test_ragged_counts_match_one_batch_and_write_nothing_beyond(qctx, logged):
    import torch

    scene, view, log = logged["cover_static"]
    qctx.upload(scene)
    reps = -(-100003 // len(log))
    rays = rays_of(np.tile(log, (reps, 1))[:100003])
    whole = qctx.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    for n in (0, 1, 63, 64, 65, 100003):
        pad = 64 * 72
        d_hits = torch.full((n * 72 + pad,), 0xAB, dtype=torch.uint8, device="cuda:0")
        st = qctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
        assert st.segments == n
        out = d_hits.cpu().numpy()
        assert np.all(out[n * 72:] == 0xAB), n
        assert out[:n * 72].tobytes() == whole[:n].tobytes(), n


def test_side_stream_right_after_upload_on_a_fresh_context(qctx, logged):
    import torch

    scene, view, log = logged["suzanne"]
    rays = rays_of(log)
    qctx.upload(scene)
    ref = qctx.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    side = torch.cuda.Stream(device="cuda:0")
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.zeros(len(rays) * 72, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for builder in (rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH):
        c = rtow.Context(0)
        try:
            c.set_builder(builder)
            c.upload(scene)  # no wait: the query on the side stream must find the scene complete
            c.intersect_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_AUTO,
                               side.cuda_stream, False)
            side.synchronize()
            assert d_hits.cpu().numpy().tobytes() == ref.tobytes(), builder
        finally:
            c.close()


def test_lean_upload_residency_and_argument_errors(logged):
    scene, view, log = logged["cover_static"]
    rays = rays_of(log[:1000])
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.intersect(rays, rtow.F64_STRICT)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        hits, st = c.intersect(rays, rtow.F64_FAST, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and st.segments == len(rays)
        with pytest.raises(rtow.RtowError) as q:
            c.intersect(rays, rtow.F64_FAST, rtow.KERNEL_BVH)
        import torch

        buf = torch.zeros((40, 60, 3), dtype=torch.float64, device="cuda:0")
        cfg.kernel = rtow.KERNEL_BVH
        with pytest.raises(rtow.RtowError) as r:
            c.render_device(cfg, buf.data_ptr(), 0, False)
        assert "(-4)" in str(q.value) and str(q.value).split(": ", 1)[1] == str(r.value).split(": ", 1)[1]
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, 0), (0, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.intersect(rays, prec, kern)
        L = rtow.lib()
        for n, pr, ph in ((-1, None, None), (1, None, None), ((1 << 31) - 63, 16, 16)):
            assert L.rtow_intersect_device(c._h, 0, 0, pr, n, ph, None, None) == rtow.RTOW_EINVAL, n
        assert L.rtow_intersect_device(c._h, 0, 0, None, 0, None, None, None) == rtow.RTOW_OK
    finally:
        c.close()


def test_queries_leave_the_render_untouched(logged):
    """A render before and after ten queries: bit-identical; the profile ring counts the render launches only."""
    import torch

    scene, view, log = logged["cover_moving"]
    rays = rays_of(log[:50000])
    c = rtow.Context(0)
    try:
        c.upload(scene)
        cfg = rtow.make_config(120, 80, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((80, 120, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        assert c.profile_collect()[1] == 1
        for k in range(10):
            c.intersect(rays, rtow.F64_STRICT if k % 2 else rtow.F64_FAST, [0, 1, 2, 3, 5][k % 5] if k % 2 else 0)
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
    finally:
        c.close()


@pytest.mark.parametrize("kernel", list(FAST_KERNELS))
def test_axis_parallel_rays_on_a_mesh(qctx, logged, kernel):
    """Directions along the axes with zero components of both signs (-e_z has x = y = -0.0) against suzanne, whose
    image feeds the 4-wide walk and the grid: bit for bit the brute force over its 968 triangles, on every walk."""
    scene, view, log = logged["suzanne"]
    qctx.upload(scene)
    g = np.linspace(-0.6, 0.6, 7) + 0.0123457  # (off the mesh's vertex coordinates: no ray along a shared edge)
    o, d = [], []
    for a in range(3):
        for s in (1.0, -1.0):
            e = s * np.eye(3)[a]  # (-1 * e: the zero components are -0.0)
            for u in g:
                for v in g:
                    p = np.zeros(3)
                    p[(a + 1) % 3], p[(a + 2) % 3] = u, v
                    p[a] = -3.0 * s
                    o.append(p), d.append(e)
    rays = rtow.make_rays(np.array(o), np.array(d), time=0.0)
    assert np.signbit(rays["direction"]).sum() > len(rays)
    want = brute_force(view, rays)
    assert np.sum(np.isfinite(want["t"])) > len(rays) // 4
    got = qctx.intersect(rays, rtow.F64_STRICT, FAST_KERNELS[kernel])
    for f in rtow.HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]) if got[f].dtype.kind == "i" else same_bits(got[f], want[f]), (kernel, f)
