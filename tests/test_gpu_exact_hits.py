"""Closest-hit and any-hit queries of both builds against the exact reference (tests/exact_hits.py) on the GPU.

Every walk (BRUTE, BVH, GRID, BVH4, with the render's fallbacks; both builders where a tree is involved) in F64_STRICT
and F64_FAST, on the rays where kernels go wrong: logged render segments, rays at and across shared edges and
vertices, tangent rays, rays at the triangle cut, rays leaving a surface, direction magnitudes from 1e-4 to 1e4, scenes
far from the origin and scenes after a refit.  On a decided ray every field must be the exact answer (t, point and a
sphere's normal within their bounds); an undecided ray's answer must be explainable by the band.  Counts per case are
printed: decided, undecided, rays whose t is not the exact t rounded, and the worst t error in units of its bound.
"""
import numpy as np
import pytest

import accel_images as ai
import exact_hits as ex
import rtow
from test_gpu_query import LOGGED, SceneView, handmade_scene, log_rays, rays_of
from test_gpu_refit import deform, motions, rays_for, scene_of

pytestmark = pytest.mark.gpu

WALKS = {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID, "bvh4": rtow.KERNEL_BVH4}
BUILDERS = {"host": rtow.BUILDER_HOST_SAH, "device": rtow.BUILDER_DEVICE_LBVH}
BUILDS = {ex.STRICT: rtow.F64_STRICT, ex.FAST: rtow.F64_FAST}
SHARE = 1e-3  # the undecided share allowed on logged and random rays


@pytest.fixture(scope="module")
def qctx():
    c = rtow.Context(0)
    yield c
    c.close()


def run_case(ctx, name, upload, scene, rays, share=None, refit=None):
    """Every walk x build x builder on `rays`; `upload` is what ctx.upload takes, `refit` (optional) a scene refitted
    over it — `scene` (exact_hits.Scene) is then the refitted geometry."""
    refs = {}
    has_tri = len(scene.tri) > 0

    def ref(build, unit_cut):
        key = (build, unit_cut and has_tri)
        if key not in refs:
            refs[key] = ex.Reference(scene, rays, build, unit_cut=key[1])
        return refs[key]

    lines = []
    for bname, builder in BUILDERS.items():
        ctx.set_builder(builder)
        try:
            ctx.upload(upload)
            if refit is not None:
                ctx.refit(refit)
            for wname, walk in WALKS.items():
                if wname == "brute" and (bname == "device" or len(scene.kind) > 4096):
                    continue  # (the brute force does not depend on the builder; 96,800 tests per ray are not a test)
                for build, prec in BUILDS.items():
                    hits, st = ctx.intersect(rays, prec, walk, want_stats=True)
                    occ = ctx.occluded(rays, prec, walk)
                    r = ref(build, build == ex.FAST and st.kernel_used == rtow.KERNEL_GRID)
                    s = ex.check(r, hits, occ, (name, bname, wname, build, st.kernel_used))
                    lines.append(f"  {bname:6s} {wname:5s}(used {st.kernel_used}) {build:6s}: decided {s['decided']}, "
                                 f"undecided {s['undecided']} (any-hit {s['occ_undecided']}), t differs {s['t_differs']}, "
                                 f"worst t err {s['worst_t_err']:.3f} of bound")
                    if share is not None:
                        assert s["undecided"] <= share * s["rays"], (name, s)
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    print(f"\n{name}: {len(rays)} rays, {sum(r.n_exact for r in refs.values())} exact pairs\n" + "\n".join(lines))


def _sub(log, n, seed):
    g = np.random.default_rng(seed)
    return log[np.sort(g.choice(len(log), size=min(n, len(log)), replace=False))]


@pytest.fixture(scope="module")
def logged():
    out = {}
    for name, (mk, w, h, spp, depth, seed) in LOGGED.items():
        hs = mk()
        cfg = rtow.make_config(w, h, 1, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        view = SceneView(hs)
        out[name] = (hs, view, ex.Scene.of(view), log_rays(hs, cfg))
    return out


@pytest.fixture(scope="module")
def big_mesh():
    import subprocess
    import sys
    import tempfile
    from conftest import REPO

    d = tempfile.mkdtemp()
    obj = f"{d}/m10.obj"
    subprocess.run([sys.executable, str(REPO / "scripts" / "make_mesh.py"), obj, "10"], check=True, capture_output=True)
    hs = rtow.HostScene.obj(obj, 16 / 9)
    assert hs.c.n_triangles == 96800
    view = SceneView(hs)
    cfg = rtow.make_config(32, 18, 1, 1, 20, seed=24, precision=rtow.F64_STRICT)
    return hs, view, ex.Scene.of(view), log_rays(hs, cfg, accel=True)


# ---- logged and random rays ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LOGGED))
def test_logged_rays(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"logged/{name}", hs, sc, rays_of(_sub(log, 5000, 1)), share=SHARE)


def test_logged_rays_big_mesh(qctx, big_mesh):
    hs, view, sc, log = big_mesh
    run_case(qctx, "logged/mesh96k", hs, sc, rays_of(_sub(log, 400, 2)), share=SHARE)


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_random_rays(qctx, logged, name):
    hs, view, sc, log = logged[name]
    g = np.random.default_rng(9)
    small = view.sph[np.abs(view.sph[:, 3]) < 10, :3] if len(view.tri) == 0 else view.tri[:, :3]
    lo, hi = small.min(0), small.max(0)
    ext = float(np.max(hi - lo))
    n = 4000
    o = g.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(n, 3))
    d = g.normal(size=(n, 3))
    rays = rtow.make_rays(o, d, time=g.random(n), tmax=np.where(g.random(n) < 0.3, g.uniform(0.1, 5, n), np.inf))
    run_case(qctx, f"random/{name}", hs, sc, rays, share=SHARE)


# ---- edges and vertices -------------------------------------------------------------------------------------------
def edge_rays(tri, n, seed):
    """Rays at points on edges (offsets eps x edge length to either side, in the plane) and at vertices, from the front
    and from the back of the triangle."""
    g = np.random.default_rng(seed)
    pick = g.choice(len(tri), size=min(n, len(tri)), replace=False)
    o, d = [], []
    for k in pick:
        A, B, C = tri[k, 0:3], tri[k, 3:6], tri[k, 6:9]
        nrm = np.cross(B - A, C - A)
        if not np.linalg.norm(nrm) > 0:
            continue
        nrm = nrm / np.linalg.norm(nrm)
        e = [(A, B), (B, C), (C, A)][g.integers(3)]
        w = np.cross(nrm, e[1] - e[0])
        ln = np.linalg.norm(e[1] - e[0])
        pts = [A, B, C]
        s = g.uniform(0.2, 0.8)
        for eps in (0.0, 1e-15, 1e-12, 1e-9, 1e-6):
            for sg in (1.0, -1.0):
                pts.append(e[0] + s * (e[1] - e[0]) + sg * eps * ln * w / max(np.linalg.norm(w), 1e-300))
        for p in pts:
            tilt = g.normal(size=3) * 0.2
            for side in (1.0, -1.0):
                dd = -side * nrm + tilt
                o.append(p - 2.0 * dd), d.append(dd)
    return rtow.make_rays(np.array(o), np.array(d), time=0.0)


def mesh_case(G, keep):
    sc = scene_of(G, keep)
    return sc, ex.Scene.class_major(G.sph, G.mov, G.tri, G.pmat)


@pytest.mark.parametrize("name", ["suzanne", "n4", "coincident", "zero_area", "flat_z", "off_1e4", "big_and_small"])
def test_edge_and_vertex_rays(qctx, logged, name):
    if name == "suzanne":
        hs, view, sc, log = logged[name]
        up, tri = hs, view.tri
    else:
        G = ai.mesh_geometry(ai.edge_meshes()[name])
        keep = []
        up, sc = mesh_case(G, keep)
        tri = G.tri
    run_case(qctx, f"edges/{name}", up, sc, edge_rays(tri, 80, 3))


# ---- tangent rays ---------------------------------------------------------------------------------------------------
def tangent_rays(centres, radii, times, seed):
    g = np.random.default_rng(seed)
    o, d, tm = [], [], []
    for c, r, t in zip(centres, radii, times):
        for eps in (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6):
            w = g.normal(size=3)
            w /= np.linalg.norm(w)
            u = np.cross(w, g.normal(size=3))
            u /= np.linalg.norm(u)
            dist = abs(r) * (1 + eps)
            L = g.uniform(2, 6) * abs(r) if abs(r) < 100 else 30.0
            o.append(c + dist * u - L * w), d.append(w * g.uniform(0.5, 2)), tm.append(t)
    return rtow.make_rays(np.array(o), np.array(d), time=np.array(tm))


def handmade_tangent_rays(view):
    c, r, t = [], [], []
    for s in view.sph:
        for _ in range(6):
            c.append(s[:3]), r.append(s[3]), t.append(0.5)
    for m in view.mov:
        for tm in (0.0, 0.25, 0.5, 1.0):
            for _ in range(3):
                c.append(m[:3] + tm * (m[3:6] - m[:3])), r.append(m[6]), t.append(tm)
    return tangent_rays(c, r, t, 4)


def cover_tangent_rays(view):
    g = np.random.default_rng(6)
    c, r, t = [view.sph[0, :3]] * 4, [view.sph[0, 3]] * 4, [0.0] * 4
    for i in g.choice(len(view.sph), 40, replace=False):
        c.append(view.sph[i, :3]), r.append(view.sph[i, 3]), t.append(0.3)
    for i in g.choice(len(view.mov), 40, replace=False):
        tm = float(g.choice([0.0, 0.5, 1.0, g.random()]))
        m = view.mov[i]
        c.append(m[:3] + tm * (m[3:6] - m[:3])), r.append(m[6]), t.append(tm)
    return tangent_rays(c, r, t, 5)


def test_tangent_rays(qctx, logged):
    """The ground sphere, the small spheres, a hollow sphere, moving spheres at several times (handmade scene and the
    moving cover scene)."""
    h = handmade_scene()
    view = SceneView(h)
    run_case(qctx, "tangent/handmade", h.c, ex.Scene.of(view), handmade_tangent_rays(view))
    hs, view, sc, log = logged["cover_moving"]
    run_case(qctx, "tangent/cover_moving", hs, sc, cover_tangent_rays(view))


# ---- the triangle cut, surfaces, direction magnitudes ------------------------------------------------------------------
def det_cut_rays(view, sc):
    g = np.random.default_rng(8)
    o, d = [], []
    for k in g.choice(len(view.tri), 150, replace=False):
        A, B, C = view.tri[k, 0:3], view.tri[k, 3:6], view.tri[k, 6:9]
        n = sc.tri_n[k]
        P = (A + B + C) / 3
        for delta in (-1e-3, -1e-9, -1e-12, 0.0, 1e-12, 1e-9, 1e-3):
            dd = -n / np.dot(n, n) * 1e-6 * (1 + delta)
            o.append(P - 100 * dd), d.append(dd)
    return rtow.make_rays(np.array(o), np.array(d))


def test_rays_at_the_det_cut(qctx, logged):
    hs, view, sc, log = logged["suzanne"]
    run_case(qctx, "det_cut/suzanne", hs, sc, det_cut_rays(view, sc))


def surface_rays(log):
    hit = log[np.isfinite(log[:, 10])]
    hit = _sub(hit, 1500, 4)
    g = np.random.default_rng(10)
    p = hit[:, 3:6] + hit[:, 10:11] * hit[:, 6:9]
    d = g.normal(size=(len(hit), 3))
    return rtow.make_rays(p, d, time=hit[:, 9])


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_rays_from_surfaces(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"surfaces/{name}", hs, sc, surface_rays(log))


def magnitude_rays(log):
    parts = []
    for k, s in enumerate((1e-4, 1e-2, 1e2, 1e4)):
        r = rays_of(_sub(log, 800, 20 + k))
        r["direction"] *= s
        parts.append(r)
    return np.concatenate(parts)


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_direction_magnitudes(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"magnitudes/{name}", hs, sc, magnitude_rays(log))


# ---- far scenes, refits ---------------------------------------------------------------------------------------------
def far_case(hs, log, offset):
    """(scene to upload, its exact_hits.Scene, rays, what keeps the upload's arrays alive): the scene and 3000 logged
    rays moved by `offset` x (1, -0.5, 0.75)."""
    G = ai.Geometry.of_scene(hs.c)
    off = np.array([offset, -0.5 * offset, 0.75 * offset])
    H = deform(G, lambda p: p + off)
    keep = []
    up = scene_of(H, keep, cam_shift=off)
    sc = ex.Scene.class_major(H.sph, H.mov, H.tri, H.pmat)
    rays = rays_of(_sub(log, 3000, 5))
    rays["origin"] += off
    return up, sc, rays, keep


@pytest.mark.parametrize("offset", [1e4, 1e5])
@pytest.mark.parametrize("name", ["cover_static", "suzanne"])
def test_far_scenes(qctx, logged, name, offset):
    hs, view, sc0, log = logged[name]
    up, sc, rays, keep = far_case(hs, log, offset)
    run_case(qctx, f"far/{name}/{offset:g}", up, sc, rays)


def refit_case(hs, motion, n):
    """(scene to upload, scene to refit over it, the refitted geometry's exact_hits.Scene, 3 n rays, keep-alive)."""
    G = ai.Geometry.of_scene(hs.c)
    keep = []
    base = scene_of(G, keep)
    H = motions(G)[motion][0]
    new = scene_of(H, keep)
    sc = ex.Scene.class_major(H.sph, H.mov, H.tri, H.pmat)
    return base, new, sc, rays_for(H, n, 7), keep


@pytest.mark.parametrize("motion", ["translate", "scale1000", "flatten"])
@pytest.mark.parametrize("name", ["cover_moving", "mesh96k"])
def test_after_refit(qctx, logged, big_mesh, name, motion):
    hs = logged["cover_moving"][0] if name == "cover_moving" else big_mesh[0]
    base, new, sc, rays, keep = refit_case(hs, motion, 1500 if name == "cover_moving" else 100)
    run_case(qctx, f"refit/{name}/{motion}", base, sc, rays, refit=new)
