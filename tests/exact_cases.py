"""The cases of the exact-hit checkers (test_gpu_exact_hits.py, test_gpu_exact_sequences.py and the host self-tests in
test_exact_hits_host.py): the logged renders with their exact_hits.Scene, and the rays where kernels go wrong — at and
across shared edges and vertices, tangent to spheres, at the triangle cut, leaving a surface, with direction magnitudes
from 1e-4 to 1e4 — and the far and refitted scenes.  Importing this module loads no library."""
import numpy as np
import pytest

import accel_images as ai
import exact_hits as ex
import rtow
from support_oracle import LOGGED, log_rays, rays_of
from support_scenes import SceneView, deform, motions, rays_for, scene_of, write_mesh_obj

BUILDS = {ex.STRICT: rtow.F64_STRICT, ex.FAST: rtow.F64_FAST}
SHARE = 1e-3  # the undecided share allowed on logged and random rays


def subsample(log, n, seed):
    g = np.random.default_rng(seed)
    return log[np.sort(g.choice(len(log), size=min(n, len(log)), replace=False))]


@pytest.fixture(scope="module")
def logged():
    """name -> (host scene, view, exact_hits.Scene, log) of the LOGGED renders at 1 spp."""
    out = {}
    for name, (mk, w, h, spp, depth, seed) in LOGGED.items():
        hs = mk()
        cfg = rtow.make_config(w, h, 1, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        view = SceneView(hs)
        out[name] = (hs, view, ex.Scene.of(view), log_rays(hs, cfg))
    return out


@pytest.fixture(scope="module")
def big_mesh(tmp_path_factory):
    """The same of the 96,800-triangle mesh: a 32x18 render at 1 spp (the checker's tree)."""
    hs = rtow.HostScene.obj(write_mesh_obj(tmp_path_factory.mktemp("mesh")), 16 / 9)
    assert hs.c.n_triangles == 96800
    view = SceneView(hs)
    cfg = rtow.make_config(32, 18, 1, 1, 20, seed=24, precision=rtow.F64_STRICT)
    return hs, view, ex.Scene.of(view), log_rays(hs, cfg, accel=True)


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


def surface_rays(log):
    hit = log[np.isfinite(log[:, 10])]
    hit = subsample(hit, 1500, 4)
    g = np.random.default_rng(10)
    p = hit[:, 3:6] + hit[:, 10:11] * hit[:, 6:9]
    d = g.normal(size=(len(hit), 3))
    return rtow.make_rays(p, d, time=hit[:, 9])


def magnitude_rays(log):
    parts = []
    for k, s in enumerate((1e-4, 1e-2, 1e2, 1e4)):
        r = rays_of(subsample(log, 800, 20 + k))
        r["direction"] *= s
        parts.append(r)
    return np.concatenate(parts)


def far_case(hs, log, offset):
    """(scene to upload, its exact_hits.Scene, rays, what keeps the upload's arrays alive): the scene and 3000 logged
    rays moved by `offset` x (1, -0.5, 0.75)."""
    G = ai.Geometry.of_scene(hs.c)
    off = np.array([offset, -0.5 * offset, 0.75 * offset])
    H = deform(G, lambda p: p + off)
    keep = []
    up = scene_of(H, keep, cam_shift=off)
    sc = ex.Scene.class_major(H.sph, H.mov, H.tri, H.pmat)
    rays = rays_of(subsample(log, 3000, 5))
    rays["origin"] += off
    return up, sc, rays, keep


def refit_case(hs, motion, n):
    """(scene to upload, scene to refit over it, the refitted geometry's exact_hits.Scene, 3 n rays, keep-alive)."""
    G = ai.Geometry.of_scene(hs.c)
    keep = []
    base = scene_of(G, keep)
    H = motions(G)[motion][0]
    new = scene_of(H, keep)
    sc = ex.Scene.class_major(H.sph, H.mov, H.tri, H.pmat)
    return base, new, sc, rays_for(H, n, 7), keep
