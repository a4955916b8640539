"""Scenes and geometry that more than one test module uses: host scenes by name, the hand-made scene and its rays, scenes
from an accel_images.Geometry and their deformations, random scenes, and the subdivided suzanne meshes.

Importing this module loads no library and starts no process: everything that needs librtow.so or liboracle.so is a
function, and SMALL builds its geometry on first use.
"""
import ctypes as C
import math
import sys
from collections.abc import Mapping
from pathlib import Path

import numpy as np

import accel_images as ai
import orc
import rtow
from conftest import GOLDEN, REPO

_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------------ host scenes ---
def cover():
    return rtow.HostScene.cover(11, 1.5, False)


def cover_moving():
    return rtow.HostScene.cover(11, 1.5, True)


def suzanne():
    return rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)


CASES = {
    # name: (scene kind, args, width, aspect, spp, nstreams, depth, seed) — same as make_fixtures.py
    "c1_3spheres": ("cover", (0, 16 / 9, True), 64, 16 / 9, 8, 2, 10, 7),
    "cover_static": ("cover", (11, 1.5, False), 60, 1.5, 4, 2, 50, 1),
    "cover_moving": ("cover", (11, 1.5, True), 60, 1.5, 4, 1, 50, 3),
    "suzanne": ("obj", (16 / 9,), 64, 16 / 9, 4, 2, 20, 5),
}


def make_scene(kind, args):
    if kind == "cover":
        return rtow.HostScene.cover(*args)
    return rtow.HostScene.obj(GOLDEN / "suzanne.obj", *args)


# ----------------------------------------------------------------------------------------------------- meshes ---
def make_mesh():
    """scripts/make_mesh.py as a module (load, subdivide, write_obj)."""
    if str(REPO / "scripts") not in sys.path:
        sys.path.insert(0, str(REPO / "scripts"))
    import make_mesh as mm

    return mm


def suzanne_tris(n_sub=1):
    """[n, 3, 3]: the suzanne fixture's triangles, each subdivided into n_sub x n_sub."""
    mm = make_mesh()
    v, f = mm.load(GOLDEN / "suzanne.obj")
    return mm.subdivide(v, f, n_sub) if n_sub > 1 else np.stack([v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]], axis=1)


def write_mesh_obj(directory, n=10, name=None):
    """Writes suzanne subdivided n x n (n = 10: the 96,800-triangle mesh) as `directory`/m<n>.obj — the file
    `python scripts/make_mesh.py OUT.obj n` writes — and returns its path."""
    mm = make_mesh()
    out = Path(directory) / (name or f"m{n}.obj")
    v, f = mm.load(GOLDEN / "suzanne.obj")
    mm.write_obj(mm.subdivide(v, f, n), out)
    return out


# ------------------------------------------------------------------------------------------------ scene views ---
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


# ---------------------------------------------------------------------------- the hand-made scene and its rays ---
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
    pi = lambda a: a.ctypes.data_as(_pi)  # noqa: E731
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


# ------------------------------------------------------------------------- scenes of an accel_images.Geometry ---
def to_scene(G, keep):
    """An rtow.Scene with G's exact binary64 coordinates and the cover scene's camera (shutter [0, 1])."""
    base = rtow.HostScene.cover(0, 1.5, False)
    sc = rtow.Scene()
    sc.camera = base.c.camera
    arrs = [np.ascontiguousarray(a, np.float64) for a in (G.sph, G.mov, G.tri)]
    pm = [np.ascontiguousarray(G.pmat[a:b], np.int32) for a, b in ((0, G.ns), (G.ns, G.ns + G.nm), (G.ns + G.nm, G.np))]
    mats = (rtow.Material * len(G.mats))()
    for i, (kind, albedo, fuzz, ir) in enumerate(G.mats):
        mats[i].kind, mats[i].fuzz, mats[i].ir = kind, fuzz, ir
        mats[i].albedo = (C.c_double * 3)(*albedo)
    sc.n_spheres, sc.sphere_geom, sc.sphere_mat = G.ns, arrs[0].ctypes.data_as(_pd), pm[0].ctypes.data_as(_pi)
    sc.n_moving, sc.moving_geom, sc.moving_mat = G.nm, arrs[1].ctypes.data_as(_pd), pm[1].ctypes.data_as(_pi)
    sc.n_triangles, sc.triangle_geom, sc.triangle_mat = G.nt, arrs[2].ctypes.data_as(_pd), pm[2].ctypes.data_as(_pi)
    sc.n_materials, sc.materials, sc.n_prims = len(G.mats), mats, G.np
    keep.extend([base, arrs, pm, mats])
    G.cam = np.array(sc.camera.origin[:])
    return sc


def resident_images(ctx):
    return {w: ctx.debug_image(w) for w in range(6)}


def _set_order(sc, G, keep, perm=None):
    """prim_kind / prim_index of sc: class-major insertion order, permuted by `perm`."""
    kind = np.array([rtow.PRIM_SPHERE] * G.ns + [rtow.PRIM_MOVING_SPHERE] * G.nm + [rtow.PRIM_TRIANGLE] * G.nt, np.int32)
    index = np.concatenate([np.arange(G.ns), np.arange(G.nm), np.arange(G.nt)]).astype(np.int32)
    if perm is not None:
        kind, index = np.ascontiguousarray(kind[perm]), np.ascontiguousarray(index[perm])
    sc.prim_kind, sc.prim_index = kind.ctypes.data_as(_pi), index.ctypes.data_as(_pi)
    keep.extend([kind, index])
    return sc


set_order = _set_order  # (the name other modules import)


def scene_of(G, keep, cam_shift=None, shutter=None):
    """An rtow.Scene of G (to_scene: the cover scene's camera) with its class-major insertion order (the oracle reads
    one), the camera translated by cam_shift and its shutter replaced; G.cam follows the camera origin."""
    sc = _set_order(to_scene(G, keep), G, keep)
    if cam_shift is not None:
        for f in ("origin", "lower_left_corner"):
            v = getattr(sc.camera, f)
            for k in range(3):
                v[k] += float(cam_shift[k])
    if shutter is not None:
        sc.camera.t0, sc.camera.t1 = shutter
    G.cam = np.array(sc.camera.origin[:])
    return sc


def _copy(G):
    return ai.Geometry(G.sph.copy(), G.mov.copy(), G.tri.copy(), G.pmat.copy(), list(G.mats), G.cam.copy())


def _points(G):
    """Every point of the geometry as [n][3] views' sources: (sphere centres, c0, c1, triangle vertices)."""
    return [G.sph[:, 0:3], G.mov[:, 0:3], G.mov[:, 3:6]] + [G.tri[:, 3 * v:3 * v + 3] for v in range(3)]


def _extent(G):
    pts = np.concatenate([p for p in _points(G) if len(p)])
    lo, hi = pts.min(0), pts.max(0)
    return lo, hi, float(max(np.max(hi - lo), 1e-3))


def deform(G, f, radius=None):
    """A copy of G with f applied to every point ([n][3] -> [n][3]) and `radius` (|r| scale) to the radii."""
    H = _copy(G)
    H.sph[:, 0:3], H.mov[:, 0:3], H.mov[:, 3:6] = f(G.sph[:, 0:3]), f(G.mov[:, 0:3]), f(G.mov[:, 3:6])
    for v in range(3):
        H.tri[:, 3 * v:3 * v + 3] = f(G.tri[:, 3 * v:3 * v + 3])
    if radius is not None:
        H.sph[:, 3] *= radius
        H.mov[:, 6] *= radius
    return H


def motions(G):
    """name -> (Geometry, camera shift): the deformations every check runs."""
    lo, hi, ext = _extent(G)
    ctr = 0.5 * (lo + hi)
    g = np.random.default_rng(5)
    a = 0.6
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    out = {
        "translate": (deform(G, lambda p: p + np.array([0.7, -0.3, 0.2]) * ext), None),
        "rotate": (deform(G, lambda p: (p - ctr) @ rot.T + ctr), None),
        "jitter": (deform(G, lambda p: p + g.normal(scale=0.02 * ext, size=p.shape)), None),
        "scale1000": (deform(G, lambda p: p * 1000.0, radius=1000.0), None),
        "flatten": (deform(G, lambda p: np.c_[p[:, 0], np.full(len(p), ctr[1]), p[:, 2]]), None),
        "camera": (_copy(G), np.array([1.5, 0.5, -2.0])),
    }
    if G.ns >= 2:
        H = _copy(G)
        H.sph[[0, G.ns - 1], 0:3] = G.sph[[G.ns - 1, 0], 0:3]
        out["swap_spheres"] = (H, None)
    if G.nm >= 1:
        H = _copy(G)
        H.mov[0, 3:6] = G.mov[0, 3:6] + np.array([0.3, 0.1, -0.2]) * ext
        out["moving_c1"] = (H, None)
    return out


def wave(G, frame, frames=16, amp=0.05):
    """A travelling sine wave along x, displacing y by amp x the extent (frame 0: unchanged)."""
    lo, hi, ext = _extent(G)
    ph = 2 * np.pi * frame / frames
    return deform(G, lambda p: p + np.c_[np.zeros(len(p)), amp * ext * np.sin(2 * np.pi * (p[:, 0] - lo[0]) / ext + ph)
                                         * (frame > 0), np.zeros(len(p))])


def rays_for(G, n, seed):
    """Camera rays toward the scene, random rays through its box, shadow rays (tmax 1) toward a light above it."""
    lo, hi, ext = _extent(G)
    g = np.random.default_rng(seed)
    tgt = g.uniform(lo, hi, size=(n, 3))
    cam = rtow.make_rays(np.repeat(G.cam[None], n, 0), tgt - G.cam, time=g.random(n))
    o = g.uniform(lo - 0.2 * ext, hi + 0.2 * ext, size=(n, 3))
    d = g.normal(size=(n, 3))
    rnd = rtow.make_rays(o, d, time=g.random(n))
    light = 0.5 * (lo + hi) + np.array([0.2, 1.5, 0.1]) * ext
    sh = rtow.make_rays(tgt, light - tgt, time=g.random(n), tmax=1.0)
    return np.concatenate([cam, rnd, sh])


def small_scenes():
    """name -> Geometry: the cover scene with moving spheres, suzanne, the meshes around the LDS limit, the edge meshes
    and the sphere edge scenes."""
    hs = cover_moving()
    out = {"cover_moving": ai.Geometry.of_scene(hs.c), "suzanne": ai.mesh_geometry(suzanne_tris(1))}
    hs.close()
    tris2 = suzanne_tris(2)
    for n in (850, 1400):
        out[f"suz{n}"] = ai.mesh_geometry(tris2[:n])
    out.update({f"edge_{k}": ai.mesh_geometry(v) for k, v in ai.edge_meshes().items()})
    out.update({f"sph_{k}": v for k, v in ai.sphere_edge_scenes().items()})
    return out


class _Small(Mapping):
    """small_scenes() behind its names: the names (what the parametrisations take) need no library, the geometry is
    built on first use, once per process."""

    def __init__(self):
        self._names = (["cover_moving", "suzanne", "suz850", "suz1400"] + [f"edge_{k}" for k in ai.edge_meshes()]
                       + [f"sph_{k}" for k in ai.sphere_edge_scenes()])
        self._built = None

    def __getitem__(self, name):
        if name not in self._names:
            raise KeyError(name)
        if self._built is None:
            self._built = small_scenes()
            assert list(self._built) == self._names
        return self._built[name]

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


SMALL = _Small()


# ---------------------------------------------------------------------------------------------- random scenes ---
def random_scene(seed, n_sph, n_mov, n_tri, keep):
    """Spheres of very different sizes over a big ground sphere, moving spheres and triangles, all three materials;
    insertion order = class-major order."""
    rng = np.random.default_rng(seed)
    base = rtow.HostScene.cover(0, 1.5, False)
    g = 0 if (n_sph == 0 and n_mov == 0) else 1  # triangle-only scenes stay triangle-only (the BVH4 kernel's case)
    sph = np.zeros((n_sph + g, 4))
    if g:
        sph[0] = [0.0, -200.5, 0.0, 200.0]  # a big ground sphere among small ones
    sph[g:, :3] = rng.uniform(-3, 3, size=(n_sph, 3)) * [1, 0.4, 1] + [0, 0.6, 0]
    sph[g:, 3] = rng.choice([0.05, 0.15, 0.4, 0.9], size=n_sph, p=[0.4, 0.4, 0.15, 0.05])
    mov = np.zeros((n_mov, 8))  # c0 xyz, c1 xyz, radius, pad
    mov[:, :3] = rng.uniform(-3, 3, size=(n_mov, 3)) * [1, 0.4, 1] + [0, 0.6, 0]
    mov[:, 3:6] = mov[:, :3] + rng.uniform(-0.4, 0.4, size=(n_mov, 3))
    mov[:, 6] = rng.uniform(0.05, 0.3, size=n_mov)
    tri = np.zeros((n_tri, 9))
    c = rng.uniform(-3, 3, size=(n_tri, 3)) * [1, 0.3, 1] + [0, 0.8, 0]
    for k in range(3):
        tri[:, 3 * k:3 * k + 3] = c + rng.uniform(-0.5, 0.5, size=(n_tri, 3))
    n_mat = 8
    mats = (rtow.Material * n_mat)()
    for i in range(n_mat):
        kind = [rtow.MAT_LAMBERTIAN, rtow.MAT_METAL, rtow.MAT_DIELECTRIC][i % 3]
        mats[i].kind = kind
        mats[i].albedo = (C.c_double * 3)(*rng.uniform(0.3, 0.95, 3))
        mats[i].fuzz = float(rng.uniform(0, 0.5)) if kind == rtow.MAT_METAL else 0.0
        mats[i].ir = 1.5
    ns, nm, nt = n_sph + g, n_mov, n_tri
    smat = rng.integers(0, n_mat, max(ns, 1)).astype(np.int32)
    smat[0] = 0  # Lambertian ground
    mmat = rng.integers(0, n_mat, max(nm, 1)).astype(np.int32)
    tmat = (rng.integers(0, n_mat // 3, max(nt, 1)) * 3).astype(np.int32)  # triangles: Lambertian only
    kinds = np.concatenate([np.zeros(ns), np.ones(nm), np.full(nt, 2)]).astype(np.int32)
    index = np.concatenate([np.arange(ns), np.arange(nm), np.arange(nt)]).astype(np.int32)
    sc = rtow.Scene()
    sc.camera = base.c.camera
    sc.n_spheres, sc.n_moving, sc.n_triangles = ns, nm, nt
    sph_c, mov_c, tri_c = np.ascontiguousarray(sph), np.ascontiguousarray(mov), np.ascontiguousarray(tri)
    sc.sphere_geom, sc.sphere_mat = sph_c.ctypes.data_as(_pd), smat.ctypes.data_as(_pi)
    sc.moving_geom, sc.moving_mat = mov_c.ctypes.data_as(_pd), mmat.ctypes.data_as(_pi)
    sc.triangle_geom, sc.triangle_mat = tri_c.ctypes.data_as(_pd), tmat.ctypes.data_as(_pi)
    sc.n_materials = n_mat
    sc.materials = mats
    sc.n_prims = ns + nm + nt
    sc.prim_kind, sc.prim_index = kinds.ctypes.data_as(_pi), index.ctypes.data_as(_pi)
    keep.extend([base, sph_c, mov_c, tri_c, mats, smat, mmat, tmat, kinds, index])
    return sc


def random_sphere_scene(hollow):
    """(scene, keep-alive): a ground sphere, a glass sphere with an inner sphere (negative radius if `hollow`) and 40
    overlapping small spheres, a material per primitive."""
    n = 40
    rng = np.random.default_rng(3)
    geom = np.zeros((n + 3, 4))
    geom[0] = [0, -100.5, -1, 100]
    geom[1] = [0, 0, -1, 0.5]
    geom[2] = [0, 0, -1, -0.45 if hollow else 0.2]  # hollow glass: negative inner radius
    geom[3:, :3] = rng.uniform(-2, 2, size=(n, 3)) + [0, 0.5, -3]
    geom[3:, 3] = rng.uniform(0.05, 0.3, size=n)
    mats = (rtow.Material * (n + 3))()
    for i in range(n + 3):
        kind = [rtow.MAT_LAMBERTIAN, rtow.MAT_DIELECTRIC, rtow.MAT_DIELECTRIC][i] if i < 3 else int(rng.integers(0, 3))
        mats[i].kind = kind
        mats[i].albedo = (C.c_double * 3)(*rng.uniform(0.2, 0.9, 3))
        mats[i].fuzz = float(rng.uniform(0, 0.4)) if kind == rtow.MAT_METAL else 0.0
        mats[i].ir = 1.5
    base = rtow.HostScene.cover(0, 2.0, False)
    sc = rtow.Scene()
    sc.camera = base.c.camera
    keep = dict(g=np.ascontiguousarray(geom), mi=np.arange(n + 3, dtype=np.int32),
                kinds=np.zeros(n + 3, dtype=np.int32), mats=mats)
    sc.n_spheres = n + 3
    sc.sphere_geom = keep["g"].ctypes.data_as(_pd)
    sc.sphere_mat = keep["mi"].ctypes.data_as(_pi)
    sc.n_materials = n + 3
    sc.materials = mats
    sc.n_prims = n + 3
    sc.prim_kind = keep["kinds"].ctypes.data_as(_pi)
    sc.prim_index = keep["mi"].ctypes.data_as(_pi)
    return sc, keep


# ------------------------------------------------------------------------------- spheres under a chosen camera ---
def look_at(lookfrom, lookat, vup, vfov=70.0, aspect=1.5):
    """The reference's pinhole camera (lens radius 0, focus distance 1)."""
    o, at, up = (np.asarray(a, float) for a in (lookfrom, lookat, vup))
    vh = 2.0 * math.tan(math.radians(vfov) / 2.0)
    w = (o - at) / np.linalg.norm(o - at)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    cam = rtow.Camera()
    hor, ver = aspect * vh * u, vh * v
    for name, val in (("origin", o), ("u", u), ("v", v), ("w", w), ("horizontal", hor), ("vertical", ver),
                      ("lower_left_corner", o - hor / 2 - ver / 2 - w)):
        setattr(cam, name, (C.c_double * 3)(*val))
    cam.lens_radius, cam.t0, cam.t1 = 0.0, 0.0, 1.0
    return cam


def sphere_scene(centres, radius, cam, keep):
    """A ground sphere (top at y = -1) plus small spheres of one radius; Lambertian ground, the three materials in turn."""
    n = len(centres)
    sph = np.zeros((n + 1, 4))
    sph[0] = [0.0, -1001.0, 0.0, 1000.0]
    sph[1:, :3] = centres
    sph[1:, 3] = radius
    mats = (rtow.Material * 4)()
    for i, (kind, alb, fuzz) in enumerate(((rtow.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0), (rtow.MAT_LAMBERTIAN, (0.8, 0.3, 0.2), 0.0),
                                           (rtow.MAT_METAL, (0.7, 0.8, 0.9), 0.1), (rtow.MAT_DIELECTRIC, (1.0, 1.0, 1.0), 0.0))):
        mats[i].kind, mats[i].albedo, mats[i].fuzz, mats[i].ir = kind, (C.c_double * 3)(*alb), fuzz, 1.5
    smat = (1 + np.arange(n + 1) % 3).astype(np.int32)
    smat[0] = 0
    kinds, index = np.zeros(n + 1, np.int32), np.arange(n + 1, dtype=np.int32)
    none_d, none_i = np.zeros(1), np.zeros(1, np.int32)
    sc = rtow.Scene()
    sc.camera = cam
    sc.n_spheres, sc.n_moving, sc.n_triangles = n + 1, 0, 0
    sc.sphere_geom, sc.sphere_mat = sph.ctypes.data_as(_pd), smat.ctypes.data_as(_pi)
    sc.moving_geom, sc.moving_mat = none_d.ctypes.data_as(_pd), none_i.ctypes.data_as(_pi)
    sc.triangle_geom, sc.triangle_mat = none_d.ctypes.data_as(_pd), none_i.ctypes.data_as(_pi)
    sc.n_materials, sc.materials = 4, mats
    sc.n_prims = n + 1
    sc.prim_kind, sc.prim_index = kinds.ctypes.data_as(_pi), index.ctypes.data_as(_pi)
    keep.extend([sph, mats, smat, kinds, index, none_d, none_i, cam])
    return sc
