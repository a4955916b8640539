"""The cases of the swept-sphere checkers (test_sweep_host.py, test_gpu_sweep.py): the hand scene, the hand-placed sweeps
around one primitive of each class, and the random sweep sets of a scene.  numpy and point_ref / sweep_ref only: importing
this module loads no library (hand_scene, which builds the rtow.Scene of the hand geometry, imports rtow itself)."""
import math

import numpy as np

import point_ref as pr
import sweep_ref as sr


# ------------------------------------------------------------------------------------------------ the hand scene ---
def hand_geometry():
    """(sph [n, 4], mov [n, 8], tri [n, 9], kind, index, material per class): about 40 primitives with every class, a
    hollow glass sphere, two equal spheres, a large sphere around everything, a sliver, a zero-area triangle, a point
    triangle, coplanar triangles sharing an edge and a creased fan; insertion order differs from class-major order."""
    g = np.random.default_rng(11)
    sph = [[0, 1, 0, 1.0], [0, 1, 0, -0.8],            # hollow glass
           [-3, 1, 0.5, 0.7], [2.5, 0.4, 2.0, 0.4], [2.5, 0.4, 2.0, 0.4],  # ... and two equal spheres
           [0, 0, 0, 40.0],                             # a large sphere around everything: cast inside it
           [-2, 2.5, -1, 0.25], [1.5, 3.0, 1.5, 0.05]]
    mov = [[3, 0.5, 0, 3, 1.5, 0, 0.5, 0], [-1, 2, 3, -2, 2.5, 2, 0.3, 0]]
    tri = [[-1, 0, -2, 1, 0, -2, 1, 2, -2], [-1, 0, -2, 1, 2, -2, -1, 2, -2],      # a quad: coplanar, one shared edge
           [2, 0, -3, 4, 0, -3, 3, 2.5, -3],
           [-4, 0, 2, -2, 0, 2, -3, 1, 3], [-2, 0, 2, -4, 0, 2, -3, 1, 1],          # a crease along a shared edge
           [-3, 1, 3, -3, 1, 1, -2, 0, 2], [-3, 1, 1, -3, 1, 3, -4, 0, 2],          # ... closing the fan at two apexes
           [0, 3, 0, 2, 3, 0, 1, 3 + 1e-7, 1e-7],                                    # a sliver
           [1, 2, 2, 2, 2, 2, 3, 2, 2],                                              # zero area: collinear
           [0.5, 2.5, -1, 0.5, 2.5, -1, 0.5, 2.5, -1]]                               # zero area: a point
    for _ in range(20):
        c = g.uniform(-4, 4, 3) * [1, 0.4, 1] + [0, 1.6, 0]
        tri.append(np.concatenate([c + g.uniform(-0.6, 0.6, 3) for _ in range(3)]))
    sph, mov, tri = (np.array(a, dtype=np.float64) for a in (sph, mov, tri))
    kind = np.array([0] * len(sph) + [1] * len(mov) + [2] * len(tri), dtype=np.int32)
    index = np.concatenate([np.arange(len(sph)), np.arange(len(mov)), np.arange(len(tri))]).astype(np.int32)
    perm = np.random.default_rng(12).permutation(len(kind))
    cmat = [(np.arange(len(a)) % 3).astype(np.int32) for a in (sph, mov, tri)]
    return sph, mov, tri, np.ascontiguousarray(kind[perm]), np.ascontiguousarray(index[perm]), cmat


def hand_records(mesh_only=False):
    """(records, material per insertion index) of the hand scene, or of its triangles alone (class-major insertion)."""
    sph, mov, tri, kind, index, cmat = hand_geometry()
    if mesh_only:
        return pr.make_records(sph[:0], mov[:0], tri), cmat[2]
    mats = np.array([cmat[k][i] for k, i in zip(kind, index)], dtype=np.int32)
    return pr.make_records(sph, mov, tri, kind, index), mats


def hand_scene(mesh_only=False):
    """An object whose .c is the rtow.Scene of the hand geometry (the cover scene's camera; three materials)."""
    import ctypes as C

    import rtow

    sph, mov, tri, kind, index, cmat = hand_geometry()
    if mesh_only:
        sph, mov, cmat = sph[:0], mov[:0], [cmat[0][:0], cmat[1][:0], cmat[2]]
        kind = np.full(len(tri), 2, dtype=np.int32)
        index = np.arange(len(tri), dtype=np.int32)
    pad = lambda a, w: np.ascontiguousarray(a if len(a) else np.zeros((1, w)))  # noqa: E731
    sph_c, mov_c, tri_c = pad(sph, 4), pad(mov, 8), pad(tri, 9)
    cm = [np.ascontiguousarray(m if len(m) else np.zeros(1, np.int32)) for m in cmat]
    mats = (rtow.Material * 3)()
    mats[0].albedo[:] = [0.5, 0.5, 0.5]
    mats[1].kind, mats[1].ir = rtow.MAT_DIELECTRIC, 1.5
    mats[2].kind, mats[2].fuzz = rtow.MAT_METAL, 0.1
    mats[2].albedo[:] = [0.7, 0.6, 0.5]
    base = rtow.HostScene.cover(0, 1.5, False)
    s = rtow.Scene()
    s.camera = base.c.camera
    base.close()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    s.n_spheres, s.sphere_geom, s.sphere_mat = len(sph), pd(sph_c), pi(cm[0])
    s.n_moving, s.moving_geom, s.moving_mat = len(mov), pd(mov_c), pi(cm[1])
    s.n_triangles, s.triangle_geom, s.triangle_mat = len(tri), pd(tri_c), pi(cm[2])
    s.n_materials, s.materials = 3, mats
    s.n_prims, s.prim_kind, s.prim_index = len(kind), pi(kind), pi(index)

    class Held:
        c = s
        keep = [sph_c, mov_c, tri_c, cm, mats, kind, index]

    return Held()


# ---------------------------------------------------------------------------------------------------- sweep sets ---
def extent(rec):
    lo, hi = pr.scene_box(rec, 30.0)
    return lo, hi, float(np.max(hi - lo))


def random_sweeps(rec, n, seed, finite=True, radii=(0.0, 0.002, 0.01, 0.05, 0.2)):
    """n sweeps through the scene's box: origins in the box grown by 30 %, directions of lengths 1e-3 .. 1e3 (tmax scaled
    so the travel is up to 1.5 extents), radii `radii` x the extent, times in [0, 1].  With `finite` every tmax is finite;
    else tmax also takes +inf and 0."""
    g = np.random.default_rng(seed)
    lo, hi, ext = extent(rec)
    o = g.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(n, 3))
    tgt = g.uniform(lo, hi, size=(n, 3))
    d = tgt - o + 0.1 * ext * g.normal(size=(n, 3))
    ln = np.linalg.norm(d, axis=1)
    scale = 10.0 ** g.choice([-3.0, 0.0, 0.0, 3.0], size=n) * g.uniform(0.5, 2.0, size=n)
    d *= (scale / ln)[:, None]
    travel = g.uniform(0.05, 1.5, size=n) * ext
    tmax = travel / scale
    if not finite:
        sel = np.arange(n) % 7
        tmax = np.where(sel == 3, np.inf, np.where(sel == 5, 0.0, tmax))
    rho = np.asarray(radii)[g.integers(len(radii), size=n)] * ext
    return sr.make_sweeps(o, d, rho, g.random(n), tmax)


def skipped_sweeps():
    """One sweep of every skipped kind, and the valid one they were made from (last)."""
    base = dict(o=[0.0, 1.0, 5.0], d=[0.0, 0.0, -1.0], radius=0.1, time=0.5, tmax=10.0)
    out = []
    nan, inf = math.nan, math.inf
    for key, vals in (("o", ([nan, 1, 5], [inf, 1, 5], [0, -inf, 5])), ("d", ([nan, 0, -1], [0, 0, 0], [inf, 0, -1], [1e200, 0, 0])),
                      ("radius", (nan, -0.1, inf, -0.0 - 1e-300)), ("time", (nan, inf, -inf)), ("tmax", (nan, -1.0, -inf))):
        for v in vals:
            out.append(dict(base, **{key: v}))
    out.append(base)
    return sr.make_sweeps([c["o"] for c in out], [c["d"] for c in out], [c["radius"] for c in out],
                          [c["time"] for c in out], [c["tmax"] for c in out])


def placed_sweeps():
    """Hand-placed sweeps around one primitive of each class of the hand scene (the first triangle of the quad, the glass
    sphere, the first moving sphere, the sliver and the zero-area triangles): face, each edge and each vertex from both
    sides, parallel to an edge and to the face, grazing at rho +- 1e-12, starts inside the slab beside the triangle,
    rho = 0, the sphere from outside, from inside the hollow glass, inside with rho > R, exact tangency, the moving sphere
    at three times, a far origin, |d| of 1e-3 and 1e3.  All tmax finite."""
    o, d, rho, tm, tmax = [], [], [], [], []

    def add(o_, d_, r_, t_=0.0, tmax_=50.0):
        o.append(o_), d.append(d_), rho.append(r_), tm.append(t_), tmax.append(tmax_)

    A, B, C = np.array([-1.0, 0, -2]), np.array([1.0, 0, -2]), np.array([1.0, 2, -2])
    nrm = np.array([0.0, 0, 1])
    G = (A + B + C) / 3
    for side in (1.0, -1.0):
        add(G + 3 * side * nrm, -side * nrm, 0.3)                       # the face
        add(G + 3 * side * nrm, -side * nrm, 0.0)                       # ... as a ray
        add(G + 3 * side * nrm + [0.1, 0, 0], -side * nrm * 1e-3, 0.3, tmax_=5e4)
        add(G + 3 * side * nrm, -side * nrm * 1e3, 0.3, tmax_=1.0)
        for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):              # each edge from outside, each vertex
            mid, out = 0.5 * (P + Q), 0.5 * (P + Q) - R
            out = out / np.linalg.norm(out)
            add(mid + 2 * out + side * 0.5 * nrm, -out - side * 0.25 * nrm, 0.3)
            add(mid + 2 * out, -out, 0.2)                               # in the plane: inside the slab, beside the triangle
            add(mid + 2 * out + 0.1 * side * nrm, -out, 0.2)
            vo = P - G
            vo = vo / np.linalg.norm(vo)
            add(P + 2 * vo + side * 0.3 * nrm, -vo - side * 0.15 * nrm, 0.25)
            add(P + 2 * vo, -vo, 0.0)                                    # a ray at a vertex, in the plane
        add(A + [-2, -0.3, side * 0.1], B - A, 0.3)                      # parallel to an edge, within reach
        add(A + [-2, -0.3, side * 0.1], (B - A) + [0, 1e-9, 0], 0.3)    # ... and nearly parallel
        add(A + [-2, -0.5, side * 0.1], B - A, 0.3)                      # parallel to an edge, out of reach
        add(G + [-3, 0, side * 0.2], [1, 0, 0], 0.3)                     # parallel to the face, within reach: start beside
        add(G + [-3, 0, side * 0.4], [1, 0, 0], 0.3)                     # parallel to the face, out of reach
        for eps in (1e-12, -1e-12):                                      # grazing passes
            add(G + [-3, 0, side * (0.3 + eps)], [1, 0, 0], 0.3)
            add(A + [-2, -(0.3 + eps), 0], B - A, 0.3)
            add([0, 1, 0] + np.array([-3, side * (1.2 + eps), 0]), [1, 0, 0], 0.2)
    # the glass sphere (0, 1, 0) R = 1 with the hollow 0.8 inside
    c = np.array([0.0, 1, 0])
    add(c + [0, 0, 5], [0, 0, -1], 0.3)                                   # from outside
    add(c + [0, 0, 5], [0, 0, -1], 0.0)
    add(c + [0.1, 0.2, 0], [0, 0, 1], 0.3)                                # from inside the hollow sphere
    add(c + [0.1, 0.2, 0], [0.3, 0.1, -1], 0.05)
    add(c, [0, 1, 0], 0.1)                                                # from the centre
    add(c + [0.1, 0, 0], [0, 0, 1], 0.9)                                  # inside with rho > R of the inner sphere
    add(c + [0.9, 0, 0], [0, 0, 1], 0.05)                                 # inside the shell, between the two surfaces
    add(c + [-5, 1.25, 0], [1, 0, 0], 0.25)                               # exact tangency: R + rho = 1.25
    add(c + [-5, 0, 1.5], [1, 0, 0], 0.5)
    add([0, 0, 0], [1, 0.2, 0.1], 0.5, tmax_=100.0)                       # out to the inner side of the large sphere
    add([0, 0, 0], [1, 0.2, 0.1], 45.0)                                   # rho > R of the large sphere: start overlap or none
    for t_ in (0.0, 0.5, 1.0):                                            # the moving sphere at three times
        add([3, 1.0, 4], [0, 0, -1], 0.2, t_)
        add([3, 3.0, 0], [0, -1, 0], 0.1, t_)
        add([1, 0.5 + t_, 0.1], [1, 0, 0], 0.3, t_)
    # a far origin: 1e6 times the scene's extent (8)
    for u in ([1.0, 0.2, 0.3], [0.0, 0.0, 1.0], [-0.5, 1.0, 0.1]):
        u = np.array(u) / np.linalg.norm(u)
        for tgt in (G, c, A, 0.5 * (A + B), np.array([3.0, 1.0, 0])):
            add(tgt + 8e6 * u, -u, 0.3, 0.5, tmax_=1e7)
            add(tgt + 8e6 * u + [0, 0.29, 0], -u * 1e3, 0.3, 0.5, tmax_=1e4)
    # the sliver and the zero-area triangles
    for tgt, up in (([1, 3, 0], [0, 1, 0]), ([1, 3, 0], [0, 0, 1]), ([2, 2, 2], [0, 1, 0]), ([2, 2, 2], [0, 0, 1]),
                    ([0.5, 2.5, -1], [0, 1, 0]), ([0.5, 2.5, -1], [1, 1, 1])):
        up = np.array(up, dtype=np.float64)
        for r_ in (0.0, 0.1):
            add(np.array(tgt) + 2 * up, -up, r_)
            add(np.array(tgt) + 2 * up + [0.05, 0, 0.02], -up, r_)
    return sr.make_sweeps(o, d, rho, tm, tmax)


def tie_cases():
    """(records, materials, sweeps, expected insertion index): two coplanar triangles sharing an edge, swept onto that edge,
    in both insertion orders, and two equal spheres."""
    t0 = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    t1 = [1, 0, 0, 1, 1, 0, 0, 1, 0]   # shares the edge (1,0,0)-(0,1,0)
    out = []
    for tris in ((t0, t1), (t1, t0)):
        rec = pr.make_records(np.zeros((0, 4)), np.zeros((0, 8)), np.array(tris, dtype=np.float64))
        q = sr.make_sweeps([[0.5, 0.5, 2.0], [0.25, 0.75, -3.0]], [[0, 0, -1], [0, 0, 1]], [0.25, 0.0], 0.0, 10.0)
        out.append((rec, np.zeros(2, np.int32), q, 0))
    s = np.array([[0, 0, 0, 0.5], [3, 0, 0, 0.5], [0, 0, 0, 0.5]])
    kind, index = np.zeros(3, np.int32), np.array([2, 1, 0], np.int32)  # insertion 0 is class 2: equal to class 0
    rec = pr.make_records(s, np.zeros((0, 8)), np.zeros((0, 9)), kind, index)
    out.append((rec, np.zeros(3, np.int32), sr.make_sweeps([[0, 0, 4.0]], [[0, 0, -1]], [0.2], 0.0, 10.0), 0))
    return out
