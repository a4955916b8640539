"""The cases of the swept-sphere checkers (test_sweep_host.py, test_gpu_sweep.py): the hand scene, the hand-placed sweeps
around one primitive of each class, and the random sweep sets of a scene.  numpy and point_ref / sweep_ref only: importing
this module loads no library (hand_scene, which builds the rtow.Scene of the hand geometry, imports rtow itself)."""
import math

import numpy as np

import point_ref as pr
import sweep_ref as sr


# ------------------------------------------------------------------------------------------------ the hand scene ---
FAR_OFFSETS = {"far1e5": (1e5, -1e5, 1e5), "far1e7": (1e7, 0.0, 0.0)}  # copies of the hand scene away from the origin


def hand_geometry(offset=None):
    """(sph [n, 4], mov [n, 8], tri [n, 9], kind, index, material per class): about 40 primitives with every class, a
    hollow glass sphere, two equal spheres, a large sphere around everything, a sliver, a zero-area triangle, a point
    triangle, coplanar triangles sharing an edge and a creased fan; insertion order differs from class-major order.
    offset: every centre and vertex moved by it (rounded once: the copy is its own scene, not an exact translate)."""
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
    if offset is not None:
        off = np.asarray(offset, dtype=np.float64)
        sph[:, 0:3] += off
        mov[:, 0:3] += off
        mov[:, 3:6] += off
        tri += np.tile(off, 3)
    kind = np.array([0] * len(sph) + [1] * len(mov) + [2] * len(tri), dtype=np.int32)
    index = np.concatenate([np.arange(len(sph)), np.arange(len(mov)), np.arange(len(tri))]).astype(np.int32)
    perm = np.random.default_rng(12).permutation(len(kind))
    cmat = [(np.arange(len(a)) % 3).astype(np.int32) for a in (sph, mov, tri)]
    return sph, mov, tri, np.ascontiguousarray(kind[perm]), np.ascontiguousarray(index[perm]), cmat


def hand_records(mesh_only=False, offset=None):
    """(records, material per insertion index) of the hand scene, or of its triangles alone (class-major insertion)."""
    sph, mov, tri, kind, index, cmat = hand_geometry(offset)
    if mesh_only:
        return pr.make_records(sph[:0], mov[:0], tri), cmat[2]
    mats = np.array([cmat[k][i] for k, i in zip(kind, index)], dtype=np.int32)
    return pr.make_records(sph, mov, tri, kind, index), mats


def hand_scene(mesh_only=False, offset=None):
    """An object whose .c is the rtow.Scene of the hand geometry (the cover scene's camera; three materials)."""
    import ctypes as C

    import rtow

    sph, mov, tri, kind, index, cmat = hand_geometry(offset)
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


RADII = (0.0, 0.002, 0.01, 0.05, 0.2)  # of the random sweeps, x the scene's extent


def random_sweeps(rec, n, seed, finite=True, radii=RADII):
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


def strict_sets(rec):
    """4,097 sweeps: the hand-placed ones (they reach every scene: the origins are around the origin), every skipped
    kind, and random ones with finite, infinite and zero tmax."""
    a, b = placed_sweeps(), skipped_sweeps()
    return np.concatenate([a, b, random_sweeps(rec, 4097 - len(a) - len(b), 5, finite=False)])


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


# -------------------------------------------------------------------------- sweeps that start at contact (chained) ---
MODES = ("random", "slide", "into", "away")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent(g, u):
    """A random unit vector across each row of the unit vectors u."""
    r = g.normal(size=u.shape)
    return _unit(r - u * (r * u).sum(1, keepdims=True))


def chained_sweeps(rec, first_queries, first_hits, seed, mode):
    """The next stage of a continuous-collision loop: one sweep from the reported `centre` of every hit of
    `first_hits` with t > 0 (the answers to `first_queries`), same radius and time — an origin whose distance to the
    reported primitive equals rho to within rounding.  Direction by `mode`: "random" (normal(3)); "slide" (a unit tangent
    plus 1e-3, 0.05 or 0.5 x the unit vector u towards `point`); "into" (u plus 0.1 x a tangent: the sweep is DECIDED — at
    a travel of min(travel, rho) it is within 0.1 rho of `point`, so the segment comes much closer than rho to the
    resting primitive whatever its shape); "away" (the opposite of "into").  Rows with rho = 0 (the origin is a point of
    the surface, no normal) are kept by "random" only.  The travel is 0.5 .. 5, |d| 1e-3, 1 or 1e3 with tmax scaled.
    Returns (sweeps, class-major id of the resting primitive per sweep)."""
    assert mode in MODES, mode
    g = np.random.default_rng(seed)
    keep = (first_hits["prim"] >= 0) & (first_hits["t"] > 0.0)
    if mode != "random":
        keep &= first_queries["radius"] > 0.0
    q1, h1 = first_queries[keep], first_hits[keep]
    n = len(q1)
    if mode == "random":
        d = _unit(g.normal(size=(n, 3)))
    else:
        u = _unit(h1["point"] - h1["centre"])
        tg = _tangent(g, u)
        if mode == "slide":
            d = _unit(tg + g.choice([1e-3, 0.05, 0.5], size=n)[:, None] * u)
        else:
            d = _unit(u + 0.1 * tg) * (1.0 if mode == "into" else -1.0)
    scale = 10.0 ** g.choice([-3.0, 0.0, 0.0, 3.0], size=n)
    travel = g.uniform(0.5, 5.0, size=n)
    q = sr.make_sweeps(h1["centre"], d * scale[:, None], q1["radius"], q1["time"], travel / scale)
    return q, rec.ins2cls[h1["prim"]]


def aimed_sweeps(seed, per=6):
    """First-stage sweeps of the hand scene aimed at every piece whose "starts outside" test a chained sweep can then
    meet: the outer side of the spheres, the inner side of the hollow glass sphere and of the R = 40 sphere around
    everything (cast from inside), a moving sphere at time 0, 0.5 and 1, the face, each edge and each vertex of a
    triangle, the sliver and the two zero-area triangles; radii 0 (a ray: the next stage starts ON the surface), 0.05,
    0.25 and 0.5.  Each is cast from 2 .. 3 away along the piece's outward direction with a jitter of a few radii."""
    g = np.random.default_rng(seed)
    o, d, rho, tm, tmax = [], [], [], [], []
    radii = (0.0, 0.05, 0.25, 0.5)

    def aim(P, out, time=0.0, jitter=1.0, reach=50.0, only=None):
        out = np.asarray(out, dtype=np.float64) / np.linalg.norm(out)
        for k in range(per):
            r = radii[k % len(radii)] if only is None else only[k % len(only)]
            side = _tangent(g, out[None])[0]
            start = np.asarray(P, dtype=np.float64) + out * g.uniform(2.0, 3.0) + side * jitter * g.uniform(0, 0.3)
            aimd = _unit(np.asarray(P, dtype=np.float64) + 0.05 * g.normal(size=3) - start)
            o.append(start), d.append(aimd * 10.0 ** g.choice([-3.0, 0.0, 3.0])), rho.append(r), tm.append(time)
            tmax.append(reach / np.linalg.norm(d[-1]))

    c = np.array([0.0, 1, 0])
    for v in ([1, 0, 0], [0, 1, 0], [0.3, 0.5, -1]):
        aim(c + _unit(np.array(v, dtype=np.float64)) * 1.0, v)                   # the glass sphere, outer side
        aim(np.array([-3, 1, 0.5]) + _unit(np.array(v, dtype=np.float64)) * 0.7, v)
    for k in range(3 * per):                                                       # inside the hollow glass sphere
        u = _unit(g.normal(size=3))
        o.append(c + 0.3 * g.uniform(-1, 1, 3)), d.append(u), rho.append((0.0, 0.05, 0.25)[k % 3]), tm.append(0.0), tmax.append(5.0)
    for k in range(3 * per):                                                       # out to the inner side of R = 40
        u = _unit(g.normal(size=3) + [0, 2.5, 0])
        o.append(np.array([0.0, 5.0, 0.0]) + g.uniform(-2, 2, 3)), d.append(u * 10.0 ** g.choice([-3.0, 0.0, 3.0]))
        rho.append((0.0, 0.5, 2.0)[k % 3]), tm.append(0.0), tmax.append(100.0 / np.linalg.norm(d[-1]))
    for t_ in (0.0, 0.5, 1.0):                                                     # the moving spheres at three times
        aim(np.array([3, 0.5 + t_, 0]) + [0, 0, 0.5], [0, 0, 1], t_)
        aim(np.array([-1 - t_, 2 + 0.5 * t_, 3 - t_]) + [0.3, 0, 0], [1, 0.2, 0], t_, only=(0.05, 0.25))
    A, B, C = np.array([2.0, 0, -3]), np.array([4.0, 0, -3]), np.array([3.0, 2.5, -3])
    G, nrm = (A + B + C) / 3, np.array([0.0, 0, 1])
    for side in (1.0, -1.0):
        aim(G, side * nrm, jitter=0.3)                                             # the face
        for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):
            mid = 0.5 * (P + Q)
            aim(mid, _unit(mid - R) + 0.3 * side * nrm, jitter=0.3)                # each edge
            aim(P, _unit(P - G) + 0.3 * side * nrm, jitter=0.1)                    # each vertex
    for P, up in (([1, 3, 0], [0, 1, 0]), ([1, 3, 0], [0, 0, 1]), ([0.3, 3, 0], [-1, 0.2, 0]),     # the sliver
                  ([2, 2, 2], [0, 1, 0]), ([1.5, 2, 2], [0, 0, 1]), ([3, 2, 2], [1, 0.1, 0]),      # zero area: collinear
                  ([0.5, 2.5, -1], [0, 1, 0]), ([0.5, 2.5, -1], [1, 1, 1])):                       # zero area: a point
        aim(P, up, jitter=0.1)
    return sr.make_sweeps(o, d, rho, tm, tmax)


def resting_sweeps():
    """Hand-made origins at contact with one primitive of the hand scene, most at a distance that binary64 holds exactly
    (c + (1.25, 0, 0) for the sphere R = 1 with rho = 0.25), each with the two neighbouring doubles on either side along
    the offset, and from each an "into", a tangent and an "away" sweep.  Returns (sweeps, is an "into" sweep)."""
    o, d, rho, tm, into = [], [], [], [], []

    def rest(P, off, r, time=0.0, inner=False):
        P, off = np.asarray(P, dtype=np.float64), np.asarray(off, dtype=np.float64)
        u = (off if inner else -off) / np.linalg.norm(off)  # towards the surface: from inside a sphere, outwards
        ax = int(np.argmax(np.abs(off)))
        tg = np.roll(np.eye(3)[ax], 1)
        tg = _unit(tg - u * (tg @ u))
        x0 = P + off
        for k in (-2, -1, 0, 1, 2):
            x = x0.copy()
            for _ in range(abs(k)):
                x[ax] = np.nextafter(x[ax], np.inf * k)
            for dirn, dec in ((u + 0.1 * tg, True), (tg, False), (tg + 1e-3 * u, False), (-(u + 0.1 * tg), False)):
                o.append(x), d.append(dirn), rho.append(r), tm.append(time), into.append(dec)

    c = np.array([0.0, 1, 0])
    rest(c, [1.25, 0, 0], 0.25), rest(c, [0, 0, 1.5], 0.5)                          # the glass sphere from outside
    rest(c, [0.55, 0, 0], 0.25, inner=True), rest(c, [0, -0.3, 0], 0.5, inner=True)  # inside the hollow sphere (R = 0.8)
    rest([0, 0, 0], [39.5, 0, 0], 0.5, inner=True), rest([0, 0, 0], [0, 38.0, 0], 2.0, inner=True)  # inside R = 40
    for t_ in (0.0, 0.5, 1.0):
        rest([3, 0.5 + t_, 0], [0, 0, 0.75], 0.25, t_)                              # the moving sphere R = 0.5
    A, B, C = np.array([2.0, 0, -3]), np.array([4.0, 0, -3]), np.array([3.0, 2.5, -3])
    rest((A + B + C) / 3, [0, 0, 0.25], 0.25), rest((A + B + C) / 3, [0, 0, -0.5], 0.5)   # the face, both sides
    for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):
        mid = 0.5 * (P + Q)
        rest(mid, 0.25 * _unit(mid - R), 0.25)                                      # each edge
        rest(P, 0.25 * _unit(P - (A + B + C) / 3), 0.25)                            # each vertex
    rest(A, [-0.25, 0, 0], 0.25), rest(B, [0.5, 0, 0], 0.5)                         # ... and two vertices exactly
    rest([1, 3, 0], [0, 0.25, 0], 0.25)                                             # the sliver
    rest([2, 2, 2], [0, 0.25, 0], 0.25), rest([1, 2, 2], [-0.25, 0, 0], 0.25)       # zero area: collinear, edge and end
    rest([0.5, 2.5, -1], [0, 0.25, 0], 0.25)                                        # zero area: a point
    return sr.make_sweeps(o, d, rho, tm, 2.0), np.array(into)


_PINNED = (
    # (old guard the row separates, origin, direction, radius): found by a search over rests above a corner (along the
    # face normal: only the vertex sphere is met) and above an edge (on its outer side, between the face's plane and the
    # in-plane perpendicular) of the hand scene's random triangles, each heading into the piece; kept where that one
    # guard dropped the piece and nothing else caught the sweep
    ("vertex", ("-0x1.295687c9df96ep+2", "0x1.2dc366a53ddb5p+1", "-0x1.9735c26a7f60ep-1"),
     ("0x1.530bd5bc4d179p+0", "0x1.3f12d4ad36748p-2", "-0x1.ced4c77604ac8p-1"), "0x1.7f1f1dfaa09b5p-1"),
    ("vertex", ("-0x1.3016b0e2ef396p+2", "0x1.18c34d317d8d3p+1", "-0x1.ad256a67244fep-1"),
     ("0x1.e9b3b1c32c288p-1", "0x1.5ddb1f46924a0p-4", "-0x1.9ab5c70c06499p-2"), "0x1.e55dc8c56d5d3p-1"),
    ("vertex", ("-0x1.2e212971f9f9dp+2", "0x1.1edb7f8350bdap+1", "-0x1.a6c7b2861edcep-1"),
     ("0x1.99c4a73e39798p+0", "-0x1.df7b9f5c35f18p-5", "-0x1.8d182ace3f6c6p-1"), "0x1.c7b1a3e46bdafp-1"),
    ("edge", ("-0x1.c636d967f3e63p+0", "0x1.10256ee002e27p+1", "-0x1.32fde646ee0f0p+1"),
     ("0x1.80ae67ad99358p+0", "-0x1.7df550aa07840p-1", "-0x1.65e3cfa8e62bcp-1"), "0x1.871cb13f49036p-1"),
    ("edge", ("-0x1.8ef1439d2270fp+1", "-0x1.025a1eec6d5f8p-1", "0x1.c177bb1a4c28cp-2"),
     ("-0x1.a5d2cf526b440p-2", "0x1.fd3d5d9337151p-2", "0x1.ec3a82a116f91p-4"), "0x1.922f187b31f7ap-1"),
    ("edge", ("-0x1.0e4e8ef01684cp+2", "0x1.f8ebe75357994p+0", "-0x1.2f2edb9883dd0p-1"),
     ("-0x1.0db9b8427dc0cp-2", "0x1.10104d78ed6acp+0", "0x1.52c3966a1ecfcp-1"), "0x1.f23c4330622e3p-1"),
)


def pinned_sweeps():
    """Resting origins of the hand scene given bit by bit: the vertex test of the earlier rule repeated the overlap
    test in the SAME arithmetic wherever the nearest point is a clamped end of an edge, so only a rest above a corner with
    both edge parameters unclamped and every rounding falling one way separates it — about one origin in 10^5.  time 0,
    tmax 2."""
    h = float.fromhex
    return sr.make_sweeps([[h(x) for x in r[1]] for r in _PINNED], [[h(x) for x in r[2]] for r in _PINNED],
                          [h(r[3]) for r in _PINNED], 0.0, 2.0)


def contact_set(rec, first, answer, seed, modes=MODES, third=("slide", "into", "random")):
    """Every chained stage of the first-stage sweeps `first`: stage 2 from the centres of `answer(first)` in each of
    `modes`, and stage 3 (`third`) from the centres of the answers to the "slide" stage — origins at contact with two
    primitives at once where stage 2 slid into a neighbour: a crease, the quad's shared edge.  answer(sweeps) gives the
    records to chain from (the mirror's, or a build's own).  Returns (sweeps, resting id per sweep, decided "into" rows)."""
    h1 = answer(first)
    qs, rests, into = [], [], []
    for k, mode in enumerate(modes):
        q2, r2 = chained_sweeps(rec, first, h1, seed + k, mode)
        qs.append(q2), rests.append(r2), into.append(np.full(len(q2), mode == "into"))
        if mode == "slide" and third:
            h2 = answer(q2)
            for j, m3 in enumerate(third):
                q3, r3 = chained_sweeps(rec, q2, h2, seed + 10 + j, m3)
                qs.append(q3), rests.append(r3), into.append(np.full(len(q3), m3 == "into"))
    return np.concatenate(qs), np.concatenate(rests), np.concatenate(into)


def chain_all(first_queries, first_hits, seed):
    """The "random" next stage for EVERY row, fit to be formed on the device: origin = the reported centre, a direction
    and a tmax that do not depend on the answer, and tmax = -1 (skipped: the miss record) where the first stage missed or
    started in contact.  Returns (sweeps, directions, tmax before the skip) — Context-side code forms the same sweeps from
    device-resident hits with the last two."""
    g = np.random.default_rng(seed)
    n = len(first_queries)
    d = _unit(g.normal(size=(n, 3))) * (10.0 ** g.choice([-3.0, 0.0, 0.0, 3.0], size=n))[:, None]
    tmax = g.uniform(0.5, 5.0, size=n) / np.linalg.norm(d, axis=1)
    keep = (first_hits["prim"] >= 0) & (first_hits["t"] > 0.0)
    q = sr.make_sweeps(first_hits["centre"], d, first_queries["radius"], first_queries["time"], np.where(keep, tmax, -1.0))
    return q, d, tmax


FIRST = {"hand": 300, "hand_mesh": 400, "cover_moving": 200, "suzanne": 200, "mesh96k": 60, "far1e5": 300, "far1e7": 300}


def thin(parts, limit):
    """Every k-th row of the parallel arrays `parts`, so that at most `limit` remain."""
    n = len(parts[0])
    if limit is None or n <= limit:
        return parts
    idx = (np.arange(limit) * n) // limit
    return tuple(p[idx] for p in parts)


def contact_sets(name, rec, answer, limit=None, radii=RADII):
    """The sweeps at contact of scene `name` with records rec: (sweeps, resting id or -1, decided "into" rows).
    hand: the three-stage chain of the aimed first stage and of 300 random sweeps, then the hand-made and the pinned
    rests; every other scene: the three-stage chain of FIRST[name] random sweeps.  The far copies (FAR_OFFSETS) add the
    random first stage itself and chain one stage.  limit: at most so many of the chained rows, evenly thinned."""
    first = random_sweeps(rec, FIRST[name], 3, radii=radii)
    if name == "hand":
        first = np.concatenate([aimed_sweeps(1), first])
    far = name in FAR_OFFSETS
    q, rest, into = thin(contact_set(rec, first, answer, 4, third=() if far else ("slide", "into", "random")), limit)
    if far:
        q, rest, into = (np.concatenate(x) for x in ((first, q), (np.full(len(first), -1), rest), (np.zeros(len(first), bool), into)))
    if name == "hand":
        r, dec = resting_sweeps()
        r = np.concatenate([r, pinned_sweeps()])
        near = pr.nearest(rec, r["origin"], r["time"])[2]
        q, rest, into = np.concatenate([q, r]), np.concatenate([rest, near]), np.concatenate([into, dec, np.zeros(len(_PINNED), bool)])
    return q, rest, into
