"""The cases of the box-overlap checkers (test_overlap_host.py, test_gpu_overlap.py): hand-placed boxes on the hand scene
(sweep_cases.hand_geometry), the lattice scene with its unit voxels (the exact-inputs set), every skipped kind, min_prim
values and the random boxes of a scene.  numpy, point_ref and overlap_ref only: importing this loads no library
(lattice_scene, which builds an rtow.Scene, imports rtow itself)."""
import math

import numpy as np

import overlap_ref as ov
import point_ref as pr

SIZES = (0.01, 0.05, 0.25)  # edge lengths of the random boxes, x the scene's extent


def extent(rec):
    lo, hi = pr.scene_box(rec, 30.0)
    return lo, hi, float(np.max(hi - lo))


def random_boxes(rec, n, seed, sizes=SIZES):
    """n boxes with centres in the scene's box grown by 10 %, edges up to `sizes` x the extent per component (three size
    classes in turn), times in [0, 1]; every eighth with a min_prim inside the scene's indices."""
    g = np.random.default_rng(seed)
    lo, hi, ext = extent(rec)
    c = g.uniform(lo - 0.1 * ext, hi + 0.1 * ext, size=(n, 3))
    half = 0.5 * ext * np.asarray(sizes)[np.arange(n) % len(sizes)][:, None] * g.uniform(0.2, 1.0, size=(n, 3))
    mp = np.where(np.arange(n) % 8 == 5, g.integers(0, max(rec.n, 1), size=n), 0)
    return ov.make_boxes(c - half, c + half, g.random(n), mp)


def skipped_boxes():
    """One box of every skipped kind, and the valid one they were made from (last)."""
    nan, inf = math.nan, math.inf
    base = dict(lo=[-1.0, 0.0, -3.0], hi=[1.0, 2.0, -1.0], time=0.5)
    out = []
    for k in range(3):
        for v in (nan, inf, -inf):
            for key in ("lo", "hi"):
                b = dict(base, **{key: list(base[key])})
                b[key][k] = v
                out.append(b)
        b = dict(base, lo=list(base["lo"]))
        b["lo"][k] = base["hi"][k] + 0.5  # lo > hi in one component
        out.append(b)
    out += [dict(base, time=v) for v in (nan, inf, -inf)]
    out.append(base)
    return ov.make_boxes([b["lo"] for b in out], [b["hi"] for b in out], [b["time"] for b in out])


def min_prim_boxes(n_prims):
    """A box around everything near the origin with min_prim below 0, 0, inside the list, at and past the last primitive."""
    mp = [-5, -1, 0, 1, 7, n_prims // 2, n_prims - 1, n_prims, n_prims + 10, 2 ** 31 - 1, -2 ** 31]
    return ov.make_boxes([[-6.0, -1.0, -6.0]] * len(mp), [[6.0, 5.0, 6.0]] * len(mp), 0.25, mp)


def placed_boxes():
    """Hand-placed boxes on the hand scene; (boxes, names)."""
    lo, hi, tm, names = [], [], [], []

    def add(name, l, h, t=0.0):
        lo.append(l), hi.append(h), tm.append(t), names.append(name)

    def about(name, c, r, t=0.0):
        c, r = np.asarray(c, dtype=np.float64), np.broadcast_to(np.asarray(r, dtype=np.float64), (3,))
        add(name, c - r, c + r, t)

    about("inside the hollow glass sphere", [0, 1, 0], 0.125)
    about("inside the glass shell", [0.875, 1, 0], 0.03125)
    about("contains a whole sphere", [-2, 2.5, -1], 0.5)
    about("contains the glass pair", [0, 1, 0], 1.25)
    about("crosses the glass surfaces", [1, 1, 0], 0.5)
    add("touches the glass sphere at a face", [1, 0.5, -0.5], [2, 1.5, 0.5])
    add("touches the R = 40 sphere with its far corner", [0, 0, 0], [24, 32, 0])
    add("far corner one ulp short of R = 40", [0, 0, 0], [24, np.nextafter(32.0, 0.0), 0])
    about("contains the quad", [0, 1, -2], [1.5, 1.5, 0.5])
    about("pierced by a triangle, no vertex inside", [3, 0.75, -3], 0.25)
    about("in a triangle's bounding box, beside it", [2.125, 2.25, -3], 0.0625)
    about("beside the quad's diagonal, in one triangle only", [0.5, 0.25, -2], 0.125)
    about("the sliver", [1, 3, 0], 0.0625)
    about("beside the sliver", [1, 3.25, 0], 0.0625)
    about("the collinear triangle", [2, 2, 2], 0.125)
    about("the point triangle", [0.5, 2.5, -1], 0.125)
    add("a rectangle in the quad's plane", [-0.5, 0.5, -2], [0.5, 1.5, -2])
    add("a rectangle across the quad", [-0.5, 1, -3], [0.5, 1, -1])
    add("a segment through the quad", [0, 1, -3], [0, 1, -1])
    add("a segment in the quad's plane along its diagonal's box", [-1, 0, -2], [1, 0, -2])
    add("a point on the quad", [0, 1, -2], [0, 1, -2])
    add("a point on the quad's shared edge", [0, 1, -2], [0, 1, -2])
    add("a point off the quad", [0, 1, -1.5], [0, 1, -1.5])
    add("the point triangle's point", [0.5, 2.5, -1], [0.5, 2.5, -1])
    add("a point of the collinear triangle", [2.5, 2, 2], [2.5, 2, 2])
    add("a point on the glass sphere", [1, 1, 0], [1, 1, 0])
    add("crosses R = 40 far out", [39, -1, -1], [1e6, 1, 1])
    about("far from the origin 1e7", [1e7, 1e7, 1e7], 1.0)
    about("far from the origin 1e12", [-1e12, 3e11, 1e12], 1e3)
    add("a huge box around everything", [-1e9, -1e9, -1e9], [1e9, 1e9, 1e9])
    add("a box around the scene inside R = 40", [-6, -1, -6], [6, 5, 6])
    for t in (0.0, 0.5, 1.0):
        about(f"the first moving sphere's start, time {t}", [3, 0.5, 0], 0.5, t)
        about(f"above the first moving sphere, time {t}", [3, 2.125, 0], 0.125, t)
        about(f"the second moving sphere's path, time {t}", [-1.5, 2.25, 2.5], 0.25, t)
        add(f"touches the first moving sphere from above at time 0.5, time {t}", [2.5, 1.5, -0.5], [3.5, 2.5, 0.5], t)
    return ov.make_boxes(lo, hi, tm), names


def strict_set(rec, n=4097, seed=5):
    """n boxes: the placed ones (they reach every scene: around the origin), every skipped kind, the min_prim values and
    random ones."""
    a, b, c = placed_boxes()[0], skipped_boxes(), min_prim_boxes(rec.n)
    return np.concatenate([a, b, c, random_boxes(rec, n - len(a) - len(b) - len(c), seed)])


# ------------------------------------------------------------------------------------------- the lattice scene ---
def lattice_geometry():
    """(sph, mov, tri, kind, index): integer vertices, centres and radii in [0, 4]^3 and beside it — every intermediate
    of the predicate against an integer or half-integer box is exact."""
    tri = []
    for i in range(4):           # the plane z = 2: unit squares along the diagonal, two triangles each
        tri += [[i, i, 2, i + 1, i, 2, i + 1, i + 1, 2], [i, i, 2, i + 1, i + 1, 2, i, i + 1, 2]]
    tri += [[1, 0, 0, 1, 4, 0, 1, 4, 4], [1, 0, 0, 1, 4, 4, 1, 0, 4]]        # the plane x = 1
    tri += [[0, 0, 0, 4, 0, 0, 0, 4, 0], [4, 0, 0, 0, 4, 0, 0, 0, 4]]        # z = 0 half, and the plane x + y + z = 4
    tri += [[0, 0, 4, 4, 4, 4, 0, 4, 0], [3, 0, 1, 3, 2, 3, 4, 0, 3]]        # skew, through lattice points
    tri += [[0, 3, 3, 4, 3, 3, 2, 3, 3], [2, 1, 3, 2, 1, 3, 2, 1, 3]]        # collinear along y = z = 3; a point
    sph = [[2, 2, 2, 1], [3, 1, 1, -1], [6, 2, 2, 5], [0, 0, 0, 5]]           # (3-4-5: corners of voxels lie ON R = 5)
    mov = [[0, 0, 8, 4, 0, 8, 1, 0], [2, 5, 2, 2, 9, 2, 2, 0]]
    sph, mov, tri = (np.array(a, dtype=np.float64) for a in (sph, mov, tri))
    kind = np.array([0] * len(sph) + [1] * len(mov) + [2] * len(tri), dtype=np.int32)
    index = np.concatenate([np.arange(len(sph)), np.arange(len(mov)), np.arange(len(tri))]).astype(np.int32)
    perm = np.random.default_rng(21).permutation(len(kind))
    return sph, mov, tri, np.ascontiguousarray(kind[perm]), np.ascontiguousarray(index[perm])


def lattice_records():
    sph, mov, tri, kind, index = lattice_geometry()
    return pr.make_records(sph, mov, tri, kind, index)


def lattice_boxes():
    """The unit voxels [i, i + 1]^3 of [-1, 5]^3 at time 0.5 (touching the geometry at faces, edges and vertices), the
    half-integer voxels of [0, 4]^3 at time 0.25, and the voxels about the moving spheres' paths."""
    g = np.stack(np.meshgrid(*[np.arange(-1, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    h = np.stack(np.meshgrid(*[np.arange(0, 4, 0.5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[::3]
    m = np.stack(np.meshgrid(np.arange(-1, 6), np.arange(-1, 2), np.arange(6, 10), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    return np.concatenate([ov.make_boxes(g, g + 1.0, 0.5), ov.make_boxes(h, h + 0.5, 0.25), ov.make_boxes(m, m + 1.0, 0.5),
                           ov.make_boxes(m, m + 1.0, 0.75)])


def lattice_scene():
    """An object whose .c is the rtow.Scene of the lattice geometry (the cover scene's camera; one material)."""
    import ctypes as C

    import rtow

    sph, mov, tri, kind, index = lattice_geometry()
    cm = [np.zeros(len(a), np.int32) for a in (sph, mov, tri)]
    mats = (rtow.Material * 1)()
    mats[0].albedo[:] = [0.5, 0.5, 0.5]
    base = rtow.HostScene.cover(0, 1.5, False)
    s = rtow.Scene()
    s.camera = base.c.camera
    base.close()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    s.n_spheres, s.sphere_geom, s.sphere_mat = len(sph), pd(sph), pi(cm[0])
    s.n_moving, s.moving_geom, s.moving_mat = len(mov), pd(mov), pi(cm[1])
    s.n_triangles, s.triangle_geom, s.triangle_mat = len(tri), pd(tri), pi(cm[2])
    s.n_materials, s.materials = 1, mats
    s.n_prims, s.prim_kind, s.prim_index = len(kind), pi(kind), pi(index)

    class Held:
        c = s
        keep = [sph, mov, tri, cm, mats, kind, index]

    return Held()


def voxel_grid(lo, hi, n):
    """The n x n x n voxels of the box [lo, hi] (boxes in x-major order)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    edges = [np.linspace(lo[k], hi[k], n + 1) for k in range(3)]
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    return ov.make_boxes(np.stack([edges[0][i], edges[1][j], edges[2][k]], axis=1),
                         np.stack([edges[0][i + 1], edges[1][j + 1], edges[2][k + 1]], axis=1))
