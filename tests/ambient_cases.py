"""The cases of the ambient query's exact checks (test_ambient_exact_host.py on the CPU, test_gpu_exact_ambient.py on the
GPU) and the point sets test_gpu_ambient.py shares with them: the normals and identities where the sample direction can
go wrong, and surface points of the logged renders, the hand-made scene and a refitted scene, all made without a GPU.
Importing this module loads no library."""
import functools
import math

import numpy as np

import ambient_exact as ax
import rtow
from exact_cases import subsample
from scatter_exact import philox_words

SEED = 20261021
DIR_SAMPLES = 4
# (pixel, sample) under SEED whose disk point lies OUTSIDE the unit circle (w3 = 2^32 - 2 and the sine polynomial's
# error: px^2 + py^2 = 1 + 6.3e-9), so the clamp of pz acts: about one identity in 2^30 does, and
# scripts/find_clamped_identities.py, which takes minutes, finds this one among pixel < 256, sample < 2^22;
# direction_cases() checks that it still is one.
CLAMPED_ID = (43, 1810345)


# ---- directions ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rim_and_centre_ids(count=8, pixel=7, log2n=22):
    """(rim [count, 2], centre [count, 2]): among the identities (pixel, 0 .. 2^log2n - 1) under SEED those with the
    largest w3 (the disk point nearest the rim: the smallest pz) and with the smallest (nearest the centre)."""
    chunk = 1 << 16  # (the seven rounds stay in the cache)
    pix = np.full(chunk, pixel, dtype=np.uint64)
    w3 = np.concatenate([np.asarray(philox_words(SEED, pix, np.arange(lo, lo + chunk, dtype=np.uint64), 0)[3], dtype=np.uint64)
                         for lo in range(0, 1 << log2n, chunk)])
    order = np.argsort(w3, kind="stable")
    ids = lambda idx: np.stack([np.full(len(idx), pixel), idx], axis=1).astype(np.uint32)  # noqa: E731
    return ids(order[-count:]), ids(order[:count])


@functools.lru_cache(maxsize=None)
def direction_cases():
    """(points, ids, labels): about 1,500 surface points (at one place: the scene does not matter to a direction) whose
    normals and identities are where the direction's arithmetic can go wrong; labels[i] names the group of point i."""
    g = np.random.default_rng(17)
    N, ids, labels = [], [], []

    def add(label, normals, these_ids=None):
        normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        N.append(normals)
        labels.extend([label] * len(normals))
        if these_ids is None:
            these_ids = np.stack([g.integers(0, 1 << 32, len(normals)), g.integers(0, 1 << 32, len(normals))], axis=1)
        ids.append(np.asarray(these_ids, dtype=np.uint32).reshape(-1, 2))

    # components from 1e-150 to 1e150, each on its own scale
    add("wide", g.choice([-1.0, 1.0], size=(1200, 3)) * 10.0 ** g.uniform(-150, 150, size=(1200, 3)))
    add("unit", g.normal(size=(150, 3)))
    # both sides of the skip rule (normal . normal < 2^-1022 is skipped); single components square with ONE rounding in
    # either build, so these sit on their side of the rule however the dot is contracted
    t = 2.0 ** -511
    skipped = [[t * (1 - 2.0 ** -53), 0, 0], [0, -1.4e-154, 0], [1e-155, 0, 0], [0, -1e-158, 0], [0, 0, 1e-160],
               [-1e-161, 0, 0], [0, 1e-163, 0], [0, 0, -1e-200], [1e-156, 1e-156, -1e-156], [1.35e154, 0, 0],
               [0, 1e200, 0], [1e154, -1e154, 1e154]]
    add("skipped", skipped)
    # live ones: at the threshold, with products that underflow one by one (1.2e-154^2 is subnormal), and up to 1e307
    live = [[t, 0, 0], [0, -t, 0], [0, 0, t], [0, 0, -t], [2e-154, 0, 0], [0, 1.5e-154, 0], [1.2e-154, 1.2e-154, -1.2e-154],
            [1.6e-154, 1e-162, -1e-170], [1e-154, -1e-154, 1e-154], [1.3e-154, 9e-155, 1e-200], [3e-154, -1e-160, 2e-154],
            [0, 1e-162, 1.5e-154], [3e153, 0, 0], [0, 0, -3e153], [7e153, 7e153, 7e153], [0, 1.3e154, 0],
            [1e153, -2e150, 3e153], [1.3e154, 1e-300, -0.0]]
    add("threshold", live * 3)
    # the axes with every pattern of signed zeros
    axes = []
    for k in range(3):
        for sg in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    v = [z1, z2]
                    v.insert(k, sg)
                    axes.append(v)
    add("axes", axes)
    # where the frame flips: N.z = +-1e-300 and +-0.0 beside x, y of order 1
    flip = []
    for nz in (1e-300, -1e-300, 0.0, -0.0, 5e-324, -5e-324):
        for _ in range(8):
            x, y = g.normal(size=2)
            flip.append([x, y, nz])
    add("flip", flip)
    # within 1e-9 and within 1e-160 of the -z pole (s + n.z = -2: the frame's a stays -1/2), and of the +z pole
    pole = []
    for eps in (1e-9, 1e-160):
        for z in (-1.0, -3.7, 1.0):
            for _ in range(6):
                ph = g.uniform(0, 2 * np.pi)
                pole.append([eps * math.cos(ph) * abs(z), eps * math.sin(ph) * abs(z), z])
    add("pole", pole)
    # the disk points nearest the rim (smallest pz) and nearest the centre, and the one the clamp acts on
    rim, centre = rim_and_centre_ids()
    w = philox_words(SEED, CLAMPED_ID[0], CLAMPED_ID[1], 0)
    (px, py, pz), _, _ = ax.disk_exact(w)
    assert (px * px + py * py - 1).sign() > 0 and pz.m == 0, "CLAMPED_ID is no clamped identity"
    for label, these in (("rim", rim), ("centre", centre), ("clamped", np.array([CLAMPED_ID] * 4))):
        nrm = g.normal(size=(len(these), 3))
        nrm[0] = [0.0, 0.0, -1.0]
        add(label, nrm, these)
    N, ids = np.concatenate(N), np.concatenate(ids)
    pts = rtow.make_surface_points(np.tile([0.0, 5.0, 0.0], (len(N), 1)), N, time=0.5)
    return pts, ids, np.array(labels)


# ---- surface points ------------------------------------------------------------------------------------------------
def scene_extent(view):
    """Largest side of the box of the scene's small primitives (not the cover scene's ground sphere)."""
    pts = []
    small = view.sph[np.abs(view.sph[:, 3]) < 100.0]
    if len(small):
        pts += [small[:, :3] - np.abs(small[:, 3:4]), small[:, :3] + np.abs(small[:, 3:4])]
    if len(view.mov):
        pts += [view.mov[:, 0:3] - view.mov[:, 6:7], view.mov[:, 3:6] + view.mov[:, 6:7]]
    if len(view.tri):
        pts.append(view.tri.reshape(-1, 3))
    pts = np.concatenate(pts)
    return float(np.max(pts.max(0) - pts.min(0)))


def _normal_at(view, p, time, ci):
    """The normal at the logged hit point p of the primitive with class index ci: the class is the one whose surface p
    lies nearest; a triangle's is its record's e1 x e2 (not unit length), a sphere's (p - c) / r."""
    found = []  # (distance of p from the surface, normal) per class that has an index ci
    if ci < len(view.tri):
        A, B, C = view.tri[ci, 0:3], view.tri[ci, 3:6], view.tri[ci, 6:9]
        n = np.cross(B - A, C - A)
        found.append((abs(np.dot(p - A, n)) / max(np.linalg.norm(n), 1e-300), n))
    spheres = []
    if ci < len(view.sph):
        spheres.append((view.sph[ci, 0:3], view.sph[ci, 3]))
    if ci < len(view.mov):
        m = view.mov[ci]
        spheres.append((m[0:3] + time * (m[3:6] - m[0:3]), m[6]))
    for c, r in spheres:
        found.append((abs(np.linalg.norm(p - c) - abs(r)), (p - c) / r))
    return min(found, key=lambda f: f[0])[1]


def log_points(view, log, n, seed, bounded=0.5):
    """(points, ids): n hit points of the log with the hit primitive's normal turned toward the arriving ray, at the
    log's times; a share `bounded` of them with max_dist = 5 % of the scene's extent, the others unbounded."""
    hit = subsample(log[np.isfinite(log[:, 10])], n, seed)
    g = np.random.default_rng(seed)
    p = hit[:, 3:6] + hit[:, 10:11] * hit[:, 6:9]
    nrm = np.array([_normal_at(view, p[i], hit[i, 9], int(hit[i, 11])) for i in range(len(hit))])
    nrm = np.where(((nrm * hit[:, 6:9]).sum(axis=1) > 0)[:, None], -nrm, nrm)
    md = np.where(g.random(len(hit)) < bounded, 0.05 * scene_extent(view), math.inf)
    ids = np.stack([g.integers(0, 1 << 32, len(hit)), g.integers(0, 1 << 32, len(hit))], axis=1).astype(np.uint32)
    return rtow.make_surface_points(p, nrm, time=hit[:, 9], max_dist=md), ids


def handmade_points():
    """About 200 hand-placed points of handmade_scene(): inside the hollow glass sphere, on the triangles' front and back,
    on the ground, and normals along the axes with signed zeros."""
    g = np.random.default_rng(9)
    p, nrm, md = [], [], []
    for _ in range(60):  # inside the negative-radius sphere (centre (0, 1, 0), r = 0.8): the shell is all around
        u = g.normal(size=3)
        p.append(np.array([0, 1, 0]) + 0.5 * u / np.linalg.norm(u)), nrm.append(g.normal(size=3)), md.append(
            g.choice([0.2, 0.4, math.inf]))
    for _ in range(40):  # on the first triangle (z = -2), front and back, and on the second (z = -3)
        a, b = sorted(g.random(2))
        q = np.array([-1, 0, -2]) * a + np.array([1, 0, -2]) * (b - a) + np.array([0, 2, -2]) * (1 - b)
        for nz in (1.0, -1.0):
            p.append(q), nrm.append([0.0, -0.0, nz]), md.append(g.choice([1.5, math.inf]))
    axes = [(1, 0.0, 0.0), (-1, 0.0, -0.0), (0.0, 1, -0.0), (-0.0, -1, 0.0), (0.0, -0.0, 1), (-0.0, 0.0, -1), (-0.0, -0.0, 1),
            (0.0, 0.0, -1)]
    for origin in ([0, 1e-9, 3], [2, 0.5, 1], [-3, 2.5, 0.5], [0.3, 0.9, 0.2], [3, 1, 4], [0, 3, 0], [0, 0.5, -1.5]):
        for ax_ in axes:
            p.append(origin), nrm.append(ax_), md.append(g.choice([0.8, 4.0, math.inf]))
    time = g.choice([0.0, 0.5, 1.0], size=len(p))
    pts = rtow.make_surface_points(np.array(p, dtype=np.float64), np.array(nrm, dtype=np.float64), time=time,
                                   max_dist=np.array(md))
    assert np.signbit(pts["normal"]).any() and 190 <= len(pts) <= 210
    return pts


N_ENCLOSED = 60  # handmade_points()[:60] lie inside the hollow sphere


def handmade_sky_points(n=24):
    """Points far above handmade_scene() (y = 50: everything else lies below y = 3.1) with normals straight up, of many
    lengths and with signed zeros beside them: every direction has d.y >= 0, so every sample is open, whatever max_dist."""
    g = np.random.default_rng(12)
    p = np.stack([g.uniform(-4, 4, n), np.full(n, 50.0), g.uniform(-4, 4, n)], axis=1)
    nrm = np.zeros((n, 3))
    nrm[:, 1] = 10.0 ** g.uniform(-100, 100, n)
    nrm[::2, 0], nrm[::3, 2] = -0.0, -0.0
    md = np.where(np.arange(n) % 2 == 0, math.inf, 30.0)
    return rtow.make_surface_points(p, nrm, time=g.choice([0.0, 0.5, 1.0], size=n), max_dist=md)


def box_points(sc, rays, seed):
    """Points of a ray set (the origin as the point, the direction as the normal: random places in and around the scene's
    box, for a scene that has no log — a refitted one); half with max_dist = 5 % of the extent."""
    g = np.random.default_rng(seed)
    md = np.where(g.random(len(rays)) < 0.5, 0.05 * scene_extent(sc), math.inf)
    ids = np.stack([g.integers(0, 1 << 32, len(rays)), g.integers(0, 1 << 32, len(rays))], axis=1).astype(np.uint32)
    return rtow.make_surface_points(rays["origin"], rays["direction"], time=rays["time"], max_dist=md), ids
