"""Reference for the first-k-hits query (rtow_first_hits): for every ray, every primitive whose hit test accepts a t in
[0.001, tmax], ordered by (t, insertion index), cut at max_hits.

Two forms of the same definition:

* `reference_oracle`: the oracle's own per-primitive entry points (orc_sphere_hit / orc_triangle_hit through
  SceneView.oracle_hit, the moving centre as SceneView computes it), one call per (ray, primitive).  The definition
  itself; usable on scenes of a few primitives.
* `reference`: a vectorised numpy restatement of the two tests (binary64, the oracle's operand order, one IEEE
  operation per numpy operation: numpy does not contract), for scenes of hundreds of primitives and meshes.
  tests/test_first_hits_host.py pins what it runs — `sphere_t` / `sphere_record`, `triangle_matrix` and `records` —
  bit for bit (t, point, normal, front) to the two oracle entry points on seeded (ray, primitive) pairs, and the whole
  of it to `reference_oracle` on the hand-made scene.  (`triangle_t` is the plain statement of the triangle test,
  kept for that test: `triangle_matrix` must agree with it on every pair.)

Both return (hits [n, max_hits] HIT_DTYPE, counts [n] int32) exactly as the query writes them: unused slots hold the
miss record.  A ray whose tmax is below 0.001 or NaN has count 0.
"""
import ctypes as C
import math

import numpy as np

import rtow

TMIN = 0.001
_pd = C.POINTER(C.c_double)


def miss_records(shape):
    out = np.zeros(shape, dtype=rtow.HIT_DTYPE)
    out["t"], out["prim"], out["kind"], out["material"] = math.inf, -1, -1, -1
    return out


def _finish(view, rays, per_ray, max_hits):
    """per_ray[j]: [(t, prim, point, normal, front)] of every accepted primitive -> the query's output."""
    hits = miss_records((len(rays), max_hits))
    counts = np.zeros(len(rays), dtype=np.int32)
    for j, found in enumerate(per_ray):
        found = sorted(found, key=lambda e: (e[0], e[1]))[:max_hits]
        counts[j] = len(found)
        for s, (t, p, pt, n, front) in enumerate(found):
            hits[j, s] = (t, pt, n, p, view.kind[p], view.prim_mat[p], front)
    return hits, counts


def empty_interval(tmax):
    return ~(np.asarray(tmax) >= TMIN)  # (NaN included)


def reference_oracle(view, rays, max_hits):
    per_ray = []
    for r in rays:
        found = []
        if not empty_interval(r["tmax"]):
            for p in range(len(view.kind)):
                h = view.oracle_hit(p, r["origin"], r["direction"], r["time"], tmax=r["tmax"])
                if h is not None:
                    found.append((h[0], p, h[1], h[2], h[3]))
        per_ray.append(found)
    return _finish(view, rays, per_ray, max_hits)


# ------------------------------------------------------------------ the two tests, vectorised (oracle/rtow_oracle.cpp) ---
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2],
                     x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], axis=-1)


def sphere_t(c, r, o, d, tmin, tmax):
    """sphere_hit_helper up to the accepted root: (ok, t).  c, o, d: [..., 3]; r, tmin, tmax: [...] (broadcast)."""
    with np.errstate(all="ignore"):
        oc = o - c
        a = _dot(d, d)
        h = _dot(oc, d)
        cc = _dot(oc, oc) - r * r
        disc = h * h - a * cc
        sq = np.sqrt(disc)
        root = (-h - sq) / a
        far = (root < tmin) | (root > tmax)
        root2 = (-h + sq) / a
        root = np.where(far, root2, root)
        ok = ~(disc < 0.0) & ~(far & ((root2 < tmin) | (root2 > tmax)))
    return ok, root


def sphere_record(c, r, o, d, t):
    """The rest of sphere_hit_helper for accepted roots: (point, normal, front)."""
    with np.errstate(all="ignore"):
        p = o + d * t[..., None]
        v = p - c
        n = v * (1.0 / np.sqrt(_dot(v, v)))[..., None]
        front = (_dot(d, n) < 0) ^ (r < 0)
        n = np.where(front[..., None], n, -n)
    return p, n, front.astype(np.int32)


def triangle_t(A, B, Cc, o, d, tmin, tmax):
    """triangle_hit: (ok, t, n).  A, B, Cc, o, d: [..., 3]."""
    with np.errstate(all="ignore"):
        e1 = B - A
        e2 = Cc - A
        n = _cross(e1, e2)
        det = -_dot(d, n)
        invdet = 1.0 / det
        ao = o - A
        dao = _cross(ao, d)
        u = _dot(e2, dao) * invdet
        v = -_dot(e1, dao) * invdet
        t = _dot(ao, n) * invdet
        ok = (det >= 1e-6) & (t >= tmin) & (t <= tmax) & (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0)
    return ok, t, n


def triangle_matrix(tri, o, d, tmin, tmax):
    """triangle_t for every (ray, triangle) pair — tri [P, 9]; o, d [R, 3]; tmax [R] — as (ok, t) [R, P]: the same
    operations on the same operands, evaluated only as far as each pair gets (det, then t, then u and v)."""
    A = tri[:, 0:3]
    e1, e2 = tri[:, 3:6] - A, tri[:, 6:9] - A
    n = _cross(e1, e2)
    with np.errstate(all="ignore"):
        det = -_dot(d[:, None, :], n[None, :, :])
        ok = np.zeros(det.shape, dtype=bool)
        T = np.full(det.shape, math.inf)
        r, p = np.nonzero(det >= 1e-6)
        invdet = 1.0 / det[r, p]
        ao = o[r] - A[p]
        t = _dot(ao, n[p]) * invdet
        m = (t >= tmin) & (t <= tmax[r])
        r, p, t, invdet, ao = r[m], p[m], t[m], invdet[m], ao[m]
        dao = _cross(ao, d[r])
        u = _dot(e2[p], dao) * invdet
        v = -_dot(e1[p], dao) * invdet
        m = (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0)
    ok[r[m], p[m]] = True
    T[r[m], p[m]] = t[m]
    return ok, T


def moving_centre(g, time):
    """SceneView.oracle_hit's moving centre: c0 + time * (c1 - c0).  g: [..., 8]; time: [...]."""
    return g[..., 0:3] + time[..., None] * (g[..., 3:6] - g[..., 0:3])


def _class_positions(view, kind, count):
    pos = np.zeros(count, dtype=np.int64)
    sel = np.nonzero(view.kind == kind)[0]
    pos[view.index[sel]] = sel
    return pos


def reference(view, rays, max_hits, chunk_pairs=3_000_000):
    """The definition, vectorised: a t matrix [rays, primitives in insertion order] per chunk of rays, then the records
    of the kept entries."""
    n_prims = len(view.kind)
    pos_s = _class_positions(view, rtow.PRIM_SPHERE, len(view.sph))
    pos_m = _class_positions(view, rtow.PRIM_MOVING_SPHERE, len(view.mov))
    pos_t = _class_positions(view, rtow.PRIM_TRIANGLE, len(view.tri))
    hits = miss_records((len(rays), max_hits))
    counts = np.zeros(len(rays), dtype=np.int32)
    step = max(1, chunk_pairs // max(n_prims, 1))
    for lo in range(0, len(rays), step):
        rs = rays[lo:lo + step]
        o, d = rs["origin"][:, None, :], rs["direction"][:, None, :]
        tmax, time = rs["tmax"][:, None], rs["time"][:, None]
        T = np.full((len(rs), n_prims), math.inf)
        OK = np.zeros((len(rs), n_prims), dtype=bool)
        if len(view.sph):
            ok, t = sphere_t(view.sph[None, :, 0:3], view.sph[None, :, 3], o, d, TMIN, tmax)
            OK[:, pos_s], T[:, pos_s] = ok, t
        if len(view.mov):
            g = np.broadcast_to(view.mov[None, :, :], (len(rs),) + view.mov.shape)
            ok, t = sphere_t(moving_centre(g, np.broadcast_to(time, g.shape[:2])), view.mov[None, :, 6], o, d, TMIN, tmax)
            OK[:, pos_m], T[:, pos_m] = ok, t
        if len(view.tri):
            ok, t = triangle_matrix(view.tri, rs["origin"], rs["direction"], TMIN, rs["tmax"])
            OK[:, pos_t], T[:, pos_t] = ok, t
        OK &= ~empty_interval(tmax)
        for j in range(len(rs)):
            cand = np.flatnonzero(OK[j])  # ascending insertion index: a stable sort keeps it within a tie
            keep = cand[np.argsort(T[j, cand], kind="stable")][:max_hits]
            counts[lo + j] = len(keep)
            if len(keep):
                hits[lo + j, :len(keep)] = records(view, rs[j], keep, T[j, keep])
    return hits, counts


def records(view, ray, prims, t):
    """HIT_DTYPE records of inserted primitives `prims` accepted at `t` by one ray."""
    out = miss_records(len(prims))
    o = np.broadcast_to(ray["origin"], (len(prims), 3))
    d = np.broadcast_to(ray["direction"], (len(prims), 3))
    kind, idx = view.kind[prims], view.index[prims]
    out["t"], out["prim"], out["kind"], out["material"] = t, prims, kind, view.prim_mat[prims]
    out["point"] = o + d * t[:, None]  # Ray::at
    out["front_face"] = 1
    s = kind != rtow.PRIM_TRIANGLE
    if s.any():
        c = np.zeros((len(prims), 3))
        r = np.zeros(len(prims))
        st, mv = kind == rtow.PRIM_SPHERE, kind == rtow.PRIM_MOVING_SPHERE
        c[st], r[st] = view.sph[idx[st], 0:3], view.sph[idx[st], 3]
        if mv.any():
            g = view.mov[idx[mv]]
            c[mv], r[mv] = moving_centre(g, np.full(len(g), ray["time"])), g[:, 6]
        p, n, front = sphere_record(c[s], r[s], o[s], d[s], t[s])
        out["point"][s], out["normal"][s], out["front_face"][s] = p, n, front
    tr = ~s
    if tr.any():
        g = view.tri[idx[tr]]
        out["normal"][tr] = _cross(g[:, 3:6] - g[:, 0:3], g[:, 6:9] - g[:, 0:3])
    return out


def same_records(got, want):
    """Every field of two HIT_DTYPE arrays equal — floats bit for bit (so -0.0 != +0.0 and NaN == NaN)."""
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def first_difference(got, want):
    g = got.reshape(-1).view(np.uint8).reshape(-1, rtow.HIT_DTYPE.itemsize)
    w = want.reshape(-1).view(np.uint8).reshape(-1, rtow.HIT_DTYPE.itemsize)
    bad = np.nonzero(np.any(g != w, axis=1))[0]
    if len(bad) == 0:
        return None
    k = int(bad[0])
    return k, len(bad), got.reshape(-1)[k], want.reshape(-1)[k]


# ------------------------------------------------------------------------------------------------ scenes ---
def build_scene(sph, mov, tri, sph_mat, mov_mat, tri_mat, kind, index):
    """A caller-owned rtow.Scene from numpy arrays (insertion order `kind` / `index`), with three materials and the
    cover scene's camera (the queries use none).  Returns an object with `.c` that keeps the arrays alive."""
    sph = np.ascontiguousarray(sph, dtype=np.float64).reshape(-1, 4)
    mov = np.ascontiguousarray(mov, dtype=np.float64).reshape(-1, 8)
    tri = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 9)
    sph_mat, mov_mat, tri_mat, kind, index = (np.ascontiguousarray(a, dtype=np.int32)
                                              for a in (sph_mat, mov_mat, tri_mat, kind, index))
    mats = (rtow.Material * 3)()
    mats[0].albedo[:] = [0.5, 0.5, 0.5]
    mats[1].kind, mats[1].ir = rtow.MAT_DIELECTRIC, 1.5
    mats[2].kind, mats[2].fuzz = rtow.MAT_METAL, 0.1
    mats[2].albedo[:] = [0.7, 0.6, 0.5]
    s = rtow.Scene()
    base = rtow.HostScene.cover(11, 1.5, False)
    s.camera = base.c.camera
    base.close()
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
    h.keep = [sph, mov, tri, sph_mat, mov_mat, tri_mat, kind, index, mats]
    return h


def ties_scene():
    """12 primitives: three bit-identical copies of one triangle and three of one sphere, inserted interleaved with the
    others (so the copies' insertion indices are 1, 4, 9 and 2, 6, 10); a ground sphere; a sphere of radius 2.5 that
    spans many grid cells; a moving sphere; two more triangles; a small sphere."""
    S = [0.4, 1.0, -4.0, 0.6]            # the copied sphere, behind the copied triangle
    T = [-2, 0, -2, 2, 0, -2, 0.3, 3, -2]  # the copied triangle, in the plane z = -2
    sph = np.array([[0, -1000, 0, 1000], S, [0, 1.2, -9.0, 2.5], S, S, [-3, 0.4, -1.0, 0.4]], dtype=np.float64)
    mov = np.array([[3, 0.5, -3, 3, 1.5, -3, 0.5, 0]], dtype=np.float64)
    tri = np.array([T, T, [-4, 0, -6, 4, 0, -6, 0, 4, -6], T, [1, 0, -1, 2, 0, -1, 1.5, 1, -1]], dtype=np.float64)
    #        pos:  0  1  2  3  4  5  6  7  8  9  10 11
    kind = [0, 2, 0, 0, 2, 1, 0, 2, 0, 2, 0, 2]
    index = [0, 0, 1, 2, 1, 0, 3, 2, 5, 3, 4, 4]
    return build_scene(sph, mov, tri, [0, 1, 0, 1, 1, 2], [0], [2, 2, 0, 2, 1], kind, index)


TIE_TRIANGLES = (1, 4, 9)  # insertion indices of the copies
TIE_SPHERES = (2, 6, 10)


def ties_rays(seed=19):
    """Rays from in front of the copied triangle through it and (most of them) the copied sphere behind it, a few along
    -z exactly (zero components), a few from inside the copied sphere, and a cloud."""
    g = np.random.default_rng(seed)
    o, d = [], []
    for _ in range(150):
        target = np.array([0.4, 1.0, -4.0]) + 0.5 * g.uniform(-1, 1, 3)
        origin = np.array([0.2, 1.0, 3.0]) + 0.3 * g.normal(size=3)
        o.append(origin), d.append(target - origin)
    for x in np.linspace(-0.1, 0.9, 11):
        o.append([x, 1.0, 2.0]), d.append([0.0, 0.0, -1.0])
    for _ in range(40):
        o.append(np.array([0.4, 1.0, -4.0]) + 0.2 * g.normal(size=3)), d.append(g.normal(size=3))
    for _ in range(100):
        o.append(g.uniform(-4, 4, 3) + [0, 2, -3]), d.append(g.normal(size=3))
    rays = rtow.make_rays(np.array(o), np.array(d), time=g.random(len(o)))
    return rays


# ------------------------------------------------------------------------------- rays that meet many primitives ---
def _scaled_segments(g, a, b):
    """Rays from a toward b with |d| scaled by exp(U(-3, 3)), seeded times; half with tmax = inf, half with a uniform
    fraction of 1.2 segment lengths in the ray's own parameter."""
    n = len(a)
    s = np.exp(g.uniform(-3, 3, size=(n, 1)))
    tmax = np.where(g.random(n) < 0.5, math.inf, g.random(n) * 1.2 / s[:, 0])
    return rtow.make_rays(a, (b - a) * s, time=g.random(n), tmax=tmax)


def chord_rays(n, seed):
    """Chords across the cover scenes' field of small spheres: both ends on the circle of radius 13 about the y axis at
    heights 0.05 .. 0.4, the far end opposite the near one within +-1 rad."""
    g = np.random.default_rng(seed)
    phi = g.uniform(0, 2 * np.pi, n)
    psi = phi + np.pi + g.uniform(-1, 1, n)
    a = np.c_[13 * np.cos(phi), g.uniform(0.05, 0.4, n), 13 * np.sin(phi)]
    b = np.c_[13 * np.cos(psi), g.uniform(0.05, 0.4, n), 13 * np.sin(psi)]
    return _scaled_segments(g, a, b)


def sheet_rays(n, seed):
    """Through accel_images.sheet_stack: from z = -0.5 to z = 1.6 through seeded points of [0.05, 0.95]^2."""
    g = np.random.default_rng(seed)
    a = np.c_[g.uniform(0.05, 0.95, size=(n, 2)), np.full(n, -0.5)]
    b = np.c_[g.uniform(0.05, 0.95, size=(n, 2)), np.full(n, 1.6)]
    return _scaled_segments(g, a, b)


def tmax_at_hits(rays, t, counts):
    """The rays that hit something, each with tmax at one of its own hits: entry j = 0, 3 or 7 of `t` [n, 8] (the
    deepest of these the ray has; j cycles over the rays) — its bits, the double below it or the double above it (cycling
    too)."""
    keep = np.flatnonzero(np.asarray(counts) > 0)
    out = rays[keep].copy()
    for m, i in enumerate(keep):
        j = max(x for x in (0, 3, 7)[:m % 3 + 1] if x < counts[i])
        v = float(t[i, j])
        out["tmax"][m] = (v, np.nextafter(v, -math.inf), np.nextafter(v, math.inf))[(m // 3) % 3]
    return out
