"""References for the closest-point queries (rtow_closest_point*): a numpy mirror of the kernel's formulas and an exact
distance (numpy and the standard library, no GPU).

Records.  The device holds, per class-major primitive: sphere (c, copysign(r^2, r)), moving sphere (c0, c1 - c0,
copysign(r^2, r), r), triangle (a, e1 = B - A, e2 = C - A, n = e1 x e2) — each an IEEE operation of the host's
(csrc/rtow_scene_records.h, no contraction).  `records(view)` rebuilds them from a support_scenes.SceneView.

Mirror.  `sphere_point` / `triangle_point` are csrc/rtow_pointq.h point_sphere / point_triangle written in numpy in the
same operation order (binary64, no contraction): the strict build's dist and point equal them bit for bit.  The radius
is R = sqrt(|r^2|) (correctly rounded), for every sphere.

Exact.  The distance to the records' geometry over the real numbers: a triangle's squared distance in Fraction (the
clamped projections onto the three edges and, when the exact e1 x e2 is not zero, the projection onto the plane if it
lies inside); a sphere's | |p - c| - R | with c = c0 + time (c1 - c0) exact and |p - c| from a 130-bit isqrt.

Bound (include/rtow.h): D - tau S <= d <= D + tau S + min(tau S k^2, h), tau = 32 u strict, 64 u fast (u = 2^-53):
S = |p - a|_1 + |e1|_1 + |e2|_1 for a triangle (k = |e1| |e2| / |e1 x e2|, h the smallest height; the k term is
absent for a sphere), S = |p - c|_1 + R (+ |c0|_1 + |time dc|_1 when moving) for a sphere.  Why: every candidate of
the triangle is a point ON it, up to the rounding of its residual (a few u S), so d never falls below D by more than
that; the best candidate is the exact one up to the rounding of its parameters — u |p - a| for an edge, u S k^2 for the
plane projection, whose Gram-form barycentrics divide by |e1 x e2|^2 — and the edges alone are within the smallest
height h of D whatever the projection does.  The fast build adds its contractions and its square root and reciprocal
(within 4e-15 relative: rtow_trace_math.h), which the factor 2 covers.

Point clause (include/rtow.h), for the reported point q of the reported primitive c, with the same tau:
  * on the surface: the exact distance from q to c's exact surface (exact_triangle_d2(q, t); | |q - c| - R | with the
    130-bit root) is <= tau S_q, S_q = |a|_1 + |e1|_1 + |e2|_1 for a triangle, |c|_1 + R for a sphere, |c0|_1 +
    |time dc|_1 + R for a moving one.  Why: q = (a + e1 s) + e2 t has at most 4 roundings per component on magnitudes
    that sum to S_q; edge parameters are clamped to [0, 1]; the plane candidate's s + t exceeds 1 by at most a few u in
    the strict build and by twice the 4e-15 of the fast reciprocal (about 36 u) in the fast one.  A sphere's unit vector
    has 3 roundings plus the root and the reciprocal, scaled by R and added to c;
  * consistent with the distance: | |p - q| - dist | <= tau (S + S_q), S the bound's: dist comes from the residual
    w - e1 s and q from a + e1 s, which differ by their own roundings only.  At a sphere's centre q = c + (R, 0, 0)
    satisfies both.
Measured on the mirror (test_point_query_host.py prints the figures): at most 0.08 of any band.

check_answers(rec, mats, pts, times, max_dist, hits, prec) asserts, for every query and with no sampling: the miss
record (dist +inf, point 0, prim = kind = material = -1); prim -> primitive c, kind and material that primitive's;
dist <= max_dist and within the band of the exact D of c; point within the two clauses; D of c within the bands of the
exact global minimum (candidates: the primitives the mirror puts within 1e-9 of the scale of its minimum, less those
whose lower bound — lower_bounds — already satisfies the inequality; compared in Fraction); hit versus miss: a miss is
wrong when some primitive's D + its band < max_dist, a hit when D - its band > max_dist, otherwise either answer is
allowed (`open` counts those); max_dist NaN or negative is always a miss, +inf never one; no field NaN, point finite.
Overflow: when D^2 of the reported primitive exceeds 2^1023 and dist is +inf, every distance of the mirror must be +inf
too (+inf <= +inf is accepted: any primitive, only with max_dist = +inf), and the point need only be finite; a miss
under a finite max_dist is then allowed (`overflow` counts both).  It returns queries, exact_pairs, worst_dist,
worst_surface and worst_consistency in units of their bands, open and overflow.  AnswerChecker is the same for many
answers to one batch.  all_sets and the functions above it are the point sets of test_gpu_exact_points.py.
"""
from __future__ import annotations

import math
from fractions import Fraction as Fr

import numpy as np

U = 2.0 ** -53
TAU = {"strict": 32 * U, "fast": 64 * U}
SPHERE, MOVING, TRIANGLE = 0, 1, 2


class Records:
    """Class-major records of a scene and the class-major -> insertion index table."""

    def __init__(self, sph, mov, tri, cls2ins=None):
        self.sph, self.mov, self.tri = sph, mov, tri
        self.ns, self.nm, self.nt = len(sph), len(mov), len(tri)
        self.n = self.ns + self.nm + self.nt
        self.cls2ins = np.arange(self.n) if cls2ins is None else cls2ins
        self.ins2cls = np.empty(self.n, dtype=np.int64)
        self.ins2cls[self.cls2ins] = np.arange(self.n)

    def kind_of(self, cid):
        cid = np.asarray(cid)
        return np.where(cid < self.ns, SPHERE, np.where(cid < self.ns + self.nm, MOVING, TRIANGLE))


def make_records(sph_geom, mov_geom, tri_geom, kind=None, index=None):
    """Records from the caller's geometry ([n,4] c r, [n,8] c0 c1 r -, [n,9] A B C), as the host forms them."""
    sg = np.asarray(sph_geom, dtype=np.float64).reshape(-1, 4)
    mg = np.asarray(mov_geom, dtype=np.float64).reshape(-1, 8)
    tg = np.asarray(tri_geom, dtype=np.float64).reshape(-1, 9)
    sph = np.empty((len(sg), 4))
    sph[:, 0:3] = sg[:, 0:3]
    sph[:, 3] = np.copysign(sg[:, 3] * sg[:, 3], sg[:, 3])
    mov = np.empty((len(mg), 8))
    mov[:, 0:3] = mg[:, 0:3]
    mov[:, 3:6] = mg[:, 3:6] - mg[:, 0:3]
    mov[:, 6] = np.copysign(mg[:, 6] * mg[:, 6], mg[:, 6])
    mov[:, 7] = mg[:, 6]
    tri = np.empty((len(tg), 12))
    a, b, c = tg[:, 0:3], tg[:, 3:6], tg[:, 6:9]
    e1, e2 = b - a, c - a
    tri[:, 0:3], tri[:, 3:6], tri[:, 6:9] = a, e1, e2
    tri[:, 9] = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]
    tri[:, 10] = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]
    tri[:, 11] = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
    cls2ins = None
    if kind is not None:
        ns, nm = len(sg), len(mg)
        base = {SPHERE: 0, MOVING: ns, TRIANGLE: ns + nm}
        cls2ins = np.empty(len(kind), dtype=np.int64)
        for i, (k, j) in enumerate(zip(kind, index)):
            cls2ins[base[int(k)] + int(j)] = i
    return Records(sph, mov, tri, cls2ins)


def records(view):
    """Records of a support_scenes.SceneView."""
    return make_records(view.sph, view.mov, view.tri, view.kind, view.index)


# ------------------------------------------------------------------------------------------------------ mirror ---
def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz


def _clamp01(x):
    return np.fmin(np.fmax(x, 0.0), 1.0)


def sphere_point(px, py, pz, cx, cy, cz, r2):
    """point_sphere: (dist, qx, qy, qz), broadcast over the arguments."""
    with np.errstate(all="ignore"):
        dx, dy, dz = px - cx, py - cy, pz - cz
        ln = np.sqrt(dx * dx + dy * dy + dz * dz)
        R = np.sqrt(np.abs(r2))
        pos = ln > 0.0
        inv = 1.0 / np.where(pos, ln, 1.0)
        qx = np.where(pos, cx + (dx * inv) * R, cx + R)
        qy = np.where(pos, cy + (dy * inv) * R, cy)
        qz = np.where(pos, cz + (dz * inv) * R, cz)
        return np.abs(ln - R), qx, qy, qz


def triangle_point(px, py, pz, t):
    """point_triangle on records t[..., 12]: (dist, qx, qy, qz), broadcast over the arguments."""
    ax, ay, az = t[..., 0], t[..., 1], t[..., 2]
    e1x, e1y, e1z = t[..., 3], t[..., 4], t[..., 5]
    e2x, e2y, e2z = t[..., 6], t[..., 7], t[..., 8]
    nx, ny, nz = t[..., 9], t[..., 10], t[..., 11]
    with np.errstate(all="ignore"):
        wx, wy, wz = px - ax, py - ay, pz - az
        d1, d2 = _dot(wx, wy, wz, e1x, e1y, e1z), _dot(wx, wy, wz, e2x, e2y, e2z)
        ee1, ee2, e12 = _dot(e1x, e1y, e1z, e1x, e1y, e1z), _dot(e2x, e2y, e2z, e2x, e2y, e2z), _dot(e1x, e1y, e1z, e2x, e2y, e2z)
        fx, fy, fz = e2x - e1x, e2y - e1y, e2z - e1z
        gx, gy, gz = wx - e1x, wy - e1y, wz - e1z
        ff, dg = _dot(fx, fy, fz, fx, fy, fz), _dot(gx, gy, gz, fx, fy, fz)
        s1 = np.where(ee1 > 0.0, _clamp01(d1 / ee1), 0.0)
        t2 = np.where(ee2 > 0.0, _clamp01(d2 / ee2), 0.0)
        u3 = np.where(ff > 0.0, _clamp01(dg / ff), 0.0)
        r1 = (wx - e1x * s1, wy - e1y * s1, wz - e1z * s1)
        r2 = (wx - e2x * t2, wy - e2y * t2, wz - e2z * t2)
        r3 = (gx - fx * u3, gy - fy * u3, gz - fz * u3)
        best = _dot(*r1, *r1)
        which = np.zeros(np.shape(best), dtype=np.int8)
        b2, b3 = _dot(*r2, *r2), _dot(*r3, *r3)
        m = b2 < best
        best, which = np.where(m, b2, best), np.where(m, 1, which)
        m = b3 < best
        best, which = np.where(m, b3, best), np.where(m, 2, which)
        nn = _dot(nx, ny, nz, nx, ny, nz)
        sn, tn = ee2 * d1 - e12 * d2, ee1 * d2 - e12 * d1
        inside = (nn > 0.0) & (sn >= 0.0) & (tn >= 0.0) & (sn + tn <= nn)
        s = np.where(inside, sn / nn, 0.0)
        tt = np.where(inside, tn / nn, 0.0)
        r0 = ((wx - e1x * s) - e2x * tt, (wy - e1y * s) - e2y * tt, (wz - e1z * s) - e2z * tt)
        b0 = _dot(*r0, *r0)
        m = inside & (b0 < best)
        best, which = np.where(m, b0, best), np.where(m, 3, which)
        q = []
        for a_, e1_, e2_, f_ in ((ax, e1x, e2x, fx), (ay, e1y, e2y, fy), (az, e1z, e2z, fz)):
            q.append(np.select([which == 0, which == 1, which == 2],
                               [a_ + e1_ * s1, a_ + e2_ * t2, (a_ + e1_) + f_ * u3], (a_ + e1_ * s) + e2_ * tt))
        return np.sqrt(best), q[0], q[1], q[2]


def prim_point(rec, cid, p, time):
    """Mirror of one primitive per query: cid [n] class-major ids, p [n, 3], time [n] -> (dist [n], point [n, 3])."""
    cid = np.asarray(cid, dtype=np.int64)
    n = len(cid)
    dist, q = np.full(n, np.inf), np.zeros((n, 3))
    time = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    k = rec.kind_of(cid)
    for kind in (SPHERE, MOVING, TRIANGLE):
        m = k == kind
        if not m.any():
            continue
        px, py, pz = p[m, 0], p[m, 1], p[m, 2]
        if kind == SPHERE:
            g = rec.sph[cid[m]]
            r = sphere_point(px, py, pz, g[:, 0], g[:, 1], g[:, 2], g[:, 3])
        elif kind == MOVING:
            g, tm = rec.mov[cid[m] - rec.ns], time[m]
            r = sphere_point(px, py, pz, g[:, 0] + tm * g[:, 3], g[:, 1] + tm * g[:, 4], g[:, 2] + tm * g[:, 5], g[:, 6])
        else:
            r = triangle_point(px, py, pz, rec.tri[cid[m] - rec.ns - rec.nm])
        dist[m] = r[0]
        q[m] = np.stack(r[1:], axis=1)
    return dist, q


def all_dists(rec, p, time, chunk=1 << 21):
    """Mirror distances of every (query, primitive): a generator of (rows slice, [rows, n_prims] array)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    time = np.broadcast_to(np.asarray(time, dtype=np.float64), (len(p),))
    rows = max(1, chunk // max(rec.n, 1))
    for i0 in range(0, len(p), rows):
        sl = slice(i0, min(i0 + rows, len(p)))
        px, py, pz = p[sl, 0:1], p[sl, 1:2], p[sl, 2:3]
        parts = []
        if rec.ns:
            g = rec.sph
            parts.append(sphere_point(px, py, pz, g[:, 0], g[:, 1], g[:, 2], g[:, 3])[0])
        if rec.nm:
            g, tm = rec.mov, time[sl, None]
            parts.append(sphere_point(px, py, pz, g[:, 0] + tm * g[:, 3], g[:, 1] + tm * g[:, 4], g[:, 2] + tm * g[:, 5],
                                      g[:, 6])[0])
        if rec.nt:
            parts.append(triangle_point(px, py, pz, rec.tri[None, :, :])[0])
        yield sl, np.concatenate(parts, axis=1)


def nearest(rec, p, time, max_dist=math.inf):
    """Mirror answer per query: (min dist [n] (inf on a miss), tied-set test function, argmin class id or -1)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    md = np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (len(p),))
    dmin = np.full(len(p), np.inf)
    arg = np.full(len(p), -1, dtype=np.int64)
    ties = {}
    for sl, D in all_dists(rec, p, time):
        dm = D.min(axis=1)
        dmin[sl] = dm
        arg[sl] = D.argmin(axis=1)
        for j in range(D.shape[0]):
            i = sl.start + j
            ties[i] = np.nonzero(D[j] == dm[j])[0]
    ok = md >= dmin  # (NaN max_dist: False)
    dmin = np.where(ok, dmin, np.inf)
    arg = np.where(ok, arg, -1)
    return dmin, ties, arg


# ------------------------------------------------------------------------------------------------------- exact ---
def _F(v):
    return Fr(float(v))


def exact_triangle_d2(p, t):
    """Exact squared distance from p to the triangle of record t (a, e1, e2)."""
    P = [_F(v) for v in p]
    a, e1, e2 = [_F(v) for v in t[0:3]], [_F(v) for v in t[3:6]], [_F(v) for v in t[6:9]]
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]  # noqa: E731
    sub = lambda x, y: [x[0] - y[0], x[1] - y[1], x[2] - y[2]]  # noqa: E731
    w = sub(P, a)

    def seg(o, d):
        r = sub(P, o)
        dd = dot(d, d)
        s = Fr(0) if dd == 0 else min(max(dot(r, d) / dd, Fr(0)), Fr(1))
        q = [r[k] - s * d[k] for k in range(3)]
        return dot(q, q)

    b = [a[k] + e1[k] for k in range(3)]
    best = min(seg(a, e1), seg(a, e2), seg(b, sub(e2, e1)))
    n = [e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0], e1[0] * e2[1] - e2[0] * e1[1]]
    nn = dot(n, n)
    if nn != 0:
        d1, d2, ee1, ee2, e12 = dot(w, e1), dot(w, e2), dot(e1, e1), dot(e2, e2), dot(e1, e2)
        s, tt = (ee2 * d1 - e12 * d2) / nn, (ee1 * d2 - e12 * d1) / nn
        if s >= 0 and tt >= 0 and s + tt <= 1:
            wn = dot(w, n)
            best = min(best, wn * wn / nn)
    return best


def _sqrt_fr(x: Fr, bits=130):
    """sqrt(x) to `bits` relative bits (rounded down), and an upper bound of its error."""
    if x == 0:
        return Fr(0), Fr(0)
    k = max(0, bits - (x.numerator.bit_length() - x.denominator.bit_length()) // 2)
    s = Fr(math.isqrt(x.numerator * 4 ** k // x.denominator), 2 ** k)
    return s, Fr(1, 2 ** k)


def exact_dist(rec, cid, p, time):
    """Exact distance from p to class-major primitive cid: (D as a Fraction, its error bound as a Fraction)."""
    k = int(rec.kind_of(cid))
    P = [_F(v) for v in p]
    if k == TRIANGLE:
        return _sqrt_fr(exact_triangle_d2(p, rec.tri[cid - rec.ns - rec.nm]))
    if k == SPHERE:
        g = rec.sph[cid]
        c = [_F(g[0]), _F(g[1]), _F(g[2])]
        r2 = g[3]
    else:
        g = rec.mov[cid - rec.ns]
        tm = _F(time)
        c = [_F(g[j]) + tm * _F(g[3 + j]) for j in range(3)]
        r2 = g[6]
    R = _F(np.sqrt(abs(r2)))
    x = sum((P[j] - c[j]) ** 2 for j in range(3))
    L, e = _sqrt_fr(x)
    return abs(L - R), e


def bound(rec, cid, p, time, prec):
    """The stated band of rtow.h for class-major primitive cid at p: (below, above) as floats (rounded up)."""
    tau = TAU[prec]
    k = int(rec.kind_of(cid))
    p = np.asarray(p, dtype=np.float64)
    if k == TRIANGLE:
        t = rec.tri[cid - rec.ns - rec.nm]
        a, e1, e2 = t[0:3], t[3:6], t[6:9]
        S = float(np.abs(p - a).sum() + np.abs(e1).sum() + np.abs(e2).sum())
        n = np.cross(e1, e2)
        ln = float(np.linalg.norm(n))
        l1, l2, l3 = float(np.linalg.norm(e1)), float(np.linalg.norm(e2)), float(np.linalg.norm(e2 - e1))
        h = ln / max(l1, l2, l3, 1e-300)
        extra = min(tau * S * (l1 * l2 / ln) ** 2, h) if ln > 0 else 0.0  # (no area: no plane candidate)
        return 1.01 * tau * S, 1.01 * (tau * S + extra)
    if k == SPHERE:
        g = rec.sph[cid]
        c = g[0:3]
        S = float(np.abs(p - c).sum() + np.sqrt(abs(g[3])))
    else:
        g = rec.mov[cid - rec.ns]
        c = g[0:3] + time * g[3:6]
        S = float(np.abs(p - c).sum() + np.sqrt(abs(g[6])) + np.abs(g[0:3]).sum() + np.abs(time * g[3:6]).sum())
    return 1.01 * tau * S, 1.01 * tau * S


def within(d, D, err, lo, hi):
    """D - lo <= d <= D + hi, with D known to within err (exact comparisons)."""
    d = _F(d)
    return D - _F(lo) - err <= d <= D + _F(hi) + err


# ----------------------------------------------------------------------------------------------------- checker ---
def scene_box(rec, max_radius=math.inf):
    """(lo, hi) of the records' geometry: triangle vertices, spheres of radius < max_radius, moving spheres at both ends."""
    pts = [rec.tri[:, 0:3], rec.tri[:, 0:3] + rec.tri[:, 3:6], rec.tri[:, 0:3] + rec.tri[:, 6:9]]
    R = np.sqrt(np.abs(rec.sph[:, 3:4]))
    keep = R[:, 0] < max_radius
    pts += [(rec.sph[:, 0:3] - R)[keep], (rec.sph[:, 0:3] + R)[keep]]
    if rec.nm:
        r = np.abs(rec.mov[:, 7:8])
        c1 = rec.mov[:, 0:3] + rec.mov[:, 3:6]
        pts += [rec.mov[:, 0:3] - r, rec.mov[:, 0:3] + r, c1 - r, c1 + r]
    pts = np.concatenate([p for p in pts if len(p)])
    return pts.min(0), pts.max(0)


def _l1(v):
    return sum(abs(x) for x in v)


def exact_geometry(rec, cid, time):
    """Exact data of class-major primitive cid at `time`: (kind, S_q, triangle record | (centre, R))."""
    k = int(rec.kind_of(cid))
    if k == TRIANGLE:
        t = rec.tri[cid - rec.ns - rec.nm]
        return k, _l1([_F(v) for v in t[0:9]]), t
    if k == SPHERE:
        g = rec.sph[cid]
        c = [_F(g[0]), _F(g[1]), _F(g[2])]
        R = _F(np.sqrt(abs(g[3])))
        return k, _l1(c) + R, (c, R)
    g = rec.mov[cid - rec.ns]
    tm = _F(time)
    c = [_F(g[j]) + tm * _F(g[3 + j]) for j in range(3)]
    R = _F(np.sqrt(abs(g[6])))
    return k, _l1([_F(g[j]) for j in range(3)]) + _l1([tm * _F(g[3 + j]) for j in range(3)]) + R, (c, R)


def header_scale(geom, p):
    """S of include/rtow.h for the distance of primitive `geom` (exact_geometry) at p, as a Fraction."""
    k, Sq, g = geom
    P = [_F(v) for v in p]
    if k == TRIANGLE:
        return _l1([P[j] - _F(g[j]) for j in range(3)]) + _l1([_F(v) for v in g[3:9]])
    c, R = g
    S = _l1([P[j] - c[j] for j in range(3)]) + R
    if k == MOVING:
        S += Sq - R  # |c0|_1 + |time dc|_1
    return S


def surface_error(geom, q):
    """Exact distance from q to the primitive's exact surface: (value as a Fraction, its error bound)."""
    k, Sq, g = geom
    if k == TRIANGLE:
        return _sqrt_fr(exact_triangle_d2(q, g))
    c, R = g
    L, e = _sqrt_fr(sum((_F(q[j]) - c[j]) ** 2 for j in range(3)))
    return abs(L - R), e


def lower_bounds(rec, cids, p, time):
    """Floats lb[j] <= the exact distance from p to class-major primitive cids[j]: for a triangle the distance to the
    box of its vertices, padded by 4 u of the record's magnitudes (a + e1 is not exact in binary64) and scaled down by
    2^-50 (six roundings of positive terms); for a sphere the mirror's distance less 16 u S (its forward error: three
    differences, the sum of squares, the root, the radius; half the strict band).  Only a preselection uses them: a
    primitive whose lower bound already satisfies the inequality at hand needs no Fraction."""
    cids = np.asarray(cids, dtype=np.int64)
    out = np.empty(len(cids))
    p = np.asarray(p, dtype=np.float64)
    k = rec.kind_of(cids)
    with np.errstate(all="ignore"):
        m = k == TRIANGLE
        if m.any():
            t = rec.tri[cids[m] - rec.ns - rec.nm]
            a, b, c = t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]
            pad = 4 * U * (np.abs(t[:, 0:3]) + np.abs(t[:, 3:6]) + np.abs(t[:, 6:9]))
            lo, hi = np.minimum(np.minimum(a, b), c) - pad, np.maximum(np.maximum(a, b), c) + pad
            d = np.maximum(np.maximum(lo - p, p - hi), 0.0)
            out[m] = np.sqrt((d * d).sum(1)) * (1.0 - 2.0 ** -50)
        m = k == SPHERE
        if m.any():
            g = rec.sph[cids[m]]
            d = sphere_point(p[0], p[1], p[2], g[:, 0], g[:, 1], g[:, 2], g[:, 3])[0]
            S = np.abs(p - g[:, 0:3]).sum(1) + np.sqrt(np.abs(g[:, 3]))
            out[m] = d - 16 * U * S
        m = k == MOVING
        if m.any():
            g = rec.mov[cids[m] - rec.ns]
            c = g[:, 0:3] + time * g[:, 3:6]
            d = sphere_point(p[0], p[1], p[2], c[:, 0], c[:, 1], c[:, 2], g[:, 6])[0]
            S = np.abs(p - c).sum(1) + np.sqrt(np.abs(g[:, 6])) + np.abs(g[:, 0:3]).sum(1) + np.abs(time * g[:, 3:6]).sum(1)
            out[m] = d - 16 * U * 1.01 * S
    return out


def _units(x, band):
    """x >= 0 in units of its band (a point triangle at the query point has a band of 0, and an error of 0)."""
    return 0.0 if x == 0 else math.inf if band == 0 else float(x / band)


OVERFLOW = Fr(2) ** 1023  # an exact squared distance above this may round to +inf in binary64


class AnswerChecker:
    """check_answers for one batch of queries, reusable for many answers to it (every kernel, build and builder): the
    mirror's distances, the exact distances and the verdict per distinct answer are computed once."""

    def __init__(self, rec, mats, pts, times, max_dist):
        self.rec, self.mats = rec, np.asarray(mats)
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        n = len(self.pts)
        self.times = np.array(np.broadcast_to(np.asarray(times, dtype=np.float64), (n,)))
        self.md = np.array(np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,)))
        lo, hi = scene_box(rec)
        scale = float(np.abs(lo).sum() + np.abs(hi).sum())
        self.dmin, self.near, self.ties = np.empty(n), [None] * n, {}
        with np.errstate(all="ignore"):
            self.band9 = np.minimum(1e-9 * (np.abs(self.pts).sum(1) + scale), 1e300)
            for sl, D in all_dists(rec, self.pts, self.times):
                dm = D.min(axis=1)
                self.dmin[sl] = dm
                band = self.band9[sl]
                for j in range(D.shape[0]):  # the primitives the mirror puts within 1e-9 of the scale of its minimum
                    self.near[sl.start + j] = np.nonzero(D[j] <= dm[j] + band[j])[0]
                    self.ties[sl.start + j] = np.nonzero(D[j] == dm[j])[0]
        self._geom, self._exact, self._band, self._memo = {}, {}, {}, {}
        # bit-identical records (coincident copies) share their exact quantities: canon[c] is the first such primitive
        self.canon = np.arange(rec.n)
        for base, recs in ((0, rec.sph), (rec.ns, rec.mov), (rec.ns + rec.nm, rec.tri)):
            if len(recs):
                _, first, inv = np.unique(np.ascontiguousarray(recs).view(np.uint64), axis=0, return_index=True,
                                          return_inverse=True)
                self.canon[base:base + len(recs)] = base + first[np.ravel(inv)]

    def mirror_dmin(self):
        """The mirror's answer as `nearest` gives it: the minimum where max_dist >= it, else +inf."""
        return np.where(self.md >= self.dmin, self.dmin, np.inf)

    # ---- memoised exact quantities
    def geom(self, i, c):
        key = (c, float(self.times[i]) if c >= self.rec.ns and c < self.rec.ns + self.rec.nm else 0.0)
        if key not in self._geom:
            self._geom[key] = exact_geometry(self.rec, c, key[1])
        return self._geom[key]

    def exact(self, i, c):
        c = int(self.canon[c])
        if (i, c) not in self._exact:
            self._exact[(i, c)] = exact_dist(self.rec, c, self.pts[i], self.times[i])
        return self._exact[(i, c)]

    def band(self, i, c, prec):
        c = int(self.canon[c])
        if (i, c, prec) not in self._band:
            lo, hi = bound(self.rec, c, self.pts[i], self.times[i], prec)
            self._band[(i, c, prec)] = (_F(lo), _F(hi))
        return self._band[(i, c, prec)]

    def candidates(self, i, ub):
        """The primitives of near[i] whose exact distance may be below ub (a Fraction or +inf)."""
        near = self.near[i]
        if ub == math.inf or len(near) <= 1:
            return near
        lim = float(ub) * (1.0 + 2.0 ** -50) + 5e-324
        return near[lower_bounds(self.rec, near, self.pts[i], self.times[i]) <= lim]

    # ---- one answer
    def _check_one(self, i, h, prec):
        """(dist err, surface err, consistency err) in units of their bands, open (hit/miss left to the band), overflow."""
        rec, p, md = self.rec, self.pts[i], float(self.md[i])
        tau = _F(TAU[prec])
        dist, q, prim = float(h["dist"]), np.array(h["point"], dtype=np.float64), int(h["prim"])
        assert not math.isnan(dist) and not np.isnan(q).any(), ("NaN in the answer", dist, q.tolist())
        assert np.all(np.isfinite(q)), ("point is not finite", q.tolist())
        no_walk = math.isnan(md) or md < 0.0
        if prim == -1:  # ---- a miss
            assert dist == math.inf and np.all(q == 0.0) and int(h["kind"]) == -1 and int(h["material"]) == -1, \
                ("not the miss record", dist, q.tolist(), int(h["kind"]), int(h["material"]))
            if no_walk:
                return 0.0, 0.0, 0.0, 0, 0
            assert md != math.inf, "a miss with max_dist = +inf on a scene with primitives"
            if self.dmin[i] == math.inf:  # every computed distance overflows: +inf <= max_dist fails
                return 0.0, 0.0, 0.0, 0, 1
            opened = 0
            for c2 in self.candidates(i, _F(md) + _F(self.band9[i])):  # (the margin: so that `opened` counts every one)
                D2, e2 = self.exact(i, int(c2))
                lo2, hi2 = self.band(i, int(c2), prec)
                assert not D2 + hi2 + e2 < _F(md), ("a miss, but a primitive is within max_dist by more than its band",
                                                    int(c2), float(D2), md)
                opened |= int(D2 - lo2 - e2 <= _F(md))
            return 0.0, 0.0, 0.0, opened, 0
        # ---- a hit
        assert not no_walk, ("a hit under a NaN or negative max_dist", md)
        assert 0 <= prim < rec.n, ("prim out of range", prim)
        c = int(rec.ins2cls[prim])
        assert int(h["kind"]) == int(rec.kind_of(c)), ("kind is not the primitive's", int(h["kind"]), int(rec.kind_of(c)))
        assert int(h["material"]) == int(self.mats[prim]), ("material is not the primitive's", int(h["material"]))
        assert dist <= md, ("dist above max_dist", dist, md)
        geom = self.geom(i, c)
        k, Sq, _ = geom
        D, err = self.exact(i, c)
        if dist == math.inf and D * D > OVERFLOW:  # ---- the overflow rule
            assert self.dmin[i] == math.inf, "dist +inf although the formulas give a finite distance to some primitive"
            return 0.0, 0.0, 0.0, 0, 1
        lo, hi = self.band(i, c, prec)
        assert within(dist, D, err, lo, hi), ("dist outside its band", c, dist, float(D), float(lo), float(hi))
        d = _F(dist)
        e_dist = _units(d - D, hi) if d >= D else _units(D - d, lo)
        # the point: on the surface, and consistent with dist
        s_err, s_e = surface_error(geom, q)
        assert s_err - s_e <= tau * Sq, ("point off the surface", c, q.tolist(), float(s_err), float(tau * Sq))
        e_surf = _units(s_err, tau * Sq)
        L, l_e = _sqrt_fr(sum((_F(p[j]) - _F(q[j])) ** 2 for j in range(3)))
        S = header_scale(geom, p)
        assert abs(L - d) - l_e <= tau * (S + Sq), ("|p - point| differs from dist", c, float(L), dist,
                                                    float(tau * (S + Sq)))
        e_cons = _units(abs(L - d), tau * (S + Sq))
        # the global minimum, and hit versus miss
        assert md == math.inf or D - lo - err <= _F(md), ("a hit on a decided miss", c, float(D), md)
        decided = md == math.inf or D + hi + err < _F(md)
        for c2 in self.candidates(i, D - lo + err):
            c2 = int(c2)
            D2, e2 = self.exact(i, c2)
            lo2, hi2 = self.band(i, c2, prec)
            # (the kernel's dist >= D - lo, and it is <= its own value for c2, <= D2 + hi2)
            assert D <= D2 + hi2 + lo + err + e2, ("a primitive is nearer by more than the bands", c, c2, float(D), float(D2))
            decided = decided or D2 + hi2 + e2 < _F(md)
        return e_dist, e_surf, e_cons, int(not decided), 0

    def check(self, hits, prec, what=""):
        n = len(self.pts)
        assert len(hits) == n, (what, len(hits), n)
        out = dict(queries=n, worst_dist=0.0, worst_surface=0.0, worst_consistency=0.0, open=0, overflow=0)
        for i in range(n):
            h = hits[i]
            key = (i, prec, h.tobytes())
            if key not in self._memo:
                try:
                    self._memo[key] = self._check_one(i, h, prec)
                except AssertionError as e:
                    raise AssertionError(f"{what} query {i} p={self.pts[i].tolist()} time={self.times[i]} "
                                         f"max_dist={self.md[i]} prim={int(h['prim'])}: {e}") from None
            r = self._memo[key]
            out["worst_dist"] = max(out["worst_dist"], r[0])
            out["worst_surface"] = max(out["worst_surface"], r[1])
            out["worst_consistency"] = max(out["worst_consistency"], r[2])
            out["open"] += r[3]
            out["overflow"] += r[4]
        out["exact_pairs"] = len(self._exact)
        return out


def check_answers(rec, mats, pts, times, max_dist, hits, prec, what=""):
    """Assert the whole contract of include/rtow.h on `hits` (the answers to the queries pts / times / max_dist) at
    tau of `prec`, query by query, and return the statistics (see the module docstring)."""
    return AnswerChecker(rec, mats, pts, times, max_dist).check(hits, prec, what)


# -------------------------------------------------------------------------------------------------- point sets ---
FAR = (10.0, 1e3, 1e6, 1e9, 1e12, 1e15, 1e18, 1e100)  # extents from the box centre
SIZES = dict(tri=10, sph=8, mov=8, far_dirs=4, near=100, random=100, mixed=203)
SIZES_BIG = dict(tri=2, sph=0, mov=0, far_dirs=1, near=7, random=7, mixed=13)  # the 96.8k mesh: under 100 points


def _box(rec):
    lo, hi = scene_box(rec, 100.0)
    return lo, hi, float(max(np.max(hi - lo), 1e-3))


def _pick(g, n, k):
    return g.choice(n, size=min(k, n), replace=False) if n else np.zeros(0, dtype=np.int64)


def _moving_centres(rec, idx, time):
    m = rec.mov[idx]
    return m[:, 0:3] + time * m[:, 3:6], np.sqrt(np.abs(m[:, 6]))


def surface_points(rec, time, seed, sizes=SIZES):
    """Points on the primitives: per sampled triangle A, B, C, an edge midpoint, an uneven edge point, the centroid and
    the centroid -1e-9, +1e-9 and +0.01 along the normal; per sampled sphere (a moving one at `time`) the centre, the
    centre + 1e-12, c + (R, 0, 0) and a point 0.9 R from the centre."""
    g = np.random.default_rng(seed)
    out = []
    for t in rec.tri[_pick(g, rec.nt, sizes["tri"])]:
        A, B, C = t[0:3], t[0:3] + t[3:6], t[0:3] + t[6:9]
        n = t[9:12]
        n = n / np.linalg.norm(n) if np.linalg.norm(n) > 0 else np.array([0.0, 0.0, 1.0])
        G = (A + B + C) / 3
        out += [A, B, C, 0.5 * (A + B), 0.3 * B + 0.7 * C, G, G - 1e-9 * n, G + 1e-9 * n, G + 0.01 * n]
    i = _pick(g, rec.ns, sizes["sph"])
    j = _pick(g, rec.nm, sizes["mov"])
    cm, rm = _moving_centres(rec, j, time)
    cs = np.concatenate([rec.sph[i, 0:3], cm])
    rs = np.concatenate([np.sqrt(np.abs(rec.sph[i, 3])), rm])
    for c, R in zip(cs, rs):
        d = g.normal(size=3)
        out += [c, c + [1e-12, 0, 0], c + [R, 0, 0], c + 0.9 * R * d / np.linalg.norm(d)]
    return np.array(out, dtype=np.float64)


def far_points(rec, seed, sizes=SIZES):
    """far_dirs random directions at each of FAR extents from the centre of the box."""
    g = np.random.default_rng(seed)
    lo, hi, ext = _box(rec)
    d = g.normal(size=(len(FAR), sizes["far_dirs"], 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return (0.5 * (lo + hi) + d * (np.array(FAR) * ext)[:, None, None]).reshape(-1, 3)


def overflow_points():
    """|p| whose square exceeds the binary64 range, on an axis and off it."""
    out = []
    for m in (1e160, 1e200, 1e307):
        out += [[m, 0.0, 0.0], [0.6 * m, -0.5 * m, 0.62 * m]]
    return np.array(out + [[1.7e308, 0.0, 0.0], [0.0, 0.0, -1.7e308]])


def near_points(rec, time, n, seed):
    """(n random points of the surfaces, each moved by up to 2 % of the extent, max_dist 5 %) — for scenes without a
    ray log."""
    g = np.random.default_rng(seed)
    lo, hi, ext = _box(rec)
    out = np.empty((n, 3))
    cid = g.integers(rec.n, size=n)
    for k, c in enumerate(cid):
        if c < rec.ns + rec.nm:
            if c < rec.ns:
                ctr, R = rec.sph[c, 0:3], math.sqrt(abs(rec.sph[c, 3]))
            else:
                cm, rm = _moving_centres(rec, [c - rec.ns], time)
                ctr, R = cm[0], rm[0]
            d = g.normal(size=3)
            out[k] = ctr + R * d / np.linalg.norm(d)
        else:
            t = rec.tri[c - rec.ns - rec.nm]
            s, u = g.random(2)
            if s + u > 1:
                s, u = 1 - s, 1 - u
            out[k] = t[0:3] + s * t[3:6] + u * t[6:9]
    return out + g.uniform(-0.02, 0.02, size=(n, 3)) * ext, 0.05 * ext


def random_points(rec, n, seed):
    lo, hi, ext = _box(rec)
    return np.random.default_rng(seed).uniform(lo - 0.05 * ext, hi + 0.05 * ext, size=(n, 3))


def mixed_lanes(rec, near, seed, strict_values=False):
    """(points, times, max_dist) of one batch in which every wave of 64 consecutive queries holds every value: time
    cycles through 0, 1, U(0, 1) and max_dist through NaN, -1, 0.5 d_min, 2 d_min, +inf (d_min: the mirror's, at the
    query's own time) — and, with strict_values, through 0 at a point ON a surface, d_min and the double below d_min,
    which the mirror decides."""
    g = np.random.default_rng(seed)
    n = len(near)
    pts = np.array(near, dtype=np.float64)
    k = np.arange(n)
    times = np.select([k % 3 == 0, k % 3 == 1], [0.0, 1.0], g.random(n))
    cyc = 8 if strict_values else 5
    sel = k % cyc  # (5 and 8 are coprime to 3: every (time, max_dist) pair occurs within 15 / 24 consecutive lanes)
    if strict_values:
        on = np.nonzero(sel == 5)[0]
        for i in on:
            s = surface_points(rec, times[i], seed + int(i), dict(tri=1, sph=1, mov=1))
            pts[i] = s[g.integers(len(s))]
    dmin = nearest(rec, pts, times)[0]
    md = np.select([sel == 0, sel == 1, sel == 2, sel == 3, sel == 4, sel == 5, sel == 6],
                   [np.nan, -1.0, 0.5 * dmin, 2.0 * dmin, np.inf, 0.0, dmin], np.nextafter(dmin, -np.inf))
    return pts, times, md


def all_sets(rec, seed, near=None, rnd=None, sizes=SIZES, refit=False):
    """[(set name, points, times, max_dist)] of a scene: surface, far, overflow, near and random at time 0 (and 0.5 and 1
    where there are moving spheres: the documented range), and the two mixed-lanes batches.  `near` ((points, max_dist))
    and `rnd` (points) replace the generated sets; after a refit the sets are surface, far and random.  No count is a
    multiple of 64."""
    out = []
    for tm in ((0.0, 0.5, 1.0) if rec.nm else (0.0,)):
        nr = near if near is not None else near_points(rec, tm, sizes["near"], seed + 3)
        rd = rnd if rnd is not None else random_points(rec, sizes["random"], seed + 2)
        sets = [("surface", surface_points(rec, tm, seed, sizes), math.inf),
                ("far", far_points(rec, seed + 1, sizes), math.inf), ("random", rd[:sizes["random"]], math.inf)]
        if not refit:
            sets += [("overflow", overflow_points(), math.inf), ("near", nr[0][:sizes["near"]], nr[1])]
        out += [(f"{s}@{tm:g}", p[:-1] if len(p) % 64 == 0 else p, tm, md) for s, p, md in sets]
    if not refit:
        nr = near if near is not None else near_points(rec, 0.5, sizes["mixed"], seed + 4)
        if len(nr[0]) < sizes["mixed"]:
            nr = near_points(rec, 0.5, sizes["mixed"], seed + 4)
        for nm, strict_values in (("mixed", False), ("mixed_strict", True)):
            out.append((nm,) + mixed_lanes(rec, nr[0][:sizes["mixed"]], seed + 5, strict_values))
    assert all(len(p) % 64 for _, p, _, _ in out)
    return out


HIT_DTYPE = np.dtype([("dist", "<f8"), ("point", "<f8", (3,)), ("prim", "<i4"), ("kind", "<i4"), ("material", "<i4"),
                      ("pad_", "<i4")])  # rtow_point_hit_t


def mirror_answers(rec, mats, pts, times, max_dist, of=None):
    """The mirror's answer records (HIT_DTYPE) to the queries; `of` ([n] class-major ids) answers with those primitives
    instead of the nearest ones, whatever max_dist says."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    times = np.broadcast_to(np.asarray(times, dtype=np.float64), (n,))
    arg = nearest(rec, pts, times, max_dist)[2] if of is None else np.asarray(of, dtype=np.int64)
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["dist"], h["prim"], h["kind"], h["material"] = np.inf, -1, -1, -1
    hit = arg >= 0
    h["dist"][hit], h["point"][hit] = prim_point(rec, arg[hit], pts[hit], times[hit])
    h["prim"][hit] = rec.cls2ins[arg[hit]]
    h["kind"][hit] = rec.kind_of(arg[hit])
    h["material"][hit] = np.asarray(mats)[h["prim"][hit]]
    return h


def stats_line(s):
    return (f"{s['queries']} queries, {s['exact_pairs']} exact pairs, worst dist {s['worst_dist']:.3f}, on-surface "
            f"{s['worst_surface']:.3f}, consistency {s['worst_consistency']:.3f} of their bands, open {s['open']}, "
            f"overflow {s['overflow']}")
