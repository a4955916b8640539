"""References for the closest-point queries (rtow_closest_point*): a numpy mirror of the kernel's formulas and an exact
distance (numpy and the standard library, no GPU).

Records.  The device holds, per class-major primitive: sphere (c, copysign(r^2, r)), moving sphere (c0, c1 - c0,
copysign(r^2, r), r), triangle (a, e1 = B - A, e2 = C - A, n = e1 x e2) — each an IEEE operation of the host's
(csrc/rtow_capi.cpp, no contraction).  `records(view)` rebuilds them from a test_gpu_query.SceneView.

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
    """Records of a test_gpu_query.SceneView."""
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
