"""References for the swept-sphere queries (rtow_sweep*): a numpy mirror of the kernel's formulas and an exact segment
distance (numpy and the standard library, no GPU).  Records, classes and the point formulas are point_ref's.

(a) Mirror.  `sphere_sweep` / `triangle_sweep` are csrc/rtow_sweep_walks.h sweep_sphere / sweep_triangle written in numpy
in the same operation order (binary64, no contraction), `answers` the scene's answer by (t, insertion index) with dist and
point through point_ref's mirror at the centre: the strict build's records equal them bit for bit.  The brute force runs
over (query, primitive) PAIRS; triangles are preselected by a slab test of the sweep against the triangle's box grown by
rho and a margin of 1e-9 of the magnitudes (a triangle outside it cannot be touched: the mirror's t differs from the
exact contact by rounding only), which keeps the 96,800-triangle mesh affordable.

(b) Exact.  Independent of the formulas: the DISTANCE FROM A SEGMENT TO A PRIMITIVE over the reals.  The sphere cast
touches primitive c somewhere on [o, p(t)] exactly when segdist(o, p(t), c) <= rho.  Triangle: the squared distance from
the segment to the triangle in Fraction — 0 when the segment pierces the triangle, otherwise the minimum of the three
segment-edge distances and the two endpoint-triangle distances (point_ref.exact_triangle_d2).  Sphere (surface): with m
the exact distance from the centre c to the segment and M the larger endpoint distance, 0 if m <= R <= M, else
min(|m - R|, |M - R|); roots by the 130-bit isqrt.  A vectorised binary64 filter with its own forward bound goes first
(`segdist_f64`: the same geometry in floating point; its error is below FILTER_U u S, see there) and only pairs within
the band plus that bound of rho go to Fraction.

(c) check_answers(rec, mats, sweeps, hits, prec): every query, no sampling.  A hit at t <= tmax (bitwise) on
c*: |D_exact(centre, c*) - rho| <= band (a start overlap: t == 0 and D_exact(o, c*) <= rho + band); dist and point meet
point_ref's two point clauses at centre; for every primitive c segdist_exact(o, centre, c) >= rho - band(c).  A miss:
segdist_exact(o, p(tmax), c) >= rho - band(c) for every c — with tmax = +inf over [o, p(T)], T the smallest power of two
at which the sweep has provably left the scene for good (Checker.horizon).  Where a primitive's segment distance is within its band of
rho either answer is allowed (`open` counts those queries: a miss with such a primitive, a hit that grazed such a primitive
on the way — one that is at rho from the hit's centre as well, across a shared edge or vertex, ties at the same t and
leaves nothing open).  Also: the miss record, skipped queries, kind / material of
the reported primitive, no NaN anywhere.

(d) Band = K u S, u = 2^-53, S = |o|_1 + |t d|_1 + rho + the primitive's magnitudes (point_ref's S_q: |a|_1 + |e1|_1 +
|e2|_1; |c|_1 + R; |c0|_1 + |time dc|_1 + R).  K counts roundings on the longest path of a candidate, each in units of
u S (a rounding of a quantity of magnitude <= S contributes <= u S to the position of the contact):
  * the root through the perpendicular (sweep_root), for a start vector w (|w| <= S) and a direction d:
      w = o - v: 1;  h = w.d: 3 products + 2 sums, relative to |w||d|: 5;  inv_a: 1 (+3 for a = d.d);  t0 = h inv_a: 1;
      q = w + d t0: 2 per component;  q.q: 5, halved by the root;  r^2 - q.q: 1;  (..) inv_a: 1;  sqrt: 1;  t0 - s: 1.
    About 9 on |t0 d| and |w|, 5 more on the half chord: 14 for a vertex or a sphere (whose R + rho and sqrt |r^2| add 2,
    and a moving centre 2 more): 18;
  * an edge adds the two projections across it — ie: 1 (+5), we, de: 5 each, we ie: 1, w - e (..): 2 per component, twice —
    about 14 on magnitudes <= S, and its own 1 / A: 28 in all, plus the axial test, which only selects;
  * the face: n.w and n.d: 5 each, sqrt(n.n): 1 (+5 halved), rho |n|: 1, the difference: 1, the quotient: 1: 17;
  * centre = o + d t: 2 per component, in every case.
(A start that a piece's arithmetic puts inside it answers t = 0: no new path, the clamp of sweep_root and max(num, 0).)
So K_strict = 32 would cover the longest path; the measured worst of the mirror against (b) over all the sets of
test_sweep_host.py is printed there (1.24 u S, on the unbounded rows) and 48 >= 4 x that, which leaves room for inputs
outside the sets:
K_STRICT = 48, K_FAST = 2 K_STRICT = 96 (the project's allowance for contraction and the 4e-15 of the fast reciprocal
and root).
"""
from __future__ import annotations

import math
from fractions import Fraction as Fr

import numpy as np

import point_ref as pr
from point_ref import MOVING, SPHERE, TRIANGLE, U, _F, _sqrt_fr

K = {"strict": 48, "fast": 96}
FILTER_U = 256  # forward bound of segdist_f64, in units of u S (see there)

QUERY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("time", "<f8"), ("direction", "<f8", (3,)), ("tmax", "<f8"),
                        ("radius", "<f8"), ("pad_", "<f8")])  # rtow_sweep_t
HIT_DTYPE = np.dtype([("t", "<f8"), ("dist", "<f8"), ("centre", "<f8", (3,)), ("point", "<f8", (3,)),
                      ("prim", "<i4"), ("kind", "<i4"), ("material", "<i4"), ("start_overlap", "<i4")])  # rtow_sweep_hit_t


def make_sweeps(o, d, radius, time=0.0, tmax=math.inf):
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(len(o), dtype=QUERY_DTYPE)
    q["origin"], q["direction"] = o, np.asarray(d, dtype=np.float64).reshape(-1, 3)
    q["time"], q["tmax"], q["radius"] = time, tmax, radius
    return q


def skipped(q):
    """The queries that get the miss record without a walk (include/rtow.h)."""
    with np.errstate(all="ignore"):
        o, d = q["origin"], q["direction"]
        a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        ok = (np.isfinite(o).all(1) & np.isfinite(q["time"]) & (q["radius"] >= 0.0) & np.isfinite(q["radius"])
              & (q["tmax"] >= 0.0) & (a > 0.0) & np.isfinite(a))
    return ~ok


# ------------------------------------------------------------------------------------------------------ mirror ---
_dot = pr._dot


GUARDS = ("outer", "inner", "vertex", "edge", "face")
"""The "starts outside this piece" tests of the rule before the present one, by piece.  They repeated the overlap test
in other arithmetic (rounded squares against rho^2 and (R +- rho)^2, not a rounded distance against rho), and a start
a few ulps from contact could fail both and belong to no branch.  `old` (a set of these names) puts a guard back into
the mirror, one piece at a time: the mutants of test_sweep_host.py, each of which the exact checker must refuse."""


def _root(w, d, h, inv_a, r, far, clamp=False):
    """sweep_root: the near (far) root of |w + d t| = r, clamped to t >= 0; +inf for none.  clamp: a negative
    r^2 - q.q counts as 0 (the kernel's far root)."""
    t0 = -(h * inv_a)
    qx, qy, qz = w[0] + d[0] * t0, w[1] + d[1] * t0, w[2] + d[2] * t0
    dd = r * r - _dot(qx, qy, qz, qx, qy, qz)
    if clamp:
        dd = np.where(dd < 0.0, 0.0, dd)
    ok = dd >= 0.0
    s = np.sqrt(np.where(ok, dd * inv_a, 0.0))
    t = t0 + s if far else t0 - s
    return np.where(ok, np.where(t > 0.0, t, np.where(t <= 0.0, 0.0, np.inf)), np.inf)


def sphere_sweep(o, d, inv_a, rho, cx, cy, cz, r2, old=()):
    """sweep_sphere: (t, start overlap), broadcast over the arguments (o, d: tuples of three arrays)."""
    with np.errstate(all="ignore"):
        ov = pr.sphere_point(o[0], o[1], o[2], cx, cy, cz, r2)[0] <= rho
        R = np.sqrt(np.abs(r2))
        w = (o[0] - cx, o[1] - cy, o[2] - cz)
        L2, h = _dot(*w, *w), _dot(*w, *d)
        ro, ri = R + rho, R - rho
        t_out = np.where(h < 0.0, _root(w, d, h, inv_a, ro, False), np.inf)
        if "outer" in old:
            t_out = np.where(L2 > ro * ro, t_out, np.inf)
        if "inner" in old:
            t_in = np.where((ri > 0.0) & (L2 < ri * ri), _root(w, d, h, inv_a, ri, True), np.inf)
        else:
            t_in = np.where(ri > 0.0, _root(w, d, h, inv_a, ri, True, clamp=True), np.inf)
        t = np.where(L2 < np.abs(r2), t_in, t_out)
        return np.where(ov, 0.0, t), ov


def _vertex(w, d, inv_a, rho, old):
    h = _dot(*w, *d)
    ok = h < 0.0
    if "vertex" in old:
        ok = (_dot(*w, *w) > rho * rho) & ok
    return np.where(ok, _root(w, d, h, inv_a, rho, False), np.inf)


def _edge(w, d, e, rho, old):
    ee = _dot(*e, *e)
    pos = ee > 0.0
    ie = 1.0 / np.where(pos, ee, 1.0)
    we, de = _dot(*w, *e), _dot(*d, *e)
    sw, sd = we * ie, de * ie
    wp = (w[0] - e[0] * sw, w[1] - e[1] * sw, w[2] - e[2] * sw)
    dp = (d[0] - e[0] * sd, d[1] - e[1] * sd, d[2] - e[2] * sd)
    A, h = _dot(*dp, *dp), _dot(*wp, *dp)
    ok = pos & (A > 0.0) & (h < 0.0)
    if "edge" in old:
        ok &= _dot(*wp, *wp) > rho * rho
    t = _root(wp, dp, h, 1.0 / np.where(ok, A, 1.0), rho, False)
    ax = we + de * t
    return np.where(ok & (ax >= 0.0) & (ax <= ee), t, np.inf)


def triangle_sweep(o, d, inv_a, rho, t, old=()):
    """sweep_triangle on records t[..., 12]: (t, start overlap), broadcast over the arguments."""
    a = (t[..., 0], t[..., 1], t[..., 2])
    e1 = (t[..., 3], t[..., 4], t[..., 5])
    e2 = (t[..., 6], t[..., 7], t[..., 8])
    n = (t[..., 9], t[..., 10], t[..., 11])
    with np.errstate(all="ignore"):
        ov = pr.triangle_point(o[0], o[1], o[2], t)[0] <= rho
        w = (o[0] - a[0], o[1] - a[1], o[2] - a[2])
        nn = _dot(*n, *n)
        wn, dn = _dot(*n, *w), _dot(*n, *d)
        num = np.abs(wn) - rho * np.sqrt(nn)
        face = (nn > 0.0) & np.where(wn > 0.0, dn < 0.0, dn > 0.0)
        if "face" in old:
            face &= num > 0.0
        tf = np.where(num <= 0.0, 0.0, num) / np.where(face, np.abs(dn), 1.0)
        p = (w[0] + d[0] * tf, w[1] + d[1] * tf, w[2] + d[2] * tf)
        d1, d2 = _dot(*p, *e1), _dot(*p, *e2)
        ee1, ee2, e12 = _dot(*e1, *e1), _dot(*e2, *e2), _dot(*e1, *e2)
        sn, tn = ee2 * d1 - e12 * d2, ee1 * d2 - e12 * d1
        face &= (sn >= 0.0) & (tn >= 0.0) & (sn + tn <= nn) & (tf < np.inf)
        best = np.where(face, tf, np.inf)
        best = np.fmin(best, _edge(w, d, e1, rho, old))
        best = np.fmin(best, _edge(w, d, e2, rho, old))
        best = np.fmin(best, _vertex(w, d, inv_a, rho, old))
        g = (w[0] - e1[0], w[1] - e1[1], w[2] - e1[2])
        f = (e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2])
        best = np.fmin(best, _edge(g, d, f, rho, old))
        best = np.fmin(best, _vertex(g, d, inv_a, rho, old))
        best = np.fmin(best, _vertex((w[0] - e2[0], w[1] - e2[1], w[2] - e2[2]), d, inv_a, rho, old))
        return np.where(ov, 0.0, best), ov


def _tri_boxes(rec):
    a, b, c = rec.tri[:, 0:3], rec.tri[:, 0:3] + rec.tri[:, 3:6], rec.tri[:, 0:3] + rec.tri[:, 6:9]
    return np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)


def _slab_pairs(q, qi, lo, hi):
    """Which of the pairs (sweep qi[k], box lo[k] .. hi[k]) can touch: a slab test on the box grown by rho and a margin."""
    with np.errstate(all="ignore"):
        o, d = q["origin"][qi], q["direction"][qi]
        rho, tmax = q["radius"][qi], q["tmax"][qi]
        pad = (rho + 1e-9 * (np.abs(o).sum(1) + np.abs(lo).sum(1) + np.abs(hi).sum(1) + rho) + 1e-300)[:, None]
        inv = 1.0 / d
        t1, t2 = ((lo - pad) - o) * inv, ((hi + pad) - o) * inv
        tn = np.fmax(np.fmin(t1, t2).max(1), 0.0)
        tf = np.fmin(np.fmax(t1, t2).min(1), tmax)
        return tn <= tf


_LEVELS = (1024, 64, 8, 1)  # triangles per block, level by level


def _morton_order(lo, hi):
    """The triangles ordered along a 30-bit Morton curve of their box centres: neighbours in space, neighbours in order."""
    c = 0.5 * (lo + hi)
    span = np.maximum(c.max(0) - c.min(0), 1e-300)
    g = np.minimum(((c - c.min(0)) / span * 1024.0).astype(np.int64), 1023)
    code = np.zeros(len(c), dtype=np.int64)
    for bit in range(10):
        for ax in range(3):
            code |= ((g[:, ax] >> bit) & 1) << (3 * bit + ax)
    return np.argsort(code, kind="stable")


def _tri_pairs(rec, q, rows, boxes):
    """(query index, triangle index) pairs the sweeps `rows` can touch: the slab test level by level on blocks of
    Morton-ordered triangles, down to the triangles themselves."""
    order = _morton_order(*boxes)
    lo, hi = boxes[0][order], boxes[1][order]
    nt = rec.nt
    a = np.repeat(rows, (nt + _LEVELS[0] - 1) // _LEVELS[0])
    b = np.tile(np.arange(0, nt, _LEVELS[0]), len(rows))  # a block is named by its first triangle
    for lv, size in enumerate(_LEVELS):
        first = np.arange(0, nt, size)
        blo, bhi = np.minimum.reduceat(lo, first), np.maximum.reduceat(hi, first)
        keep = np.zeros(len(a), dtype=bool)
        for i0 in range(0, len(a), 1 << 20):
            sl = slice(i0, i0 + (1 << 20))
            keep[sl] = _slab_pairs(q, a[sl], blo[b[sl] // size], bhi[b[sl] // size])
        a, b = a[keep], b[keep]
        if size > 1:
            fan = size // _LEVELS[lv + 1]
            a = np.repeat(a, fan)
            b = np.repeat(b, fan) + np.tile(np.arange(fan) * _LEVELS[lv + 1], len(b))
            inside = b < nt
            a, b = a[inside], b[inside]
    return a, order[b]


def pair_times(rec, q, prefilter=True, old=()):
    """Mirror t and start-overlap flag of every (query, primitive) pair that can matter: (qi, cid, t, ov) — all pairs
    of the spheres, the preselected ones of the triangles; skipped queries have none."""
    rows = np.nonzero(~skipped(q))[0]
    parts = []
    d_all = q["direction"]
    with np.errstate(all="ignore"):
        inv_a_all = 1.0 / (d_all[:, 0] * d_all[:, 0] + d_all[:, 1] * d_all[:, 1] + d_all[:, 2] * d_all[:, 2])

    def args(qi):
        o, d = q["origin"][qi], q["direction"][qi]
        return (o[:, 0], o[:, 1], o[:, 2]), (d[:, 0], d[:, 1], d[:, 2]), inv_a_all[qi], q["radius"][qi]

    if rec.ns and len(rows):
        qi, ci = np.repeat(rows, rec.ns), np.tile(np.arange(rec.ns), len(rows))
        g = rec.sph[ci]
        t, ov = sphere_sweep(*args(qi), g[:, 0], g[:, 1], g[:, 2], g[:, 3], old)
        parts.append((qi, ci, t, ov))
    if rec.nm and len(rows):
        qi, ci = np.repeat(rows, rec.nm), np.tile(np.arange(rec.nm), len(rows))
        g, tm = rec.mov[ci], q["time"][qi]
        t, ov = sphere_sweep(*args(qi), g[:, 0] + tm * g[:, 3], g[:, 1] + tm * g[:, 4], g[:, 2] + tm * g[:, 5], g[:, 6],
                             old)
        parts.append((qi, rec.ns + ci, t, ov))
    if rec.nt and len(rows):
        if prefilter:
            qi, ci = _tri_pairs(rec, q, rows, _tri_boxes(rec))
        else:
            qi, ci = np.repeat(rows, rec.nt), np.tile(np.arange(rec.nt), len(rows))
        ts, ovs = [], []
        for i0 in range(0, len(qi), 1 << 18):
            sl = slice(i0, i0 + (1 << 18))
            t, ov = triangle_sweep(*args(qi[sl]), rec.tri[ci[sl]], old)
            ts.append(t), ovs.append(ov)
        if ts:
            parts.append((qi, rec.ns + rec.nm + ci, np.concatenate(ts), np.concatenate(ovs)))
    if not parts:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0), np.zeros(0, dtype=bool)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def answers(rec, mats, q, prefilter=True, old=()):
    """The mirror's answer records (HIT_DTYPE): the minimum by (t, insertion index) over the accepted pairs.  old: the
    guards of the earlier rule to put back (GUARDS)."""
    n = len(q)
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["t"], h["dist"], h["prim"], h["kind"], h["material"] = np.inf, np.inf, -1, -1, -1
    qi, cid, t, ov = pair_times(rec, q, prefilter, old)
    ok = (t <= q["tmax"][qi]) & (t < np.inf)
    qi, cid, t, ov = qi[ok], cid[ok], t[ok], ov[ok]
    ins = rec.cls2ins[cid]
    order = np.lexsort((ins, t, qi))
    qi, cid, t, ov, ins = qi[order], cid[order], t[order], ov[order], ins[order]
    first = np.ones(len(qi), dtype=bool)
    first[1:] = qi[1:] != qi[:-1]
    qi, cid, t, ov, ins = qi[first], cid[first], t[first], ov[first], ins[first]
    d = q["direction"][qi]
    centre = q["origin"][qi] + d * t[:, None]
    h["t"][qi], h["centre"][qi] = t, centre
    h["dist"][qi], h["point"][qi] = pr.prim_point(rec, cid, centre, q["time"][qi])
    h["prim"][qi], h["kind"][qi], h["material"][qi] = ins, rec.kind_of(cid), np.asarray(mats)[ins]
    h["start_overlap"][qi] = ov
    return h


def diff_fields(a, b):
    """The fields in which two HIT_DTYPE arrays differ bitwise: {field: number of records}."""
    out = {}
    for f in HIT_DTYPE.names:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        w = x.dtype.itemsize
        bad = (x.view(f"u{w}") != y.view(f"u{w}")).reshape(len(a), -1).any(1)
        if bad.any():
            out[f] = (int(bad.sum()), np.nonzero(bad)[0][:5].tolist())
    return out


# ------------------------------------------------------------------------------------------------------- exact ---
def _fdot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _fsub(x, y):
    return [x[0] - y[0], x[1] - y[1], x[2] - y[2]]


def _pt_seg_d2(p, a, u):
    """Exact squared distance from point p to the segment a + s u, s in [0, 1]."""
    r = _fsub(p, a)
    uu = _fdot(u, u)
    s = Fr(0) if uu == 0 else min(max(_fdot(r, u) / uu, Fr(0)), Fr(1))
    q = [r[k] - s * u[k] for k in range(3)]
    return _fdot(q, q)


def _seg_seg_d2(p, u, q, v):
    """Exact squared distance between the segments p + s u and q + t v: the minimum of a convex quadratic over the unit
    square is its free minimum when that lies inside, else it lies on the boundary — an endpoint against a segment."""
    p1, q1 = [p[k] + u[k] for k in range(3)], [q[k] + v[k] for k in range(3)]
    best = min(_pt_seg_d2(p, q, v), _pt_seg_d2(p1, q, v), _pt_seg_d2(q, p, u), _pt_seg_d2(q1, p, u))
    uu, vv, uv = _fdot(u, u), _fdot(v, v), _fdot(u, v)
    det = uu * vv - uv * uv
    if det > 0:
        r = _fsub(p, q)
        ur, vr = _fdot(u, r), _fdot(v, r)
        s, t = (uv * vr - vv * ur) / det, (uu * vr - uv * ur) / det
        if 0 <= s <= 1 and 0 <= t <= 1:
            w = [r[k] + s * u[k] - t * v[k] for k in range(3)]
            best = min(best, _fdot(w, w))
    return best


def exact_seg_triangle_d2(p0, p1, t):
    """Exact squared distance from the segment [p0, p1] (Fractions) to the triangle of record t (a, e1, e2)."""
    a, e1, e2 = [_F(v) for v in t[0:3]], [_F(v) for v in t[3:6]], [_F(v) for v in t[6:9]]
    u = _fsub(p1, p0)
    n = [e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0], e1[0] * e2[1] - e2[0] * e1[1]]
    nn = _fdot(n, n)
    if nn != 0:
        s0, s1 = _fdot(n, _fsub(p0, a)), _fdot(n, _fsub(p1, a))
        if s0 != s1 and s0 * s1 <= 0:  # the segment crosses the plane: inside the triangle?
            lam = s0 / (s0 - s1)
            w = [p0[k] + lam * u[k] - a[k] for k in range(3)]
            d1, d2, ee1, ee2, e12 = _fdot(w, e1), _fdot(w, e2), _fdot(e1, e1), _fdot(e2, e2), _fdot(e1, e2)
            sn, tn = ee2 * d1 - e12 * d2, ee1 * d2 - e12 * d1
            if sn >= 0 and tn >= 0 and sn + tn <= nn:
                return Fr(0)
    b = [a[k] + e1[k] for k in range(3)]
    best = min(_seg_seg_d2(p0, u, a, e1), _seg_seg_d2(p0, u, a, e2), _seg_seg_d2(p0, u, b, _fsub(e2, e1)))
    f0, f1 = [float(v) for v in p0], [float(v) for v in p1]
    if all(_F(x) == y for x, y in zip(f0, p0)):
        best = min(best, pr.exact_triangle_d2(f0, t))
    else:
        best = min(best, _exact_triangle_d2_fr(p0, a, e1, e2, n, nn))
    if all(_F(x) == y for x, y in zip(f1, p1)):
        best = min(best, pr.exact_triangle_d2(f1, t))
    else:
        best = min(best, _exact_triangle_d2_fr(p1, a, e1, e2, n, nn))
    return best


def _exact_triangle_d2_fr(P, a, e1, e2, n, nn):
    """point_ref.exact_triangle_d2 for a point given in Fractions (the exact end p(tmax) of a miss)."""
    b = [a[k] + e1[k] for k in range(3)]
    best = min(_pt_seg_d2(P, a, e1), _pt_seg_d2(P, a, e2), _pt_seg_d2(P, b, _fsub(e2, e1)))
    if nn != 0:
        w = _fsub(P, a)
        d1, d2, ee1, ee2, e12 = _fdot(w, e1), _fdot(w, e2), _fdot(e1, e1), _fdot(e2, e2), _fdot(e1, e2)
        s, tt = (ee2 * d1 - e12 * d2) / nn, (ee1 * d2 - e12 * d1) / nn
        if s >= 0 and tt >= 0 and s + tt <= 1:
            wn = _fdot(w, n)
            best = min(best, wn * wn / nn)
    return best


def exact_segdist(rec, cid, p0, p1, time):
    """Exact distance from the segment [p0, p1] (Fractions) to class-major primitive cid: (value, its error bound)."""
    k = int(rec.kind_of(cid))
    if k == TRIANGLE:
        return _sqrt_fr(exact_seg_triangle_d2(p0, p1, rec.tri[cid - rec.ns - rec.nm]))
    _, _, (c, R) = pr.exact_geometry(rec, cid, time)
    m2 = _pt_seg_d2(c, p0, _fsub(p1, p0))
    M2 = max(_fdot(_fsub(p0, c), _fsub(p0, c)), _fdot(_fsub(p1, c), _fsub(p1, c)))
    if m2 <= R * R <= M2:
        return Fr(0), Fr(0)
    (m, e0), (M, e1) = _sqrt_fr(m2), _sqrt_fr(M2)
    return (abs(m - R), e0) if abs(m - R) <= abs(M - R) else (abs(M - R), e1)


# ------------------------------------------------------------------------------- the binary64 filter of (b) ---
def _pt_seg_f(p, a, u):
    r = p - a
    uu = (u * u).sum(1)
    s = np.clip((r * u).sum(1) / np.where(uu > 0, uu, 1.0), 0.0, 1.0)
    w = r - s[:, None] * u
    return (w * w).sum(1)


def _seg_seg_f(p, u, q, v):
    """Squared distance between segment pairs in binary64 and a flag `near parallel` (the free minimum is then not
    trusted: such pairs go to the exact path)."""
    best = np.minimum(np.minimum(_pt_seg_f(p, q, v), _pt_seg_f(p + u, q, v)), np.minimum(_pt_seg_f(q, p, u), _pt_seg_f(q + v, p, u)))
    uu, vv, uv = (u * u).sum(1), (v * v).sum(1), (u * v).sum(1)
    det = uu * vv - uv * uv
    par = det <= 1e-6 * uu * vv
    r = p - q
    ur, vr = (u * r).sum(1), (v * r).sum(1)
    sd = np.where(par, 1.0, det)
    s, t = (uv * vr - vv * ur) / sd, (uu * vr - uv * ur) / sd
    inside = ~par & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    w = r + s[:, None] * u - t[:, None] * v
    return np.where(inside, np.minimum(best, (w * w).sum(1)), best), par & (uu > 0) & (vv > 0)


def segdist_f64(rec, cid, p0, p1, time):
    """The segment distance of (b) in binary64 for pairs (class-major cid[k], segment p0[k] .. p1[k], time[k]):
    (distance, doubtful).  The same construction as the exact path in floating point; every term is a difference or a
    projection of quantities of magnitude <= S, so its error is a small multiple of u S except where the free minimum of
    two nearly parallel segments is ill-determined — those pairs are flagged doubtful and go to the exact path.  The
    checker sends every pair within FILTER_U u S (+ the band) of rho to the exact path as well; test_sweep_host.py
    checks the filter against the exact distance on every pair that went there and on a sample of those that did not."""
    n = len(cid)
    out, doubt = np.full(n, np.inf), np.zeros(n, dtype=bool)
    k = rec.kind_of(cid)
    with np.errstate(all="ignore"):
        for kind in (SPHERE, MOVING):
            m = k == kind
            if not m.any():
                continue
            if kind == SPHERE:
                g = rec.sph[cid[m]]
                c, R = g[:, 0:3], np.sqrt(np.abs(g[:, 3]))
            else:
                g = rec.mov[cid[m] - rec.ns]
                c, R = g[:, 0:3] + time[m, None] * g[:, 3:6], np.sqrt(np.abs(g[:, 6]))
            mm = np.sqrt(_pt_seg_f(c, p0[m], p1[m] - p0[m]))
            MM = np.sqrt(np.maximum(((p0[m] - c) ** 2).sum(1), ((p1[m] - c) ** 2).sum(1)))
            out[m] = np.where((mm <= R) & (R <= MM), 0.0, np.minimum(np.abs(mm - R), np.abs(MM - R)))
        m = k == TRIANGLE
        if m.any():
            t = rec.tri[cid[m] - rec.ns - rec.nm]
            a, e1, e2, nrm = t[:, 0:3], t[:, 3:6], t[:, 6:9], t[:, 9:12]
            q0, q1 = p0[m], p1[m]
            u = q1 - q0
            d2, par = _seg_seg_f(q0, u, a, e1)
            for qq, vv in ((a, e2), (a + e1, e2 - e1)):
                x, pp = _seg_seg_f(q0, u, qq, vv)
                d2, par = np.minimum(d2, x), par | pp
            dd = np.sqrt(d2)
            dd = np.minimum(dd, pr.triangle_point(q0[:, 0], q0[:, 1], q0[:, 2], t)[0])
            dd = np.minimum(dd, pr.triangle_point(q1[:, 0], q1[:, 1], q1[:, 2], t)[0])
            s0, s1 = (nrm * (q0 - a)).sum(1), (nrm * (q1 - a)).sum(1)
            cross = (s0 * s1 <= 0) & (s0 != s1)
            lam = s0 / np.where(cross, s0 - s1, 1.0)
            w = q0 + lam[:, None] * u - a
            d1_, d2_ = (w * e1).sum(1), (w * e2).sum(1)
            ee1, ee2, e12, nn = (e1 * e1).sum(1), (e2 * e2).sum(1), (e1 * e2).sum(1), (nrm * nrm).sum(1)
            sn, tn = ee2 * d1_ - e12 * d2_, ee1 * d2_ - e12 * d1_
            tol = 1e-6 * nn
            pierce = cross & (sn >= -tol) & (tn >= -tol) & (sn + tn <= nn + tol)
            sure = cross & (sn >= tol) & (tn >= tol) & (sn + tn <= nn - tol)
            out[m] = np.where(sure, 0.0, dd)
            doubt[m] = par | (pierce & ~sure)
    return out, doubt


# ----------------------------------------------------------------------------------------------------- checker ---
def _fr3(v):
    return [_F(x) for x in v]


class Checker:
    """check_answers for one batch of sweeps, reusable for many answers to it: the exact quantities are memoised per
    (query, primitive, end of the segment).  A miss with tmax = +inf is checked over [o, p(T)], T from `horizon`."""

    def __init__(self, rec, mats, q):
        self.rec, self.mats, self.q = rec, np.asarray(mats), q
        self.skip = skipped(q)
        self._seg, self._memo = {}, {}
        self.boxes = _tri_boxes(rec) if rec.nt else None
        self.filter_worst = 0.0  # |filter - exact| over the pairs that went to the exact path, in units of u S
        self.exact_pairs = 0

    # ---- scales and bands
    def scale(self, i, t, c):
        """S of the band for query i at parameter t and primitive c, as a Fraction."""
        q = self.q[i]
        tt = _F(t)
        S = sum(abs(_F(x)) for x in q["origin"]) + sum(abs(tt * _F(x)) for x in q["direction"]) + _F(q["radius"])
        return S + pr.exact_geometry(self.rec, c, float(q["time"]))[1]

    def seg(self, i, c, end_key, p1):
        """Exact distance from [o, p1] to primitive c for query i (memoised on the end's key)."""
        key = (i, c, end_key)
        if key not in self._seg:
            q = self.q[i]
            self._seg[key] = exact_segdist(self.rec, c, _fr3(q["origin"]), p1, float(q["time"]))
            self.exact_pairs += 1
        return self._seg[key]

    # ---- an unbounded miss: where the sweep has left the scene for good
    def scene_bounds(self, time):
        """(lo, hi, largest primitive magnitude) as Fractions: a box that CONTAINS every primitive at `time`.  The corners
        are formed in binary64 and moved outwards by 8 u x the magnitudes of their terms (a vertex a + e, a sphere's
        c +- R and a moving centre c0 + time dc +- R carry at most three roundings of terms of that magnitude)."""
        rec = self.rec
        los, his, mags = [], [], []
        if rec.nt:
            t = rec.tri
            v = np.stack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]])
            slack = 8 * U * (np.abs(t[:, 0:3]) + np.abs(t[:, 3:6]) + np.abs(t[:, 6:9]))
            los.append((v.min(0) - slack).min(0)), his.append((v.max(0) + slack).max(0))
            mags.append(np.abs(t[:, 0:9]).sum(1).max())
        for g, c, R, m in ((rec.sph, rec.sph[:, 0:3], np.sqrt(np.abs(rec.sph[:, 3])), np.abs(rec.sph[:, 0:3])),
                           (rec.mov, rec.mov[:, 0:3] + time * rec.mov[:, 3:6], np.sqrt(np.abs(rec.mov[:, 6])),
                            np.abs(rec.mov[:, 0:3]) + np.abs(time * rec.mov[:, 3:6]))):
            if len(g):
                slack = 8 * U * (m + R[:, None])
                los.append(((c - R[:, None]) - slack).min(0)), his.append(((c + R[:, None]) + slack).max(0))
                mags.append((m.sum(1) + R).max())
        lo, hi = np.min(los, axis=0), np.max(his, axis=0)
        return _fr3(lo), _fr3(hi), _F(1.0001 * max(mags))

    def horizon(self, i, prec):
        """For a sweep with tmax = +inf: (T, axis).  T is the smallest power of two such that p(T) lies beyond the box
        of all primitives grown by rho + band(T) on `axis`, along which the sweep moves away from the box — shown here
        in exact arithmetic.  From T on the centre is farther than rho + band from that face of the box and receding,
        so nothing is touched after T: the unbounded miss is the miss over [o, p(T)], with the band of t = T."""
        q = self.q[i]
        o, d, rho = _fr3(q["origin"]), _fr3(q["direction"]), _F(q["radius"])
        lo, hi, mag = self.scene_bounds(float(q["time"]))
        k = max(range(3), key=lambda j: abs(d[j]))  # |d_k| >= |d|_1 / 3: the band's growth K u T |d|_1 cannot keep up
        l1o, l1d, ku = sum(abs(x) for x in o), sum(abs(x) for x in d), K[prec] * _F(U)
        gap = (hi[k] - o[k]) if d[k] > 0 else (o[k] - lo[k])  # how far the face it leaves through is ahead (may be < 0)
        est = float(max(gap + rho, 0) / abs(d[k]))
        T = Fr(2) ** (math.frexp(est)[1] - 2 if est > 0.0 else -1074)
        while not T * abs(d[k]) > gap + rho + ku * (l1o + T * l1d + rho + mag):
            T *= 2
        beyond = o[k] + T * d[k]  # the claim, once more, on the coordinate itself
        band = ku * (l1o + T * l1d + rho + mag)
        assert (beyond > hi[k] + rho + band) if d[k] > 0 else (beyond < lo[k] - rho - band)
        assert float(T) < math.inf and math.frexp(float(T))[0] == 0.5
        return T, k

    # ---- the clause over every primitive: nothing within rho - band of the segment [o, end]
    def _clear(self, i, t, end_f, end_fr, end_key, prec, skip_c=-1):
        """Asserts segdist_exact(o, end, c) >= rho - band(c) for every c; returns whether some primitive other than
        skip_c is within its band of rho (the query is open)."""
        rec, q = self.rec, self.q[i]
        rho = float(q["radius"])
        one = self.q[i:i + 1].copy()
        one["tmax"] = t
        cands = [np.arange(rec.ns + rec.nm)]
        if rec.nt:
            cands.append(rec.ns + rec.nm + _tri_pairs(rec, one, np.zeros(1, dtype=np.int64), self.boxes)[1])
        cid = np.concatenate(cands).astype(np.int64)
        n = len(cid)
        o = np.repeat(q["origin"][None], n, 0)
        fd, doubt = segdist_f64(rec, cid, o, np.repeat(np.asarray(end_f, dtype=np.float64)[None], n, 0),
                                np.full(n, float(q["time"])))
        S_hi = float(self.scale(i, t, int(cid[0]))) if n else 0.0
        # (one scale for the preselection: the largest primitive magnitudes matter only through a generous margin)
        mag = np.abs(q["origin"]).sum() + abs(t) * np.abs(q["direction"]).sum() + rho
        margin = (FILTER_U + 2 * K[prec]) * U * (mag + self._prim_mag(cid, float(q["time"])))
        near = doubt | (np.abs(fd - rho) <= margin)
        assert not np.any(~near & (fd < rho)) or self._confirm_below(i, cid[~near & (fd < rho)], end_key, end_fr, t, prec), \
            "unreachable"
        opened = False
        for c in cid[near]:
            c = int(c)
            D, e = self.seg(i, c, end_key, end_fr)
            band = K[prec] * _F(U) * self.scale(i, t, c)
            assert D + e >= _F(rho) - band, ("a primitive is within rho - band of the travelled segment", c, float(D), rho,
                                              float(band))
            if c != skip_c and abs(D - _F(rho)) <= band + e:
                # a graze on the way leaves the answer open; a primitive that is at rho from the END of a hit's segment
                # as well (a shared edge or vertex, a coincident copy) ties with the reported one at the same t
                tie = False
                if skip_c >= 0:
                    De, ee = pr.exact_dist(rec, c, np.asarray(end_f, dtype=np.float64), float(q["time"]))
                    tie = abs(De - _F(rho)) <= band + ee
                opened = opened or not tie
            j = int(np.nonzero(cid == c)[0][0])
            if not doubt[j]:
                self.filter_worst = max(self.filter_worst, abs(float(D) - fd[j]) / (U * float(self.scale(i, t, c))))
        return opened

    def _confirm_below(self, i, cids, end_key, end_fr, t, prec):
        """Primitives the filter puts well below rho: the exact distance decides (and fails the check)."""
        for c in cids:
            c = int(c)
            D, e = self.seg(i, c, end_key, end_fr)
            band = K[prec] * _F(U) * self.scale(i, t, c)
            assert D + e >= _F(float(self.q[i]["radius"])) - band, \
                ("a primitive is within rho - band of the travelled segment", c, float(D), float(self.q[i]["radius"]))
        return True

    def _prim_mag(self, cid, time):
        rec = self.rec
        out = np.zeros(len(cid))
        k = rec.kind_of(cid)
        m = k == SPHERE
        out[m] = np.abs(rec.sph[cid[m], 0:3]).sum(1) + np.sqrt(np.abs(rec.sph[cid[m], 3]))
        m = k == MOVING
        g = rec.mov[cid[m] - rec.ns]
        out[m] = np.abs(g[:, 0:3]).sum(1) + np.abs(time * g[:, 3:6]).sum(1) + np.sqrt(np.abs(g[:, 6]))
        m = k == TRIANGLE
        out[m] = np.abs(rec.tri[cid[m] - rec.ns - rec.nm, 0:9]).sum(1)
        return out

    # ---- one answer
    def _check_one(self, i, h, prec):
        """(contact residual, surface, consistency) in units of their bands, open."""
        rec, q = self.rec, self.q[i]
        t, dist, prim = float(h["t"]), float(h["dist"]), int(h["prim"])
        centre, point = np.array(h["centre"], dtype=np.float64), np.array(h["point"], dtype=np.float64)
        assert not (math.isnan(t) or math.isnan(dist) or np.isnan(centre).any() or np.isnan(point).any()), "NaN in the answer"
        rho, tmax = float(q["radius"]), float(q["tmax"])
        if prim == -1:  # ---- a miss
            assert (t == math.inf and dist == math.inf and np.all(centre == 0.0) and np.all(point == 0.0)
                    and int(h["kind"]) == -1 and int(h["material"]) == -1 and int(h["start_overlap"]) == 0), "not the miss record"
            if self.skip[i]:
                return 0.0, 0.0, 0.0, 0
            o, d = _fr3(q["origin"]), _fr3(q["direction"])
            if tmax == math.inf:
                tmax = float(self.horizon(i, prec)[0])
            end = [o[k] + _F(tmax) * d[k] for k in range(3)]
            opened = self._clear(i, tmax, [float(x) for x in end], end, ("tmax", prec), prec)
            return 0.0, 0.0, 0.0, int(opened)
        # ---- a hit
        assert not self.skip[i], "a hit on a skipped query"
        assert 0 <= prim < rec.n, ("prim out of range", prim)
        c = int(rec.ins2cls[prim])
        assert int(h["kind"]) == int(rec.kind_of(c)), "kind is not the primitive's"
        assert int(h["material"]) == int(self.mats[prim]), "material is not the primitive's"
        assert 0.0 <= t <= tmax, ("t outside [0, tmax]", t, tmax)
        ov = int(h["start_overlap"])
        assert ov in (0, 1) and (ov == 0 or t == 0.0), ("start_overlap without t == 0", ov, t)
        tau, u = _F(pr.TAU[prec]), _F(U)
        for k in range(3):  # centre = o + d t, two roundings
            ex = _F(q["origin"][k]) + _F(t) * _F(q["direction"][k])
            assert abs(_F(centre[k]) - ex) <= 4 * u * (abs(_F(q["origin"][k])) + abs(_F(t) * _F(q["direction"][k]))), \
                ("centre is not origin + direction t", k)
        band = K[prec] * u * self.scale(i, t, c)
        D, err = pr.exact_dist(rec, c, centre, float(q["time"]))
        if ov:
            assert D - err <= _F(rho) + band, ("start overlap, but the primitive is beyond rho + band at o", c, float(D), rho)
            e_contact = max(0.0, float((D - _F(rho)) / band)) if band else 0.0
        else:
            assert abs(D - _F(rho)) - err <= band, ("the centre is not at rho from the primitive", c, float(D), rho, float(band))
            e_contact = float(abs(D - _F(rho)) / band) if band else 0.0
        # dist and point: point_ref's two clauses at the centre
        geom = pr.exact_geometry(rec, c, float(q["time"]))
        Sq = geom[1]
        s_err, s_e = pr.surface_error(geom, point)
        assert s_err - s_e <= tau * Sq, ("point off the surface", c, float(s_err), float(tau * Sq))
        L, l_e = _sqrt_fr(sum((_F(centre[k]) - _F(point[k])) ** 2 for k in range(3)))
        S = pr.header_scale(geom, centre)
        assert abs(L - _F(dist)) - l_e <= tau * (S + Sq), ("|centre - point| differs from dist", c, float(L), dist)
        lo, hi = pr.bound(rec, c, centre, float(q["time"]), prec)
        assert pr.within(dist, D, err, lo, hi), ("dist outside point_ref's band", c, dist, float(D))
        e_surf = pr._units(s_err, tau * Sq)
        e_cons = pr._units(abs(L - _F(dist)), tau * (S + Sq))
        opened = False
        if t > 0.0:  # nothing was passed through on the way
            opened = self._clear(i, t, centre, _fr3(centre), ("hit", h["centre"].tobytes()), prec, skip_c=c)
        return e_contact, e_surf, e_cons, int(opened)

    def check(self, hits, prec, what=""):
        n = len(self.q)
        assert len(hits) == n, (what, len(hits), n)
        out = dict(queries=n, hits=int((hits["prim"] >= 0).sum()), worst_contact=0.0, worst_surface=0.0,
                   worst_consistency=0.0, open=0)
        for i in range(n):
            h = hits[i]
            key = (i, prec, h.tobytes())
            if key not in self._memo:
                try:
                    self._memo[key] = self._check_one(i, h, prec)
                except AssertionError as e:
                    raise AssertionError(f"{what} sweep {i} {self.q[i]} -> {h}: {e}") from None
            r = self._memo[key]
            out["worst_contact"] = max(out["worst_contact"], r[0])
            out["worst_surface"] = max(out["worst_surface"], r[1])
            out["worst_consistency"] = max(out["worst_consistency"], r[2])
            out["open"] += r[3]
        out["exact_pairs"], out["filter_worst"] = self.exact_pairs, self.filter_worst
        return out


def check_answers(rec, mats, q, hits, prec, what=""):
    """Assert the whole contract of include/rtow.h on `hits` (the answers to the sweeps q) with the band of
    `prec`, query by query, and return the statistics (see the module docstring)."""
    return Checker(rec, mats, q).check(hits, prec, what)


def stats_line(s):
    return (f"{s['queries']} sweeps, {s['hits']} hits, {s['exact_pairs']} exact pairs, worst contact {s['worst_contact']:.3f}, "
            f"on-surface {s['worst_surface']:.3f}, consistency {s['worst_consistency']:.3f} of their bands, open {s['open']}, "
            f"filter within {s['filter_worst']:.1f} u S of the exact distance")
