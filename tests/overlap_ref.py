"""Reference for the box-overlap query (rtow_overlap, include/rtow.h): a numpy mirror of the kernel's predicate
(csrc/rtow_overlap_walks.h) in its written operation order — the strict reference, bit for bit — and an independent
exact reference in Fraction with the band of the contract.  numpy and point_ref only: importing this loads no library.

The band.  For a pair (box, primitive) and a separating axis L, s_L is the exact signed gap and E_L the sum of the
magnitudes of the monomials of s_L expanded in the inputs as given (the record's fields, lo, hi, time); of a min or a max
E takes the branch the exact values select, the larger sum on an exact tie (the two vertices of an edge project alike
across it).  A pair is decided NO when some axis has s_L > K u E_L, YES when every axis with L != 0 has s_L < -K u E_L,
u = 2^-53; anything else is undecided.  A triangle has 13 axes on the exact vertices a, a + e1, a + e2 with the exact
cross product; a sphere the two gaps dmin^2 - R^2 and R^2 - dmax^2.

K.  No monomial of a computed gap passes more than 9 roundings: the moving sphere's centre c0 + time dc has 2, the
difference from lo or hi 1, the square doubles that and adds 1, the two sums add 2 (a fixed sphere: 5); the normal axis
has 2 in the stored n, 1 in each product and 2 in the sums (5); a cross axis 1 in v1 or v2, 1 in f = e2 - e1, the
product and the difference (4); a box normal 1.  (1 + u)^9 - 1 < 9.000001 u, so K_strict = 10 leaves a whole unit for
the terms of second order (a clamp that the rounded values open by a few u contributes its square), and
K_fast = 2 K_strict = 20: contraction only removes roundings.

per pair the references give r = max over the axes with L != 0 of s_L / (u E_L): NO iff r > K, YES iff r < -K.
"""
import math
from fractions import Fraction as Fr

import numpy as np

import point_ref as pr

U = 2.0 ** -53
K = {"strict": 10, "fast": 20}
MAX_IDS = 8
BOX_DTYPE = np.dtype([("lo", "<f8", (3,)), ("hi", "<f8", (3,)), ("time", "<f8"), ("min_prim", "<i4"), ("pad_", "<i4")])
FAR = 1e-9  # the float filter: a gap beyond FAR x E is decided without Fraction (float error is below 20 u E)


def make_boxes(lo, hi, time=0.0, min_prim=0):
    l = np.asarray(lo, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(len(l), dtype=BOX_DTYPE)
    q["lo"], q["hi"], q["time"], q["min_prim"] = l, np.asarray(hi, dtype=np.float64).reshape(-1, 3), time, min_prim
    return q


def skipped(q):
    """Queries that are answered count 0, ids -1 without a walk."""
    v = np.concatenate([q["lo"], q["hi"], q["time"][:, None]], axis=1)
    return ~np.all(np.isfinite(v), axis=1) | np.any(q["lo"] > q["hi"], axis=1)


# ------------------------------------------------------------------------------------------------------ mirror ---
def _tri_fields(t):
    return t[..., 0:3], t[..., 3:6], t[..., 6:9], t[..., 9:12]


def tri_bounds(rec):
    """min / max of a, a + e1, a + e2 per component: the predicate's box-normal axes."""
    a, e1, e2, _ = _tri_fields(rec.tri)
    v1, v2 = a + e1, a + e2
    return np.fmin(np.fmin(a, v1), v2), np.fmax(np.fmax(a, v1), v2)


def mirror_triangle_gaps(lo, hi, t):
    """[m, 13] gaps of m pairs in the kernel's operation order: > 0 separates (the kernel compares the two sides; the
    difference here adds one rounding to a gap, never a sign)."""
    a, e1, e2, n = _tri_fields(t)
    v1, v2 = a + e1, a + e2
    f = e2 - e1
    out = []
    for c in range(3):
        out.append(np.fmax(np.fmin(np.fmin(a[:, c], v1[:, c]), v2[:, c]) - hi[:, c],
                           lo[:, c] - np.fmax(np.fmax(a[:, c], v1[:, c]), v2[:, c])))
    d = (n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]
    x0, x1, y0, y1, z0, z1 = n[:, 0] * lo[:, 0], n[:, 0] * hi[:, 0], n[:, 1] * lo[:, 1], n[:, 1] * hi[:, 1], n[:, 2] * lo[:, 2], n[:, 2] * hi[:, 2]
    bmax = (np.fmax(x0, x1) + np.fmax(y0, y1)) + np.fmax(z0, z1)
    bmin = (np.fmin(x0, x1) + np.fmin(y0, y1)) + np.fmin(z0, z1)
    out.append(np.fmax(d - bmax, bmin - d))

    def sep(p, q, gp, P, gm, M):
        a0, a1, b0, b1 = gp * lo[:, P], gp * hi[:, P], gm * lo[:, M], gm * hi[:, M]
        bmax, bmin = np.fmax(a0, a1) - np.fmin(b0, b1), np.fmin(a0, a1) - np.fmax(b0, b1)
        return np.fmax(np.fmin(p, q) - bmax, bmin - np.fmax(p, q))

    X, Y, Z = 0, 1, 2
    for g, u, w in ((e1, a, v2), (e2, a, v1), (f, a, v1)):
        out.append(sep(u[:, Z] * g[:, Y] - u[:, Y] * g[:, Z], w[:, Z] * g[:, Y] - w[:, Y] * g[:, Z], g[:, Y], Z, g[:, Z], Y))
        out.append(sep(u[:, X] * g[:, Z] - u[:, Z] * g[:, X], w[:, X] * g[:, Z] - w[:, Z] * g[:, X], g[:, Z], X, g[:, X], Z))
        out.append(sep(u[:, Y] * g[:, X] - u[:, X] * g[:, Y], w[:, Y] * g[:, X] - w[:, X] * g[:, Y], g[:, X], Y, g[:, Y], X))
    return np.stack(out, axis=1)


def mirror_sphere_gaps(lo, hi, s, r2):
    """[m, 2]: dmin^2 - |r2|, |r2| - dmax^2 in the kernel's order."""
    near = np.fmax(np.fmax(lo - s, s - hi), 0.0)
    far = np.fmax(s - lo, hi - s)
    dmin2 = (near[:, 0] * near[:, 0] + near[:, 1] * near[:, 1]) + near[:, 2] * near[:, 2]
    dmax2 = (far[:, 0] * far[:, 0] + far[:, 1] * far[:, 1]) + far[:, 2] * far[:, 2]
    R2 = np.abs(r2)
    return np.stack([dmin2 - R2, R2 - dmax2], axis=1)


def _centres(rec, cid, time):
    """Centres and r2 of the sphere-class ids `cid` (class-major) at the times `time`, in the kernel's order."""
    cid = np.asarray(cid)
    s, r2 = np.empty((len(cid), 3)), np.empty(len(cid))
    fx = cid < rec.ns
    s[fx], r2[fx] = rec.sph[cid[fx], 0:3], rec.sph[cid[fx], 3]
    m = rec.mov[cid[~fx] - rec.ns]
    s[~fx], r2[~fx] = m[:, 0:3] + time[~fx, None] * m[:, 3:6], m[:, 6]
    return s, r2


def _tri_candidates(q, live, vlo, vhi, margin=None, chunk=None):
    """(query, triangle) pairs the box-normal axes do not separate — exactly (the mirror), or by `margin` = (scale per
    triangle component, FAR) loosely."""
    qi_all, ti_all = [], []
    idx = np.nonzero(live)[0]
    nt = len(vlo)
    step = max(1, (chunk or (1 << 22)) // max(nt, 1))
    for s in range(0, len(idx), step):
        sel = idx[s:s + step]
        lo, hi = q["lo"][sel][:, None, :], q["hi"][sel][:, None, :]
        if margin is None:
            keep = np.all((vlo[None] <= hi) & (vhi[None] >= lo), axis=2)
        else:
            slack = FAR * (margin[None] + np.maximum(np.abs(lo), np.abs(hi)))
            keep = np.all((vlo[None] - hi <= slack) & (lo - vhi[None] <= slack), axis=2)
        a, b = np.nonzero(keep)
        qi_all.append(sel[a]), ti_all.append(b)
    if not qi_all:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(qi_all), np.concatenate(ti_all)


def pairs(rec, q):
    """The mirror: (query index, class-major id) of every overlapping pair of the live queries (min_prim not applied),
    sorted by query."""
    live = ~skipped(q)
    idx = np.nonzero(live)[0]
    qi, ci = [], []
    nsp = rec.ns + rec.nm
    if nsp and len(idx):
        a = np.repeat(idx, nsp)
        c = np.tile(np.arange(nsp), len(idx))
        s, r2 = _centres(rec, c, q["time"][a])
        g = mirror_sphere_gaps(q["lo"][a], q["hi"][a], s, r2)
        ok = np.all(g <= 0.0, axis=1)
        qi.append(a[ok]), ci.append(c[ok])
    if rec.nt and len(idx):
        vlo, vhi = tri_bounds(rec)
        a, t = _tri_candidates(q, live, vlo, vhi)
        g = mirror_triangle_gaps(q["lo"][a], q["hi"][a], rec.tri[t])
        ok = np.all(g <= 0.0, axis=1)
        qi.append(a[ok]), ci.append(t[ok] + nsp)
    if not qi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    qi, ci = np.concatenate(qi), np.concatenate(ci)
    order = np.lexsort((ci, qi))
    return qi[order], ci[order]


def full_sets(rec, q):
    """Per query the ascending insertion indices of its whole set (min_prim applied): a list of int64 arrays."""
    qi, ci = pairs(rec, q)
    ins = rec.cls2ins[ci]
    keep = ins >= np.maximum(q["min_prim"][qi], 0)
    qi, ins = qi[keep], ins[keep]
    order = np.lexsort((ins, qi))
    qi, ins = qi[order], ins[order]
    cut = np.searchsorted(qi, np.arange(len(q) + 1))
    return [ins[cut[i]:cut[i + 1]] for i in range(len(q))]


def answers(rec, q, max_ids=MAX_IDS, sets=None):
    """(counts int32 [n], ids int32 [n, max_ids]) the strict build must return."""
    sets = full_sets(rec, q) if sets is None else sets
    counts = np.array([len(s) for s in sets], dtype=np.int32)
    ids = np.full((len(q), max_ids), -1, dtype=np.int32)
    for i, s in enumerate(sets):
        ids[i, :min(len(s), max_ids)] = s[:max_ids]
    return counts, ids


def paged(rec, q, max_ids):
    """What a caller gets by paging with min_prim through `answers`: a list of arrays, one per query."""
    q = q.copy()
    out = [[] for _ in range(len(q))]
    todo = np.arange(len(q))
    while len(todo):
        counts, ids = answers(rec, q[todo], max_ids)
        for row, i in enumerate(todo):
            out[i].append(ids[row, :min(int(counts[row]), max_ids)])
        more = counts > max_ids
        todo = todo[more]
        q["min_prim"][todo] = ids[more, max_ids - 1] + 1
    return [np.concatenate(p).astype(np.int64) for p in out]


# ------------------------------------------------------------------------------------- the exact reference ---
# One body for both number types: numpy float arrays (the filter; E is then the LARGER of a min's or max's branches,
# which only sends more pairs on to Fraction) and Fraction scalars (the decision; E follows the selected branch).
class _Float:
    exact = False
    zero = 0.0

    @staticmethod
    def pick(v1, e1, v2, e2, greater):
        return (np.maximum(v1, v2) if greater else np.minimum(v1, v2)), np.maximum(e1, e2)

    @staticmethod
    def is_zero(x):
        return x == 0.0


class _Exact:
    exact = True
    zero = Fr(0)

    @staticmethod
    def pick(v1, e1, v2, e2, greater):
        if v1 == v2:
            return v1, max(e1, e2)
        return (v1, e1) if (v1 > v2) == greater else (v2, e2)

    @staticmethod
    def is_zero(x):
        return x == 0


def _axis_gap(N, L, Labs, verts, lo, hi):
    """(s_L, E_L, L == 0) for the axis L (three components with the magnitude sums Labs of their monomials); verts:
    three (offset d, with a the vertex is a + d) as (a, d) component lists."""
    a, ds = verts
    ps = []
    for d in ds:
        p = sum((L[c] * (a[c] + d[c]) for c in range(3)), N.zero)
        e = sum((Labs[c] * (abs(a[c]) + abs(d[c])) for c in range(3)), N.zero)
        ps.append((p, e))
    tmin = ps[0]
    tmax = ps[0]
    for p in ps[1:]:
        tmin = N.pick(*tmin, *p, False)
        tmax = N.pick(*tmax, *p, True)
    bmax, bmin = (N.zero, N.zero), (N.zero, N.zero)
    for c in range(3):
        t0, t1 = (L[c] * lo[c], Labs[c] * abs(lo[c])), (L[c] * hi[c], Labs[c] * abs(hi[c]))
        g, l = N.pick(*t0, *t1, True), N.pick(*t0, *t1, False)
        bmax, bmin = (bmax[0] + g[0], bmax[1] + g[1]), (bmin[0] + l[0], bmin[1] + l[1])
    s, e = N.pick(tmin[0] - bmax[0], tmin[1] + bmax[1], bmin[0] - tmax[0], bmin[1] + tmax[1], True)
    zero = N.is_zero(L[0]) & N.is_zero(L[1]) & N.is_zero(L[2])
    return s, e, zero


def _triangle_axes(N, a, e1, e2):
    """The 13 axes as (L, Labs)."""
    one, z = N.zero + 1, N.zero
    axes = [([one, z, z], [one, z, z]), ([z, one, z], [z, one, z]), ([z, z, one], [z, z, one])]
    n, nabs = [], []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        n.append(e1[i] * e2[j] - e1[j] * e2[i])
        nabs.append(abs(e1[i] * e2[j]) + abs(e1[j] * e2[i]))
    axes.append((n, nabs))
    f = [e2[c] - e1[c] for c in range(3)]
    for g, gabs in ((e1, [abs(x) for x in e1]), (e2, [abs(x) for x in e2]), (f, [abs(e2[c]) + abs(e1[c]) for c in range(3)])):
        axes.append(([z, -g[2], g[1]], [z, gabs[2], gabs[1]]))
        axes.append(([g[2], z, -g[0]], [gabs[2], z, gabs[0]]))
        axes.append(([-g[1], g[0], z], [gabs[1], gabs[0], z]))
    return axes


def triangle_gaps(N, a, e1, e2, lo, hi):
    """13 x (s, E, zero axis)."""
    zero3 = [N.zero, N.zero, N.zero]
    return [_axis_gap(N, L, Labs, (a, (zero3, e1, e2)), lo, hi) for L, Labs in _triangle_axes(N, a, e1, e2)]


def sphere_gaps(N, c0, dc, time, r2, lo, hi):
    """2 x (s, E, False): dmin^2 - R^2 and R^2 - dmax^2."""
    dmin2, dmax2 = (N.zero, N.zero), (N.zero, N.zero)
    for c in range(3):
        s, es = c0[c] + time * dc[c], abs(c0[c]) + abs(time * dc[c])
        near = N.pick(lo[c] - s, abs(lo[c]) + es, s - hi[c], es + abs(hi[c]), True)
        near = N.pick(*near, N.zero, N.zero, True)
        far = N.pick(s - lo[c], es + abs(lo[c]), hi[c] - s, abs(hi[c]) + es, True)
        dmin2 = (dmin2[0] + near[0] * near[0], dmin2[1] + near[1] * near[1])
        dmax2 = (dmax2[0] + far[0] * far[0], dmax2[1] + far[1] * far[1])
    R2 = abs(r2)
    return [(dmin2[0] - R2, dmin2[1] + R2, False), (R2 - dmax2[0], R2 + dmax2[1], False)]


def _ratio(gaps):
    """max over the axes with L != 0 of s / (u E), exactly (Fraction gaps); s = 0 with E = 0 counts as 0."""
    r = None
    for s, e, zero in gaps:
        if zero:
            continue
        v = Fr(0) if s == 0 else (s / (Fr(U) * e) if e != 0 else (Fr(10) ** 30 if s > 0 else -Fr(10) ** 30))
        r = v if r is None or v > r else r
    return Fr(-10) ** 31 if r is None else r  # (no axis at all cannot happen: the box normals are never zero)


def _fr(v):
    return [Fr(float(x)) for x in v]


def exact_pair(rec, cid, lo, hi, time):
    """r of one pair, exactly: a Fraction."""
    lo, hi = _fr(lo), _fr(hi)
    if cid < rec.ns:
        g = rec.sph[cid]
        return _ratio(sphere_gaps(_Exact, _fr(g[0:3]), _fr([0, 0, 0]), Fr(0), Fr(float(g[3])), lo, hi))
    if cid < rec.ns + rec.nm:
        g = rec.mov[cid - rec.ns]
        return _ratio(sphere_gaps(_Exact, _fr(g[0:3]), _fr(g[3:6]), Fr(float(time)), Fr(float(g[6])), lo, hi))
    t = rec.tri[cid - rec.ns - rec.nm]
    return _ratio(triangle_gaps(_Exact, _fr(t[0:3]), _fr(t[3:6]), _fr(t[6:9]), lo, hi))


def exact_axis_gaps(rec, cid, lo, hi, time):
    """The exact (s, E, zero) rows of one pair, in the mirror's axis order."""
    lo, hi = _fr(lo), _fr(hi)
    if cid < rec.ns:
        g = rec.sph[cid]
        return sphere_gaps(_Exact, _fr(g[0:3]), _fr([0, 0, 0]), Fr(0), Fr(float(g[3])), lo, hi)
    if cid < rec.ns + rec.nm:
        g = rec.mov[cid - rec.ns]
        return sphere_gaps(_Exact, _fr(g[0:3]), _fr(g[3:6]), Fr(float(time)), Fr(float(g[6])), lo, hi)
    t = rec.tri[cid - rec.ns - rec.nm]
    return triangle_gaps(_Exact, _fr(t[0:3]), _fr(t[3:6]), _fr(t[6:9]), lo, hi)


def _float_ratio(gaps):
    """The filter's r per pair (float arrays): far from 0 where the float gaps decide with a margin of FAR / u."""
    r = None
    for s, e, zero in gaps:
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(e > 0, s / (U * e), np.where(s > 0, np.inf, np.where(s < 0, -np.inf, 0.0)))
        v = np.where(zero, -np.inf, v)
        r = v if r is None else np.maximum(r, v)
    return r


class Classified:
    """Every pair of the live queries of `q` that is not far apart, with its r: qi, ci (class-major), r (float; exact to
    a relative 1e-12 where |r| < FAR / u, a far value of the right sign elsewhere).  Pairs not listed are decided NO."""

    def __init__(self, rec, q):
        self.rec, self.q = rec, q
        live = ~skipped(q)
        idx = np.nonzero(live)[0]
        qi, ci, r = [], [], []
        nsp = rec.ns + rec.nm
        cols = lambda m: [m[:, 0], m[:, 1], m[:, 2]]  # noqa: E731
        if nsp and len(idx):
            a = np.repeat(idx, nsp)
            c = np.tile(np.arange(nsp), len(idx))
            fx = c < rec.ns
            c0, dc, r2 = np.zeros((len(c), 3)), np.zeros((len(c), 3)), np.zeros(len(c))
            c0[fx], r2[fx] = rec.sph[c[fx], 0:3], rec.sph[c[fx], 3]
            m = rec.mov[c[~fx] - rec.ns]
            c0[~fx], dc[~fx], r2[~fx] = m[:, 0:3], m[:, 3:6], m[:, 6]
            t = np.where(fx, 0.0, q["time"][a])
            qi.append(a), ci.append(c)
            r.append(_float_ratio(sphere_gaps(_Float, cols(c0), cols(dc), t, r2, cols(q["lo"][a]), cols(q["hi"][a]))))
        if rec.nt and len(idx):
            vlo, vhi = tri_bounds(rec)
            ta, te1, te2, _ = _tri_fields(rec.tri)
            scale = np.abs(ta) + np.maximum(np.abs(te1), np.abs(te2))
            a, t = _tri_candidates(q, live, vlo, vhi, margin=scale)
            T = rec.tri[t]
            qi.append(a), ci.append(t + nsp)
            r.append(_float_ratio(triangle_gaps(_Float, cols(T[:, 0:3]), cols(T[:, 3:6]), cols(T[:, 6:9]), cols(q["lo"][a]), cols(q["hi"][a]))))
        self.qi = np.concatenate(qi) if qi else np.zeros(0, np.int64)
        self.ci = np.concatenate(ci) if ci else np.zeros(0, np.int64)
        self.r = np.concatenate(r) if r else np.zeros(0)
        self.n_pairs = len(idx) * rec.n
        near = np.nonzero(np.abs(self.r) < FAR / U)[0]
        self.n_exact = len(near)
        for j in near:
            i = self.qi[j]
            self.r[j] = float(exact_pair(rec, int(self.ci[j]), q["lo"][i], q["hi"][i], q["time"][i]))
        self.ins = rec.cls2ins[self.ci]
        order = np.lexsort((self.ins, self.qi))
        self.qi, self.ci, self.r, self.ins = self.qi[order], self.ci[order], self.r[order], self.ins[order]
        self.cut = np.searchsorted(self.qi, np.arange(len(q) + 1))

    def undecided(self, k):
        return int((np.abs(self.r) <= k).sum())

    def closed_sets(self):
        """The exact closed-set answer per query (r <= 0; min_prim applied): for inputs on which the predicate is exact."""
        out = []
        for i in range(len(self.q)):
            s = slice(self.cut[i], self.cut[i + 1])
            ins = self.ins[s][self.r[s] <= 0.0]
            out.append(ins[ins >= max(int(self.q["min_prim"][i]), 0)])
        return out


def check_answers(cl, counts, ids, max_ids, prec, what=""):
    """Asserts the contract on a build's answers to cl.q: every decided pair answered correctly, ids ascending, distinct,
    >= min_prim and padded with -1, counts consistent.  ids may be None (counts only).  Returns the number of undecided
    pairs the answers were free in."""
    k = K[prec]
    q, rec = cl.q, cl.rec
    dead = skipped(q)
    assert counts.shape == (len(q),) and (ids is None or ids.shape == (len(q), max_ids)), (what, counts.shape)
    free = 0
    for i in range(len(q)):
        row = None if ids is None else ids[i]
        if dead[i]:
            assert counts[i] == 0 and (row is None or np.all(row == -1)), (what, i, "skipped query answered")
            continue
        s = slice(cl.cut[i], cl.cut[i + 1])
        mp = max(int(q["min_prim"][i]), 0)
        part = cl.ins[s] >= mp
        ins, r = cl.ins[s][part], cl.r[s][part]
        yes, maybe = ins[r < -k], ins[np.abs(r) <= k]
        free += len(maybe)
        c = int(counts[i])
        assert len(yes) <= c <= len(yes) + len(maybe), (what, i, c, len(yes), len(maybe))
        if row is None:
            continue
        m = min(c, max_ids)
        got = row[:m]
        assert np.all(row[m:] == -1) and np.all(got >= mp) and np.all(got < rec.n), (what, i, row, c)
        assert np.all(np.diff(got) > 0), (what, i, "ids not ascending and distinct", row)
        allowed = np.concatenate([yes, maybe])
        assert np.all(np.isin(got, allowed)), (what, i, "reports a pair decided NO", got, allowed)
        must = yes if c <= max_ids else yes[yes < got[-1]]
        assert np.all(np.isin(must, got)), (what, i, "misses a pair decided YES", got, must)
    return free


def mirror_residual(rec, q, limit=400, seed=1):
    """The worst |mirror gap - exact gap| / (u E_L) over the axes of up to `limit` pairs of the loose candidates of q (the
    mirror's gap carries one rounding more than the kernel's comparison: its final difference)."""
    cl_q = ~skipped(q)
    nsp = rec.ns + rec.nm
    qi, ci = [], []
    idx = np.nonzero(cl_q)[0]
    if nsp and len(idx):
        qi.append(np.repeat(idx, nsp)), ci.append(np.tile(np.arange(nsp), len(idx)))
    if rec.nt and len(idx):
        vlo, vhi = tri_bounds(rec)
        ta, te1, te2, _ = _tri_fields(rec.tri)
        a, t = _tri_candidates(q, cl_q, vlo, vhi, margin=np.abs(ta) + np.maximum(np.abs(te1), np.abs(te2)))
        qi.append(a), ci.append(t + nsp)
    qi, ci = np.concatenate(qi), np.concatenate(ci)
    pick = np.random.default_rng(seed).permutation(len(qi))[:limit]
    worst = 0.0
    for j in pick:
        i, c = int(qi[j]), int(ci[j])
        lo, hi = q["lo"][i:i + 1], q["hi"][i:i + 1]
        if c < nsp:
            s, r2 = _centres(rec, np.array([c]), q["time"][i:i + 1])
            mg = mirror_sphere_gaps(lo, hi, s, r2)[0]
        else:
            mg = mirror_triangle_gaps(lo, hi, rec.tri[c - nsp:c - nsp + 1])[0]
        for g, (s, e, zero) in zip(mg, exact_axis_gaps(rec, c, lo[0], hi[0], q["time"][i])):
            if e != 0 and math.isfinite(g):
                worst = max(worst, float(abs(Fr(float(g)) - s) / (Fr(U) * e)))
    return worst
