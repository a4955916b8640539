"""References for the k-nearest queries (rtow_nearest*): the strict answer from the numpy mirror of the kernel's formulas
and the checker of the fast build's contract (numpy and the standard library, no GPU).  Everything is built on
point_ref.py: the mirror (all_dists, prim_point), the exact distance (exact_dist), the bands (bound) and the cheap lower
bounds (lower_bounds).

Strict.  reference(rec, mats, pts, times, max_dist, k) is the definition of include/rtow.h evaluated with the mirror:
per query the mirror's distance to every primitive, ordered by (dist, insertion index), filtered by dist <= max_dist and
cut at k; each kept entry's record (dist, point, insertion index, kind, material) is the one the closest-point query
writes for that primitive (prim_point); the slots past the count hold the miss record.  The strict build must equal it
in every field, bit for bit (same_answers / first_difference).

Fast.  FastChecker.check(hits, counts, k) asserts the fast clauses of include/rtow.h on every answer, none sampled:
  * shape: 0 <= count <= k, the slots below the count are hits and those at and past it are the miss record (dist +inf,
    point 0, prim = kind = material = -1); max_dist NaN or negative gives count 0;
  * per entry: prim names a primitive, kind and material are that primitive's, dist <= max_dist, dist within the
    closest-point band of the exact distance D of that primitive (D - lo <= dist <= D + hi, point_ref.bound at 64 u), the
    point on the primitive's surface within tau S_q and consistent with dist within tau (S + S_q) — the clauses of
    rtow_closest_point, with the same functions point_ref.AnswerChecker uses; no field NaN;
  * order: dist non-decreasing, primitives distinct, entries with bit-equal dist in insertion order;
  * completeness by the bands: with thr = dist[k - 1] when count == k and thr = max_dist when count < k, every
    unreported primitive c has D(c) + up(c) >= thr (up: the upper band).  A primitive whose lower bound
    (point_ref.lower_bounds) is already above thr satisfies it without Fraction arithmetic; the others are computed
    exactly.  With thr = +inf nothing whose mirror distance is finite may be left out.
It returns the number of queries, entries, exact pairs and the worst dist error in units of its band.
"""
from __future__ import annotations

import math

import numpy as np

import point_ref as pr

HIT_DTYPE = pr.HIT_DTYPE
MAX_NEAREST = 8


def miss_records(shape):
    h = np.zeros(shape, dtype=HIT_DTYPE)
    h["dist"], h["prim"], h["kind"], h["material"] = np.inf, -1, -1, -1
    return h


def nearest_ids(rec, pts, times, max_dist, k):
    """Per query the class-major ids of the first k of N (rows padded with -1) and the counts, from the mirror."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    md = np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,))
    ids = np.full((n, k), -1, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int32)
    ins = np.asarray(rec.cls2ins)
    for sl, D in pr.all_dists(rec, pts, times):
        for j in range(D.shape[0]):
            i = sl.start + j
            d = D[j]
            with np.errstate(invalid="ignore"):
                inside = d <= md[i]  # (NaN max_dist: nothing)
            if len(d) > k:  # only what can make the cut: everything up to the k-th smallest distance, ties included
                inside &= d <= np.partition(d, k - 1)[k - 1]
            cand = np.nonzero(inside)[0]
            order = cand[np.lexsort((ins[cand], d[cand]))][:k]
            ids[i, :len(order)] = order
            counts[i] = len(order)
    return ids, counts


def records_of(rec, mats, pts, times, ids):
    """[n, k] HIT_DTYPE: the closest-point record of class-major primitive ids[i, j] at query i (-1: the miss record)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n, k = ids.shape
    times = np.broadcast_to(np.asarray(times, dtype=np.float64), (n,))
    mats = np.asarray(mats)
    h = miss_records((n, k))
    for j in range(k):
        hit = ids[:, j] >= 0
        if not hit.any():
            continue
        c = ids[hit, j]
        col = h[:, j]
        d, q = pr.prim_point(rec, c, pts[hit], times[hit])
        prim = np.asarray(rec.cls2ins)[c]
        col["dist"][hit], col["point"][hit], col["prim"][hit] = d, q, prim
        col["kind"][hit] = rec.kind_of(c)
        col["material"][hit] = mats[prim]
        h[:, j] = col
    return h


def reference(rec, mats, pts, times, max_dist, k):
    """(hits [n, k] HIT_DTYPE, counts [n] int32): the strict answer."""
    assert 1 <= k <= MAX_NEAREST
    ids, counts = nearest_ids(rec, pts, times, max_dist, k)
    return records_of(rec, mats, pts, times, ids), counts


def permuted_records(G, seed):
    """(perm, records, material per insertion index) of an accel_images.Geometry inserted in a seeded random order:
    insertion position i holds class-major primitive perm[i]."""
    perm = np.random.default_rng(seed).permutation(G.np)
    kind = np.array([pr.SPHERE] * G.ns + [pr.MOVING] * G.nm + [pr.TRIANGLE] * G.nt)[perm]
    index = np.concatenate([np.arange(G.ns), np.arange(G.nm), np.arange(G.nt)])[perm]
    return perm, pr.make_records(G.sph, G.mov, G.tri, kind, index), G.pmat[perm]


FIELDS = ("dist", "point", "prim", "kind", "material")


def same_answers(a, b):
    """Every field of the contract equal, floating-point ones bit for bit (the pad is not part of it)."""
    if a.shape != b.shape:
        return False
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        if not np.array_equal(x, y):
            return False
    return True


def first_difference(a, b):
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        xb, yb = (x.view(np.uint64), y.view(np.uint64)) if x.dtype.kind == "f" else (x, y)
        bad = np.argwhere(xb != yb)
        if len(bad):
            w = tuple(int(v) for v in bad[0])
            return (f, w, x[w].tolist(), y[w].tolist())
    return None


# ------------------------------------------------------------------------------------------------ fast checker ---
class FastChecker:
    """The fast contract for one batch of queries, reusable for many answers to it (every kernel): the mirror's
    distances and the exact quantities are computed once."""

    def __init__(self, rec, mats, pts, times, max_dist, prec="fast"):
        self.rec, self.mats, self.prec = rec, np.asarray(mats), prec
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        n = len(self.pts)
        self.times = np.array(np.broadcast_to(np.asarray(times, dtype=np.float64), (n,)))
        self.md = np.array(np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,)))
        self.mirror = np.empty((n, rec.n))
        for sl, D in pr.all_dists(rec, self.pts, self.times):
            self.mirror[sl] = D
        self._lb, self._exact, self._band, self._geom = {}, {}, {}, {}
        self.tau = pr._F(pr.TAU[prec])

    # ---- memoised quantities
    def lower(self, i):
        if i not in self._lb:
            self._lb[i] = pr.lower_bounds(self.rec, np.arange(self.rec.n), self.pts[i], self.times[i])
        return self._lb[i]

    def exact(self, i, c):
        if (i, c) not in self._exact:
            self._exact[(i, c)] = pr.exact_dist(self.rec, c, self.pts[i], self.times[i])
        return self._exact[(i, c)]

    def band(self, i, c):
        if (i, c) not in self._band:
            lo, hi = pr.bound(self.rec, c, self.pts[i], self.times[i], self.prec)
            self._band[(i, c)] = (pr._F(lo), pr._F(hi))
        return self._band[(i, c)]

    def geom(self, i, c):
        key = (c, float(self.times[i]) if self.rec.ns <= c < self.rec.ns + self.rec.nm else 0.0)
        if key not in self._geom:
            self._geom[key] = pr.exact_geometry(self.rec, c, key[1])
        return self._geom[key]

    # ---- one entry: the closest-point clauses for its primitive
    def _entry(self, i, h):
        rec, p, md = self.rec, self.pts[i], float(self.md[i])
        dist, q, prim = float(h["dist"]), np.array(h["point"], dtype=np.float64), int(h["prim"])
        assert not math.isnan(dist) and np.all(np.isfinite(q)), ("NaN or a point that is not finite", dist, q.tolist())
        assert 0 <= prim < rec.n, ("prim out of range", prim)
        c = int(rec.ins2cls[prim])
        assert int(h["kind"]) == int(rec.kind_of(c)), ("kind is not the primitive's", int(h["kind"]))
        assert int(h["material"]) == int(self.mats[prim]), ("material is not the primitive's", int(h["material"]))
        assert dist <= md, ("dist above max_dist", dist, md)
        D, err = self.exact(i, c)
        if dist == math.inf and D * D > pr.OVERFLOW:  # the overflow rule of rtow_closest_point
            return c, 0.0
        lo, hi = self.band(i, c)
        assert pr.within(dist, D, err, lo, hi), ("dist outside its band", c, dist, float(D), float(lo), float(hi))
        d = pr._F(dist)
        e_dist = pr._units(d - D, hi) if d >= D else pr._units(D - d, lo)
        geom = self.geom(i, c)
        Sq = geom[1]
        s_err, s_e = pr.surface_error(geom, q)
        assert s_err - s_e <= self.tau * Sq, ("point off the surface", c, q.tolist(), float(s_err), float(self.tau * Sq))
        L, l_e = pr._sqrt_fr(sum((pr._F(p[j]) - pr._F(q[j])) ** 2 for j in range(3)))
        S = pr.header_scale(geom, p)
        assert abs(L - d) - l_e <= self.tau * (S + Sq), ("|p - point| differs from dist", c, float(L), dist)
        return c, e_dist

    def _check_one(self, i, hits, count, k):
        rec, md = self.rec, float(self.md[i])
        assert 0 <= count <= k, ("count outside [0, k]", count)
        miss = miss_records(())
        for j in range(count, k):
            assert all(np.array_equal(hits[j][f], miss[f]) for f in FIELDS), ("not the miss record past the count", j)
        for j in range(count):
            assert int(hits[j]["prim"]) >= 0, ("a miss record below the count", j)
        if math.isnan(md) or md < 0.0:
            assert count == 0, ("entries under a NaN or negative max_dist", count)
            return 0.0
        cids, worst = [], 0.0
        for j in range(count):
            c, e = self._entry(i, hits[j])
            cids.append(c)
            worst = max(worst, e)
        dist = np.array([float(hits[j]["dist"]) for j in range(count)])
        prim = [int(hits[j]["prim"]) for j in range(count)]
        assert np.all(np.diff(dist) >= 0), ("dist decreases", dist.tolist())
        assert len(set(prim)) == count, ("a primitive twice", prim)
        for j in range(1, count):
            assert dist[j] != dist[j - 1] or prim[j] > prim[j - 1], ("a tie out of insertion order", j, prim)
        # completeness by the bands
        thr = float(dist[k - 1]) if count == k else md
        left = np.ones(rec.n, dtype=bool)
        left[cids] = False
        if thr == math.inf:
            bad = np.nonzero(left & np.isfinite(self.mirror[i]))[0]
            assert len(bad) == 0, ("primitives at a finite distance left out of an unbounded answer", bad[:4].tolist())
            return worst
        lim = thr * (1.0 - 2.0 ** -50)  # (a lower bound above this is above thr less its own rounding: decided)
        for c in np.nonzero(left & ~(self.lower(i) > lim))[0]:
            c = int(c)
            D, err = self.exact(i, c)
            hi = self.band(i, c)[1]
            assert D + hi + err >= pr._F(thr), ("a nearer primitive is left out by more than its band", c, float(D), thr)
        return worst

    def check(self, hits, counts, k, what=""):
        n = len(self.pts)
        assert hits.shape == (n, k) and len(counts) == n, (what, hits.shape, len(counts))
        out = dict(queries=n, entries=int(np.sum(counts)), worst_dist=0.0)
        for i in range(n):
            try:
                out["worst_dist"] = max(out["worst_dist"], self._check_one(i, hits[i], int(counts[i]), k))
            except AssertionError as e:
                raise AssertionError(f"{what} query {i} p={self.pts[i].tolist()} time={self.times[i]} "
                                     f"max_dist={self.md[i]} count={int(counts[i])}: {e}") from None
        out["exact_pairs"] = len(self._exact)
        return out
