"""References for the k-nearest queries (rtow_nearest*): the strict answer from the numpy mirror of the kernel's formulas
and the checker of the fast build's contract (numpy and the standard library, no GPU).  Everything is built on
point_ref.py: the mirror (all_dists, prim_point), the exact distance (exact_dist), the bands (bound) and the cheap lower
bounds (lower_bounds).

Strict.  reference(rec, mats, pts, times, max_dist, k) is the definition of include/rtow.h evaluated with the mirror:
per query the mirror's distance to every primitive, ordered by (dist, insertion index), filtered by dist <= max_dist and
cut at k; each kept entry's record (dist, point, insertion index, kind, material) is the one the closest-point query
writes for that primitive (prim_point); the slots past the count hold the miss record.  The strict build must equal it
in every field, bit for bit (same_answers / first_difference).

Exact.  FastChecker.check(hits, counts, k, what, prec) asserts the clauses of include/rtow.h at tau of `prec` (64 u for
the fast build, 32 u for the strict one) on every answer, none sampled:
  * shape: 0 <= count <= k, the slots below the count are hits and those at and past it are the miss record (dist +inf,
    point 0, prim = kind = material = -1); max_dist NaN or negative gives count 0;
  * per entry: prim names a primitive, kind and material are that primitive's, dist <= max_dist, dist within the
    closest-point band of the exact distance D of that primitive (D - lo <= dist <= D + hi, point_ref.bound at 64 u), the
    point on the primitive's surface within tau S_q and consistent with dist within tau (S + S_q) — the clauses of
    rtow_closest_point, with the same functions point_ref.AnswerChecker uses; no field NaN;
  * order: dist non-decreasing, primitives distinct, entries with bit-equal dist in insertion order;
  * completeness by the bands: with thr = dist[k - 1] when count == k and thr = max_dist when count < k, every
    unreported primitive c has D(c) + up(c) >= thr (up: the upper band).  A primitive whose lower bound
    (point_ref.lower_bounds) is already above thr, or whose lower bound plus upper band reaches thr, satisfies it
    without Fraction arithmetic (FastChecker's docstring proves both); the others are computed exactly.  With
    thr = +inf nothing whose mirror distance is finite may be left out;
  * overflow: an entry whose exact squared distance exceeds point_ref.OVERFLOW may carry dist +inf (FastChecker).
It returns the number of queries, entries and exact pairs, the worst dist, on-surface and consistency errors in units of
their bands, the lists short of k, the answers that took the overflow rule and the completeness decisions that needed
exact arithmetic (stats_line prints them).
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


def nearest_ids(rec, pts, times, max_dist, k, mirror=None):
    """Per query the class-major ids of the first k of N (rows padded with -1) and the counts, from the mirror
    (`mirror`: its [n, n_prims] distances where the caller has them already)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    md = np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,))
    ids = np.full((n, k), -1, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int32)
    ins = np.asarray(rec.cls2ins)
    for sl, D in (pr.all_dists(rec, pts, times) if mirror is None else [(slice(0, n), mirror)]):
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


def reference(rec, mats, pts, times, max_dist, k, mirror=None):
    """(hits [n, k] HIT_DTYPE, counts [n] int32): the strict answer."""
    assert 1 <= k <= MAX_NEAREST
    ids, counts = nearest_ids(rec, pts, times, max_dist, k, mirror)
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
def upper_bands(rec, p, time, prec):
    """Floats hi'[c] <= the upper band hi(c) of point_ref.bound for every class-major primitive c at p: tau S, without
    bound's factor 1.01 and without a triangle's plane term (which is >= 0).  S is summed here in another order than in
    bound, which moves it by a few u relative — far inside the 1 % bound puts on top."""
    p = np.asarray(p, dtype=np.float64)
    S = np.empty(rec.n)
    with np.errstate(all="ignore"):
        g = rec.sph
        S[:rec.ns] = np.abs(p - g[:, 0:3]).sum(1) + np.sqrt(np.abs(g[:, 3]))
        g = rec.mov
        c = g[:, 0:3] + time * g[:, 3:6]
        S[rec.ns:rec.ns + rec.nm] = (np.abs(p - c).sum(1) + np.sqrt(np.abs(g[:, 6])) + np.abs(g[:, 0:3]).sum(1)
                                     + np.abs(time * g[:, 3:6]).sum(1))
        t = rec.tri
        S[rec.ns + rec.nm:] = np.abs(p - t[:, 0:3]).sum(1) + np.abs(t[:, 3:6]).sum(1) + np.abs(t[:, 6:9]).sum(1)
        return pr.TAU[prec] * S


class FastChecker:
    """The contract of include/rtow.h for one batch of queries at tau of `prec` ("fast": 64 u, "strict": 32 u), reusable
    for many answers to it (every kernel, builder, build and k): the mirror's distances are computed once, the exact
    quantities once per (query, distinct record) — bit-identical records (coincident copies) share them through `canon`,
    as in point_ref.AnswerChecker — the verdict on an entry once per (query, prec, record bytes), the completeness
    verdict once per (query, prec, thr, set of reported primitives) and the verdict on a whole list once per
    (query, prec, k, count, its bytes).

    Completeness without Fractions.  The clause is D(c) + hi(c) >= thr for every unreported primitive c (D exact, hi
    the upper band of point_ref.bound).  Two decisions need no exact arithmetic, both from lb(c) =
    point_ref.lower_bounds, a float with lb(c) <= D(c):
      (1) lb(c) > thr (1 - 2^-50).  Then D(c) > thr - 2^-50 thr, and hi(c) >= tau S(c) >= 2^-48 D(c) (S >= D: the 1-norm
          of p - a, or |p - c|_1 + R, is at least the distance to the primitive), which is above 2^-50 thr.
      (2) down(lb(c) + hi'(c)) >= thr, hi' = upper_bands <= hi and down() the next double below the rounded sum.  A
          rounded sum of two doubles is within one ulp of the real sum, so down(fl(x + y)) <= x + y, and
          D(c) + hi(c) >= lb(c) + hi'(c) >= down(fl(lb(c) + hi'(c))) >= thr.  This is what decides at far points, where
          every primitive is within one band of every other and (1) never holds.
    lb(c) <= D(c) as lower_bounds states it: a triangle's vertices a, a + e1, a + e2 are exact sums of the record's
    values, the computed ones are off by at most u (|a| + |e1|) and the box is padded by 4 u (|a| + |e1| + |e2|), which
    also covers the rounding of the padded plane; the distance to that box takes six roundings of positive terms and
    is scaled by 1 - 2^-50 = 1 - 8 u.  A sphere's mirror distance is off by at most 5 u S (the differences, the sum of
    squares, the root, the last subtraction; a moving centre adds 2 u (|c0|_1 + |time dc|_1), part of its S) and 16 u S
    is taken off.  Two cases are NOT covered by that reasoning and are excluded here: a bound that is not finite (the
    squares overflowed: it says nothing) and a positive bound below 1e-140 (its squares are subnormal and may have
    rounded up): both are replaced by 0, which sends the primitive to the exact comparison.

    Overflow (the rule of rtow_closest_point, for lists).  An entry whose exact squared distance exceeds
    point_ref.OVERFLOW may carry dist +inf (its point need only be finite); +inf <= max_dist holds only for
    max_dist = +inf.  The threshold of such an answer is +inf, and then only primitives whose mirror distance is +inf
    may be left out; entries tied at +inf are in insertion order like every tie.  `overflow` counts the answers with
    such an entry.
    """

    def __init__(self, rec, mats, pts, times, max_dist, prec="fast"):
        self.rec, self.mats, self.prec = rec, np.asarray(mats), prec
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        n = len(self.pts)
        self.times = np.array(np.broadcast_to(np.asarray(times, dtype=np.float64), (n,)))
        self.md = np.array(np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,)))
        self.mirror = np.empty((n, rec.n))
        for sl, D in pr.all_dists(rec, self.pts, self.times):
            self.mirror[sl] = D
        self._lb, self._ub, self._sorted, self._exact, self._band, self._geom = {}, {}, {}, {}, {}, {}
        self._entries, self._complete, self._lists, self._point = {}, {}, {}, {}
        self.decided = {"box": 0, "band": 0, "exact": 0}  # completeness decisions per (query, primitive), by what decided
        if not hasattr(rec, "canon"):  # (once per scene: a sort of its records)
            rec.canon = np.arange(rec.n)
            for base, recs in ((0, rec.sph), (rec.ns, rec.mov), (rec.ns + rec.nm, rec.tri)):
                if len(recs):
                    _, first, inv = np.unique(np.ascontiguousarray(recs).view(np.uint64), axis=0, return_index=True,
                                              return_inverse=True)
                    rec.canon[base:base + len(recs)] = base + first[np.ravel(inv)]
        self.canon = rec.canon
        self._miss = miss_records(())

    # ---- memoised quantities
    def lower(self, i):
        if i not in self._lb:
            lb = pr.lower_bounds(self.rec, np.arange(self.rec.n), self.pts[i], self.times[i])
            self._lb[i] = np.where(np.isfinite(lb) & ~((lb > 0.0) & (lb < 1e-140)), lb, 0.0)
        return self._lb[i]

    def _cheap(self, i, prec):
        """(lb, sb, max(lb, sb)) of query i: what the two cheap completeness decisions read, once for every threshold
        (sb: the rounded-down sum of decision (2))."""
        if (i, prec) not in self._sorted:
            lb = self.lower(i)
            with np.errstate(all="ignore"):
                sb = np.nextafter(lb + self.upper(i, prec), -np.inf)
            sb = np.where(np.isnan(sb), -np.inf, sb)  # (NaN: decides nothing)
            self._sorted[(i, prec)] = (lb, sb, np.maximum(lb, sb))
        return self._sorted[(i, prec)]

    def upper(self, i, prec):
        if i not in self._ub:  # (tau is a power of two: tau S is exact for either)
            self._ub[i] = upper_bands(self.rec, self.pts[i], self.times[i], "strict")
        return self._ub[i] * (pr.TAU[prec] / pr.TAU["strict"])

    def exact(self, i, c):
        c = int(self.canon[c])
        if (i, c) not in self._exact:
            self._exact[(i, c)] = pr.exact_dist(self.rec, c, self.pts[i], self.times[i])
        return self._exact[(i, c)]

    def band(self, i, c, prec=None):
        prec = prec or self.prec
        c = int(self.canon[c])
        if (i, c, prec) not in self._band:
            lo, hi = pr.bound(self.rec, c, self.pts[i], self.times[i], prec)
            self._band[(i, c, prec)] = (pr._F(lo), pr._F(hi))
        return self._band[(i, c, prec)]

    def geom(self, i, c):
        c = int(self.canon[c])
        key = (c, float(self.times[i]) if self.rec.ns <= c < self.rec.ns + self.rec.nm else 0.0)
        if key not in self._geom:
            self._geom[key] = pr.exact_geometry(self.rec, c, key[1])
        return self._geom[key]

    # ---- one entry: the closest-point clauses for its primitive
    def _entry(self, i, h, prec):
        """(class-major id, dist / on-surface / consistency error in units of their bands, took the overflow rule)."""
        rec, p, md = self.rec, self.pts[i], float(self.md[i])
        tau = pr._F(pr.TAU[prec])
        dist, q, prim = float(h["dist"]), np.array(h["point"], dtype=np.float64), int(h["prim"])
        assert not math.isnan(dist) and np.all(np.isfinite(q)), ("NaN or a point that is not finite", dist, q.tolist())
        assert 0 <= prim < rec.n, ("prim out of range", prim)
        c = int(rec.ins2cls[prim])
        assert int(h["kind"]) == int(rec.kind_of(c)), ("kind is not the primitive's", int(h["kind"]))
        assert int(h["material"]) == int(self.mats[prim]), ("material is not the primitive's", int(h["material"]))
        assert dist <= md, ("dist above max_dist", dist, md)
        D, err = self.exact(i, c)
        if dist == math.inf and D * D > pr.OVERFLOW:  # the overflow rule
            return c, 0.0, 0.0, 0.0, 1
        lo, hi = self.band(i, c, prec)
        assert dist != math.inf, ("dist outside its band", c, dist, "+inf, and the exact square is in range")
        assert pr.within(dist, D, err, lo, hi), ("dist outside its band", c, dist, float(D), float(lo), float(hi))
        d = pr._F(dist)
        e_dist = pr._units(d - D, hi) if d >= D else pr._units(D - d, lo)
        key = (i, int(self.canon[c]), q.tobytes())  # (what does not depend on tau: once for both)
        if key not in self._point:
            geom = self.geom(i, c)
            self._point[key] = (geom[1], pr.surface_error(geom, q), pr.header_scale(geom, p),
                                pr._sqrt_fr(sum((pr._F(p[j]) - pr._F(q[j])) ** 2 for j in range(3))))
        Sq, (s_err, s_e), S, (L, l_e) = self._point[key]
        assert s_err - s_e <= tau * Sq, ("point off the surface", c, q.tolist(), float(s_err), float(tau * Sq))
        assert abs(L - d) - l_e <= tau * (S + Sq), ("|p - point| differs from dist", c, float(L), dist)
        return c, e_dist, pr._units(s_err, tau * Sq), pr._units(abs(L - d), tau * (S + Sq)), 0

    def _completeness(self, i, prec, thr, cids):
        """Assert the completeness clause for the primitives not in `cids`; the number of them that needed Fractions."""
        rec = self.rec
        left = np.ones(rec.n, dtype=bool)
        left[cids] = False
        if thr == math.inf:
            bad = np.nonzero(left & np.isfinite(self.mirror[i]))[0]
            assert len(bad) == 0, ("primitives at a finite distance left out of an unbounded answer", bad[:4].tolist())
            return 0
        # only the primitives with max(lb, sb) <= thr can be open: every other one has lb > thr or sb > thr and is decided
        # by (1) or (2)
        lb, sb, m = self._cheap(i, prec)
        lim = thr * (1.0 - 2.0 ** -50)  # (a lower bound above this is above thr less its own rounding: decided)
        cand = np.nonzero(m <= thr)[0]
        cand = cand[left[cand]]
        by_box = lb[cand] > lim
        by_band = sb[cand] >= thr
        todo = np.unique(self.canon[cand[~by_box & ~by_band]])  # (bit-identical records: one comparison)
        n_box = int(np.count_nonzero(lb > lim)) - sum(bool(lb[c] > lim) for c in cids)
        self.decided["box"] += n_box
        self.decided["band"] += int(left.sum()) - n_box - int(np.sum(~by_box & ~by_band))
        self.decided["exact"] += len(todo)
        for c in todo:
            c = int(c)
            D, err = self.exact(i, c)
            hi = self.band(i, c, prec)[1]
            assert D + hi + err >= pr._F(thr), ("a nearer primitive is left out by more than its band", c, float(D), thr)
        return len(todo)

    def _check_one(self, i, hits, count, k, prec):
        """(worst dist, on-surface, consistency error; took the overflow rule; completeness pairs that needed Fractions)."""
        md = float(self.md[i])
        assert 0 <= count <= k, ("count outside [0, k]", count)
        miss = self._miss
        for j in range(count, k):
            assert all(np.array_equal(hits[j][f], miss[f]) for f in FIELDS), ("not the miss record past the count", j)
        for j in range(count):
            assert int(hits[j]["prim"]) >= 0, ("a miss record below the count", j)
        if math.isnan(md) or md < 0.0:
            assert count == 0, ("entries under a NaN or negative max_dist", count)
            return 0.0, 0.0, 0.0, 0, 0
        cids, worst, over = [], [0.0, 0.0, 0.0], 0
        for j in range(count):
            key = (i, prec, hits[j].tobytes())
            if key not in self._entries:
                self._entries[key] = self._entry(i, hits[j], prec)
            e = self._entries[key]
            cids.append(e[0])
            worst = [max(a, b) for a, b in zip(worst, e[1:4])]
            over |= e[4]
        dist = np.array([float(hits[j]["dist"]) for j in range(count)])
        prim = [int(hits[j]["prim"]) for j in range(count)]
        assert np.all(dist[1:] >= dist[:-1]), ("dist decreases", dist.tolist())
        assert len(set(prim)) == count, ("a primitive twice", prim)
        for j in range(1, count):
            assert dist[j] != dist[j - 1] or prim[j] > prim[j - 1], ("a tie out of insertion order", j, prim)
        # completeness by the bands
        thr = float(dist[k - 1]) if count == k else md
        key = (i, prec, thr, frozenset(cids))
        if key not in self._complete:
            self._complete[key] = self._completeness(i, prec, thr, cids)
        return worst[0], worst[1], worst[2], over, self._complete[key]

    def check(self, hits, counts, k, what="", prec=None):
        prec = prec or self.prec
        n = len(self.pts)
        assert hits.shape == (n, k) and len(counts) == n, (what, hits.shape, len(counts))
        out = dict(queries=n, entries=int(np.sum(counts)), worst_dist=0.0, worst_surface=0.0, worst_consistency=0.0,
                   short=int(np.sum(np.asarray(counts) < k)), overflow=0, exact_decisions=0)
        for i in range(n):
            key = (i, prec, k, int(counts[i]), hits[i].tobytes())
            if key not in self._lists:
                try:
                    self._lists[key] = self._check_one(i, hits[i], int(counts[i]), k, prec)
                except AssertionError as e:
                    raise AssertionError(f"{what} query {i} p={self.pts[i].tolist()} time={self.times[i]} "
                                         f"max_dist={self.md[i]} count={int(counts[i])}: {e}") from None
            r = self._lists[key]
            out["worst_dist"] = max(out["worst_dist"], r[0])
            out["worst_surface"] = max(out["worst_surface"], r[1])
            out["worst_consistency"] = max(out["worst_consistency"], r[2])
            out["overflow"] += r[3]
            out["exact_decisions"] += r[4]
        out["exact_pairs"] = len(self._exact)
        return out


def stats_line(s):
    return (f"{s['queries']} queries, {s['entries']} entries, {s['exact_pairs']} exact pairs, worst dist "
            f"{s['worst_dist']:.3f}, on-surface {s['worst_surface']:.3f}, consistency {s['worst_consistency']:.3f} of "
            f"their bands, {s['short']} lists short of k, overflow {s['overflow']}, {s['exact_decisions']} completeness "
            f"decisions by exact arithmetic")
