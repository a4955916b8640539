"""The cases of the k-nearest checkers (test_gpu_nearest.py, test_gpu_exact_nearest.py and the host self-tests in
test_nearest_host.py): the strict comparison, the mixed batch around the j-th distance, the point sets of a scene with
their checkers, and the coincident mesh with two materials.  Importing this module loads no library."""
import math

import numpy as np

import accel_images as ai
import nearest_ref as nr
import point_ref as pr
import rtow

KS_STRICT = (1, 2, 5, 8)  # against one k = 8 reference, cut earlier
KS_FAST = (1, 3, 8)
KTH = (0, 3, 7)  # the entries whose distance mixed_kth puts max_dist around
GREY_AND_WHITE = ((ai.MAT_LAMBERTIAN, (0.3, 0.3, 0.3), 0.0, 1.5), (ai.MAT_LAMBERTIAN, (0.8, 0.8, 0.8), 0.0, 1.5))


def cut(ref8, k):
    """The strict answer for k from the one for 8: the same sorted list, cut earlier."""
    hits, counts = ref8
    return np.ascontiguousarray(hits[:, :k]), np.minimum(counts, k).astype(np.int32)


def assert_strict(got, want, what):
    (h, c), (rh, rc) = got, want
    assert np.array_equal(c, rc), (what, "counts", np.nonzero(c != rc)[0][:4].tolist())
    assert nr.same_answers(h, rh), (what, nr.first_difference(h, rh))


def kth_dists(rec, pts, times):
    """[n, 8] the mirror's j-th distances of an unbounded query at each query's own time (+inf past the primitives)."""
    ids, _ = nr.nearest_ids(rec, pts, times, math.inf, nr.MAX_NEAREST)
    d = np.full(ids.shape, np.inf)
    for j in range(ids.shape[1]):
        m = ids[:, j] >= 0
        d[m, j] = pr.prim_point(rec, ids[m, j], pts[m], times[m])[0]
    return d


N_KTH = 13  # max_dist values of mixed_kth: coprime to the 3 times, and every pair occurs within 39 consecutive lanes


def mixed_kth(rec, near, seed):
    """(points, times, max_dist) of one batch in which every wave of 64 consecutive queries holds every value: time
    cycles through 0, 1, U(0, 1) and max_dist through NaN, -1, +inf, for j in KTH the mirror's j-th distance d_j (at the
    query's own time; the last one a scene with fewer primitives has), the double below it and half of it, and 2 d_3."""
    g = np.random.default_rng(seed)
    pts = np.array(near, dtype=np.float64)
    n = len(pts)
    k = np.arange(n)
    times = np.select([k % 3 == 0, k % 3 == 1], [0.0, 1.0], g.random(n))
    d = kth_dists(rec, pts, times)
    last = min(rec.n, nr.MAX_NEAREST) - 1
    vals = [np.full(n, np.nan), np.full(n, -1.0), np.full(n, np.inf)]
    for j in KTH:
        dj = d[:, min(j, last)]
        vals += [dj, np.nextafter(dj, -np.inf), 0.5 * dj]
    vals.append(2.0 * d[:, min(3, last)])
    assert len(vals) == N_KTH and math.gcd(N_KTH, 3) == 1 and n % 64
    sel = k % N_KTH
    return pts, times, np.select([sel == v for v in range(N_KTH)], vals)


def kth_lanes(j, what):
    """The residue of mixed_kth's max_dist cycle that holds d_j ("at"), the double below ("below") or half ("half")."""
    return 3 + 3 * KTH.index(j) + ("at", "below", "half").index(what)


def nearest_sets(rec, seed, near=None, rnd=None, sizes=pr.SIZES, refit=False):
    """pr.all_sets and, except after a refit, the mixed_kth batch on the points of its mixed batch."""
    sets = pr.all_sets(rec, seed, near, rnd, sizes, refit)
    if not refit:
        mixed = next(s for s in sets if s[0] == "mixed")
        sets.append(("mixed_kth",) + mixed_kth(rec, mixed[1], seed + 6))
    assert all(len(s[1]) % 64 for s in sets)
    return sets


def joined(sets):
    """The lanes of all `sets` as one set, those of mixed_kth first: ([(name, points, times, max_dist)], number of
    mixed_kth lanes).  For the 96.8k mesh, where a far or overflowing lane cannot prune and walks the whole mesh (about
    0.2 s a call with k = 8, on its own or beside 86 others): one call per walk, build and k instead of one per set."""
    sets = sorted(sets, key=lambda s: s[0] != "mixed_kth")
    lanes = lambda v, n: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))  # noqa: E731
    pts = np.concatenate([s[1] for s in sets])
    times = np.concatenate([lanes(s[2], len(s[1])) for s in sets])
    md = np.concatenate([lanes(s[3], len(s[1])) for s in sets])
    assert len(pts) % 64
    return [("+".join(s[0] for s in sets), pts, times, md)], len(sets[0][1]) if sets[0][0] == "mixed_kth" else 0


class Batch:
    """One point set: its queries (per-lane times and radii), the exact checker of its answers, and the strict
    reference for k = 8 (computed on first use: on the big mesh once, shared by both builders).  `kth`: the number of
    leading lanes that are mixed_kth's (all of them in the set of that name)."""

    def __init__(self, rec, mats, name, pts, times, md, kth=0):
        self.name, self.rec, self.mats = name, rec, mats
        self.kth = len(pts) if name == "mixed_kth" else kth
        self.ck = nr.FastChecker(rec, mats, pts, times, md)
        self.pts, self.times, self.md = self.ck.pts, self.ck.times, self.ck.md
        self.queries = rtow.make_point_queries(self.pts, self.times, self.md)
        self._ref8 = None

    @property
    def ref8(self):
        if self._ref8 is None:
            self._ref8 = nr.reference(self.rec, self.mats, self.pts, self.times, self.md, nr.MAX_NEAREST, self.ck.mirror)
        return self._ref8

    def check_kth(self, hits, counts, k, what):
        """mixed_kth, strict: the counts at d_j and at the double below it, straight from the unbounded list."""
        n = self.kth
        if not n:
            return
        if not hasattr(self, "free8"):
            self.free8 = nr.reference(self.rec, self.mats, self.pts[:n], self.times[:n], math.inf, nr.MAX_NEAREST,
                                      self.ck.mirror[:n])[0]["dist"]
        sel, md, counts = np.arange(n) % N_KTH, self.md[:n], counts[:n]
        for j in KTH:
            at, below = sel == kth_lanes(j, "at"), sel == kth_lanes(j, "below")
            dj = md[at][:, None]
            # j + 1 entries and the tie that follows, capped at k: everything of the sorted list that is <= d_j
            assert np.array_equal(counts[at], np.minimum(np.sum(self.free8[at] <= dj, axis=1), k)), (what, "at d", j)
            dj = np.nextafter(md[below], np.inf)[:, None]
            assert np.array_equal(counts[below], np.minimum(np.sum(self.free8[below] < dj, axis=1), k)), (what, "below d", j)


def add_stats(total, s):
    t = total if total else dict(s, queries=0, entries=0, short=0, overflow=0, exact_decisions=0)
    for f in ("worst_dist", "worst_surface", "worst_consistency"):
        t[f] = max(t[f], s[f])
    for f in ("queries", "entries", "short", "overflow"):
        t[f] += s[f]
    return t


def finish_stats(total, batches, prec):
    """exact_pairs and exact_decisions of a scene and build: the work done, each memoised verdict counted once."""
    total["exact_pairs"] = sum(len(b.ck._exact) for b in batches)
    total["exact_decisions"] = sum(n for b in batches for key, n in b.ck._complete.items() if key[1] == prec)
    return total


def coincident_two_materials():
    """(Geometry, stack size): the forty bit-identical triangles of `coincident` with materials alternating by insertion
    index, and twenty distinct triangles around them so that the builders make real leaves."""
    stack = ai.edge_meshes()["coincident"]
    return ai.mesh_geometry(np.concatenate([stack, ai.unit_mesh(20, 13)]), mats=GREY_AND_WHITE), len(stack)
