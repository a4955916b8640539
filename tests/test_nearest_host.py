"""k-nearest queries without a GPU: the exports and constants, the argument checks that need no device, the reference of
tests/nearest_ref.py against the closest-point mirror and its own definition, and the fast checker against corrupted
answers (it must reject each); and the exact checker on the point sets of test_gpu_exact_nearest.py with the strict
reference as the answer, at both taus, with one lane of a wave corrupted in each of the ways a wrong bound would.

Measured on one CPU core, the checker's wall time for both taus and k = 1, 3, 8 and its exact (query, primitive) pairs
(test_reference_meets_every_clause_on_the_exact_sets prints them); in brackets the closest-point checker on the same
scene's sets, one answer at one tau (test_point_query_host.py): handmade 6.4 s, 5357 pairs (0.9 s); cover_moving 7.8 s,
7831 (0.9 s); suzanne 11.6 s, 6913 (2.1 s); coincident_two_materials 4.8 s, 2089 (coincident: 1.5 s); the 96.8k mesh
12.6 s with its fixture, 1144.  Completeness decisions that went to Fractions: 142, 0, 12772, 2038 and 3924 — against
24748 / 3.3 M / 3.5 M / 132198 / 32.7 M decided by the box bound and 658 / 92436 / 49906 / 13090 / 1.19 M by the band."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import accel_images as ai
import nearest_cases as nc
import nearest_ref as nr
import point_cases as xp
import point_ref as pr
import rtow
from support_fixtures import big_mesh, logged  # noqa: F401
from support_oracle import same_bits
from support_scenes import SceneView, handmade_scene


def _geometry(name):
    return ai.mesh_geometry(ai.edge_meshes()[name]) if name in ai.edge_meshes() else ai.sphere_edge_scenes()[name]


def _points_around(rec, n, seed):
    return np.concatenate([pr.surface_points(rec, 0.0, seed), pr.random_points(rec, n, seed + 1)])


def test_symbols_constants_and_null_context():
    L = rtow.lib()
    for name in ("rtow_nearest_device", "rtow_nearest"):
        assert name in rtow.EXPORTS and hasattr(L, name)
    assert rtow.MAX_NEAREST == 8 == nr.MAX_NEAREST
    assert L.rtow_abi_version() == 9 == rtow.RTOW_ABI_VERSION
    header = (rtow.REPO_ROOT / "include" / "rtow.h").read_text()
    assert "#define RTOW_MAX_NEAREST 8" in header
    assert "int rtow_nearest_device(" in header and "int rtow_nearest(" in header
    q = rtow.make_point_queries([[0, 0, 0]])
    hits = np.zeros((1, 1), dtype=rtow.POINT_HIT_DTYPE)
    counts = np.zeros(1, dtype=np.int32)
    assert L.rtow_nearest(None, rtow.F64_STRICT, 0, q.ctypes.data_as(C.c_void_p), 1, 1, hits.ctypes.data_as(C.c_void_p),
                          counts.ctypes.data_as(C.c_void_p), None) == rtow.RTOW_EINVAL
    assert b"ctx" in L.rtow_last_error()
    assert L.rtow_nearest_device(None, rtow.F64_STRICT, 0, None, 0, 1, None, None, None, None) == rtow.RTOW_EINVAL
    assert nr.HIT_DTYPE == rtow.POINT_HIT_DTYPE


def test_first_entry_is_the_closest_point_mirror():
    """k = 1 is pr.nearest: dist bit for bit, prim the LOWEST tied insertion index, point that primitive's."""
    scene = handmade_scene()
    view = SceneView(scene)
    rec = pr.records(view)
    pts = _points_around(rec, 150, 3)
    for tm in (0.0, 0.5, 1.0):
        for md in (math.inf, 0.4):
            dmin, ties, _ = pr.nearest(rec, pts, tm, md)
            hits, counts = nr.reference(rec, view.prim_mat, pts, tm, md, 1)
            assert same_bits(hits["dist"][:, 0], dmin)
            assert np.array_equal(counts, np.isfinite(dmin).astype(np.int32))
            for i in np.nonzero(counts)[0]:
                assert hits["prim"][i, 0] == rec.cls2ins[ties[i]].min(), i
            # and the first entry of a longer list is the same record
            h8, _ = nr.reference(rec, view.prim_mat, pts, tm, md, 8)
            assert nr.same_answers(np.ascontiguousarray(h8[:, :1]), hits)
    assert set(np.unique(counts)) == {0, 1}


@pytest.mark.parametrize("name", ["coincident", "same_centre"])
def test_ties_come_in_insertion_order_under_a_permuted_insertion(name):
    G = _geometry(name)
    _, rec, mats = nr.permuted_records(G, 5)
    assert not np.array_equal(rec.cls2ins, np.arange(rec.n))
    pts = _points_around(rec, 60, 7)
    if name == "same_centre":  # midway between two shells, and the centre
        R = np.sqrt(np.abs(rec.sph[:, 3]))
        c = rec.sph[0, 0:3]
        pts = np.concatenate([pts, [c + [0.5 * (R[j] + R[j + 1]), 0, 0] for j in range(len(R) - 1)], [c]])
    hits, counts = nr.reference(rec, mats, pts, 0.0, math.inf, 8)
    tied = 0
    for i in range(len(pts)):
        d, p = hits["dist"][i, :counts[i]], hits["prim"][i, :counts[i]]
        assert np.all(np.diff(d) >= 0) and len(set(p)) == len(p), i
        eq = np.diff(d) == 0
        assert np.all(np.diff(p)[eq] > 0), (i, p)
        tied += int(eq.sum())
    assert tied > (100 if name == "coincident" else -1), tied  # (same_centre: the midpoints tie where rounding allows)
    if name == "coincident":  # forty copies: every list is the eight lowest insertion indices
        assert np.all(hits["prim"] == np.arange(8))
    # the reference is its own definition: the full sort of the mirror's matrix, cut at k
    for sl, D in pr.all_dists(rec, pts, 0.0):
        for j in range(D.shape[0]):
            order = sorted(range(rec.n), key=lambda c: (D[j, c], rec.cls2ins[c]))[:8]
            assert list(hits["prim"][sl.start + j]) == [rec.cls2ins[c] for c in order]


def test_counts_are_the_size_of_the_set_cut_at_k():
    G = _geometry("n4")
    rec = pr.make_records(G.sph, G.mov, G.tri)
    pts = _points_around(rec, 40, 9)
    hits, counts = nr.reference(rec, G.pmat, pts, 0.0, math.inf, 8)
    assert np.all(counts == 4)  # fewer primitives than k
    assert np.all(hits["prim"][:, 4:] == -1) and np.all(np.isinf(hits["dist"][:, 4:])) and np.all(hits["point"][:, 4:] == 0)
    assert np.all(np.sort(hits["prim"][:, :4], axis=1) == np.arange(4))
    # a radius between the second and third distances: two entries; NaN and negative: none
    d2, d3 = hits["dist"][:, 1], hits["dist"][:, 2]
    sel = d3 > d2
    md = np.where(sel, 0.5 * (d2 + d3), math.inf)
    h, c = nr.reference(rec, G.pmat, pts, 0.0, md, 8)
    assert np.all(c[sel] == 2) and nr.same_answers(np.ascontiguousarray(h[sel][:, :2]), np.ascontiguousarray(hits[sel][:, :2]))
    for bad in (math.nan, -1.0, -1e-300):
        h, c = nr.reference(rec, G.pmat, pts, 0.0, bad, 8)
        assert np.all(c == 0) and nr.same_answers(h, nr.miss_records(h.shape))
    # max_dist equal to the j-th distance is inclusive
    h, c = nr.reference(rec, G.pmat, pts, 0.0, d2, 8)
    assert np.all(c[sel] == 2)
    h, c = nr.reference(rec, G.pmat, pts, 0.0, np.nextafter(d2, -np.inf), 8)
    assert np.all(c[sel & (hits["dist"][:, 0] < d2)] == 1)


def _corrupt(hits, counts, rec, mats, pts, mirror, how):
    """A copy of the strict answer, wrong in one way, in every query that allows it; the number of queries changed."""
    h, c = hits.copy(), counts.copy()
    changed = 0
    for i in range(len(h)):
        n = int(c[i])
        if how == "swapped" and n >= 2 and h["dist"][i, 0] < h["dist"][i, n - 1]:
            h[i, [0, n - 1]] = h[i, [n - 1, 0]]
        elif how == "dropped" and n >= 3:
            h[i, 1:n - 1] = h[i, 2:n].copy()
            h[i, n - 1] = nr.miss_records(())
            c[i] = n - 1
        elif how == "duplicate" and n >= 2:
            h[i, 1] = h[i, 0]
        elif how == "farther" and n >= 1:
            # the farthest primitive of the scene, with its own correct record, in the last reported slot
            far = int(np.argmax(np.where(np.isfinite(mirror[i]), mirror[i], -1.0)))
            if rec.cls2ins[far] in h["prim"][i, :n] or mirror[i, far] < 1.5 * h["dist"][i, n - 1] + 1e-3:
                continue
            h[i, n - 1] = nr.records_of(rec, mats, pts[i:i + 1], 0.0, np.array([[far]]))[0, 0]
        elif how == "count" and n >= 1:
            c[i] = n - 1
        elif how == "past_count" and n < h.shape[1] and n >= 1:
            h[i, n] = h[i, n - 1]
            h["prim"][i, n] = -1  # (not a duplicate: a record that is neither a hit nor the miss record)
        else:
            continue
        changed += 1
    return h, c, changed


@pytest.mark.parametrize("how", ["swapped", "dropped", "duplicate", "farther", "count", "past_count"])
def test_fast_checker_accepts_the_mirror_and_rejects_corrupted_answers(how):
    G = ai.mesh_geometry(ai.unit_mesh(30, 21))
    rec = pr.make_records(G.sph, G.mov, G.tri)
    pts = pr.random_points(rec, 12, 23)
    k = 8
    md = 0.35 if how == "past_count" else math.inf  # (a radius: counts below k)
    ck = nr.FastChecker(rec, G.pmat, pts, 0.0, md)
    hits, counts = nr.reference(rec, G.pmat, pts, 0.0, md, k)
    s = ck.check(hits, counts, k, "mirror")  # the strict mirror meets the fast contract
    assert s["queries"] == len(pts) and s["worst_dist"] < 1.0
    if how == "past_count":
        assert np.any((counts >= 1) & (counts < k)), counts
    bad_h, bad_c, changed = _corrupt(hits, counts, rec, G.pmat, pts, ck.mirror, how)
    assert changed >= 3, (how, changed)
    with pytest.raises(AssertionError):
        ck.check(bad_h, bad_c, k, how)
    # and each corrupted query alone is rejected, not only the first one
    rejected = 0
    for i in range(len(pts)):
        if bad_h[i].tobytes() == hits[i].tobytes() and bad_c[i] == counts[i]:
            continue
        one = nr.FastChecker(rec, G.pmat, pts[i:i + 1], 0.0, md)
        with pytest.raises(AssertionError):
            one.check(bad_h[i:i + 1], bad_c[i:i + 1], k, how)
        rejected += 1
    assert rejected == changed


# ---- the exact checker on the point sets of test_gpu_exact_nearest.py, the strict reference as the answer ----
_KEEP = []
_CASES = {}


def _exact_case(name, logged, big_mesh=None):
    """(records, materials, batches) of a case of test_gpu_exact_nearest.py, built once."""
    if name not in _CASES:
        if name == "mesh96k":
            hs, view, log = big_mesh
            rec, mats = pr.records(view), view.prim_mat
            ps = xp.point_sets(rec, log, pr.SIZES_BIG["mixed"], 9)
            sets = nc.nearest_sets(rec, xp.SEED, ps["near"], ps["random"][0], sizes=pr.SIZES_BIG)
        elif name == "coincident_two_materials":
            G, _ = nc.coincident_two_materials()
            _, rec, mats = xp.geometry_case(G, _KEEP)
            sets = nc.nearest_sets(rec, xp.SEED)
        else:
            _, rec, mats, near, rnd = xp.small_case(name, logged, _KEEP)
            sets = nc.nearest_sets(rec, xp.SEED, near, rnd)
        _CASES[name] = rec, mats, [nc.Batch(rec, mats, *s) for s in sets]
    return _CASES[name]


@pytest.mark.parametrize("name", ["handmade", "cover_moving", "suzanne", "coincident_two_materials", "mesh96k"])
def test_reference_meets_every_clause_on_the_exact_sets(request, logged, name):
    """The strict reference alone stays inside every clause, at 32 u and at 64 u, for k = 1, 3 and 8 — mixed_kth, the far
    sets and the overflow sets included.  (Were it not so, the header's band would not cover a list entry the way it
    covers a minimum.)"""
    t0 = time.perf_counter()
    rec, mats, batches = _exact_case(name, logged, request.getfixturevalue("big_mesh") if name == "mesh96k" else None)
    for prec in ("strict", "fast"):
        total = None
        for b in batches:
            for k in nc.KS_FAST:
                hits, counts = nc.cut(b.ref8, k)
                total = nc.add_stats(total, b.ck.check(hits, counts, k, (name, b.name, prec, k), prec))
                b.check_kth(hits, counts, k, (name, k))
            if b.name.startswith("overflow"):
                assert np.all(np.isinf(b.ref8[0]["dist"][:, :min(rec.n, 8)])) and np.all(b.ref8[1] == min(rec.n, 8))
        nc.finish_stats(total, batches, prec)
        print(f"\nnearest {name} {prec}: {sum(len(b.pts) for b in batches)} points in {len(batches)} sets; answers: "
              f"{nr.stats_line(total)}")
        assert total["overflow"] > 0 and total["short"] > 0
        assert total["worst_dist"] < 1.0 and total["worst_surface"] < 1.0 and total["worst_consistency"] < 1.0
    decided = {w: sum(b.ck.decided[w] for b in batches) for w in ("box", "band", "exact")}
    print(f"nearest {name}: checker {time.perf_counter() - t0:.1f} s; completeness decided by the box {decided['box']}, by "
          f"the band {decided['band']}, by exact arithmetic {decided['exact']}")
    assert decided["band"] > 0  # (the far sets: every primitive within one band of every other)


def test_mixed_kth_holds_every_value_in_every_wave(logged):
    rec, mats, batches = _exact_case("cover_moving", logged)
    b = next(b for b in batches if b.name == "mixed_kth")
    n = len(b.pts)
    assert n == pr.SIZES["mixed"] and n % 64
    sel = np.arange(n) % nc.N_KTH
    for w0 in range(0, n - 63, 64):
        w = slice(w0, w0 + 64)
        kinds = {(int(s), 0 if t == 0.0 else 1 if t == 1.0 else 2) for s, t in zip(sel[w], b.times[w])}
        assert len(kinds) == 3 * nc.N_KTH, (w0, len(kinds))
    assert np.all(np.isnan(b.md[sel == 0])) and np.all(b.md[sel == 1] == -1.0) and np.all(np.isinf(b.md[sel == 2]))
    hits, counts = b.ref8
    free = nr.reference(rec, mats, b.pts, b.times, math.inf, 8)[0]["dist"]
    for j in nc.KTH:
        at, below, half = (sel == nc.kth_lanes(j, w) for w in ("at", "below", "half"))
        assert same_bits(b.md[at], np.ascontiguousarray(free[at, j]))  # d_j itself
        assert np.all(counts[at] >= j + 1) and np.all(counts[below] <= j) and np.all(counts[half] <= j)
        assert np.all(b.md[below] < free[below, j]) and np.all(b.md[half] == 0.5 * free[half, j])
    assert np.all(counts[sel <= 1] == 0)


def _one_lane(b, want):
    """The first query of a batch for which want(i, hits[i], count) holds."""
    hits, counts = b.ref8
    return next(i for i in range(len(b.pts)) if want(i, hits[i], int(counts[i])))


def _rejects(b, i, hits, counts, why, k=8):
    """The whole batch with lane i corrupted is rejected at both taus, naming that query; untouched it passes."""
    good = nc.cut(b.ref8, k)
    assert np.sum(np.any(hits.view(np.uint8).reshape(len(hits), -1) != good[0].view(np.uint8).reshape(len(hits), -1), axis=1)
                  | (counts != good[1])) == 1
    for prec in ("strict", "fast"):
        b.ck.check(good[0], good[1], k, "reference", prec)
        with pytest.raises(AssertionError, match=rf"query {i} .*{why}"):
            b.ck.check(hits, counts, k, "corrupted", prec)


def test_checker_rejects_one_corrupted_lane_of_a_wave(logged):
    rec, mats, batches = _exact_case("cover_moving", logged)
    by_name = {b.name: b for b in batches}
    kth, rnd = by_name["mixed_kth"], by_name["random@0.5"]
    assert len(kth.pts) > 64 and len(rnd.pts) > 64
    sel = np.arange(len(kth.pts)) % nc.N_KTH

    def free(i):  # the unbounded list of lane i of mixed_kth
        return nr.reference(rec, mats, kth.pts[i:i + 1], kth.times[i:i + 1], math.inf, 8)[0][0]

    # entry j replaced by the next primitives: the list without entry j, closed up, the ninth nearest at its end
    i = _one_lane(rnd, lambda i, h, n: n == 8 and h["dist"][3] < 0.9 * h["dist"][7])
    order = np.argsort(rnd.ck.mirror[i], kind="stable")
    assert rnd.ck.mirror[i][order[8]] > rnd.ck.mirror[i][order[7]]
    hits, counts = (a.copy() for a in rnd.ref8)
    hits[i, 3:7] = hits[i, 4:8].copy()
    hits[i, 7] = nr.records_of(rec, mats, rnd.pts[i:i + 1], rnd.times[i:i + 1], np.array([[order[8]]]))[0, 0]
    _rejects(rnd, i, hits, counts, "a nearer primitive is left out")

    # a primitive dropped inside max_dist in a mixed_kth lane (max_dist = d_7: the nearest one is well inside)
    i = _one_lane(kth, lambda i, h, n: sel[i] == nc.kth_lanes(7, "at") and n == 8 and h["dist"][0] < 0.9 * h["dist"][7])
    hits, counts = (a.copy() for a in kth.ref8)
    hits[i, 0:7] = hits[i, 1:8].copy()
    hits[i, 7] = nr.miss_records(())
    counts[i] = 7
    _rejects(kth, i, hits, counts, "a nearer primitive is left out")

    # an entry kept above max_dist (max_dist = d_3 / 2 with the unbounded list's first four entries: its neighbour's radius)
    i = _one_lane(kth, lambda i, h, n: sel[i] == nc.kth_lanes(3, "half") and n < 4)
    hits, counts = (a.copy() for a in kth.ref8)
    hits[i, :4], counts[i] = free(i)[:4], 4
    _rejects(kth, i, hits, counts, "dist above max_dist")

    # a list under a NaN radius that is not all miss records
    i = _one_lane(kth, lambda i, h, n: sel[i] == 0)
    hits, counts = (a.copy() for a in kth.ref8)
    hits[i, 0] = free(i)[0]
    _rejects(kth, i, hits, counts, "a miss record|not the miss record|entries under a NaN")
    hits, counts = (a.copy() for a in kth.ref8)
    hits[i, 0], counts[i] = free(i)[0], 1
    _rejects(kth, i, hits, counts, "entries under a NaN")


def test_checker_rejects_swapped_ties_and_a_twin_s_material(logged):
    rec, mats, batches = _exact_case("coincident_two_materials", logged)
    b = next(b for b in batches if b.name == "random@0")
    assert len(b.pts) > 64
    # the stack of forty coincident triangles is nearest somewhere: a list that is one tie, in insertion order
    i = _one_lane(b, lambda i, h, n: n == 8 and h["dist"][0] == h["dist"][1] and h["prim"][1] == h["prim"][0] + 1)
    hits, counts = (a.copy() for a in b.ref8)
    assert mats[hits["prim"][i, 0]] != mats[hits["prim"][i, 1]]
    hits[i, [0, 1]] = hits[i, [1, 0]]
    _rejects(b, i, hits, counts, "a tie out of insertion order")
    hits, counts = (a.copy() for a in b.ref8)
    hits["material"][i, 0] = hits["material"][i, 1]  # the record of entry 0 with its twin's material
    _rejects(b, i, hits, counts, "material is not the primitive's")


def test_checker_takes_the_overflow_rule_and_holds_it(logged):
    rec, mats, batches = _exact_case("suzanne", logged)
    b = next(b for b in batches if b.name.startswith("overflow"))
    hits, counts = b.ref8
    assert np.all(np.isinf(hits["dist"])) and np.all(hits["prim"] == np.arange(8))  # ties at +inf: insertion order
    s = b.ck.check(hits, counts, 8, "overflow", "fast")
    assert s["overflow"] == len(b.pts) and s["exact_decisions"] == 0
    bad = hits.copy()
    bad[2, [3, 4]] = bad[2, [4, 3]]
    with pytest.raises(AssertionError, match="query 2 .*a tie out of insertion order"):
        b.ck.check(bad, counts, 8, "swapped", "fast")
    # +inf is no licence on a query whose distances are finite
    r = next(b for b in batches if b.name == "random@0")
    bad = r.ref8[0].copy()
    bad["dist"][5, 7] = np.inf
    with pytest.raises(AssertionError, match="query 5 .*dist outside its band"):
        r.ck.check(bad, r.ref8[1], 8, "inf", "fast")
