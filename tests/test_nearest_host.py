"""k-nearest queries without a GPU: the exports and constants, the argument checks that need no device, the reference of
tests/nearest_ref.py against the closest-point mirror and its own definition, and the fast checker against corrupted
answers (it must reject each)."""
import ctypes as C
import math

import numpy as np
import pytest

import accel_images as ai
import nearest_ref as nr
import point_ref as pr
import rtow
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
