"""Closest-point queries, host side (no GPU): the entry points, the layouts, make_point_queries, and the numpy mirror of
the kernel's formulas (point_ref.py) against the exact distance on the hand-made scene, slivers, points on edges and
vertices, a sphere's centre and points inside the hollow glass; and the checker of whole answers
(point_ref.check_answers) on the mirror's answers for every scene and point set of test_gpu_exact_points.py, on a
perturbed mirror at the fast tau, and on corrupted answers, each of which it must reject."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import accel_images as ai
import point_ref as pr
import rtow
import point_cases as xp
from conftest import REPO
from support_oracle import LOGGED, log_rays
from support_scenes import SceneView, handmade_scene, motions


def test_point_query_symbols_are_exported_and_declared():
    L = rtow.lib()
    header = (REPO / "include" / "rtow.h").read_text()
    for name in ("rtow_closest_point", "rtow_closest_point_device"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert rtow.lib().rtow_abi_version() == 9


def test_null_context_is_einval():
    L = rtow.lib()
    q = rtow.make_point_queries([[0, 0, 0]])
    out = np.zeros(1, dtype=rtow.POINT_HIT_DTYPE)
    out["dist"] = 7.0
    rc = L.rtow_closest_point(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, q.ctypes.data_as(C.c_void_p), 1,
                              out.ctypes.data_as(C.c_void_p), None)
    assert rc == rtow.RTOW_EINVAL
    assert b"NULL" in L.rtow_last_error()
    assert out["dist"][0] == 7.0
    rc = L.rtow_closest_point_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, None, 0, None, None, None)
    assert rc == rtow.RTOW_EINVAL


def test_layouts_match_the_header():
    assert C.sizeof(rtow.PointQuery) == 48 and C.sizeof(rtow.PointHit) == 48
    assert rtow.POINT_QUERY_DTYPE.itemsize == 48 and rtow.POINT_HIT_DTYPE.itemsize == 48
    want_q = {"point": 0, "time": 24, "max_dist": 32, "pad_": 40}
    want_h = {"dist": 0, "point": 8, "prim": 32, "kind": 36, "material": 40, "pad_": 44}
    for name, off in want_q.items():
        assert getattr(rtow.PointQuery, name).offset == off and rtow.POINT_QUERY_DTYPE.fields[name][1] == off
    for name, off in want_h.items():
        assert getattr(rtow.PointHit, name).offset == off and rtow.POINT_HIT_DTYPE.fields[name][1] == off


def test_make_point_queries_fills_every_field():
    q = rtow.make_point_queries([[1, 2, 3], [4, 5, 6]], time=[0.25, 0.5], max_dist=2.5)
    assert np.array_equal(q["point"], [[1, 2, 3], [4, 5, 6]])
    assert np.array_equal(q["time"], [0.25, 0.5])
    assert np.array_equal(q["max_dist"], [2.5, 2.5])
    assert np.array_equal(q["pad_"], [0.0, 0.0])
    q = rtow.make_point_queries(np.zeros((3, 3)))
    assert np.all(q["time"] == 0.0) and np.all(np.isinf(q["max_dist"]))


def _check_mirror_against_exact(rec, pts, times, prec="strict"):
    """Every (point, primitive): the mirror's distance within the stated band of the exact one, finite, never NaN."""
    checked = 0
    for i, (p, tm) in enumerate(zip(pts, times)):
        d, q = pr.prim_point(rec, np.arange(rec.n), np.repeat(p[None], rec.n, 0), tm)
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)), (i, p)
        for cid in range(rec.n):
            D, err = pr.exact_dist(rec, cid, p, tm)
            lo, hi = pr.bound(rec, cid, p, tm, prec)
            assert pr.within(d[cid], D, err, lo, hi), (i, p.tolist(), cid, d[cid], float(D), lo, hi)
            checked += 1
    return checked


def test_mirror_against_exact_on_the_handmade_scene():
    view = SceneView(handmade_scene())
    rec = pr.records(view)
    g = np.random.default_rng(3)
    pts = [g.uniform([-5, -1, -4], [5, 4, 3]) for _ in range(40)]
    # on edges, vertices and faces of the triangles, the sphere centres, inside the hollow glass, on the spheres
    for t in view.tri:
        A, B, Cc = t[0:3], t[3:6], t[6:9]
        pts += [A, B, Cc, 0.5 * (A + B), 0.3 * B + 0.7 * Cc, (A + B + Cc) / 3, (A + B + Cc) / 3 + [0, 0, 0.7]]
    for s in view.sph:
        if abs(s[3]) < 100:
            pts += [s[0:3], s[0:3] + [0, 0.9 * abs(s[3]), 0], s[0:3] + [abs(s[3]), 0, 0]]
    pts.append(np.array([0.0, 1.0, 0.85]))  # between the glass sphere (r 1) and its hollow (r -0.8)
    pts = np.array(pts, dtype=np.float64)
    times = np.concatenate([np.zeros(len(pts) - 6), [0.0, 0.5, 1.0, 0.25, 0.75, 1.0]])
    assert _check_mirror_against_exact(rec, pts, times) > 400


def test_mirror_on_slivers_and_degenerate_triangles():
    tri = np.array([
        [0, 0, 0, 1, 0, 0, 2, 0, 0],            # collinear: zero area
        [0, 0, 0, 0, 0, 0, 0, 0, 0],            # a point
        [0, 0, 0, 1, 0, 0, 1, 0, 0],            # two equal vertices
        [0, 0, 0, 1, 1e-9, 0, 2, 2e-9 + 1e-17, 0],  # a sliver
        [0, 0, 0, 1e3, 0, 0, 0, 1e-7, 1e-9],    # long and thin
        [1, 1, 1, 1 + 1e-12, 1, 1, 1, 1 + 1e-12, 1],  # tiny
    ], dtype=np.float64)
    rec = pr.make_records(np.zeros((0, 4)), np.zeros((0, 8)), tri)
    g = np.random.default_rng(11)
    pts = list(g.normal(size=(30, 3)) * 2) + [[0.5, 0, 0], [2, 0, 0], [1, 1e-9, 0], [500, 0, 0], [1, 1, 1], [0, 0, 0]]
    pts = np.array(pts, dtype=np.float64)
    _check_mirror_against_exact(rec, pts, np.zeros(len(pts)))
    # a degenerate triangle answers as its edges do: the collinear one is the segment [0, 2] on x
    d, q = pr.prim_point(rec, np.zeros(len(pts), dtype=np.int64), pts, 0.0)
    seg = np.hypot(np.hypot(pts[:, 0] - np.clip(pts[:, 0], 0, 2), pts[:, 1]), pts[:, 2])
    assert np.allclose(d, seg, rtol=1e-14, atol=1e-15)


def test_sphere_centre_and_max_dist_semantics_of_the_mirror():
    rec = pr.make_records(np.array([[1.0, 2.0, 3.0, -0.5]]), np.zeros((0, 8)), np.zeros((0, 9)))
    d, q = pr.prim_point(rec, np.array([0]), np.array([[1.0, 2.0, 3.0]]), 0.0)
    assert d[0] == 0.5 and np.array_equal(q[0], [1.5, 2.0, 3.0])
    p = np.array([[4.0, 2.0, 3.0]] * 4)
    dmin, ties, arg = pr.nearest(rec, p, 0.0, [2.5, np.nextafter(2.5, 0), math.nan, -1.0])
    assert dmin[0] == 2.5 and arg[0] == 0
    assert np.all(np.isinf(dmin[1:])) and np.all(arg[1:] == -1)


def test_fast_bound_holds_for_the_mirror_with_perturbed_arithmetic():
    """The fast band is twice the strict one: a mirror whose every distance is off by 8 u S (far more than a contraction
    moves it) still lies inside it on the hand-made scene."""
    view = SceneView(handmade_scene())
    rec = pr.records(view)
    p = np.array([0.2, 0.4, -1.0])
    for cid in range(rec.n):
        D, err = pr.exact_dist(rec, cid, p, 0.0)
        lo_s, hi_s = pr.bound(rec, cid, p, 0.0, "strict")
        lo_f, hi_f = pr.bound(rec, cid, p, 0.0, "fast")
        assert lo_f >= 2 * lo_s * 0.99 and hi_f >= lo_f
        d, _ = pr.prim_point(rec, np.array([cid]), p[None], 0.0)
        assert pr.within(d[0] + 0.25 * lo_f, D, err, lo_f, hi_f)


@pytest.mark.parametrize("prec", ["strict", "fast"])
def test_bound_is_finite_for_well_shaped_triangles(prec):
    rec = pr.make_records(np.zeros((0, 4)), np.zeros((0, 8)), np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0.0]]))
    lo, hi = pr.bound(rec, 0, np.array([0.2, 0.2, 1.0]), 0.0, prec)
    assert 0 < lo <= hi < 1e-13


# ---- the checker of whole answers (point_ref.check_answers) on the scenes and point sets of test_gpu_exact_points.py ----
class _Logged(dict):
    """support_fixtures' `logged` fixture, one scene at a time (the oracle renders on the CPU)."""

    def __missing__(self, name):
        mk, w, h, spp, depth, seed = LOGGED[name]
        scene = mk()
        cfg = rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        self[name] = (scene, SceneView(scene), log_rays(scene, cfg))
        return self[name]


_LOGGED = _Logged()
_KEEP = []


@functools.lru_cache(maxsize=None)
def _case(name):
    """(records, materials, point sets) of a case of test_gpu_exact_points.py: a small scene, or `scene/motion`."""
    if "/" in name:
        scene, motion = name.split("/")
        H = motions(ai.Geometry.of_scene(_LOGGED[scene][0].c))[motion][0]
        _, rec, mats = xp.geometry_case(H, _KEEP)
        return rec, mats, pr.all_sets(rec, xp.SEED, refit=True)
    _, rec, mats, near, rnd = xp.small_case(name, _LOGGED, _KEEP)
    return rec, mats, pr.all_sets(rec, xp.SEED, near, rnd)


SMALL_CASES = ["handmade"] + list(LOGGED) + xp.EDGE_MESHES + xp.SPHERE_SCENES + [f"{n}/{m}" for n, m in xp.REFITS]


@pytest.mark.parametrize("name", SMALL_CASES)
def test_checker_accepts_the_mirror_on_every_point_set(name):
    """The mirror's own answers pass at the strict tau, far inside every band (the figures are printed)."""
    rec, mats, sets = _case(name)
    for sname, pts, times, md in sets:
        s = pr.check_answers(rec, mats, pts, times, md, pr.mirror_answers(rec, mats, pts, times, md), "strict", (name, sname))
        print(f"{name}/{sname}: {pr.stats_line(s)}")
        assert s["overflow"] == (len(pts) if sname.startswith("overflow") else 0)
        assert s["open"] == 0 or sname == "mixed_strict"  # (max_dist = d_min and the double below it: the band's)


def _scales(rec, c, p, tm):
    """(S, S_q) of primitive c at p as floats."""
    geom = pr.exact_geometry(rec, c, tm)
    return float(pr.header_scale(geom, p)), float(geom[1])


@pytest.mark.parametrize("name", ["handmade", "cover_moving", "suzanne", "zero_area", "far_moving", "suzanne/scale1000"])
def test_checker_accepts_a_perturbed_mirror_at_the_fast_tau(name):
    """dist off by 8 u S and point off by 8 u S_q in a random direction, on every answer: inside the fast clauses."""
    rec, mats, sets = _case(name)
    g = np.random.default_rng(5)
    for sname, pts, times, md in sets:
        if sname == "mixed_strict":
            continue  # (max_dist equal to the distance: values for the mirror to decide)
        h = pr.mirror_answers(rec, mats, pts, times, md)
        tms = np.broadcast_to(np.asarray(times, dtype=np.float64), (len(pts),))
        for i in np.nonzero((h["prim"] >= 0) & np.isfinite(h["dist"]))[0]:
            S, Sq = _scales(rec, int(rec.ins2cls[h["prim"][i]]), pts[i], tms[i])
            d = g.normal(size=3)
            h["point"][i] += 8 * pr.U * Sq * d / np.linalg.norm(d)
            h["dist"][i] = abs(h["dist"][i] + g.choice([-8, 8]) * pr.U * S)
        s = pr.check_answers(rec, mats, pts, times, md, h, "fast", (name, sname))
        # (the perturbation is there: some direction has 0.4 of its length along the normal, 8 u x 0.4 / 64 u = 0.05)
        assert s["worst_surface"] > 0.04 or sname.startswith("overflow"), (name, sname, s)


def _one(name, sname, pick):
    """(records, materials, point, time, max_dist, the mirror's answer) of one query of a set: pick(answers) -> index."""
    rec, mats, sets = _case(name)
    _, pts, times, md = next(s for s in sets if s[0] == sname)
    h = pr.mirror_answers(rec, mats, pts, times, md)
    i = pick(h)
    tm = np.broadcast_to(np.asarray(times, dtype=np.float64), (len(pts),))[i]
    m = np.broadcast_to(np.asarray(md, dtype=np.float64), (len(pts),))[i]
    return rec, mats, pts[i:i + 1], tm, m, h[i:i + 1].copy()


def _rejected(case, h, prec, why):
    rec, mats, p, tm, md = case[:5]
    with pytest.raises(AssertionError, match=why):
        pr.check_answers(rec, mats, p, tm, md, h, prec)


@pytest.mark.parametrize("prec", ["strict", "fast"])
@pytest.mark.parametrize("name,sname", [("suzanne", "random@0"), ("cover_moving", "random@0.5"), ("suzanne", "far@0")])
def test_checker_rejects_a_distance_three_bands_off(name, sname, prec):
    case = _one(name, sname, lambda h: 17)
    rec, mats, p, tm, md, h = case
    pr.check_answers(rec, mats, p, tm, md, h, prec)
    lo, hi = pr.bound(rec, int(rec.ins2cls[h["prim"][0]]), p[0], tm, prec)
    for delta in (3 * hi, -3 * lo):
        bad = h.copy()
        bad["dist"] += delta
        _rejected(case, bad, prec, "dist outside its band")


def _face_query():
    """The query 0.01 above the centroid of the first sampled triangle of suzanne's surface set: the plane candidate."""
    return _one("suzanne", "surface@0", lambda h: 8)


@pytest.mark.parametrize("prec", ["strict", "fast"])
def test_checker_rejects_a_point_off_the_surface(prec):
    case = _face_query()
    rec, mats, p, tm, md, h = case
    pr.check_answers(rec, mats, p, tm, md, h, prec)
    c = int(rec.ins2cls[h["prim"][0]])
    n = rec.tri[c - rec.ns - rec.nm, 9:12]
    bad = h.copy()
    bad["point"] += 3 * pr.TAU[prec] * _scales(rec, c, p[0], tm)[1] * n / np.linalg.norm(n)
    _rejected(case, bad, prec, "point off the surface")
    # and a moving sphere's: the answer to a point off it, moved towards the query point
    case = _one("cover_moving", "surface@0.5", lambda h: np.nonzero((h["kind"] == pr.MOVING) & (h["dist"] > 1e-3))[0][0])
    rec, mats, p, tm, md, h = case
    c = int(rec.ins2cls[h["prim"][0]])
    assert c < rec.ns + rec.nm
    pr.check_answers(rec, mats, p, tm, md, h, prec)
    bad = h.copy()
    d = p[0] - h["point"][0]
    bad["point"] += 3 * pr.TAU[prec] * _scales(rec, c, p[0], tm)[1] * d / np.linalg.norm(d)
    _rejected(case, bad, prec, "point off the surface")


def test_checker_rejects_another_feasible_point_of_the_same_triangle():
    """The right distance with the wrong edge's projection (here a vertex): on the surface, but |p - q| is not dist."""
    case = _face_query()
    rec, mats, p, tm, md, h = case
    t = rec.tri[int(rec.ins2cls[h["prim"][0]]) - rec.ns - rec.nm]
    for q in (t[0:3], t[0:3] + t[3:6], t[0:3] + 0.5 * t[6:9]):
        bad = h.copy()
        bad["point"][0] = q
        _rejected(case, bad, "fast", "differs from dist")


def test_checker_rejects_a_primitive_farther_than_the_bands():
    for name, sname in (("suzanne", "random@0"), ("cover_moving", "near@1"), ("coincident", "far@0"), ("suzanne", "far@0")):
        case = _one(name, sname, lambda h: 5)
        rec, mats, p, tm, md, h = case
        d_all = next(pr.all_dists(rec, p, tm))[1][0]
        far = np.nonzero(d_all > d_all.min() * (1 + 1e-9) + 1e-9)[0]
        if name == "coincident":
            assert len(far) == 0  # (forty copies of one triangle: each of them is an answer)
            for c2 in (0, 39):
                pr.check_answers(rec, mats, p, tm, md, pr.mirror_answers(rec, mats, p, tm, md, of=[c2]), "strict")
            continue
        c2 = far[np.argmin(d_all[far])]  # the second nearest: consistent in itself, and not the nearest
        case = case[:4] + (np.inf,)
        _rejected(case,pr.mirror_answers(rec, mats, p, tm, np.inf, of=[c2]), "fast", "nearer by more than the bands")


def test_checker_rejects_kind_and_material_of_another_primitive():
    case = _one("cover_moving", "near@0", lambda h: 3)
    rec, mats, p, tm, md, h = case
    bad = h.copy()
    bad["kind"] = (h["kind"] + 1) % 3
    _rejected(case, bad, "fast", "kind is not the primitive's")
    other = next(m for m in mats if m != h["material"][0])
    bad = h.copy()
    bad["material"] = other
    _rejected(case, bad, "fast", "material is not the primitive's")
    bad = h.copy()
    bad["prim"] = rec.n
    _rejected(case, bad, "fast", "prim out of range")


def test_checker_rejects_a_hit_on_a_decided_miss_and_the_reverse():
    rec, mats, sets = _case("cover_moving")
    _, pts, times, md = next(s for s in sets if s[0] == "mixed")
    free = pr.mirror_answers(rec, mats, pts, times, np.inf)
    miss = pr.mirror_answers(rec, mats, pts, times, -1.0)
    assert np.all(miss["prim"] == -1)
    seen = set()
    for i in range(15):  # one of each (time, max_dist) pair
        case = (rec, mats, pts[i:i + 1], times[i], md[i])
        if np.isnan(md[i]) or md[i] < 0:
            _rejected(case, free[i:i + 1], "fast", "a hit under a NaN or negative max_dist")
            seen.add("none")
        elif md[i] < free["dist"][i]:
            _rejected(case, free[i:i + 1], "fast", "dist above max_dist")
            bad = free[i:i + 1].copy()
            bad["dist"] = md[i]  # (a hit that claims to be inside: not this primitive's distance)
            _rejected(case, bad, "fast", "dist outside its band")
            seen.add("half")
        else:
            _rejected(case, miss[i:i + 1], "fast", "a miss, but a primitive is within max_dist|a miss with max_dist = \\+inf")
            seen.add("twice" if np.isfinite(md[i]) else "inf")
    assert seen == {"none", "half", "twice", "inf"}


def test_checker_rejects_nan_and_a_nonzero_point_on_a_miss():
    case = _one("cover_moving", "near@0", lambda h: 3)
    rec, mats, p, tm, md, h = case
    for f, k in (("dist", None), ("point", 0), ("point", 2)):
        bad = h.copy()
        if k is None:
            bad[f] = np.nan
        else:
            bad[f][0, k] = np.nan
        _rejected(case, bad, "fast", "NaN in the answer")
    bad = h.copy()
    bad["point"][0, 1] = np.inf
    _rejected(case, bad, "fast", "point is not finite")
    case = case[:4] + (0.5 * h["dist"][0],)
    miss = pr.mirror_answers(rec, mats, p, tm, case[4])
    pr.check_answers(rec, mats, p, tm, case[4], miss, "fast")
    for f, v in (("point", [0.0, 1e-300, 0.0]), ("dist", 1e300), ("kind", 0), ("material", 0)):
        bad = miss.copy()
        bad[f][0] = v
        _rejected(case, bad, "fast", "not the miss record|NaN")
    bad = miss.copy()
    bad["dist"] = np.nan
    _rejected(case, bad, "fast", "NaN in the answer")
