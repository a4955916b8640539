"""Closest-point queries, host side (no GPU): the entry points, the layouts, make_point_queries, and the numpy mirror of
the kernel's formulas (point_ref.py) against the exact distance on the hand-made scene, slivers, points on edges and
vertices, a sphere's centre and points inside the hollow glass."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import point_ref as pr
import rtow
from conftest import REPO
from test_gpu_query import SceneView, handmade_scene


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
