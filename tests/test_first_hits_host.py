"""First-k-hits queries without a GPU: the exports and constants, the argument checks that need no device, and the
reference of tests/first_hits_ref.py — its vectorised form pinned bit for bit to the oracle's two hit tests, and its
first entry to the closest-hit brute force of tests/support_oracle.py."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

import first_hits_ref as fr
import orc
import rtow
from support_oracle import brute_force
from support_scenes import SceneView, handmade_rays, handmade_scene

PAIRS = 10_000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_constants_and_null_context():
    L = rtow.lib()
    for name in ("rtow_first_hits_device", "rtow_first_hits"):
        assert name in rtow.EXPORTS and hasattr(L, name)
    assert rtow.MAX_HITS == 8
    assert L.rtow_abi_version() == 9 == rtow.RTOW_ABI_VERSION
    header = (rtow.REPO_ROOT / "include" / "rtow.h").read_text()
    assert "#define RTOW_MAX_HITS 8" in header
    rays = rtow.make_rays([[0, 0, 0]], [[0, 0, 1]])
    hits = np.zeros((1, 1), dtype=rtow.HIT_DTYPE)
    counts = np.zeros(1, dtype=np.int32)
    assert L.rtow_first_hits(None, rtow.F64_STRICT, 0, rays.ctypes.data_as(C.c_void_p), 1, 1,
                             hits.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), None) == rtow.RTOW_EINVAL
    assert b"ctx" in L.rtow_last_error()
    assert L.rtow_first_hits_device(None, rtow.F64_STRICT, 0, None, 0, 1, None, None, None, None) == rtow.RTOW_EINVAL


def _oracle_sphere(c, r, o, d, tmax):
    L = orc.lib()
    t, f = C.c_double(), C.c_int()
    p, n = (C.c_double * 3)(), (C.c_double * 3)()
    ok = L.orc_sphere_hit((C.c_double * 3)(*c), float(r), (C.c_double * 3)(*o), (C.c_double * 3)(*d), fr.TMIN, float(tmax),
                          C.byref(t), p, n, C.byref(f))
    return (t.value, np.array(p[:]), np.array(n[:]), f.value) if ok else None


def _oracle_triangle(g, o, d, tmax):
    L = orc.lib()
    t = C.c_double()
    p, n = (C.c_double * 3)(), (C.c_double * 3)()
    ok = L.orc_triangle_hit((C.c_double * 3)(*g[0:3]), (C.c_double * 3)(*g[3:6]), (C.c_double * 3)(*g[6:9]),
                            (C.c_double * 3)(*o), (C.c_double * 3)(*d), fr.TMIN, float(tmax), C.byref(t), p, n)
    return (t.value, np.array(p[:]), np.array(n[:])) if ok else None


def _view(sph=None, mov=None, tri=None, kind=None):
    """What fr.records reads of a SceneView, for seeded primitives: pair j's primitive is inserted at position j."""
    kind = np.asarray(kind, dtype=np.int32)
    index = np.zeros(len(kind), dtype=np.int32)
    for k in (rtow.PRIM_SPHERE, rtow.PRIM_MOVING_SPHERE, rtow.PRIM_TRIANGLE):
        index[kind == k] = np.arange(int((kind == k).sum()))
    z = np.zeros((0, 1))
    return SimpleNamespace(sph=z if sph is None else sph, mov=z if mov is None else mov, tri=z if tri is None else tri,
                           kind=kind, index=index, prim_mat=np.arange(len(kind), dtype=np.int32) % 3)


def _record(view, o, d, time, j, t):
    """fr.records — the code the reference builds its hit records with — for pair j accepted at t."""
    ray = rtow.make_rays([o], [d], time=time)[0]
    rec = fr.records(view, ray, np.array([j]), np.array([t]))[0]
    assert rec["prim"] == j and rec["kind"] == view.kind[j] and rec["material"] == view.prim_mat[j]
    return rec


def _tmax(g, n):
    """inf for half the pairs, else a seeded finite bound of the order of the scene."""
    return np.where(g.random(n) < 0.5, math.inf, 8.0 * g.random(n))


def test_vectorised_sphere_test_is_the_oracles_bit_for_bit():
    """10,000 seeded (ray, sphere) pairs: rays aimed at the sphere from outside, rays from inside it, rays that miss,
    axis-parallel rays with -0.0 components; positive and negative radii; centres moved as a moving sphere's are."""
    g = np.random.default_rng(101)
    c = g.uniform(-3, 3, (PAIRS, 3))
    r = g.uniform(0.2, 2.0, PAIRS) * np.where(g.random(PAIRS) < 0.4, -1.0, 1.0)
    mode = g.integers(0, 4, PAIRS)
    u = g.normal(size=(PAIRS, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = np.where((mode == 1)[:, None], c + u * (np.abs(r) * g.random(PAIRS))[:, None],  # inside
                 c + u * (np.abs(r) * g.uniform(1.5, 6.0, PAIRS))[:, None])
    d = np.where((mode == 2)[:, None], g.normal(size=(PAIRS, 3)),  # anywhere: mostly misses
                 (c + np.abs(r)[:, None] * g.uniform(-0.9, 0.9, (PAIRS, 3))) - o + 0.0)
    ax = mode == 3
    d[ax] = -np.eye(3)[g.integers(0, 3, int(ax.sum()))]  # (-1 * e: the zero components are -0.0)
    # half the centres go through the moving-sphere formula first
    mv = np.concatenate([c, c + g.normal(size=(PAIRS, 3)), r[:, None], np.zeros((PAIRS, 1))], axis=1)
    time = g.random(PAIRS)
    moved = g.random(PAIRS) < 0.5
    c = np.where(moved[:, None], fr.moving_centre(mv, time), c)
    # the scene fr.records sees: pair j's sphere at insertion position j, static (its centre and radius) or moving (mv)
    view = _view(sph=np.concatenate([c, r[:, None]], axis=1)[~moved], mov=mv[moved],
                 kind=np.where(moved, rtow.PRIM_MOVING_SPHERE, rtow.PRIM_SPHERE))
    tmax = _tmax(g, PAIRS)
    ok, t = fr.sphere_t(c, r, o, d, fr.TMIN, tmax)
    p, n, front = fr.sphere_record(c, r, o, d, t)
    seen = {"hit": 0, "inside": 0, "negative": 0, "miss": 0}
    for j in range(PAIRS):
        want = _oracle_sphere(c[j], r[j], o[j], d[j], tmax[j])
        assert bool(ok[j]) == (want is not None), j
        if want is None:
            seen["miss"] += 1
            continue
        seen["hit"] += 1
        seen["inside"] += mode[j] == 1
        seen["negative"] += r[j] < 0
        assert bits(t[j]) == bits(want[0]) and np.array_equal(bits(p[j]), bits(want[1])), j
        assert np.array_equal(bits(n[j]), bits(want[2])) and front[j] == want[3], j
        rec = _record(view, o[j], d[j], time[j], j, t[j])
        assert bits(rec["t"]) == bits(want[0]) and np.array_equal(bits(rec["point"]), bits(want[1])), j
        assert np.array_equal(bits(rec["normal"]), bits(want[2])) and rec["front_face"] == want[3], j
    assert min(seen.values()) > 500, seen


def test_vectorised_triangle_test_is_the_oracles_bit_for_bit():
    """10,000 seeded (ray, triangle) pairs: rays through the triangle from both sides, rays in its plane, rays whose
    determinant is scaled to the 1e-6 cut (either side of it, and on it as nearly as rounding allows), rays that miss.
    Pinned to orc_triangle_hit: fr.triangle_matrix (what fr.reference runs: the pairs are the diagonals of 100 x 100
    blocks), fr.records (point and normal of the reference's records) and fr.triangle_t (the plain statement); the
    blocks' other 990,000 pairs must agree between triangle_matrix and triangle_t."""
    g = np.random.default_rng(102)
    tri = g.uniform(-2, 2, (PAIRS, 9))
    A, B, Cc = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    w = g.dirichlet([1, 1, 1], PAIRS)
    inside = w[:, 0:1] * A + w[:, 1:2] * B + w[:, 2:3] * Cc
    nrm = np.cross(B - A, Cc - A)
    mode = g.integers(0, 4, PAIRS)
    o = inside + g.normal(size=(PAIRS, 3)) * 2.0
    d = inside - o
    out = mode == 1  # aimed beside the triangle
    d[out] += g.normal(size=(int(out.sum()), 3)) * 1.5
    plane = mode == 2  # in the triangle's plane: origin on it, direction along an edge combination
    o[plane] = inside[plane] + (B - A)[plane] * g.normal(size=(int(plane.sum()), 1))
    d[plane] = (B - A)[plane] * g.normal(size=(int(plane.sum()), 1)) + (Cc - A)[plane] * g.normal(size=(int(plane.sum()), 1))
    cut = mode == 3  # det = -d.n scaled to 1e-6 times a factor in {1 - 1e-12, 1, 1 + 1e-12, 0.5, 2}
    det = -np.einsum("ij,ij->i", d, nrm)
    f = g.choice([1 - 1e-12, 1.0, 1 + 1e-12, 0.5, 2.0], PAIRS)
    scale = np.where(cut, 1e-6 * f / np.where(det == 0, 1.0, det), 1.0)
    d = d * scale[:, None]
    tmax = np.where(cut, math.inf, _tmax(g, PAIRS))
    ok, t, n = fr.triangle_t(A, B, Cc, o, d, fr.TMIN, tmax)
    p = o + d * t[:, None]
    ok_m, t_m = np.zeros(PAIRS, dtype=bool), np.zeros(PAIRS)
    B_ = 100
    for lo in range(0, PAIRS, B_):
        blk = slice(lo, lo + B_)
        okb, tb = fr.triangle_matrix(tri[blk], o[blk], d[blk], fr.TMIN, tmax[blk])  # [ray, triangle]
        ok_m[blk], t_m[blk] = np.diagonal(okb), np.diagonal(tb)
        okp, tp, _ = fr.triangle_t(A[None, blk], B[None, blk], Cc[None, blk], o[blk, None], d[blk, None], fr.TMIN,
                                   tmax[blk, None])
        assert np.array_equal(okb, okp) and np.array_equal(bits(tb[okb]), bits(tp[okp])), lo
        assert np.all(np.isinf(tb[~okb]))
    view = _view(tri=tri, kind=np.full(PAIRS, rtow.PRIM_TRIANGLE))
    seen = {"hit": 0, "miss": 0, "plane": 0, "cut_hit": 0, "cut_miss": 0}
    for j in range(PAIRS):
        want = _oracle_triangle(tri[j], o[j], d[j], tmax[j])
        assert bool(ok[j]) == (want is not None) == bool(ok_m[j]), (j, mode[j])
        seen["plane"] += mode[j] == 2
        if mode[j] == 3:
            seen["cut_hit" if want is not None else "cut_miss"] += 1
        if want is None:
            seen["miss"] += 1
            continue
        seen["hit"] += 1
        assert bits(t[j]) == bits(want[0]) and np.array_equal(bits(p[j]), bits(want[1])), j
        assert np.array_equal(bits(n[j]), bits(want[2])), j
        assert bits(t_m[j]) == bits(want[0]), j
        rec = _record(view, o[j], d[j], 0.0, j, t_m[j])
        assert np.array_equal(bits(rec["point"]), bits(want[1])) and np.array_equal(bits(rec["normal"]), bits(want[2])), j
        assert rec["front_face"] == 1, j
    assert min(seen.values()) > 300, seen


def test_vectorised_reference_equals_the_oracle_loop_on_the_handmade_scene():
    scene = handmade_scene()
    view = SceneView(scene)
    rays = handmade_rays()
    g = np.random.default_rng(11)
    finite = rays.copy()
    finite["tmax"] = g.choice([0.0005, 0.3, 1.0, 2.5, 6.0, 50.0], size=len(rays)) * g.random(len(rays)) * 2.0
    finite["tmax"][:3] = [math.nan, 0.000999, 0.001]
    for rs in (rays, finite):
        for k in (1, 3, 8):
            hv, cv = fr.reference(view, rs, k)
            ho, co = fr.reference_oracle(view, rs, k)
            assert np.array_equal(cv, co) and fr.same_records(hv, ho), (k, fr.first_difference(hv, ho))
    assert cv[0] == 0 and cv[1] == 0
    assert set(np.unique(cv)) >= {0, 1, 2, 3}


def test_first_entry_is_the_closest_hit_brute_force():
    """Entry 0 equals the hittable-list brute force of support_oracle.py in every field (no ties for the first place
    among these rays), and every list is ascending in (t, insertion index) with distinct primitives."""
    scene = handmade_scene()
    view = SceneView(scene)
    rays = handmade_rays()
    want = brute_force(view, rays)
    hits, counts = fr.reference(view, rays, 8)
    assert np.array_equal(bits(hits["t"][:, 0]), bits(want["t"]))
    assert fr.same_records(np.ascontiguousarray(hits[:, 0]), want)
    assert np.array_equal(counts > 0, np.isfinite(want["t"]))
    for j in range(len(rays)):
        t, p = hits["t"][j, :counts[j]], hits["prim"][j, :counts[j]]
        assert np.all(np.diff(t) >= 0) and len(set(p)) == len(p), j
        assert np.all(np.diff(p)[np.diff(t) == 0] > 0), j  # (a tie deeper in the list: by insertion index)
        assert np.all(np.isinf(hits["t"][j, counts[j]:])) and np.all(hits["prim"][j, counts[j]:] == -1)
    assert counts.max() >= 4


def test_ties_scene_reference_keeps_the_lowest_insertion_indices():
    scene = fr.ties_scene()
    view = SceneView(scene)
    rays = fr.ties_rays()
    hits, counts = fr.reference(view, rays, 8)
    ho, co = fr.reference_oracle(view, rays, 8)
    assert np.array_equal(counts, co) and fr.same_records(hits, ho)
    tri3 = sph3 = 0
    for j in range(len(rays)):
        prims = list(hits["prim"][j, :counts[j]])
        for group in (fr.TIE_TRIANGLES, fr.TIE_SPHERES):
            if group[0] in prims:
                k = prims.index(group[0])
                assert tuple(prims[k:k + 3]) == group, (j, prims)  # all three, adjacent, in index order
                assert len(set(bits(hits["t"][j, k:k + 3]))) == 1
                tri3 += group is fr.TIE_TRIANGLES
                sph3 += group is fr.TIE_SPHERES
    assert tri3 > 100 and sph3 > 100, (tri3, sph3)
