"""Self-tests of the exact ray-query reference (tests/exact_hits.py), no GPU: constructed cases with known answers, the
oracle's binary64 brute force against it (which checks the strict band), and planted faults the checker must reject."""
import math

import numpy as np
import pytest

import exact_hits as ex
import rtow
from test_gpu_query import LOGGED, SceneView, brute_force, log_rays, rays_of


def _scene(sph=(), mov=(), tri=()):
    sph, mov, tri = np.reshape(np.asarray(sph, float), (-1, 4)), np.reshape(np.asarray(mov, float), (-1, 8)), \
        np.reshape(np.asarray(tri, float), (-1, 9))
    pmat = np.arange(len(sph) + len(mov) + len(tri), dtype=np.int32) % 3
    return ex.Scene.class_major(sph, mov, tri, pmat)


def _ref(scene, o, d, time=0.0, tmax=math.inf, build=ex.STRICT):
    return ex.Reference(scene, rtow.make_rays(np.reshape(o, (-1, 3)), np.reshape(d, (-1, 3)), time=time, tmax=tmax),
                        build)


# two triangles sharing the edge (1,0,0)-(0,1,0) of the plane z = 0, both facing +z
SHARED = _scene(tri=[[0, 0, 0, 1, 0, 0, 0, 1, 0], [1, 0, 0, 1, 1, 0, 0, 1, 0]])


@pytest.mark.parametrize("build", [ex.STRICT, ex.FAST])
def test_ray_through_a_shared_edge_hits_both_with_a_tie(build):
    r = _ref(SHARED, [0.5, 0.5, 1], [0, 0, -1], build=build)
    assert r.ties[0] == (0, 1) and r.t[0] == 1.0 and r.front[0] == 1
    assert r.occ[0] and not r.decided[0]  # (the edge tests are exactly 0: inside every band)
    inside = _ref(SHARED, [[0.25, 0.25, 1], [0.75, 0.75, 1]], [[0, 0, -1], [0, 0, -1]], build=build)
    assert inside.ties == [(0,), (1,)] and inside.decided.all() and inside.occ_decided.all()


def test_ray_through_a_vertex_and_past_it():
    r = _ref(SHARED, [[0, 0, 1], [-1e-3, 0, 1], [1, 1, 2]], [[0, 0, -1], [0, 0, -1], [0, 0, -1]])
    assert r.ties[0] == (0,) and not r.decided[0]
    assert r.ties[1] == () and r.decided[1] and not r.occ[1]
    assert r.ties[2] == (1,) and r.t[2] == 2.0 and not r.decided[2]


def test_tangent_sphere_ray_is_a_hit_and_undecided():
    s = _scene(sph=[[0, 0, 0, 1.0]])
    r = _ref(s, [[-5, 1, 0], [-5, 1 + 2 ** -50, 0], [-5, 1 + 2 ** -30, 0], [-5, 0.5, 0]], [[1, 0, 0]] * 4)
    assert r.ties[0] == (0,) and r.t[0] == 5.0 and r.front[0] == 0  # disc = 0: d.(p - c) = 0 is not < 0
    assert not r.decided[0] and r.occ[0]
    assert r.ties[1] == () and not r.decided[1]  # just outside: a miss, inside the band of the tangent
    assert r.ties[2] == () and r.decided[2]  # (disc = -2^-29: decided)
    assert r.ties[3] == (0,) and r.decided[3] and r.front[3] == 1


def test_t_exactly_at_tmax_is_inclusive():
    r = _ref(SHARED, [[0.25, 0.25, 1]] * 2, [[0, 0, -1]] * 2, tmax=np.array([1.0, np.nextafter(1.0, 0)]))
    assert r.ties[0] == (0,) and r.occ[0] and not r.decided[0]
    assert r.ties[1] == () and not r.occ[1] and not r.decided[1]
    far = _ref(SHARED, [[0.25, 0.25, 1]] * 2, [[0, 0, -1]] * 2, tmax=np.array([1.5, 0.5]))
    assert far.ties == [(0,), ()] and far.decided.all() and list(far.occ) == [True, False]


def test_det_exactly_at_the_cut():
    dz = np.array([1e-6, np.nextafter(1e-6, 0), 2e-6])
    r = _ref(SHARED, np.tile([0.25, 0.25, 1.0], (3, 1)), np.c_[np.zeros(3), np.zeros(3), -dz])
    assert r.ties[0] == (0,) and r.t[0] == 1.0 / 1e-6 and not r.decided[0]  # det = 1e-6 exactly: a hit
    assert r.ties[1] == () and not r.decided[1]
    assert r.ties[2] == (0,) and r.decided[2]
    # the fast GRID walk's cut on the unit direction: det / |d| = 1 >= 1e-6 for all three
    u = ex.Reference(SHARED, rtow.make_rays(np.tile([0.25, 0.25, 1.0], (3, 1)), np.c_[np.zeros(3), np.zeros(3), -dz]),
                     ex.FAST, unit_cut=True)
    assert u.ties == [(0,), (0,), (0,)] and u.decided.all()


def test_hollow_sphere_entered_from_inside():
    s = _scene(sph=[[0, 0, 0, -1.0], [0, 0, 0, 2.0]])
    r = _ref(s, [[0, 0, 0], [0, 0, -5]], [[1, 0, 0], [0, 0, 1]])
    assert r.ties[0] == (0,) and r.t[0] == 1.0 and r.front[0] == 1 and r.decided[0]  # far root, inward: front
    assert r.ties[1] == (1,) and r.t[1] == 3.0 and r.front[1] == 1 and r.decided[1]
    assert [c.prim for c in r.cands[1]] == [0, 1]  # the hollow sphere hit from outside, behind: front 0
    assert [c.front for c in r.cands[1]] == [0, 1]


@pytest.mark.parametrize("time,x,hit", [(0.0, 0.0, True), (1.0, 2.0, True), (0.5, 1.0, True), (1.0, 0.0, False),
                                        (0.5, 1.5, True), (0.5, 1.5 + 2 ** -20, False)])
def test_moving_sphere_at_shutter_times(time, x, hit):
    s = _scene(mov=[[0, 0, 0, 2, 0, 0, 0.5, 0]])
    r = _ref(s, [x, 0, 5], [0, 0, -1], time=time)
    assert bool(r.ties[0]) == hit
    if hit and x != 1.5:
        assert r.t[0] == 4.5 and r.decided[0]


# ---- against the oracle's binary64 brute force --------------------------------------------------------------------
def _random_rays(view, n, seed):
    g = np.random.default_rng(seed)
    small = view.sph[np.abs(view.sph[:, 3]) < 10, :3]  # (the box of the small primitives, not the ground sphere's)
    pts = np.concatenate([p for p in (small, view.tri[:, :3]) if len(p)])
    lo, hi = pts.min(0), pts.max(0)
    ext = float(np.max(hi - lo))
    o = g.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(n, 3))
    d = g.normal(size=(n, 3)) * np.exp(g.uniform(-2, 2, size=(n, 1)))
    return rtow.make_rays(o, d, time=g.random(n), tmax=np.where(g.random(n) < 0.3, g.uniform(0.1, 5, n), np.inf))


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in ("cover_moving", "suzanne"):
        mk, w, h, spp, depth, seed = LOGGED[name]
        hs = mk()
        cfg = rtow.make_config(w // 2, h // 2, 1, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        view = SceneView(hs)
        out[name] = (view, ex.Scene.of(view), log_rays(hs, cfg))
    return out


def _oracle_hits(view, rays):
    """The oracle's brute force over [0.001, inf), a hit beyond the ray's tmax reported as a miss (as the query does)."""
    h = brute_force(view, rays)
    h[h["t"] > rays["tmax"]] = (np.inf, (0, 0, 0), (0, 0, 0), -1, -1, -1, 0)
    return h


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
@pytest.mark.parametrize("source", ["logged", "random"])
def test_the_oracle_is_exact_on_every_decided_ray(scenes, name, source):
    """The oracle (binary64, the reference's expressions: what the strict build reproduces bit for bit) must give the
    exact primitive, front_face and t within the strict bound on every decided ray, and an explainable answer on the
    others; at most 1e-3 of the rays are undecided."""
    view, sc, log = scenes[name]
    if source == "logged":
        g = np.random.default_rng(3)
        rays = rays_of(log[g.choice(len(log), size=min(len(log), 4000), replace=False)])
    else:
        rays = _random_rays(view, 4000, 11)
    ref = ex.Reference(sc, rays, ex.STRICT)
    assert ref.decided.mean() >= 1 - 1e-3, int((~ref.decided).sum())
    assert 0.05 < ref.occ.mean() < 0.98
    k = np.random.default_rng(4).choice(len(rays), size=400, replace=False)
    k = np.union1d(k, np.nonzero(~ref.decided)[0])
    sub = ex.Reference(sc, rays[k], ex.STRICT)
    hits = _oracle_hits(view, rays[k])
    st = ex.check(sub, hits, np.isfinite(hits["t"]) & (hits["t"] <= rays["tmax"][k]), (name, source))
    print(f"\n{name}/{source}: {ref.decided.sum()} decided, {(~ref.decided).sum()} undecided of {len(rays)}; "
          f"oracle worst t error {st['worst_t_err']:.3f} of its bound, {st['exact_pairs']} exact pairs")


# ---- the checker rejects planted faults ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(scenes):
    view, sc, log = scenes["cover_moving"]
    rays = np.concatenate([_random_rays(view, 300, 17), rays_of(log[::max(1, len(log) // 300)])])
    rays["tmax"] = np.inf
    ref = ex.Reference(sc, rays, ex.STRICT)
    hits = _oracle_hits(view, rays)
    ex.check(ref, hits, np.isfinite(hits["t"]))  # the unmodified answers pass
    return view, sc, rays, ref, hits


def _first(ref, cond):
    i = next(i for i in range(len(ref.rays)) if ref.decided[i] and cond(i))
    return i


def test_the_checker_rejects_planted_faults(planted):
    view, sc, rays, ref, hits = planted
    occ = np.isfinite(hits["t"])

    def rejected(mutate, occ_mutate=None):
        h, o = hits.copy(), occ.copy()
        mutate(h)
        if occ_mutate:
            occ_mutate(o)
        with pytest.raises(ex.CheckError):
            ex.check(ref, h, o)

    hit = _first(ref, lambda i: ref.ties[i] and sc.kind[ref.ties[i][0]] != ex.TRIANGLE)
    miss = _first(ref, lambda i: not ref.ties[i])
    two = _first(ref, lambda i: len([c for c in ref.cands[i] if c.status == ex.HIT]) >= 2)
    second = sorted((c for c in ref.cands[two] if c.status == ex.HIT), key=lambda c: c.t)[1]

    def scale_t(h):
        h["t"][hit] *= 1 + 1e-10
    rejected(scale_t)

    def second_nearest(h):
        p = second.prim
        h[two] = (second.t, rays["origin"][two] + second.t * rays["direction"][two], h["normal"][two], p, view.kind[p],
                  view.prim_mat[p], second.front)
    rejected(second_nearest)

    def to_miss(h):
        h[hit] = (np.inf, (0, 0, 0), (0, 0, 0), -1, -1, -1, 0)
    rejected(to_miss)
    rejected(lambda h: None, lambda o: o.__setitem__(hit, False))

    def to_hit(h):
        h[miss] = hits[hit]
    rejected(to_hit)
    rejected(lambda h: None, lambda o: o.__setitem__(miss, True))

    def flip_front(h):
        h["front_face"][hit] ^= 1
    rejected(flip_front)

    def material(h):
        h["material"][hit] = (h["material"][hit] + 1) % 4
    rejected(material)

    def kind(h):
        h["kind"][hit] = ex.TRIANGLE
    rejected(kind)

    def sphere_normal(h):
        h["normal"][hit] = -h["normal"][hit]
    rejected(sphere_normal)


def test_the_checker_rejects_a_triangle_normal_one_ulp_off(scenes):
    view, sc, log = scenes["suzanne"]
    rays = rays_of(log[:300])
    ref = ex.Reference(sc, rays, ex.STRICT)
    hits = _oracle_hits(view, rays)
    ex.check(ref, hits)
    i = _first(ref, lambda i: bool(ref.ties[i]))
    h = hits.copy()
    h["normal"][i, 1] = np.nextafter(h["normal"][i, 1], np.inf)
    with pytest.raises(ex.CheckError, match="normal"):
        ex.check(ref, h)
