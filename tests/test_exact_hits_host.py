"""Self-tests of the exact ray-query reference (tests/exact_hits.py), no GPU: constructed cases with known answers, the
oracle's binary64 brute force against it (which checks the strict band), and planted faults the checker must reject;
then the same for the first-k-hits sequence checker: the strict build's binary64 mirror (tests/first_hits_ref.py) on
every ray family of tests/test_gpu_exact_sequences.py, planted faults, and what the deep families must be."""
import math

import numpy as np
import pytest

import accel_images as ai
import exact_hits as ex
import first_hits_ref as fr
import rtow
import exact_cases as gx
from exact_cases import SHARE
from support_oracle import LOGGED, brute_force, log_rays, rays_of
from support_scenes import SceneView, handmade_rays, handmade_scene


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


# ---- first-k-hits sequences: the checker accepts the truth ----------------------------------------------------------
# first_hits_ref.reference is the binary64 mirror of the strict build (the GPU tests pin the build to it bit for bit), so
# what the GPU tests of tests/test_gpu_exact_sequences.py feed the checker is proved here first: same ray families, same
# reference, no GPU.
DEEP = (8, 3, 1)


def _cut(h8, c8, k):
    return np.ascontiguousarray(h8[:, :k]), np.minimum(c8, k).astype(np.int32)


def _accepts(name, view, sc, rays, ks=(8,)):
    """check_sequences passes on the strict mirror's sequences; returns (reference, hits, counts, stats at ks[0])."""
    ref = ex.Reference(sc, rays, ex.STRICT)
    h8, c8 = fr.reference(view, rays, 8)
    stats = [ex.check_sequences(ref, *_cut(h8, c8, k), k, (name, k)) for k in ks]
    assert all(s["unordered_equal_t"] == 0 for s in stats)
    print(f"\nsequences {name}: {len(rays)} rays, decided {stats[0]['decided']}, undecided {stats[0]['undecided']}, "
          f"worst t err {stats[0]['worst_t_err']:.3f} of bound")
    return ref, h8, c8, stats[0]


def _sheets(layers, m):
    G = ai.mesh_geometry(ai.sheet_stack(layers, m, 73))
    return ex.Scene.class_major(G.sph, G.mov, G.tri, G.pmat)  # (it has SceneView's fields: the mirror reads it too)


@pytest.fixture(scope="module")
def covers():
    out = {}
    for name, moving in (("cover_static", False), ("cover_moving", True)):
        hs = rtow.HostScene.cover(11, 1.5, moving)
        view = SceneView(hs)
        out[name] = (hs, view, ex.Scene.of(view))
    return out


def _deep_case(covers, name):
    if name.startswith("cover"):
        hs, view, sc = covers[name]
        return view, sc, fr.chord_rays(3000, 71)
    sc = _sheets(*{"sheets10x6": (10, 6), "sheets12x16": (12, 16)}[name])
    return sc, sc, fr.sheet_rays(2000, 74)


@pytest.mark.parametrize("name", ["cover_static", "cover_moving", "sheets10x6", "sheets12x16"])
def test_deep_sequences_are_accepted_and_the_inputs_are_deep_and_decided(covers, name):
    """Chords and sheet stacks: the checker accepts the mirror at max_hits 8, 3 and 1; from the reference alone, at least
    20 % of the rays have 8 or more exact hits, at least 10 % have 1 to 7, and at most SHARE are undecided at 8 under
    either band."""
    view, sc, rays = _deep_case(covers, name)
    assert np.isfinite(rays["tmax"]).mean() > 0.4 and np.isinf(rays["tmax"]).mean() > 0.4
    ln = np.linalg.norm(rays["direction"], axis=1)
    assert ln.max() / ln.min() > 100
    ref, h8, c8, st = _accepts(name, view, sc, rays, DEEP)
    for r in (ref, ex.Reference(sc, rays, ex.FAST)):
        n_hit = np.array([sum(c.status == ex.HIT for c in cs) for cs in r.cands])
        assert np.mean(n_hit >= 8) >= 0.2 and np.mean((n_hit >= 1) & (n_hit <= 7)) >= 0.1, (name, r.build)
        assert np.mean(~ex.sequence_decided(r, 8)) <= SHARE, (name, r.build)
    assert np.mean(c8 == 8) >= 0.2


@pytest.mark.parametrize("name", ["cover_static", "sheets12x16"])
def test_tmax_at_and_around_hits_is_accepted_and_mostly_undecided(covers, name):
    view, sc, rays = _deep_case(covers, name)
    rays = rays[:1500]
    h8, c8 = fr.reference(view, rays, 8)
    at = fr.tmax_at_hits(rays, h8["t"], c8)
    assert len(at) >= 1000 and np.all(np.isfinite(at["tmax"]))
    ref, h, c, st = _accepts(f"tmax_at_hits/{name}", view, sc, at, DEEP)
    assert st["undecided"] >= 0.5 * len(at)
    fast = ex.Reference(sc, at, ex.FAST)
    assert np.mean(~ex.sequence_decided(fast, 8)) >= 0.5


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_logged_and_random_rays_are_accepted_and_decided(scenes, name):
    view, sc, log = scenes[name]
    g = np.random.default_rng(3)
    for source, rays in (("logged", rays_of(log[g.choice(len(log), size=min(len(log), 2000), replace=False)])),
                         ("random", _random_rays(view, 2000, 11))):
        ref, h8, c8, st = _accepts(f"{source}/{name}", view, sc, rays)
        assert st["undecided"] <= SHARE * len(rays)
        assert np.mean(~ex.sequence_decided(ex.Reference(sc, rays, ex.FAST), 8)) <= SHARE


def test_handmade_and_ties_scenes_are_accepted():
    h = handmade_scene()
    view = SceneView(h)
    ref, h8, c8, st = _accepts("handmade", view, ex.Scene.of(view), handmade_rays(), DEEP)
    assert np.sum(h8["front_face"][h8["prim"] >= 0] == 0) > 50  # the hollow glass: far roots, front_face 0
    h = fr.ties_scene()
    view = SceneView(h)
    ref, h8, c8, st = _accepts("ties", view, ex.Scene.of(view), fr.ties_rays(), DEEP + (2,))
    assert st["undecided"] > 50  # (exact ties are never decided)


@pytest.mark.parametrize("name", ["n4", "coincident", "zero_area", "big_and_small"])
def test_edge_and_vertex_rays_are_accepted(name):
    G = ai.mesh_geometry(ai.edge_meshes()[name])
    sc = ex.Scene.class_major(G.sph, G.mov, G.tri, G.pmat)
    _accepts(f"edges/{name}", sc, sc, gx.edge_rays(G.tri, 80, 3), DEEP if name == "coincident" else (8,))


def test_the_other_families_of_the_closest_hit_tests_are_accepted(scenes, covers):
    """Tangent rays, the det cut, rays from surfaces, direction magnitudes, a far scene and a refitted one: the rays the
    GPU tests use (a seeded subset where they are many)."""
    h = handmade_scene()
    view = SceneView(h)
    _accepts("tangent/handmade", view, ex.Scene.of(view), gx.handmade_tangent_rays(view))
    view, sc, log = scenes["cover_moving"]
    _accepts("tangent/cover_moving", view, sc, gx.cover_tangent_rays(view))
    _accepts("surfaces/cover_moving", view, sc, gx.surface_rays(log)[::2])
    view, sc, log = scenes["suzanne"]
    _accepts("det_cut/suzanne", view, sc, gx.det_cut_rays(view, sc))
    _accepts("magnitudes/suzanne", view, sc, gx.magnitude_rays(log)[::4])
    hs, view, sc = covers["cover_static"]
    up, far, rays, keep = gx.far_case(hs, scenes["cover_moving"][2], 1e5)
    _accepts("far/cover_static/1e5", far, far, rays[::3])
    hs, view, sc = covers["cover_moving"]
    base, new, moved, rays, keep = gx.refit_case(hs, "flatten", 300)
    _accepts("refit/cover_moving/flatten", moved, moved, rays)


# ---- first-k-hits sequences: planted faults ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq(covers):
    hs, view, sc = covers["cover_moving"]
    rays = fr.chord_rays(1200, 71)
    ref = ex.Reference(sc, rays, ex.STRICT)
    h8, c8 = fr.reference(view, rays, 8)
    ex.check_sequences(ref, h8, c8, 8)  # the unmodified answers pass
    return view, sc, rays, ref, h8, c8


def _decided_ray(ref, k, cond):
    dec = ex.sequence_decided(ref, k)
    return next(i for i in range(len(ref.rays)) if dec[i] and cond(i))


def _record(view, rays, i, c):
    """The record of decided candidate c on ray i (its exact values)."""
    return fr.records(view, rays[i], np.array([c.prim]), np.array([c.t]))[0]


def test_the_sequence_checker_rejects_planted_faults(seq):
    view, sc, rays, ref, h8, c8 = seq
    MISS = fr.miss_records(1)[0]

    def rejected(mutate, match=None):
        h, c = h8.copy(), c8.copy()
        mutate(h, c)
        with pytest.raises(ex.CheckError, match=match):
            ex.check_sequences(ref, h, c, 8)

    n_hit = [sum(c.status == ex.HIT for c in cs) for cs in ref.cands]
    part = _decided_ray(ref, 8, lambda i: 4 <= n_hit[i] <= 7)          # a list that does not fill
    full = _decided_ray(ref, 8, lambda i: n_hit[i] >= 10)              # one that does, with decided hits behind the cut
    cut = _decided_ray(ref, 8, lambda i: n_hit[i] >= 3 and np.isfinite(rays["tmax"][i]))
    sph = _decided_ray(ref, 8, lambda i: n_hit[i] >= 2 and h8["kind"][i, 1] != ex.TRIANGLE)

    def drop_middle(h, c):
        h[part, 1:7] = h8[part, 2:8]
        c[part] -= 1
    rejected(drop_middle, "missing")

    def swap(h, c):
        h[part, 1], h[part, 2] = h8[part, 2], h8[part, 1]
    rejected(swap, "descends")

    def swap_prims_only(h, c):  # (t kept ascending: the primitives' other fields swapped)
        h[part, 1], h[part, 2] = h8[part, 2], h8[part, 1]
        h["t"][part, 1], h["t"][part, 2] = h8["t"][part, 1], h8["t"][part, 2]
    rejected(swap_prims_only)

    def twice(h, c):
        h[part, 2] = h8[part, 1]
    rejected(twice, "twice")

    def farther_last(h, c):
        far = sorted((x for x in ref.cands[full] if x.status == ex.HIT), key=lambda x: x.t)[9]
        h[full, 7] = _record(view, rays, full, far)
    rejected(farther_last, "missing in front of the last entry")

    def count_small(h, c):
        h[part, c8[part] - 1] = MISS
        c[part] -= 1
    rejected(count_small, "missing")

    def count_large(h, c):
        c[part] += 1
    rejected(count_large, "miss record below count")

    def beyond_tmax(h, c):  # the next hit behind the ray's tmax, appended
        inf = rays[cut:cut + 1].copy()
        inf["tmax"] = np.inf
        hh, cc = fr.reference(view, inf, 8)
        assert cc[0] > c8[cut] and hh["t"][0, c8[cut]] > rays["tmax"][cut]
        h[cut, c8[cut]] = hh[0, c8[cut]]
        c[cut] += 1
    rejected(beyond_tmax, "cannot hit within tmax")

    def move_t(h, c):
        x = next(x for x in ref.cands[part] if x.prim == h8["prim"][part, 1])
        h["t"][part, 1] += 2 * x.E
    rejected(move_t, "exact")

    def tail(h, c):
        h[part, 7] = h8[part, 0]
    rejected(tail, "no miss record")

    def tail_fields(h, c):  # (a miss record's prim with another field left over)
        h["material"][part, 7] = 0
    rejected(tail_fields, "no miss record")

    def flip_front(h, c):
        h["front_face"][sph, 1] ^= 1
    rejected(flip_front, "front")

    def material(h, c):
        h["material"][sph, 1] = (h["material"][sph, 1] + 1) % 3
    rejected(material, "material")

    def kind(h, c):
        h["kind"][sph, 1] = ex.TRIANGLE
    rejected(kind, "kind")

    def sphere_normal(h, c):
        h["normal"][sph, 1] = -h["normal"][sph, 1]
    rejected(sphere_normal, "normal")

    def point(h, c):
        h["point"][sph, 1] += 1e-9
    rejected(point, "point")

    # the cuts: a decided ray's list cut one short, and the (k+1)-th hit in place of the k-th
    for k in (1, 3):
        i = _decided_ray(ref, k, lambda i: n_hit[i] >= k + 2)
        hk, ck = _cut(h8, c8, k)
        ex.check_sequences(ref, hk, ck, k)
        bad = hk.copy()
        bad[i, k - 1] = h8[i, k]
        with pytest.raises(ex.CheckError, match="missing"):
            ex.check_sequences(ref, bad, ck, k)
        short = ck.copy()
        short[i] -= 1
        bad = hk.copy()
        bad[i, k - 1] = MISS
        with pytest.raises(ex.CheckError, match="missing"):
            ex.check_sequences(ref, bad, short, k)


def test_an_exact_tie_in_swapped_order_is_accepted():
    """Two triangles sharing an edge, a ray through the edge: both hit at t = 1 exactly.  Which comes first is the
    band's to decide when the computed t differ; bit-equal t must come in index order unless the walk sorts another
    quantity (the fast GRID walk)."""
    rays = rtow.make_rays(np.array([[0.5, 0.5, 1.0]]), np.array([[0.0, 0.0, -1.0]]))
    ref = ex.Reference(SHARED, rays, ex.STRICT)
    assert not ex.sequence_decided(ref, 2)[0] and not ex.sequence_decided(ref, 1)[0]
    h, c = fr.reference(SHARED, rays, 2)
    assert list(h["prim"][0]) == [0, 1] and h["t"][0, 0] == h["t"][0, 1] == 1.0
    ex.check_sequences(ref, h, c, 2)
    sw = h.copy()
    sw[0, 0], sw[0, 1] = h[0, 1], h[0, 0]
    with pytest.raises(ex.CheckError, match="index order"):
        ex.check_sequences(ref, sw, c, 2)
    assert ex.check_sequences(ref, sw, c, 2, sorted_by_index=False)["unordered_equal_t"] == 1
    sw["t"][0, 1] = np.nextafter(1.0, 2.0)  # (within the bound of the exact t)
    ex.check_sequences(ref, sw, c, 2)
    one = sw[:, :1].copy()  # either member alone is a list of one the band allows
    ex.check_sequences(ref, one, np.array([1], np.int32), 1)
