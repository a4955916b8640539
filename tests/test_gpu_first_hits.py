"""First-k-hits (ordered multi-hit) ray queries (rtow_first_hits / rtow_first_hits_device) on the GPU.

The strict build is compared bit for bit — every field of every slot, the unused ones and the counts — with the
reference of tests/first_hits_ref.py (every primitive's oracle hit test, sorted by (t, insertion index), cut at
max_hits): on the hand-made scene, on a scene of exact ties and duplicates, on the cover scenes (rows of spheres: full
lists) and on the meshes, under every strategy and both builders.  Then its relations to the any-hit and closest-hit
queries, the fast build against the strict one, the result after a refit, and the contracts.
"""
import ctypes as C
import math

import numpy as np
import pytest

import first_hits_ref as fr
import rtow
from support_fixtures import big_mesh, fctx, logged  # noqa: F401
from support_oracle import FAST_CASES, LOGGED, expected_kernel, rays_of, seeded_finite_tmax
from support_scenes import SMALL, SceneView, _copy, handmade_rays, handmade_scene, motions, rays_for, scene_of
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu

HIT = rtow.HIT_DTYPE.itemsize  # 72
S = rtow.F64_STRICT


def assert_equal(got, want, what):
    """(hits, counts) pairs: counts equal, every slot's every field bit for bit."""
    assert np.array_equal(got[1], want[1]), (what, "counts", np.nonzero(got[1] != want[1])[0][:5])
    assert fr.same_records(got[0], want[0]), (what, fr.first_difference(got[0], want[0]))


def cut(ref8, k):
    """The reference for max_hits = k from the one for 8 (the definition: a prefix)."""
    return np.ascontiguousarray(ref8[0][:, :k]), np.minimum(ref8[1], k).astype(np.int32)


# ------------------------------------------------------------------------------------------ 1. hand-made scene ---
@pytest.fixture(scope="module")
def handmade():
    scene = handmade_scene()
    view = SceneView(scene)
    sets = {"inf": handmade_rays(), "finite": seeded_finite_tmax(handmade_rays())}
    refs = {(w, k): fr.reference_oracle(view, rs, k) for w, rs in sets.items() for k in (1, 3, 8)}
    return scene, view, sets, refs


@pytest.mark.parametrize("kernel", list(WALKS))
def test_handmade_scene_equals_the_oracle_reference(fctx, handmade, kernel):
    """The glass shell and the hollow sphere (far roots, front_face 0), insertion order differing from class order, +-0
    direction components, the moving sphere at three shutter times; tmax = inf and the occlusion test's seeded finite
    tmax; max_hits 1, 3 and 8."""
    scene, view, sets, refs = handmade
    fctx.upload(scene.c)
    assert np.signbit(sets["inf"]["direction"]).any()
    for (what, k), want in refs.items():
        hits, counts, st = fctx.first_hits(sets[what], k, S, WALKS[kernel], want_stats=True)
        assert hits.shape == (len(sets[what]), k) and counts.dtype == np.int32
        assert st.kernel_used == expected_kernel(view, WALKS[kernel]), (kernel, st.kernel_used)
        assert st.segments == len(hits) and st.samples == 0
        assert_equal((hits, counts), want, (kernel, what, k))
    ref8 = refs[("inf", 8)]
    assert ref8[1].max() >= 4 and (ref8[1] == 0).sum() > 100
    assert np.sum(ref8[0]["front_face"][ref8[0]["prim"] >= 0] == 0) > 50


# --------------------------------------------------------------------------------------- 2. ties and duplicates ---
@pytest.fixture(scope="module")
def ties():
    scene = fr.ties_scene()
    view = SceneView(scene)
    rays = fr.ties_rays()
    return scene, view, rays, fr.reference_oracle(view, rays, 8)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("kernel", list(WALKS))
def test_exact_ties_keep_the_lowest_insertion_indices(fctx, ties, kernel, builder):
    """Three bit-identical copies of a triangle and of a sphere, interleaved with other primitives, and a sphere spanning
    many grid cells: a tie is reported in insertion order, cut at the lowest indices when it straddles slot max_hits; no
    primitive appears twice; the same under every kernel and builder (each equals the reference)."""
    scene, view, rays, ref8 = ties
    fctx.set_builder(BUILDERS[builder])
    try:
        fctx.upload(scene.c)
        for k in (1, 2, 4, 8):
            hits, counts = fctx.first_hits(rays, k, S, WALKS[kernel])
            assert_equal((hits, counts), cut(ref8, k), (kernel, builder, k))
            straddle = 0
            for j in range(len(rays)):
                prims = list(hits["prim"][j, :counts[j]])
                assert len(set(prims)) == len(prims), (j, prims)
                for group in (fr.TIE_TRIANGLES, fr.TIE_SPHERES):
                    got = [p for p in prims if p in group]
                    assert tuple(got) == group[:len(got)], (kernel, builder, k, j, prims)
                    straddle += 0 < len(got) < 3
            if k in (2, 4):
                assert straddle > 50, (k, straddle)
    finally:
        fctx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------------------------------------ 3. cover scenes ---
def lattice_rays(seed):
    """Horizontal rays at y = 0.2 (the small spheres' centre height) along +-x and +-z, 500 per direction on a lattice
    across the field, seeded shutter times: each crosses a whole row of spheres."""
    g = np.random.default_rng(seed)
    w = np.linspace(-10.6, 10.6, 500)
    o, d = [], []
    for a, s in ((0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)):
        oo = np.zeros((len(w), 3))
        oo[:, 1] = 0.2
        oo[:, a], oo[:, 2 - a] = -13.0 * s, w
        o.append(oo), d.append(np.repeat((s * np.eye(3)[a])[None], len(w), 0))
    return rtow.make_rays(np.concatenate(o), np.concatenate(d), time=g.random(4 * len(w)))


@pytest.fixture(scope="module")
def cover(logged):
    out = {}
    for name in ("cover_static", "cover_moving"):
        scene, view, log = logged[name]
        g = np.random.default_rng(31)
        rows = log[g.choice(len(log), size=2000, replace=False)]
        t = np.where(np.isfinite(rows[:, 10]), rows[:, 10], 5.0)
        mixed = np.where(g.random(len(rows)) < 0.3, math.inf, t * g.choice([0.5, 1.0, 4.0, 60.0], size=len(rows)))
        lat = lattice_rays(32)
        rays = np.concatenate([lat, rays_of(rows, tmax=mixed)])
        out[name] = (scene, view, rays, len(lat), fr.reference(view, rays, 8))
    return out


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("kernel", ["brute", "bvh", "grid"])
@pytest.mark.parametrize("name", ["cover_static", "cover_moving"])
def test_cover_scenes_rows_of_spheres(fctx, cover, name, kernel, builder):
    scene, view, rays, n_lat, ref8 = cover[name]
    counts = ref8[1]
    # against a vacuous test, from the reference alone: full lists and partly filled ones both occur
    assert np.mean(counts[:n_lat] == 8) >= 0.1, np.mean(counts[:n_lat] == 8)
    assert np.mean((counts > 0) & (counts < 8)) >= 0.1, np.mean((counts > 0) & (counts < 8))
    fctx.set_builder(BUILDERS[builder])
    try:
        fctx.upload(scene)
        hits, cnt, st = fctx.first_hits(rays, 8, S, WALKS[kernel], want_stats=True)
        assert st.kernel_used == WALKS[kernel]
        assert_equal((hits, cnt), ref8, (name, kernel, builder))
    finally:
        fctx.set_builder(rtow.BUILDER_AUTO)


# ----------------------------------------------------------------------------------------------------- 4. meshes ---
def mesh_rays(log, n=20000, seed=41):
    """Primaries and later segments of the log (mixed tmax on the later ones), topped up to n with seeded perturbed
    copies when the log is shorter."""
    g = np.random.default_rng(seed)
    rows = log[:n]
    if len(rows) < n:
        extra = log[g.integers(0, len(log), n - len(rows))].copy()
        extra[:, 6:9] += 0.05 * g.normal(size=(len(extra), 3)) * np.linalg.norm(extra[:, 6:9], axis=1, keepdims=True)
        extra[:, 10] = math.inf
        rows = np.concatenate([rows, extra])
    t = np.where(np.isfinite(rows[:, 10]), rows[:, 10], 3.0)
    tmax = np.where((rows[:, 2] == 0) | (g.random(n) < 0.5), math.inf, t * g.choice([0.7, 1.0, 3.0, 40.0], size=n))
    return rays_of(rows, tmax=tmax)


@pytest.fixture(scope="module")
def meshes(logged, big_mesh):
    out = {}
    for name, (scene, view, log) in (("suzanne", logged["suzanne"]), ("mesh96k", big_mesh)):
        rays = mesh_rays(log)
        assert (log[:20000, 2] == 0).sum() > 1000  # primaries among them
        g = np.random.default_rng(42)
        pick = np.sort(g.choice(len(rays), size=500, replace=False))
        out[name] = (scene, view, rays, pick, fr.reference(view, rays[pick], 8))
    return out


@pytest.mark.parametrize("max_hits", [4, 8])
@pytest.mark.parametrize("name", ["suzanne", "mesh96k"])
def test_meshes_same_sequences_under_every_kernel_and_builder(fctx, meshes, name, max_hits):
    """Suzanne (the 4-wide image staged whole) and the 96,800-triangle mesh (64-byte nodes read from L2): identical bytes
    under BVH, GRID and BVH4 with both builders on 20,000 rays, equal to the reference on 500 of them."""
    scene, view, rays, pick, ref8 = meshes[name]
    first = None
    try:
        for bn, b in BUILDERS.items():
            fctx.set_builder(b)
            fctx.upload(scene)
            for kn in ("bvh", "grid", "bvh4"):
                hits, counts, st = fctx.first_hits(rays, max_hits, S, WALKS[kn], want_stats=True)
                if kn != "grid":
                    assert st.kernel_used == WALKS[kn], (name, bn, kn)
                assert st.node_tests > 0 and st.prim_tests > 0
                if first is None:
                    first = (hits, counts)
                    assert_equal((np.ascontiguousarray(hits[pick]), counts[pick]), cut(ref8, max_hits), (name, bn, kn))
                    assert counts.max() >= 2 and (counts == 0).any()
                else:
                    assert_equal((hits, counts), first, (name, bn, kn, max_hits))
    finally:
        fctx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------------- 5. relations to the existing queries ---
@pytest.mark.parametrize("kernel", ["bvh", "grid"])
@pytest.mark.parametrize("name", list(LOGGED))
def test_relations_to_occluded_and_intersect(fctx, logged, name, kernel):
    """On logged rays with the six tmax cases of the occlusion test: count > 0 == occluded; entry 0 has the closest
    hit's t (its bits) wherever that lies within tmax, and its primitive wherever the second entry's t differs; and
    first_hits(8) cut at k equals first_hits(k) byte for byte, k = 1 .. 7."""
    scene, view, log = logged[name]
    fctx.upload(scene)
    log = log[:12000]
    k = WALKS[kernel]
    t = log[:, 10]
    hit = np.isfinite(t)
    g = np.random.default_rng(17)
    tf = np.where(hit, t, g.uniform(0.01, 30.0, len(t)))
    cases = {"inf": np.full(len(t), math.inf), "t_hit": tf, "below": np.nextafter(tf, 0.0),
             "short": np.full(len(t), 0.000999), "fraction": tf * g.random(len(t)),
             "beyond": tf * (1.0 + g.random(len(t)))}
    for what, tmax in cases.items():
        rays = rays_of(log, tmax=tmax)
        h8, c8 = fctx.first_hits(rays, 8, S, k)
        assert np.array_equal(c8 > 0, fctx.occluded(rays, S, k)), (name, kernel, what)
        one = fctx.intersect(rays, S, k)
        within = np.isfinite(one["t"])  # (rtow_intersect reports a hit only within tmax)
        assert np.array_equal(c8 > 0, within), (name, kernel, what)
        assert np.array_equal(h8["t"][:, 0].view(np.uint64), one["t"].view(np.uint64)), (name, kernel, what)
        clear = within & ((c8 < 2) | (h8["t"][:, 1] != h8["t"][:, 0]))
        assert fr.same_records(np.ascontiguousarray(h8[clear, 0]), one[clear]), (name, kernel, what)
        assert clear.sum() >= 0.99 * within.sum()
        for kk in range(1, 8):
            hk, ck = fctx.first_hits(rays, kk, S, k)
            assert_equal((hk, ck), cut((h8, c8), kk), (name, kernel, what, kk))


# ------------------------------------------------------------------------------------------ 6. fast against strict ---
SHARE = 1e-3  # the project's share of undecided rays


@pytest.mark.parametrize("name,kernel", FAST_CASES)
def test_fast_agrees_with_strict(fctx, logged, big_mesh, name, kernel):
    """max_hits = 4 on the rays of test_gpu_query.py::test_fast_agrees_with_strict: counts and primitive sequences agree
    on >= 99.9 % of the rays; where they agree |t_fast - t_strict| <= 1e-9 t_strict.  Observed on the MI355X (printed
    per case): the sequences agree on every ray of every case; the worst relative difference in
    t is 1.8e-10 (cover_moving, GRID), 1.6e-10 on the static cover scene, 4.8e-14 on suzanne, 2.8e-15 on the 96.8k mesh."""
    scene, view, log = big_mesh if name == "mesh96k" else logged[name]
    fctx.upload(scene)
    rays = rays_of(log)
    hs, cs = fctx.first_hits(rays, 4, rtow.F64_STRICT, WALKS[kernel])
    hf, cf = fctx.first_hits(rays, 4, rtow.F64_FAST, WALKS[kernel])
    agree = (cs == cf) & np.all(hs["prim"] == hf["prim"], axis=1)
    share = float(np.mean(~agree))
    used = (hs["prim"] >= 0) & agree[:, None]
    rel = np.abs(hf["t"][used] - hs["t"][used]) / hs["t"][used]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"\nfirst_hits {name}/{kernel}: sequences differ on {int((~agree).sum())} of {len(rays)} rays "
          f"(share {share:.2e}), worst rel dt {worst:.3e}, mean count {cs.mean():.3f}")
    assert share <= SHARE, share
    assert np.all(rel <= 1e-9), worst


# --------------------------------------------------------------------------------------------------- 7. after refit ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_after_refit_equals_the_reference_of_the_new_geometry(fctx, name, builder):
    G = SMALL[name]
    keep = []
    fctx.set_builder(BUILDERS[builder])
    try:
        for mname in ("rotate", "jitter"):
            H, shift = motions(G)[mname]
            B = scene_of(H, keep, cam_shift=shift)
            fctx.upload(scene_of(_copy(G), keep))
            fctx.refit(B)

            class Held:
                c = B

            view = SceneView(Held)
            rays = rays_for(H, 400, seed=7)
            want = fr.reference(view, rays, 8)
            assert want[1].max() >= 2
            for kn, k in WALKS.items():
                got = fctx.first_hits(rays, 8, S, k)
                assert_equal(got, want, (name, builder, mname, kn))
    finally:
        fctx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------------------------------------------ 8. contracts ---
def contract_rays(logged, n=1000):
    scene, view, log = logged["cover_static"]
    lat = lattice_rays(50)[::4]
    g = np.random.default_rng(51)
    rows = log[g.choice(len(log), size=n - len(lat), replace=False)]
    return scene, np.concatenate([lat, rays_of(rows, tmax=np.where(g.random(len(rows)) < 0.5, math.inf, 3.0))])


def test_ragged_counts_canaries_and_null_counts(fctx, logged):
    import torch

    scene, rays = contract_rays(logged)
    fctx.upload(scene)
    k = 3
    whole_h, whole_c = fctx.first_hits(rays, k, S, rtow.KERNEL_AUTO)
    assert whole_c.max() == k and (whole_c == 0).any()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    for n in (1, 63, 64, 65, 1000):
        pad = 4 * HIT
        d_hits = torch.full((n * k * HIT + pad,), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_cnt = torch.full((n + 16,), -0x54545455, dtype=torch.int32, device="cuda:0")
        st = fctx.first_hits_device(d_rays.data_ptr(), n, k, d_hits.data_ptr(), d_cnt.data_ptr(), S, rtow.KERNEL_AUTO, 0,
                                    True)
        assert st.segments == n
        out, cnt = d_hits.cpu().numpy(), d_cnt.cpu().numpy()
        assert np.all(out[n * k * HIT:] == 0xAB) and np.all(cnt[n:] == -0x54545455), n
        assert out[:n * k * HIT].tobytes() == whole_h[:n].tobytes(), n
        assert np.array_equal(cnt[:n], whole_c[:n]), n
        # without counts
        d_hits2 = torch.full((n * k * HIT + pad,), 0xAB, dtype=torch.uint8, device="cuda:0")
        fctx.first_hits_device(d_rays.data_ptr(), n, k, d_hits2.data_ptr(), 0, S, rtow.KERNEL_AUTO)
        torch.cuda.synchronize()
        assert d_hits2.cpu().numpy().tobytes() == out.tobytes(), n


def test_zero_rays_launch_nothing(fctx, logged):
    import torch

    scene, rays = contract_rays(logged)
    fctx.upload(scene)
    d_hits = torch.full((4 * HIT,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.full((4,), 7, dtype=torch.int32, device="cuda:0")
    st = fctx.first_hits_device(0, 0, 4, d_hits.data_ptr(), d_cnt.data_ptr(), S, rtow.KERNEL_AUTO, 0, True)
    assert st.segments == 0 and st.prim_tests == 0 and st.node_tests == 0 and st.kernel_ms == 0.0
    assert np.all(d_hits.cpu().numpy() == 0xAB) and np.all(d_cnt.cpu().numpy() == 7)
    assert rtow.lib().rtow_first_hits_device(fctx._h, 0, 0, None, 0, 1, None, None, None, None) == rtow.RTOW_OK
    hits, counts = fctx.first_hits(np.empty(0, dtype=rtow.RAY_DTYPE), 5, S)
    assert hits.shape == (0, 5) and counts.shape == (0,)


def test_argument_errors_and_lean_upload_residency(logged):
    import torch

    scene, rays = contract_rays(logged)
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.first_hits(rays, 4, S)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        hits, counts, st = c.first_hits(rays, 4, rtow.F64_FAST, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and st.segments == len(rays)
        with pytest.raises(rtow.RtowError) as q:
            c.first_hits(rays, 4, rtow.F64_FAST, rtow.KERNEL_BVH)
        with pytest.raises(rtow.RtowError) as i:
            c.intersect(rays, rtow.F64_FAST, rtow.KERNEL_BVH)
        assert "(-4)" in str(q.value) and str(q.value).split(": ", 1)[1] == str(i.value).split(": ", 1)[1]
        for prec, kern, k in ((rtow.F32, rtow.KERNEL_AUTO, 4), (rtow.F64_FAST, rtow.KERNEL_REFTREE, 4),
                              (rtow.F64_STRICT, rtow.KERNEL_REFTREE, 4), (7, 0, 4), (0, 9, 4), (0, 0, 0), (0, 0, 9),
                              (0, 0, -1)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.first_hits(rays, k, prec, kern)
        L = rtow.lib()
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
        d_hits = torch.zeros(16 * 4 * HIT + 64, dtype=torch.uint8, device="cuda:0")
        d_cnt = torch.zeros(64, dtype=torch.int32, device="cuda:0")
        pr, ph, pc = d_rays.data_ptr(), d_hits.data_ptr(), d_cnt.data_ptr()
        call = lambda r, n, k, h, cn: L.rtow_first_hits_device(  # noqa: E731
            c._h, 1, 0, C.c_void_p(r) if r else None, n, k, C.c_void_p(h) if h else None, C.c_void_p(cn) if cn else None,
            None, None)
        for what, args in (("rays + 8", (pr + 8, 4, 4, ph, pc)), ("hits + 4", (pr, 4, 4, ph + 4, pc)),
                           ("counts + 2", (pr, 4, 4, ph, pc + 2))):
            assert call(*args) == rtow.RTOW_EINVAL, what
            assert b"aligned" in L.rtow_last_error(), what
        for what, args in (("n < 0", (pr, -1, 4, ph, pc)), ("NULL rays", (0, 1, 4, ph, pc)), ("NULL hits", (pr, 1, 4, 0, pc)),
                           ("n too large", (pr, (1 << 31) - 63, 4, ph, pc))):
            assert call(*args) == rtow.RTOW_EINVAL, what
        assert call(pr, 4, 4, ph, 0) == rtow.RTOW_OK  # (NULL counts is allowed)
        torch.cuda.synchronize()
        assert np.all(d_cnt.cpu().numpy() == 0)
    finally:
        c.close()


def test_side_stream_right_after_upload_on_a_fresh_context(fctx, logged):
    import torch

    scene, view, log = logged["suzanne"]
    rays = mesh_rays(log, n=20000)
    fctx.upload(scene)
    ref_h, ref_c = fctx.first_hits(rays, 4, S, rtow.KERNEL_AUTO)
    side = torch.cuda.Stream(device="cuda:0")
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.zeros(len(rays) * 4 * HIT, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(len(rays), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for builder in BUILDERS.values():
        c = rtow.Context(0)
        try:
            c.set_builder(builder)
            c.upload(scene)  # no wait: the query on the side stream must find the scene complete
            c.first_hits_device(d_rays.data_ptr(), len(rays), 4, d_hits.data_ptr(), d_cnt.data_ptr(), S, rtow.KERNEL_AUTO,
                                side.cuda_stream, False)
            side.synchronize()
            assert d_hits.cpu().numpy().tobytes() == ref_h.tobytes(), builder
            assert np.array_equal(d_cnt.cpu().numpy(), ref_c), builder
        finally:
            c.close()


def test_two_calls_identical_kernel_used_and_brute_counts_its_tests(fctx, logged, handmade):
    scene, view, log = logged["cover_moving"]
    fctx.upload(scene)
    rays = np.concatenate([lattice_rays(60), rays_of(log[:20000])])
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        for k in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            a = fctx.first_hits(rays, 5, prec, k)
            hb, cb, st = fctx.first_hits(rays, 5, prec, k, want_stats=True)
            assert a[0].tobytes() == hb.tobytes() and np.array_equal(a[1], cb), (prec, k)
            want = {rtow.KERNEL_AUTO: rtow.KERNEL_GRID, rtow.KERNEL_BVH4: rtow.KERNEL_BVH}.get(k, k)
            assert st.kernel_used == want, (prec, k)
            assert st.node_tests > 0 and st.prim_tests > 0 and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
            assert st.segments == len(rays) and st.samples == 0 and st.local_rows == 0
    hscene, hview, sets, refs = handmade
    fctx.upload(hscene.c)
    _, _, st = fctx.first_hits(sets["finite"], 8, S, rtow.KERNEL_AUTO, want_stats=True)
    walked = int((sets["finite"]["tmax"] >= 0.001).sum())
    assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0
    assert st.prim_tests == walked * len(hview.kind)  # (a ray with an empty interval skips the walk)


def test_first_hits_leave_the_render_and_the_closest_hit_query_untouched(logged):
    """A render and an rtow_intersect before and after ten first-hits calls: bit-identical; the profile ring counts the
    render launches only."""
    import torch

    scene, view, log = logged["cover_moving"]
    rays = rays_of(log[:30000])
    c = rtow.Context(0)
    try:
        c.upload(scene)
        cfg = rtow.make_config(120, 80, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((80, 120, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        hits_before = c.intersect(rays, S, rtow.KERNEL_BVH)
        assert c.profile_collect()[1] == 1
        for k in range(10):
            c.first_hits(rays, 1 + k % 8, rtow.F64_STRICT if k % 2 else rtow.F64_FAST, k % 4)
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
        assert c.intersect(rays, S, rtow.KERNEL_BVH).tobytes() == hits_before.tobytes()
    finally:
        c.close()
