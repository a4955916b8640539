"""k-nearest queries (rtow_nearest / rtow_nearest_device) on the GPU.

The strict build is checked ANSWER BY ANSWER against the reference of nearest_ref.py — the numpy mirror's distance matrix
sorted by (dist, insertion index), filtered by max_dist and cut at k: every field bit for bit, prim exact (the tie rule
names one primitive) — for k in {1, 2, 5, 8} under BRUTE, BVH, GRID (answered by BVH), BVH4 and AUTO with both builders,
on the hand-made scene, the cover scenes, suzanne (also inserted in a permuted order), the edge meshes and the sphere
scenes, and on the 96.8k mesh; after a refit; k = 1 against the closest-point query.  The fast build goes through
nearest_ref.FastChecker.  The contracts (max_dist, ragged counts, guards, NULL counts, errors, residency, ordering, no
side effects) close the file.
"""
import math

import numpy as np
import pytest

import accel_images as ai
import nearest_ref as nr
import point_ref as pr
import rtow
from nearest_cases import assert_strict, cut
from point_cases import KERNELS, point_sets
from support_fixtures import big_mesh, logged, pctx  # noqa: F401
from support_oracle import LOGGED, rays_of, same_bits
from support_scenes import SceneView, _set_order, deform, handmade_scene, scene_of, suzanne_tris, to_scene
from support_tables import BUILDERS

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 8)
EDGE = ["n4", "coincident", "zero_area"]
SPHERES = ["negative_radius", "same_centre"]
GREYS = tuple((ai.MAT_LAMBERTIAN, (g, g, g), 0.0, 1.5) for g in (0.3, 0.5, 0.7))


def upload(ctx, sc, builder):
    ctx.set_builder(builder)
    ctx.upload(sc)


def case(name, logged, keep):
    """(scene to upload, records, material per insertion index, ray log or None, times) of a scene by name."""
    if name == "handmade":
        hs = handmade_scene()
        keep.append(hs)
        view = SceneView(hs)
        return hs.c, pr.records(view), view.prim_mat, None, (0.0, 0.5, 1.0)
    if name in LOGGED:
        hs, view, log = logged[name]
        return hs.c, pr.records(view), view.prim_mat, log, ((0.0, 0.5, 1.0) if name == "cover_moving" else (0.0,))
    if name == "suzanne_permuted":
        G = ai.mesh_geometry(suzanne_tris(1), mats=GREYS)
        perm, rec, mats = nr.permuted_records(G, 3)
        return _set_order(to_scene(G, keep), G, keep, perm), rec, mats, None, (0.0,)
    # (the edge meshes carry one material here; bit-identical triangles with different materials are the case of
    # test_gpu_exact_nearest.py::test_material_follows_the_primitive_on_coincident_triangles)
    G = ai.mesh_geometry(ai.edge_meshes()[name]) if name in EDGE else ai.sphere_edge_scenes()[name]
    return scene_of(G, keep), pr.make_records(G.sph, G.mov, G.tri), G.pmat, None, (0.0,)


def sets_of(rec, log, tm, n=400):
    """near (where there is a ray log), volume, random and the special points (vertices, edge points, centres)."""
    sets = point_sets(rec, log, n, 7)
    sets["special"] = (pr.surface_points(rec, tm, 11), math.inf)
    return sets


# ---------------------------------------------------------------------------------------------------- strict ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["handmade"] + list(LOGGED) + EDGE + SPHERES + ["suzanne_permuted"])
def test_strict_equals_the_reference_every_kernel(pctx, logged, name, builder):
    keep = []
    sc, rec, mats, log, times = case(name, logged, keep)
    upload(pctx, sc, BUILDERS[builder])
    ties = 0
    for tm in times:
        for sname, (pts, md) in sets_of(rec, log, tm).items():
            ref8 = nr.reference(rec, mats, pts, tm, md, 8)
            d = ref8[0]["dist"]
            ties += int(np.sum((d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])))
            q = rtow.make_point_queries(pts, tm, md)
            for kname, kern in KERNELS.items():
                _, cp = pctx.closest_point(q[:1], rtow.F64_STRICT, kern, want_stats=True)
                for k in KS:
                    hits, counts, st = pctx.nearest(q, k, rtow.F64_STRICT, kern, want_stats=True)
                    assert_strict((hits, counts), cut(ref8, k), (name, builder, tm, sname, kname, k))
                    assert st.segments == len(pts)
                    assert st.kernel_used == cp.kernel_used, (name, builder, kname, st.kernel_used)
                if name in LOGGED or name == "handmade":
                    # GRID is answered by BVH; AUTO takes the 4-wide image where there is one (triangle meshes, both
                    # builders), else the binary one; BVH4 falls back to BVH on a scene with spheres
                    b4 = rtow.KERNEL_BVH4 if rec.ns + rec.nm == 0 else rtow.KERNEL_BVH
                    want = {rtow.KERNEL_GRID: rtow.KERNEL_BVH, rtow.KERNEL_AUTO: b4, rtow.KERNEL_BVH4: b4}.get(kern, kern)
                    assert cp.kernel_used == want, (name, builder, kname, cp.kernel_used)
    if name == "coincident":
        assert ties > 1000  # (forty copies of one triangle: every list is one tie, in insertion order)
    if name == "n4":
        assert rec.n == 4  # fewer primitives than k: counts of 4 under k = 5 and 8


_BIG = {}


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mesh_strict_and_pruning(pctx, big_mesh, builder):
    scene, view, log = big_mesh
    rec = pr.records(view)
    upload(pctx, scene.c, BUILDERS[builder])
    sets = point_sets(rec, log, 300, 9)
    for sname in ("near", "random"):
        pts, md = sets[sname]
        if sname not in _BIG:  # (the mirror over 96.8k triangles: once per point set, for both builders)
            _BIG[sname] = nr.reference(rec, view.prim_mat, pts, 0.0, md, 8)
        q = rtow.make_point_queries(pts, 0.0, md)
        for kname in ("bvh", "bvh4", "auto"):
            hits, counts, st = pctx.nearest(q, 8, rtow.F64_STRICT, KERNELS[kname], want_stats=True)
            assert_strict((hits, counts), _BIG[sname], ("m96k", builder, sname, kname))
            if sname == "near":
                assert st.kernel_used in (rtow.KERNEL_BVH, rtow.KERNEL_BVH4)
                per_query = st.prim_tests / len(pts)
                print(f"m96k {builder} {kname}: {per_query:.1f} primitive tests, {st.node_tests / len(pts):.1f} node tests"
                      f" per query (k = 8, near set)")
                # the ball of max_dist (5 % of the extent) limits what any k can reach: the closest-point test's bound
                assert per_query <= 0.02 * rec.n, (builder, kname, per_query)


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_k1_is_the_closest_point_query(pctx, logged, name):
    """On the same queries, strict and fast: dist bit for bit on every query, and the whole record (point included) bit
    for bit wherever the two queries name the same primitive.  They name different primitives only in an exact tie —
    the closest-point query may report any of the tied primitives, with that primitive's point, the k-nearest query the
    lowest insertion index — and two triangles tie exactly along a shared edge with points that differ in the last bits
    (on suzanne: 158 of 300 random queries tie, 61 with differing points, by the mirror).  There the closest-point
    record must be, bit for bit, a later entry of the k = 8 list at the same dist (or that list is all one tie)."""
    scene, view, log = logged[name]
    rec = pr.records(view)
    upload(pctx, scene.c, rtow.BUILDER_HOST_SAH)
    other = 0
    for sname, (pts, md) in point_sets(rec, log, 300, 15).items():
        q = rtow.make_point_queries(pts, 0.5, md)
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            for kern in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_BVH4, rtow.KERNEL_AUTO):
                cp = pctx.closest_point(q, prec, kern)
                hits, counts = pctx.nearest(q, 1, prec, kern)
                what = (name, sname, prec, kern)
                first = np.ascontiguousarray(hits[:, 0])
                assert same_bits(first["dist"], cp["dist"]), what
                assert np.array_equal(counts, (cp["prim"] >= 0).astype(np.int32)), what
                same = first["prim"] == cp["prim"]
                assert nr.same_answers(first[same], cp[same]), (what, nr.first_difference(first[same], cp[same]))
                if same.all():
                    continue
                h8, _ = pctx.nearest(q, 8, prec, kern)
                for i in np.nonzero(~same)[0]:
                    other += 1
                    assert first["prim"][i] < cp["prim"][i], (what, i)  # the tie goes to the lowest insertion index
                    tied = h8[i][h8["dist"][i].view(np.uint64) == cp["dist"][i:i + 1].view(np.uint64)]
                    found = [j for j in range(len(tied)) if nr.same_answers(tied[j:j + 1], cp[i:i + 1])]
                    assert len(found) == 1 or len(tied) == 8, (what, i, tied["prim"].tolist(), int(cp["prim"][i]))
    if name == "suzanne":
        assert other > 0  # (a mesh: ties along shared edges)


# ------------------------------------------------------------------------------------------------------ fast ---
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_fast_build_meets_its_contract(pctx, logged, name):
    scene, view, log = logged[name]
    rec = pr.records(view)
    upload(pctx, scene.c, rtow.BUILDER_HOST_SAH)
    sets = point_sets(rec, log, 150, 13)
    tm = 0.5
    short = 0
    for sname in ("random", "near"):
        pts, md = sets[sname]
        q = rtow.make_point_queries(pts, tm, md)
        ck = nr.FastChecker(rec, view.prim_mat, pts, tm, md)
        for kern in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_BVH4):
            hits, counts = pctx.nearest(q, 8, rtow.F64_FAST, kern)
            s = ck.check(hits, counts, 8, (name, sname, kern))
            print(f"{name} {sname} kernel {kern}: {s['entries']} entries, {s['exact_pairs']} exact pairs, worst dist "
                  f"{s['worst_dist']:.3f} of its band")
            if sname == "near":
                short += int(np.sum(counts < 8))
            else:
                assert np.all(counts == 8)
    assert short > 0  # the near set's radius leaves lists short of k


# ------------------------------------------------------------------------------------------------- semantics ---
def test_max_dist_semantics(pctx, logged):
    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    upload(pctx, scene.c, rtow.BUILDER_HOST_SAH)
    pts, _ = point_sets(rec, log, 200, 17)["near"]
    full, _ = nr.reference(rec, view.prim_mat, pts, 0.0, math.inf, 8)
    d = full["dist"]
    for kern in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
        for j in (0, 3, 6):
            alone = d[:, j + 1] > d[:, j]  # no tie follows entry j
            assert alone.sum() > 100
            h, c = pctx.nearest(rtow.make_point_queries(pts, 0.0, d[:, j]), 8, rtow.F64_STRICT, kern)
            assert np.all(c[alone] == j + 1)  # equal to the j-th distance: inclusive
            assert nr.same_answers(np.ascontiguousarray(h[alone][:, :j + 1]), np.ascontiguousarray(full[alone][:, :j + 1]))
            assert np.all(h["prim"][alone][:, j + 1:] == -1)
            below = np.nextafter(d[:, j], -np.inf)
            first = alone & ((d[:, j] > d[:, j - 1]) if j else True)
            h, c = pctx.nearest(rtow.make_point_queries(pts, 0.0, below), 8, rtow.F64_STRICT, kern)
            assert np.all(c[first] == j)  # the double just below: entry j is out
        for md in (math.nan, -1.0, -1e-300):
            h, c, st = pctx.nearest(rtow.make_point_queries(pts, 0.0, md), 8, rtow.F64_STRICT, kern, want_stats=True)
            assert np.all(c == 0) and nr.same_answers(h, nr.miss_records(h.shape))
            assert st.prim_tests == 0 and st.node_tests == 0  # the walk is skipped


def test_ragged_guards_null_counts_side_stream_and_errors(logged):
    import torch

    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    pts, md = point_sets(rec, log, 130, 23)["near"]
    q = rtow.make_point_queries(pts, 0.0, md)
    k = 5
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.nearest(q, k, rtow.F64_STRICT)
        c.upload(scene.c)
        dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
        dh = torch.full((len(q) * k * 48 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        dc = torch.full((len(q) + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        # a side stream right after the upload on a fresh context: ordered behind it
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        c2 = rtow.Context(0)
        try:
            c2.upload(scene.c)
            c2.nearest_device(dq.data_ptr(), len(q), k, dh.data_ptr(), dc.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_BVH,
                              stream=s.cuda_stream)
            s.synchronize()
        finally:
            c2.close()
        ref_h, ref_c = c.nearest(q, k, rtow.F64_STRICT, rtow.KERNEL_BVH)
        assert_strict((ref_h, ref_c), nr.reference(rec, view.prim_mat, pts, 0.0, md, k), "host form")
        got_h, got_c = dh.cpu().numpy(), dc.cpu().numpy()
        assert got_h[: len(q) * k * 48].tobytes() == ref_h.tobytes() and np.all(got_h[len(q) * k * 48:] == 0xAB)
        assert np.array_equal(got_c[: len(q)], ref_c) and np.all(got_c[len(q):] == 0x5A5A5A5A)
        # n == 0 launches nothing; ragged n leaves the guards alone, with and without counts
        st = c.nearest_device(0, 0, k, 0, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.segments == 0 and st.prim_tests == 0
        for n in (1, 63, 64, 65, 130):
            for with_counts in (True, False):
                dh.fill_(0xCD)
                dc.fill_(0x5A5A5A5A)
                c.nearest_device(dq.data_ptr(), n, k, dh.data_ptr(), dc.data_ptr() if with_counts else 0, rtow.F64_STRICT,
                                 rtow.KERNEL_BVH)
                torch.cuda.synchronize()
                g, gc = dh.cpu().numpy(), dc.cpu().numpy()
                assert g[: n * k * 48].tobytes() == ref_h[:n].tobytes(), n
                assert np.all(g[n * k * 48:] == 0xCD), n
                assert np.array_equal(gc[:n], ref_c[:n]) if with_counts else np.all(gc[:n] == 0x5A5A5A5A), n
                assert np.all(gc[n:] == 0x5A5A5A5A), n
        # errors: k out of range, binary32, the reference tree, misaligned buffers
        for bad_k in (0, 9, -1):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.nearest(q, bad_k, rtow.F64_STRICT)
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.nearest_device(dq.data_ptr(), 4, bad_k, dh.data_ptr(), dc.data_ptr(), rtow.F64_STRICT)
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_STRICT, rtow.KERNEL_REFTREE),
                           (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, rtow.KERNEL_AUTO), (rtow.F64_STRICT, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.nearest(q, k, prec, kern)
        for args in ((dq.data_ptr() + 8, dh.data_ptr(), dc.data_ptr()), (dq.data_ptr(), dh.data_ptr() + 8, dc.data_ptr()),
                     (dq.data_ptr(), dh.data_ptr(), dc.data_ptr() + 2)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.nearest_device(args[0], 4, k, args[1], args[2], rtow.F64_STRICT, rtow.KERNEL_BVH)
        assert np.all(dh.cpu().numpy()[130 * k * 48:] == 0xCD)  # (the refused calls wrote nothing)
    finally:
        c.close()


def test_lean_upload_residency(logged):
    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    pts, md = point_sets(rec, log, 100, 29)["near"]
    q = rtow.make_point_queries(pts, 0.0, md)
    c = rtow.Context(0)
    try:
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        h, n, st = c.nearest(q, 8, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0  # AUTO never fails on a resident scene
        assert_strict((h, n), nr.reference(rec, view.prim_mat, pts, 0.0, md, 8), "lean auto")
        for kern in (rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
                c.nearest(q, 8, rtow.F64_STRICT, kern)
    finally:
        c.close()


def test_refit_equals_the_reference_and_a_fresh_upload(pctx):
    G = ai.mesh_geometry(suzanne_tris(1), mats=GREYS)
    keep = []
    pctx.set_builder(rtow.BUILDER_HOST_SAH)
    pctx.upload(scene_of(G, keep))
    H = deform(G, lambda p: p * np.array([1.2, 0.9, 1.0]) + np.array([0.1, -0.2, 0.3]))
    pctx.refit(scene_of(H, keep))
    rec = pr.make_records(H.sph, H.mov, H.tri)
    pts = np.random.default_rng(19).uniform(-2, 2, size=(400, 3))
    want = nr.reference(rec, H.pmat, pts, 0.0, math.inf, 8)
    q = rtow.make_point_queries(pts)
    fresh = rtow.Context(0)
    try:
        fresh.set_builder(rtow.BUILDER_HOST_SAH)
        fresh.upload(scene_of(H, keep))
        for kern in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_BVH4):
            a = pctx.nearest(q, 8, rtow.F64_STRICT, kern)
            assert_strict(a, want, ("refit", kern))
            b = fresh.nearest(q, 8, rtow.F64_STRICT, kern)
            assert_strict(b, want, ("fresh", kern))
            assert a[0].tobytes() == b[0].tobytes()  # (the tie rule: the same primitives, whatever the leaf order)
    finally:
        fresh.close()


def test_nearest_queries_leave_the_render_and_closest_point_untouched(logged):
    scene, view, log = logged["cover_moving"]
    rec = pr.records(view)
    pts, md = point_sets(rec, log, 300, 31)["near"]
    q = rtow.make_point_queries(pts, 0.3, md)
    rays = rays_of(log[:2000])
    cfg = rtow.make_config(64, 48, 4, 2, 20, seed=5, precision=rtow.F64_STRICT)
    a = rtow.Context(0)
    b = rtow.Context(0)
    try:
        img_a, _ = a.render(scene, cfg)
        a.upload(scene.c)
        cp_a = a.closest_point(q, rtow.F64_STRICT, rtow.KERNEL_BVH)
        hit_a = a.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_GRID)
        img_b, _ = b.render(scene, cfg)
        b.upload(scene.c)
        for kern in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_AUTO):
            for k in (1, 8):
                b.nearest(q, k, rtow.F64_STRICT, kern)
                b.nearest(q, k, rtow.F64_FAST, kern)
        cp_b = b.closest_point(q, rtow.F64_STRICT, rtow.KERNEL_BVH)
        hit_b = b.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_GRID)
        img_c, _ = b.render(scene, cfg)
        assert np.array_equal(img_a, img_b) and np.array_equal(img_a, img_c)
        assert cp_a.tobytes() == cp_b.tobytes() and hit_a.tobytes() == hit_b.tobytes()
    finally:
        a.close()
        b.close()
