"""Closest-point queries (rtow_closest_point / rtow_closest_point_device) on the GPU.

The strict build is checked POINT BY POINT against the numpy mirror of the kernel's formulas (point_ref.py): dist and
point bit for bit, prim one of the exactly tied minima, under BRUTE, BVH, GRID (answered by BVH), BVH4 and AUTO with both
builders, on the hand-made scene, the cover scene (static, and moving at three times), suzanne and the 96.8k mesh; and
after a deformed refit.  The fast build is checked against the exact distance within the bound of include/rtow.h.
Pruning is checked by its counters; the contracts (max_dist, ragged counts, ordering, residency, errors, no side effect
on the render or the ray queries) close the file.
"""
import math

import numpy as np
import pytest

import accel_images as ai
import point_ref as pr
import rtow
from point_cases import KERNELS, check_strict, point_sets
from support_fixtures import big_mesh, logged, pctx  # noqa: F401
from support_oracle import LOGGED, rays_of, same_bits
from support_scenes import SceneView, deform, handmade_scene, scene_of, suzanne_tris
from support_tables import BUILDERS

pytestmark = pytest.mark.gpu


class Expected:
    """The mirror's answer for a point set: min dist, tied class ids, per query."""

    def __init__(self, rec, pts, time, md):
        self.rec, self.pts, self.time = rec, pts, time
        self.md = np.broadcast_to(np.asarray(md, dtype=np.float64), (len(pts),))
        self.dmin, self.ties, _ = pr.nearest(rec, pts, time, self.md)


def upload(ctx, scene, builder):
    ctx.set_builder(builder)
    ctx.upload(scene.c)


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(LOGGED) + ["handmade"])
def test_strict_equals_the_mirror_every_kernel(pctx, logged, name, builder):
    if name == "handmade":
        scene = handmade_scene()
        view, log = SceneView(scene), None
    else:
        scene, view, log = logged[name]
    rec = pr.records(view)
    upload(pctx, scene, BUILDERS[builder])
    times = (0.0, 0.5, 1.0) if name in ("cover_moving", "handmade") else (0.0,)
    sets = point_sets(rec, log, 400, 7)
    if name == "handmade":
        extra = np.concatenate([view.tri[:, 0:3], view.tri[:, 3:6], 0.5 * (view.tri[:, 0:3] + view.tri[:, 6:9]),
                                view.sph[:, 0:3], [[0.0, 1.0, 0.85]]])
        sets["special"] = (extra, math.inf)
    for tm in times:
        for sname, (pts, md) in sets.items():
            exp = Expected(rec, pts, tm, md)
            q = rtow.make_point_queries(pts, tm, md)
            for kname, k in KERNELS.items():
                hits, st = pctx.closest_point(q, rtow.F64_STRICT, k, want_stats=True)
                check_strict(exp, view.prim_mat, hits, (name, builder, tm, sname, kname))
                assert st.segments == len(pts)
                # GRID is answered by BVH; AUTO takes the 4-wide image where there is one (triangle meshes, both
                # builders), else the binary one; BVH4 falls back to BVH on a scene with spheres
                b4 = rtow.KERNEL_BVH4 if bool(np.all(view.kind == rtow.PRIM_TRIANGLE)) else rtow.KERNEL_BVH
                want = {rtow.KERNEL_GRID: rtow.KERNEL_BVH, rtow.KERNEL_AUTO: b4, rtow.KERNEL_BVH4: b4}.get(k, k)
                assert st.kernel_used == want, (name, builder, kname, st.kernel_used)


_BIG = {}


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mesh_strict_and_pruning(pctx, big_mesh, builder):
    scene, view, log = big_mesh
    rec = pr.records(view)
    upload(pctx, scene, BUILDERS[builder])
    sets = point_sets(rec, log, 300, 9)
    for sname in ("near", "random"):
        pts, md = sets[sname]
        if sname not in _BIG:  # (the mirror over 96.8k triangles: once per point set, for both builders)
            _BIG[sname] = Expected(rec, pts, 0.0, md)
        exp = _BIG[sname]
        q = rtow.make_point_queries(pts, 0.0, md)
        for kname in ("bvh", "bvh4", "auto"):
            hits, st = pctx.closest_point(q, rtow.F64_STRICT, KERNELS[kname], want_stats=True)
            check_strict(exp, view.prim_mat, hits, ("m96k", builder, sname, kname))
            if sname == "near" and st.kernel_used in (rtow.KERNEL_BVH, rtow.KERNEL_BVH4):
                per_query = st.prim_tests / len(pts)
                # the walks prune: a ball of 5 % of the extent covers well under 2 % of the surface
                assert per_query <= 0.02 * rec.n, (builder, kname, per_query)


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_fast_build_within_its_bound(pctx, logged, name):
    scene, view, log = logged[name]
    rec = pr.records(view)
    upload(pctx, scene, rtow.BUILDER_HOST_SAH)
    pts, _ = point_sets(rec, log, 150, 13)["random"]
    tm = 0.5
    q = rtow.make_point_queries(pts, tm)
    # dist within the band of the exact distance of the reported primitive, and that primitive one the band allows: no
    # primitive is exactly nearer by more than the bands (point_ref.check_answers, which also checks the point)
    ck = pr.AnswerChecker(rec, view.prim_mat, pts, tm, math.inf)
    for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_BVH4):
        hits = pctx.closest_point(q, rtow.F64_FAST, k)
        assert np.all(hits["prim"] >= 0)
        ck.check(hits, "fast", (name, k))


def test_max_dist_semantics(pctx, logged):
    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    upload(pctx, scene, rtow.BUILDER_HOST_SAH)
    pts, _ = point_sets(rec, log, 200, 17)["near"]
    dmin, _, _ = pr.nearest(rec, pts, 0.0)
    for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
        h = pctx.closest_point(rtow.make_point_queries(pts, 0.0, dmin), rtow.F64_STRICT, k)
        assert np.all(h["prim"] >= 0) and same_bits(h["dist"], dmin)  # equal to the distance: a hit
        below = np.nextafter(dmin, -np.inf)
        h = pctx.closest_point(rtow.make_point_queries(pts, 0.0, below), rtow.F64_STRICT, k)
        assert np.all(h["prim"] == -1) and np.all(np.isinf(h["dist"]))  # just below: a miss
        for md in (math.nan, -1.0, -1e-300):
            h, st = pctx.closest_point(rtow.make_point_queries(pts, 0.0, md), rtow.F64_STRICT, k, want_stats=True)
            assert np.all(h["prim"] == -1) and np.all(h["kind"] == -1) and np.all(np.isinf(h["dist"]))
            assert st.prim_tests == 0 and st.node_tests == 0  # the walk is skipped
        h = pctx.closest_point(rtow.make_point_queries(pts, 0.0, math.inf), rtow.F64_STRICT, k)
        assert same_bits(h["dist"], dmin)


def test_refit_equals_the_mirror_and_a_fresh_upload(pctx):
    G = ai.mesh_geometry(suzanne_tris(1))
    keep = []
    pctx.set_builder(rtow.BUILDER_HOST_SAH)
    pctx.upload(scene_of(G, keep))
    H = deform(G, lambda p: p * np.array([1.2, 0.9, 1.0]) + np.array([0.1, -0.2, 0.3]))
    pctx.refit(scene_of(H, keep))
    rec = pr.make_records(H.sph, H.mov, H.tri)
    pts = np.random.default_rng(19).uniform(-2, 2, size=(500, 3))
    exp = Expected(rec, pts, 0.0, math.inf)
    q = rtow.make_point_queries(pts)
    fresh = rtow.Context(0)
    try:
        fresh.set_builder(rtow.BUILDER_HOST_SAH)
        fresh.upload(scene_of(H, keep))
        for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_BVH4):
            a = pctx.closest_point(q, rtow.F64_STRICT, k)
            check_strict(exp, H.pmat, a, ("refit", k))
            b = fresh.closest_point(q, rtow.F64_STRICT, k)
            # (the refitted tree keeps the uploaded leaf order, the fresh one has its own: an exact tie may name
            # another of the tied primitives, with that primitive's point)
            check_strict(exp, H.pmat, b, ("fresh", k))
            assert same_bits(a["dist"], b["dist"]), k
    finally:
        fresh.close()


def test_zero_ragged_side_stream_and_alignment(logged):
    import torch

    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    pts, md = point_sets(rec, log, 300, 23)["near"]
    q = rtow.make_point_queries(pts, 0.0, md)
    c = rtow.Context(0)
    try:
        c.upload(scene.c)
        # a side stream right after the upload on a fresh context: ordered behind it
        s = torch.cuda.Stream()
        dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
        dh = torch.full((len(q) * 48 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c2 = rtow.Context(0)
        try:
            c2.upload(scene.c)
            c2.closest_point_device(dq.data_ptr(), len(q), dh.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_BVH,
                                    stream=s.cuda_stream)
            s.synchronize()
        finally:
            c2.close()
        ref = c.closest_point(q, rtow.F64_STRICT, rtow.KERNEL_BVH)
        got = dh.cpu().numpy()
        assert got[: len(q) * 48].tobytes() == ref.tobytes()
        assert np.all(got[len(q) * 48:] == 0xAB)  # nothing beyond n
        # n == 0 launches nothing; ragged counts equal one batch
        st = c.closest_point_device(0, 0, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.segments == 0 and st.prim_tests == 0
        for n in (1, 63, 64, 65, 129, len(q) - 1):
            dh.fill_(0xCD)
            c.closest_point_device(dq.data_ptr(), n, dh.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_BVH)
            torch.cuda.synchronize()
            g = dh.cpu().numpy()
            assert g[: n * 48].tobytes() == ref[:n].tobytes(), n
            assert np.all(g[n * 48:] == 0xCD), n
        # misaligned buffers are refused
        for args in ((dq.data_ptr() + 8, dh.data_ptr()), (dq.data_ptr(), dh.data_ptr() + 8)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.closest_point_device(args[0], 4, args[1], rtow.F64_STRICT, rtow.KERNEL_BVH)
    finally:
        c.close()


def test_lean_upload_residency_errors_and_kernel_used(logged):
    scene, view, log = logged["cover_static"]
    rec = pr.records(view)
    pts, md = point_sets(rec, log, 100, 29)["near"]
    q = rtow.make_point_queries(pts, 0.0, md)
    exp = Expected(rec, pts, 0.0, md)
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.closest_point(q, rtow.F64_STRICT)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        h, st = c.closest_point(q, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0
        check_strict(exp, view.prim_mat, h, "lean auto")
        for k in (rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
                c.closest_point(q, rtow.F64_STRICT, k)
        for prec, k in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_STRICT, rtow.KERNEL_REFTREE),
                        (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, rtow.KERNEL_AUTO), (rtow.F64_STRICT, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.closest_point(q, prec, k)
    finally:
        c.close()


def test_point_queries_leave_the_render_and_the_ray_queries_untouched(logged):
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
        hit_a = a.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_GRID)
        img_b, _ = b.render(scene, cfg)
        b.upload(scene.c)
        for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_AUTO):
            b.closest_point(q, rtow.F64_STRICT, k)
            b.closest_point(q, rtow.F64_FAST, k)
        hit_b = b.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_GRID)
        img_c, _ = b.render(scene, cfg)
        assert np.array_equal(img_a, img_b) and np.array_equal(img_a, img_c)
        assert hit_a.tobytes() == hit_b.tobytes()
    finally:
        a.close()
        b.close()
