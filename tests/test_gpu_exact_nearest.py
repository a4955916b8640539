"""k-nearest lists of both builds against exact distances (tests/nearest_ref.py: FastChecker) on the GPU.

Every walk (BRUTE, BVH, GRID answered by BVH, BVH4, AUTO, with their fallbacks; both builders) in F64_STRICT (k = 1, 2,
5, 8) and F64_FAST (k = 1, 3, 8), with per-lane times and radii, on the point sets of the closest-point checker
(point_ref.all_sets: on vertices, edges and faces and 1e-9 off them, at sphere centres and 1e-12 off them, from 10 to
1e100 extents outside the scene, where squares overflow, near the surfaces with a short max_dist, and the two batches
whose lanes mix times and radii) and one more mixed batch, nearest_cases.mixed_kth, whose radii sit at, just below and at
half of the mirror's 1st, 4th and 8th distance — on the hand-made scene, the cover scenes, suzanne, the edge meshes, the
sphere edge scenes and the 96.8k mesh (the binary16 top of the 4-wide tree with the spill stack), and after translate,
scale1000 and flatten refits, where the strict lists must also equal, byte for byte, those of a fresh upload.

The strict build must equal the reference (nearest_ref.reference with the set's per-lane times and radii) bit for bit
and pass the exact checker at 32 u; in mixed_kth its counts at d_j and at the double below are also asserted straight
from the unbounded list.  The fast build must pass the exact checker at 64 u.  No query is sampled or exempted.  One
line per scene and build is printed: queries, entries, exact pairs, the worst dist, on-surface and consistency errors in
units of their bands, the lists short of k, and the completeness decisions that needed exact arithmetic.  (On the 96.8k
mesh the sets go to the device joined into one batch, nearest_cases.joined: a far query walks the whole mesh in one
lane, so there the calls are the cost.)

The last test uploads bit-identical triangles with alternating materials: every record of every query that reports
both prim and material must carry the material of the primitive it names.
"""
import math

import numpy as np
import pytest

import accel_images as ai
import big_mixed as bm
import nearest_cases as nc
import nearest_ref as nr
import point_ref as pr
import rtow
from point_cases import EDGE_MESHES, KERNELS, REFITS, SEED, SPHERE_SCENES, geometry_case, point_sets, small_case
from support_fixtures import big_mesh, fresh, logged, pctx  # noqa: F401
from support_oracle import LOGGED
from support_scenes import motions, scene_of
from support_tables import BUILDERS

pytestmark = pytest.mark.gpu

BUILDS = {"strict": (rtow.F64_STRICT, nc.KS_STRICT), "fast": (rtow.F64_FAST, nc.KS_FAST)}


def run_case(ctx, name, upload, rec, mats, sets, refit=None, brute=True, node_bytes=None, fresh=None, kth=0, resident=None):
    """Every kernel x build x builder x k on every point set of `sets` (nearest_cases.nearest_sets); `upload` is what
    ctx.upload takes, `refit` (optional) a scene refitted over it — `rec` and `mats` are then the refitted geometry's,
    and `fresh` a second context that uploads `refit` itself; `kth`: see nearest_cases.Batch; resident(ctx, builder name): assertions on
    what the upload left resident."""
    batches = [nc.Batch(rec, mats, *s, kth=kth) for s in sets]
    mesh = rec.ns + rec.nm == 0
    b4 = rtow.KERNEL_BVH4 if mesh else rtow.KERNEL_BVH
    want = {rtow.KERNEL_GRID: rtow.KERNEL_BVH, rtow.KERNEL_AUTO: b4, rtow.KERNEL_BVH4: b4}
    total = {}
    for bname, builder in BUILDERS.items():
        ctx.set_builder(builder)
        try:
            ctx.upload(upload)
            if refit is not None:
                ctx.refit(refit)
                fresh.set_builder(builder)
                fresh.upload(refit)
            if node_bytes is not None:
                assert ctx.build_info().bvh4_node_bytes == node_bytes, (name, bname)
            if resident is not None:
                resident(ctx, bname)
            for kname, kern in KERNELS.items():
                if kname == "brute" and (bname == "device" or not brute):
                    continue  # (the brute force does not depend on the builder; 96,800 tests per query are not a test)
                for build, (prec, ks) in BUILDS.items():
                    for b in batches:
                        for k in ks:
                            what = (name, b.name, bname, kname, build, k)
                            hits, counts, st = ctx.nearest(b.queries, k, prec, kern, want_stats=True)
                            assert st.kernel_used == want.get(kern, kern), (what, st.kernel_used)
                            assert st.segments == len(b.pts), what
                            if build == "strict":
                                nc.assert_strict((hits, counts), nc.cut(b.ref8, k), what)
                                b.check_kth(hits, counts, k, what)
                                if fresh is not None:
                                    fh, fc = fresh.nearest(b.queries, k, prec, kern)
                                    assert fh.tobytes() == hits.tobytes() and fc.tobytes() == counts.tobytes(), what
                            total[build] = nc.add_stats(total.get(build), b.ck.check(hits, counts, k, what, build))
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
            if fresh is not None:
                fresh.set_builder(rtow.BUILDER_AUTO)
    for build, t in total.items():
        nc.finish_stats(t, batches, build)
        print(f"\nnearest {name} {build}: {sum(len(b.pts) for b in batches)} points in {len(batches)} sets; answers: "
              f"{nr.stats_line(t)}")
    return total


@pytest.mark.parametrize("name", ["handmade"] + list(LOGGED) + EDGE_MESHES + SPHERE_SCENES)
def test_small_scenes(pctx, logged, name):
    keep = []
    upload, rec, mats, near, rnd = small_case(name, logged, keep)
    total = run_case(pctx, name, upload, rec, mats, nc.nearest_sets(rec, SEED, near, rnd))
    assert total["strict"]["overflow"] > 0 and total["fast"]["overflow"] > 0  # (the overflow set took the overflow rule)
    assert total["strict"]["short"] > 0 and total["fast"]["short"] > 0


def test_big_mesh(pctx, big_mesh):
    hs, view, log = big_mesh
    rec = pr.records(view)
    ps = point_sets(rec, log, pr.SIZES_BIG["mixed"], 9)
    sets = nc.nearest_sets(rec, SEED, ps["near"], ps["random"][0], sizes=pr.SIZES_BIG)
    assert sum(len(s[1]) for s in sets) <= 100
    assert {"far@0", "overflow@0", "mixed", "mixed_strict", "mixed_kth"} <= {s[0] for s in sets}
    sets, kth = nc.joined(sets)  # (every set, in one call per walk, build and k)
    total = run_case(pctx, "mesh96k", hs.c, rec, view.prim_mat, sets, brute=False, node_bytes=64, kth=kth)
    assert kth == pr.SIZES_BIG["mixed"] and total["strict"]["overflow"] > 0 and total["fast"]["overflow"] > 0


@pytest.mark.parametrize("name,motion", REFITS + [("mesh96k", "scale1000")])
def test_after_refit(pctx, fresh, logged, big_mesh, name, motion):
    big = name == "mesh96k"
    G = ai.Geometry.of_scene((big_mesh if big else logged[name])[0].c)
    keep = []
    base = scene_of(G, keep)
    new, rec, mats = geometry_case(motions(G)[motion][0], keep)
    sets = nc.nearest_sets(rec, SEED, sizes=pr.SIZES_BIG if big else pr.SIZES, refit=True)
    if big:
        sets, _ = nc.joined(sets)
    run_case(pctx, f"refit/{name}/{motion}", base, rec, mats, sets, refit=new, brute=not big, fresh=fresh)


# ---------------------------------------------------------------------- material follows the primitive on twins ---
def _twin_queries(G, stack):
    """Rays through the coincident stack and through the other triangles, and points around both."""
    g = np.random.default_rng(3)
    tri = G.tri.reshape(-1, 3, 3)
    w = g.dirichlet([1.0, 1.0, 1.0], size=len(tri) * 4)
    target = np.einsum("nk,nkj->nj", w, np.repeat(tri, 4, axis=0))
    origin = target + g.normal(size=target.shape) * 0.7 + [0.0, 0.0, 3.0]
    d = target - origin
    rays = rtow.make_rays(origin, d / np.linalg.norm(d, axis=1, keepdims=True))
    pts = np.concatenate([target + g.normal(size=target.shape) * 0.02, g.uniform(-0.2, 1.2, size=(61, 3)),
                          tri[0].mean(0) + g.normal(size=(40, 3)) * 1e-3])
    return rays, pts, slice(len(pts) - 40, len(pts))


@pytest.mark.parametrize("refit", [False, True], ids=["upload", "translate"])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_material_follows_the_primitive_on_coincident_triangles(pctx, builder, refit):
    G, stack = nc.coincident_two_materials()
    keep = []
    mats = np.asarray(G.pmat)
    assert len(set(mats[:stack].tolist())) == 2 and np.all(mats[:stack:2] != mats[1:stack:2])
    pctx.set_builder(BUILDERS[builder])
    try:
        pctx.upload(scene_of(G, keep))
        if refit:
            G = motions(G)["translate"][0]
            pctx.refit(scene_of(G, keep))
            assert np.array_equal(mats, G.pmat)
        rec = pr.make_records(G.sph, G.mov, G.tri)
        rays, pts, at_stack = _twin_queries(G, stack)
        q = rtow.make_point_queries(pts)
        ref8 = nr.reference(rec, mats, pts, 0.0, math.inf, 8)
        assert np.all(ref8[0]["prim"][at_stack] == np.arange(8))  # (by the mirror: the stack is nearest there, one tie)
        for kname in ("bvh", "bvh4", "auto"):
            kern = KERNELS[kname]
            for prec in (rtow.F64_STRICT, rtow.F64_FAST):
                what = (builder, refit, kname, prec)
                seen = set()
                h = pctx.intersect(rays, prec, kern)
                hit = h["prim"] >= 0
                assert hit.sum() > len(rays) // 2, what
                assert np.array_equal(h["material"][hit], mats[h["prim"][hit]]), (what, "intersect")
                seen |= set(h["prim"][hit].tolist())
                fh, fc = pctx.first_hits(rays, 8, prec, kern)
                for j in range(8):
                    m = fc > j
                    assert np.array_equal(fh["material"][m, j], mats[fh["prim"][m, j]]), (what, "first_hits", j)
                    seen |= set(fh["prim"][m, j].tolist())
                cp = pctx.closest_point(q, prec, kern)
                assert np.all(cp["prim"] >= 0), what
                assert np.array_equal(cp["material"], mats[cp["prim"]]), (what, "closest_point")
                nh, ncnt = pctx.nearest(q, 8, prec, kern)
                assert np.all(ncnt == 8), what
                assert np.array_equal(nh["material"], mats[nh["prim"]]), (what, "nearest")
                # against the stack: the eight lowest insertion indices, each with its own material
                assert np.all(nh["prim"][at_stack] == np.arange(8)), (what, nh["prim"][at_stack][:2].tolist())
                assert np.all(nh["material"][at_stack] == mats[:8]), what
                if prec == rtow.F64_STRICT:
                    nc.assert_strict((nh, ncnt), ref8, what)
                # the rays met twins of both materials, so a swapped pairing could not have gone unseen
                assert len({int(mats[p]) for p in seen if p < stack}) == 2, (what, sorted(seen)[:8])
    finally:
        pctx.set_builder(rtow.BUILDER_AUTO)


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
def test_big_mixed(pctx):
    c = bm.case()
    total = run_case(pctx, "big_mixed", c.hs.c, c.rec, c.mats, bm.nearest_sets(c), resident=bm.resident)
    assert total["strict"]["overflow"] > 0 and total["strict"]["short"] > 0 and total["fast"]["short"] > 0
