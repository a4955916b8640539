"""Closest-point queries of both builds against the exact nearest points (tests/point_ref.py: check_answers) on the GPU.

Every walk (BRUTE, BVH, GRID answered by BVH, BVH4, AUTO, with their fallbacks; both builders) in F64_STRICT and
F64_FAST, at the points where kernels go wrong: on vertices, edges and faces and 1e-9 off them, at sphere centres and
1e-12 off them, from 10 to 1e100 extents outside the scene, where squares overflow, near the surfaces with a short
max_dist, and in batches whose lanes mix times and max_dist values (NaN, negative, half and twice the distance, +inf,
and for the mirror to decide 0 on a surface, the distance itself and the double below it) — on the hand-made scene, the
cover scenes, suzanne, the edge meshes, the sphere edge scenes and the 96.8k mesh (the binary16 top of the 4-wide tree
with the spill stack), and after translate, scale1000 and flatten refits.  The strict build must equal the mirror bit for
bit (point_cases.check_strict) and pass check_answers at 32 u; the fast build must pass check_answers at 64 u:
dist within the header's band of the exact distance of the reported primitive, point on that primitive's exact surface
and consistent with dist, that primitive within the bands of the exact minimum, hit versus miss exact where max_dist
decides it, the miss record, no NaN.  No query is sampled or exempted.  One line per scene and build is printed: queries,
exact pairs, the worst dist, on-surface and consistency errors in units of their bands, hit/miss answers left open.
"""
import pytest

import accel_images as ai
import big_mixed as bm
import point_ref as pr
import rtow
from point_cases import (EDGE_MESHES, KERNELS, REFITS, SEED, SPHERE_SCENES, check_strict, geometry_case, point_sets,
                         small_case)
from support_fixtures import big_mesh, logged, pctx  # noqa: F401
from support_oracle import LOGGED
from support_scenes import motions, scene_of
from support_tables import BUILDERS

pytestmark = pytest.mark.gpu

BUILDS = {"strict": rtow.F64_STRICT, "fast": rtow.F64_FAST}


class Batch:
    """One point set: its queries, the checker of its answers, and what check_strict reads (the mirror's answer)."""

    def __init__(self, rec, mats, name, pts, times, md):
        self.name = name
        self.ck = pr.AnswerChecker(rec, mats, pts, times, md)
        self.queries = rtow.make_point_queries(self.ck.pts, self.ck.times, self.ck.md)
        self.rec, self.pts, self.time, self.md = rec, self.ck.pts, self.ck.times, self.ck.md
        self.dmin, self.ties = self.ck.mirror_dmin(), self.ck.ties


def run_case(ctx, name, upload, rec, mats, sets, refit=None, brute=True, node_bytes=None, resident=None):
    """Every kernel x build x builder on every point set of `sets` (point_ref.all_sets); `upload` is what ctx.upload
    takes, `refit` (optional) a scene refitted over it — `rec` and `mats` are then the refitted geometry's;
    resident(ctx, builder name): assertions on what the upload left resident."""
    batches = [Batch(rec, mats, *s) for s in sets]
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
            if node_bytes is not None:
                assert ctx.build_info().bvh4_node_bytes == node_bytes, (name, bname)
            if resident is not None:
                resident(ctx, bname)
            for kname, k in KERNELS.items():
                if kname == "brute" and (bname == "device" or not brute):
                    continue  # (the brute force does not depend on the builder; 96,800 tests per query are not a test)
                for build, prec in BUILDS.items():
                    for b in batches:
                        what = (name, b.name, bname, kname, build)
                        hits, st = ctx.closest_point(b.queries, prec, k, want_stats=True)
                        assert st.kernel_used == want.get(k, k), (what, st.kernel_used)
                        assert st.segments == len(b.pts), what
                        if build == "strict":
                            check_strict(b, mats, hits, what)
                        s = b.ck.check(hits, build, what)
                        t = total.setdefault(build, dict(s, queries=0, open=0, overflow=0))
                        for f in ("worst_dist", "worst_surface", "worst_consistency"):
                            t[f] = max(t[f], s[f])
                        for f in ("queries", "open", "overflow"):
                            t[f] += s[f]
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    for build, t in total.items():
        t["exact_pairs"] = sum(len(b.ck._exact) for b in batches)
        print(f"\npoints {name} {build}: {sum(len(b.pts) for b in batches)} points in {len(batches)} sets; answers: "
              f"{pr.stats_line(t)}")
    return total


@pytest.mark.parametrize("name", ["handmade"] + list(LOGGED) + EDGE_MESHES + SPHERE_SCENES)
def test_small_scenes(pctx, logged, name):
    keep = []
    upload, rec, mats, near, rnd = small_case(name, logged, keep)
    total = run_case(pctx, name, upload, rec, mats, pr.all_sets(rec, SEED, near, rnd))
    assert total["strict"]["overflow"] > 0 and total["fast"]["overflow"] > 0  # (the overflow set took the overflow rule)


def test_big_mesh(pctx, big_mesh):
    hs, view, log = big_mesh
    rec = pr.records(view)
    ps = point_sets(rec, log, pr.SIZES_BIG["mixed"], 9)
    sets = pr.all_sets(rec, SEED, ps["near"], ps["random"][0], sizes=pr.SIZES_BIG)
    assert sum(len(s[1]) for s in sets) <= 100
    run_case(pctx, "mesh96k", hs.c, rec, view.prim_mat, sets, brute=False, node_bytes=64)


@pytest.mark.parametrize("name,motion", REFITS + [("mesh96k", "scale1000")])
def test_after_refit(pctx, logged, big_mesh, name, motion):
    big = name == "mesh96k"
    G = ai.Geometry.of_scene((big_mesh if big else logged[name])[0].c)
    keep = []
    base = scene_of(G, keep)
    new, rec, mats = geometry_case(motions(G)[motion][0], keep)
    sets = pr.all_sets(rec, SEED, sizes=pr.SIZES_BIG if big else pr.SIZES, refit=True)
    run_case(pctx, f"refit/{name}/{motion}", base, rec, mats, sets, refit=new, brute=not big)


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
def test_big_mixed(pctx):
    c = bm.case()
    total = run_case(pctx, "big_mixed", c.hs.c, c.rec, c.mats, bm.point_sets(c), resident=bm.resident)
    assert total["strict"]["overflow"] > 0 and total["fast"]["overflow"] > 0


@pytest.mark.parametrize("motion", bm.REFITS)
def test_big_mixed_after_refit(pctx, motion):
    c, new = bm.case(), bm.refitted(motion)
    sets = pr.all_sets(new.rec, SEED, sizes=dict(bm.POINT_SIZES, random=50), refit=True)
    assert sum(len(s[1]) for s in sets) <= 500
    run_case(pctx, f"big_mixed/refit/{motion}", c.hs.c, new.rec, new.mats, sets, refit=new.hs.c, resident=bm.resident)
