"""Closest-hit and any-hit queries of both builds against the exact reference (tests/exact_hits.py) on the GPU.

Every walk (BRUTE, BVH, GRID, BVH4, with the render's fallbacks; both builders where a tree is involved) in F64_STRICT
and F64_FAST, on the rays where kernels go wrong: logged render segments, rays at and across shared edges and
vertices, tangent rays, rays at the triangle cut, rays leaving a surface, direction magnitudes from 1e-4 to 1e4, scenes
far from the origin and scenes after a refit.  On a decided ray every field must be the exact answer (t, point and a
sphere's normal within their bounds); an undecided ray's answer must be explainable by the band.  Counts per case are
printed: decided, undecided, rays whose t is not the exact t rounded, and the worst t error in units of its bound.
"""
import numpy as np
import pytest

import accel_images as ai
import big_mixed as bm
import exact_hits as ex
import rtow
from exact_cases import (BUILDS, SHARE, big_mesh, cover_tangent_rays, det_cut_rays, edge_rays, far_case,  # noqa: F401
                         handmade_tangent_rays, logged, magnitude_rays, mesh_case, refit_case, subsample, surface_rays)
from support_fixtures import qctx  # noqa: F401
from support_oracle import LOGGED, rays_of
from support_scenes import SceneView, handmade_scene, rays_for
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu


def run_case(ctx, name, upload, scene, rays, share=None, refit=None, resident=None, used=None):
    """Every walk x build x builder on `rays`; `upload` is what ctx.upload takes, `refit` (optional) a scene refitted
    over it — `scene` (exact_hits.Scene) is then the refitted geometry.  resident(ctx, builder name): assertions on what
    the upload left resident; used: walk name -> the kernel_used the closest-hit launch
    must report (the any-hit launch of the same request returns no statistics).  Returns the stats of every combination."""
    refs = {}
    has_tri = len(scene.tri) > 0

    def ref(build, unit_cut):
        key = (build, unit_cut and has_tri)
        if key not in refs:
            refs[key] = ex.Reference(scene, rays, build, unit_cut=key[1])
        return refs[key]

    lines, out = [], []
    for bname, builder in BUILDERS.items():
        ctx.set_builder(builder)
        try:
            ctx.upload(upload)
            if refit is not None:
                ctx.refit(refit)
            if resident is not None:
                resident(ctx, bname)
            for wname, walk in WALKS.items():
                if wname == "brute" and (bname == "device" or len(scene.kind) > 4096):
                    continue  # (the brute force does not depend on the builder; 96,800 tests per ray are not a test)
                for build, prec in BUILDS.items():
                    hits, st = ctx.intersect(rays, prec, walk, want_stats=True)
                    occ = ctx.occluded(rays, prec, walk)
                    assert used is None or st.kernel_used == used[wname], (name, bname, wname, build, st.kernel_used)
                    r = ref(build, build == ex.FAST and st.kernel_used == rtow.KERNEL_GRID)
                    s = ex.check(r, hits, occ, (name, bname, wname, build, st.kernel_used))
                    out.append(dict(s, build=build, walk=wname, builder=bname, used=st.kernel_used))
                    lines.append(f"  {bname:6s} {wname:5s}(used {st.kernel_used}) {build:6s}: decided {s['decided']}, "
                                 f"undecided {s['undecided']} (any-hit {s['occ_undecided']}), t differs {s['t_differs']}, "
                                 f"worst t err {s['worst_t_err']:.3f} of bound")
                    if share is not None:
                        assert s["undecided"] <= share * s["rays"], (name, s)
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    print(f"\n{name}: {len(rays)} rays, {sum(r.n_exact for r in refs.values())} exact pairs\n" + "\n".join(lines))
    return out


# ---- logged and random rays ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LOGGED))
def test_logged_rays(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"logged/{name}", hs, sc, rays_of(subsample(log, 5000, 1)), share=SHARE)


def test_logged_rays_big_mesh(qctx, big_mesh):
    hs, view, sc, log = big_mesh
    run_case(qctx, "logged/mesh96k", hs, sc, rays_of(subsample(log, 400, 2)), share=SHARE)


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_random_rays(qctx, logged, name):
    hs, view, sc, log = logged[name]
    g = np.random.default_rng(9)
    small = view.sph[np.abs(view.sph[:, 3]) < 10, :3] if len(view.tri) == 0 else view.tri[:, :3]
    lo, hi = small.min(0), small.max(0)
    ext = float(np.max(hi - lo))
    n = 4000
    o = g.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(n, 3))
    d = g.normal(size=(n, 3))
    rays = rtow.make_rays(o, d, time=g.random(n), tmax=np.where(g.random(n) < 0.3, g.uniform(0.1, 5, n), np.inf))
    run_case(qctx, f"random/{name}", hs, sc, rays, share=SHARE)


# ---- edges and vertices -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["suzanne", "n4", "coincident", "zero_area", "flat_z", "off_1e4", "big_and_small"])
def test_edge_and_vertex_rays(qctx, logged, name):
    if name == "suzanne":
        hs, view, sc, log = logged[name]
        up, tri = hs, view.tri
    else:
        G = ai.mesh_geometry(ai.edge_meshes()[name])
        keep = []
        up, sc = mesh_case(G, keep)
        tri = G.tri
    run_case(qctx, f"edges/{name}", up, sc, edge_rays(tri, 80, 3))


# ---- tangent rays ---------------------------------------------------------------------------------------------------
def test_tangent_rays(qctx, logged):
    """The ground sphere, the small spheres, a hollow sphere, moving spheres at several times (handmade scene and the
    moving cover scene)."""
    h = handmade_scene()
    view = SceneView(h)
    run_case(qctx, "tangent/handmade", h.c, ex.Scene.of(view), handmade_tangent_rays(view))
    hs, view, sc, log = logged["cover_moving"]
    run_case(qctx, "tangent/cover_moving", hs, sc, cover_tangent_rays(view))


# ---- the triangle cut, surfaces, direction magnitudes ------------------------------------------------------------------
def test_rays_at_the_det_cut(qctx, logged):
    hs, view, sc, log = logged["suzanne"]
    run_case(qctx, "det_cut/suzanne", hs, sc, det_cut_rays(view, sc))


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_rays_from_surfaces(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"surfaces/{name}", hs, sc, surface_rays(log))


@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_direction_magnitudes(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"magnitudes/{name}", hs, sc, magnitude_rays(log))


# ---- far scenes, refits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [1e4, 1e5])
@pytest.mark.parametrize("name", ["cover_static", "suzanne"])
def test_far_scenes(qctx, logged, name, offset):
    hs, view, sc0, log = logged[name]
    up, sc, rays, keep = far_case(hs, log, offset)
    run_case(qctx, f"far/{name}/{offset:g}", up, sc, rays)


@pytest.mark.parametrize("motion", ["translate", "scale1000", "flatten"])
@pytest.mark.parametrize("name", ["cover_moving", "mesh96k"])
def test_after_refit(qctx, logged, big_mesh, name, motion):
    hs = logged["cover_moving"][0] if name == "cover_moving" else big_mesh[0]
    base, new, sc, rays, keep = refit_case(hs, motion, 1500 if name == "cover_moving" else 100)
    run_case(qctx, f"refit/{name}/{motion}", base, sc, rays, refit=new)


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
@pytest.mark.parametrize("name", bm.RAY_SETS)
def test_big_mixed(qctx, name):
    c = bm.case()
    rays, share = bm.ray_sets(c)[name]
    run_case(qctx, f"big_mixed/{name}", c.hs.c, c.exact, rays, share=share, resident=bm.resident, used=bm.used())


@pytest.mark.parametrize("motion", bm.REFITS)
def test_big_mixed_after_refit(qctx, motion):
    c, new = bm.case(), bm.refitted(motion)
    run_case(qctx, f"big_mixed/refit/{motion}", c.hs.c, new.exact, rays_for(new.G, 160, 7), refit=new.hs.c,
             resident=bm.resident, used=bm.used())
