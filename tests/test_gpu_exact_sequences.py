"""First-k-hits sequences of both builds against the exact reference (tests/exact_hits.py: sequence_decided,
check_sequences) on the GPU.

Every walk (BRUTE, BVH, GRID, BVH4, with the render's fallbacks; both builders) in F64_STRICT and F64_FAST, max_hits 8
(and 3 and 1 on the deep and tie-rich families), on rays that meet many primitives — chords through the cover scenes,
rays through stacks of wavy sheets, with |d| from e^-3 to e^3 and a finite tmax on half of them —, on rays whose tmax
sits at, just below and just above one of their own hits, and on the ray families of test_gpu_exact_hits.py.  On a
decided ray the primitive sequence and the count must be the exact ones; on every ray the list must be one the band
allows (no decided hit lost in front of the cut, none invented, t within its bound, t non-decreasing).  One line per
combination is printed: decided, undecided, the worst t error in units of its bound, equal-t pairs out of index order.
"""
import hashlib

import numpy as np
import pytest

import accel_images as ai
import big_mixed as bm
import exact_hits as ex
import first_hits_ref as fr
import rtow
from exact_cases import (BUILDS, SHARE, big_mesh, cover_tangent_rays, det_cut_rays, edge_rays, far_case,  # noqa: F401
                         handmade_tangent_rays, logged, magnitude_rays, mesh_case, refit_case, surface_rays)
from support_fixtures import qctx  # noqa: F401
from support_scenes import SceneView, handmade_rays, handmade_scene
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu

DEEP = (8, 3, 1)  # max_hits on the deep and tie-rich families


def run_case(ctx, name, upload, scene, rays, ks=(8,), share=None, refit=None, node_bytes=None, resident=None, used=None):
    """test_gpu_exact_hits.run_case for first_hits: every walk x build x builder x max_hits on `rays`.  The fast GRID
    walk applies the triangle cut to the unit direction and sorts distances (unit_cut, sorted_by_index=False).  resident
    and used: as in test_gpu_exact_hits.run_case.  Returns the stats of every combination."""
    refs = {}
    seen = {}
    has_tri = len(scene.tri) > 0

    def ref(build, unit_cut):
        key = (build, unit_cut and has_tri)
        if key not in refs:
            refs[key] = ex.Reference(scene, rays, build, unit_cut=key[1])
        return key, refs[key]

    lines, out = [], []
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
            for wname, walk in WALKS.items():
                if wname == "brute" and (bname == "device" or len(scene.kind) > 4096):
                    continue  # (as in test_gpu_exact_hits.run_case)
                for build, prec in BUILDS.items():
                    for k in ks:
                        hits, counts, st = ctx.first_hits(rays, k, prec, walk, want_stats=True)
                        assert used is None or st.kernel_used == used[wname], (name, bname, wname, build, st.kernel_used)
                        grid_fast = build == ex.FAST and st.kernel_used == rtow.KERNEL_GRID
                        key, r = ref(build, grid_fast)
                        # the same bytes against the same reference under the same rules: the same verdict
                        key += (k, grid_fast, hashlib.sha1(hits.tobytes() + counts.tobytes()).digest())
                        if key not in seen:
                            seen[key] = ex.check_sequences(r, hits, counts, k, (name, bname, wname, build, st.kernel_used, k),
                                                           sorted_by_index=not grid_fast)
                        s = seen[key]
                        out.append(dict(s, build=build, walk=wname, builder=bname, used=st.kernel_used, k=k))
                        lines.append(f"  {bname:6s} {wname:5s}(used {st.kernel_used}) {build:6s} k={k}: decided "
                                     f"{s['decided']}, undecided {s['undecided']}, worst t err {s['worst_t_err']:.3f} of "
                                     f"bound, equal t out of index order {s['unordered_equal_t']}")
                        if share is not None:
                            assert s["undecided"] <= share * s["rays"], (name, s)
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    print(f"\nsequences {name}: {len(rays)} rays, {sum(r.n_exact for r in refs.values())} exact pairs\n" + "\n".join(lines))
    return out


def sheets(layers, m):
    """(scene to upload, exact_hits.Scene, keep-alive) of a sheet stack."""
    G = ai.mesh_geometry(ai.sheet_stack(layers, m, 73))
    keep = []
    up, sc = mesh_case(G, keep)
    return up, sc, keep


SHEETS = {"10x6": (10, 6, 128), "12x16": (12, 16, 64)}  # layers, m, bytes per 4-wide node


# ---- deep sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cover_static", "cover_moving"])
def test_chords_through_the_cover_scenes(qctx, logged, name):
    hs, view, sc, log = logged[name]
    run_case(qctx, f"chords/{name}", hs, sc, fr.chord_rays(1500, 71), ks=DEEP, share=SHARE)


@pytest.mark.parametrize("name", list(SHEETS))
def test_sheet_stacks(qctx, name):
    layers, m, node_bytes = SHEETS[name]
    up, sc, keep = sheets(layers, m)
    assert len(sc.tri) == layers * 2 * m * m
    run_case(qctx, f"sheets/{name}", up, sc, fr.sheet_rays(2000, 74), ks=DEEP, share=SHARE, node_bytes=node_bytes)


# ---- tmax at and around the ray's own hits ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cover_static", "cover_moving", "sheets"])
def test_tmax_at_and_around_hits(qctx, logged, name):
    """tmax = the strict build's own t of entry 0, 3 or 7, the double below it, the double above it.  Most rays are
    undecided by construction (no cap); the band still forbids losing a decided earlier entry or inventing one."""
    if name == "sheets":
        up, sc, keep = sheets(12, 16)
        rays = fr.sheet_rays(1500, 75)
    else:
        up, sc = logged[name][0], logged[name][2]
        rays = fr.chord_rays(1500, 72)
    qctx.upload(up)
    h8, c8 = qctx.first_hits(rays, 8, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    at = fr.tmax_at_hits(rays, h8["t"], c8)
    assert len(at) >= 1000
    for s in run_case(qctx, f"tmax_at_hits/{name}", up, sc, at, ks=DEEP):
        if s["k"] == 8:
            assert s["undecided"] >= 0.5 * s["rays"], s


# ---- the families of test_gpu_exact_hits.py ------------------------------------------------------------------------------
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
    run_case(qctx, f"edges/{name}", up, sc, edge_rays(tri, 80, 3), ks=DEEP if name == "coincident" else (8,))


def test_tangent_rays(qctx, logged):
    h = handmade_scene()
    view = SceneView(h)
    run_case(qctx, "tangent/handmade", h.c, ex.Scene.of(view), handmade_tangent_rays(view))
    hs, view, sc, log = logged["cover_moving"]
    run_case(qctx, "tangent/cover_moving", hs, sc, cover_tangent_rays(view))


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


# ---- the hand-made scene and the scene of exact ties ------------------------------------------------------------------
def test_handmade_scene(qctx):
    """The hollow glass: far roots and front_face 0."""
    h = handmade_scene()
    run_case(qctx, "handmade", h.c, ex.Scene.of(SceneView(h)), handmade_rays(), ks=DEEP)


def test_scene_of_exact_ties(qctx):
    """Bit-identical copies of a triangle and of a sphere: exact ties that straddle the cut at max_hits 1 and 3."""
    h = fr.ties_scene()
    run_case(qctx, "ties", h.c, ex.Scene.of(SceneView(h)), fr.ties_rays(), ks=DEEP + (2,))


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
@pytest.mark.parametrize("name", bm.SEQUENCE_SETS)
def test_big_mixed(qctx, name):
    c = bm.case()
    rays, share = bm.sequence_sets(c)[name]
    run_case(qctx, f"big_mixed/{name}", c.hs.c, c.exact, rays, ks=(8, 1), share=share, resident=bm.resident, used=bm.used())


def test_big_mixed_tmax_at_and_around_hits(qctx):
    c = bm.case()
    rays = bm.sequence_sets(c)["logged"][0]
    qctx.upload(c.hs.c)
    h8, c8 = qctx.first_hits(rays, 8, rtow.F64_STRICT, rtow.KERNEL_BVH)
    at = fr.tmax_at_hits(rays, h8["t"], c8)
    assert len(at) > 300
    run_case(qctx, "big_mixed/tmax_at_hits", c.hs.c, c.exact, at, ks=(8, 1), resident=bm.resident, used=bm.used())
