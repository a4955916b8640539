"""Ambient queries of both builds against the exact reference (tests/ambient_exact.py) on the GPU.

Directions: about 1,500 points x 4 samples whose normals and identities are where the direction's arithmetic can go wrong
(ambient_cases.direction_cases) — every exported component within the build's derived bound of the exact direction, the
strict ones also the numpy mirror's bits, the skipped points dead.  Records: on each build's own exported rays every
sample's visibility is decided by exact_hits, and open, bent, sky and samples are held to it (ambient_exact.check_records)
under every walk with the render's fallbacks and both builders, on the logged scenes, the 96,800-triangle mesh, the
hand-made scene and a refitted scene.  The worst direction and sky errors (as fractions of their bounds) and the undecided
and left-out counts are printed per case; the caps on the latter two are asserted.
"""
import numpy as np
import pytest

import ambient_cases as ac
import ambient_exact as ax
import ambient_ref
import big_mixed as bm
import exact_hits as ex
import rtow
from exact_cases import BUILDS, SHARE, big_mesh, logged, refit_case  # noqa: F401
from support_fixtures import qctx  # noqa: F401
from support_scenes import SceneView, handmade_scene
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu

SAMPLES = 8


# ---- directions ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs():
    pts, ids, labels = ac.direction_cases()
    pixel, sample = ambient_ref.identities(len(pts), ac.DIR_SAMPLES, ids)
    assert np.array_equal(ambient_ref.skipped(pts), labels == "skipped")  # (the rule, as the cases name it)
    return pts, ids, labels, ambient_ref.skipped(pts), ax.exact_directions(pts["normal"], ac.SEED, pixel, sample)


@pytest.mark.parametrize("build", list(BUILDS))
def test_directions_lie_within_the_bound_of_the_exact_ones(qctx, dirs, build):
    pts, ids, labels, skip, exact = dirs
    hm = handmade_scene()  # (held for the whole test: the scene's arrays live in the holder, not in hm.c)
    qctx.upload(hm.c)
    mirror = ambient_ref.rays(pts, ac.DIR_SAMPLES, ac.SEED, ids)
    for kname, kernel in (("bvh", rtow.KERNEL_BVH), ("auto", rtow.KERNEL_AUTO)):
        out, rays = qctx.ambient(pts, ac.DIR_SAMPLES, ac.SEED, ids, 0, BUILDS[build], kernel, want_rays=True)
        what = f"directions {build} {kname}"
        # the skip rule first: a point on the wrong side of it shows here, before any arithmetic is judged
        dead = rays["tmax"][:, 0] == -1.0
        assert np.array_equal(dead, skip), (what, "skipped points", labels[dead != skip], pts["normal"][dead != skip])
        assert not out[skip].view(np.uint8).any() and np.all(out["samples"][~skip] == ac.DIR_SAMPLES), what
        for f in ("origin", "time", "tmax"):
            assert rays[f].tobytes() == mirror[f].tobytes(), (what, f)
        assert not rays["direction"][skip].any(), what
        worst = ax.check_directions(exact, rays["direction"], build, what, live=~skip)
        if build == ex.STRICT:
            assert rays.tobytes() == mirror.tobytes(), what
        with np.errstate(invalid="ignore"):
            ratio = np.abs(rays["direction"] - exact[0]) / exact[1][build]
        print(f"\n{what}: worst {worst:.3f} of the bound; per group: "
              + ", ".join(f"{k} {np.nanmax(ratio[labels == k]):.3f}" for k in dict.fromkeys(labels) if k != "skipped"))


# ---- records -------------------------------------------------------------------------------------------------------
def run_records(ctx, name, upload, sc, pts, ids, samples, build, refit=None, after=None, resident=None, used=None):
    """Every walk x builder of `build` on the points; `after(out)`: further assertions on every answer; resident and used:
    as in test_gpu_exact_hits.run_case.  Returns walk name -> the host builder's (records, exported rays)."""
    refs = {}
    has_tri = len(sc.tri) > 0
    lines, got = [], {}
    for bname, builder in BUILDERS.items():
        ctx.set_builder(builder)
        try:
            ctx.upload(upload)
            if refit is not None:
                ctx.refit(refit)
            if resident is not None:
                resident(ctx, bname)
            for wname, walk in WALKS.items():
                if wname == "brute" and (bname == "device" or len(sc.kind) > 4096):
                    continue  # (the brute force does not depend on the builder; 96,800 tests per ray are not a test)
                out, rays, st = ctx.ambient(pts, samples, ac.SEED, ids, 0, BUILDS[build], walk, want_rays=True,
                                            want_stats=True)
                assert used is None or st.kernel_used == used[wname], (name, bname, wname, build, st.kernel_used)
                got.setdefault(wname, (out, rays))
                unit_cut = build == ex.FAST and st.kernel_used == rtow.KERNEL_GRID and has_tri
                key = (rays.tobytes(), unit_cut)
                if key not in refs:  # (one reference, one set of exact directions per exported ray set)
                    refs[key] = (ex.Reference(sc, rays.reshape(-1).copy(), build, unit_cut=unit_cut),
                                 ax.Exact(pts, rays, samples, build, ac.SEED, ids))
                what = (name, bname, wname, build, st.kernel_used)
                s = ax.check_records(refs[key][0], pts, rays, out, samples, build, what=str(what), exact=refs[key][1])
                lines.append(f"  {bname:6s} {wname:5s}(used {st.kernel_used}) {build:6s}: " + ax.line(s))
                assert s["undecided"] <= SHARE * s["rays"], (what, s)
                assert s["left_out"] <= 0.01 * s["points"], (what, s)
                assert 0 < out["open"].sum() < s["rays"], what
                if after is not None:
                    after(out)
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    # the strict build's rays are one set of bits under every walk; the fast build's may differ from walk to walk in the
    # last bits (each instantiation is contracted on its own), and every set is checked against its own reference
    assert build != ex.STRICT or len(refs) == 1, "the strict build's exported rays depend on the walk"
    print(f"\n{name}: {len(pts)} points x {samples} samples, {len(refs)} references\n" + "\n".join(lines))
    return got


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_records_on_logged_scenes(qctx, logged, name, build):
    hs, view, sc, log = logged[name]
    pts, ids = ac.log_points(view, log, 300, 40 + ["cover_moving", "suzanne"].index(name))
    run_records(qctx, f"records/{name}", hs, sc, pts, ids, SAMPLES, build)


@pytest.mark.parametrize("build", list(BUILDS))
def test_records_on_the_large_mesh(qctx, big_mesh, build):
    hs, view, sc, log = big_mesh
    pts, ids = ac.log_points(view, log, 100, 44)
    run_records(qctx, "records/mesh96k", hs, sc, pts, ids, 4, build)


@pytest.mark.parametrize("build", list(BUILDS))
def test_records_on_the_handmade_scene(qctx, build):
    """Besides the checker: inside the hollow sphere with max_dist = inf every sample is closed, so bent and sky are
    +0.0; far above the scene, normals up, every sample is open."""
    hm = handmade_scene()
    pts = np.concatenate([ac.handmade_points(), ac.handmade_sky_points()])
    closed = (np.arange(len(pts)) < ac.N_ENCLOSED) & np.isinf(pts["max_dist"])
    above = pts["point"][:, 1] == 50.0
    assert closed.sum() >= 10 and above.sum() == 24

    def after(out):
        assert np.all(out["open"][closed] == 0.0) and np.all(out["samples"][closed] == SAMPLES)
        assert not out["bent"][closed].view(np.uint64).any() and not out["sky"][closed].view(np.uint64).any()
        assert np.all(out["open"][above] == SAMPLES)

    run_records(qctx, "records/handmade", hm.c, ex.Scene.of(SceneView(hm)), pts, None, SAMPLES, build, after=after)


@pytest.mark.parametrize("build", list(BUILDS))
def test_records_after_a_refit(qctx, logged, build):
    hs = logged["cover_moving"][0]
    base, new, sc, rays, keep = refit_case(hs, "translate", 200)
    pts, ids = ac.box_points(sc, rays[200:400], 5)
    run_records(qctx, "records/refit/cover_moving/translate", base, sc, pts, ids, SAMPLES, build, refit=new)


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("samples", bm.AMBIENT_SAMPLES)
def test_big_mixed(qctx, samples, build):
    c = bm.case()
    pts, ids = bm.ambient_points(c)
    got = run_records(qctx, f"big_mixed/{samples}", c.hs.c, c.exact, pts, ids, samples, build, resident=bm.resident,
                      used=bm.used())
    if build == ex.STRICT:  # strict answers do not depend on the walk
        for w in ("bvh", "grid", "bvh4"):
            assert got[w][0].tobytes() == got["brute"][0].tobytes() and got[w][1].tobytes() == got["brute"][1].tobytes(), w
