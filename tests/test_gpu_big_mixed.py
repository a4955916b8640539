"""`big_mixed` (tests/big_mixed.py) on the GPU: a scene with every primitive class, every material kind and the hand
scene's hard primitives whose BVH image AND grid image exceed the 160 KiB a workgroup can stage in LDS, so that every launch
on it runs a global-memory instantiation (Image<false>) — the ones the small scenes never reach and the 96,800-triangle mesh
reaches with triangles only.

Each query kind goes through the exact checker it already has.  Closest hit, first k hits, closest point, k nearest,
ambient, path step and the guides have their `test_big_mixed*` in their own test_gpu_exact_*.py module, beside the helper
that checks them; here are the sweeps (the strict mirror and the exact checker of test_gpu_sweep.py), the radiance and the
strict render against the oracle image, the independence of strict answers from the walk and the batch, and the images
after a refit.  Nothing has a tolerance of its own; every upload asserts the image sizes (big_mixed.resident), every launch
the kernel it reports.  test_big_mixed_host.py shows, without a GPU, that the query sets are admissible.
"""
import numpy as np
import pytest
import torch

import accel_images as ai
import big_mixed as bm
import rtow
import sweep_cases
import sweep_ref as sr
from support_fixtures import fresh, qctx  # noqa: F401
from support_oracle import assert_hits_equal, primaries, same_bits, sum_in_order
from support_scenes import resident_images
from support_tables import BUILDERS, KERNELS, WALKS

pytestmark = pytest.mark.gpu

# what each requested walk must report on a mixed scene with a grid (support_oracle.expected_kernel): BVH4 walks meshes only
USED = bm.used()
resident = bm.resident
POINT_KERNELS = dict(WALKS, auto=rtow.KERNEL_AUTO)  # (the point walks answer GRID, BVH4 and AUTO with the BVH)


@pytest.fixture(scope="module")
def mixed(qctx):
    """The scene, uploaded once with each builder: big_mixed.resident asserts what identifies the instantiation every
    test on it runs (its docstring has the selection rule), and the four image sizes are printed."""
    c = bm.case()
    for bname, builder in BUILDERS.items():
        qctx.set_builder(builder)
        qctx.upload(c.hs.c)
        bvh, grid = resident(qctx, bname)
        print(f"\nbig_mixed, {bname} builder: {c.G.ns} spheres, {c.G.nm} moving spheres, {c.G.nt} triangles; BVH image "
              f"{bvh} bytes, grid image {grid} bytes")
    qctx.set_builder(rtow.BUILDER_AUTO)
    return c


@pytest.fixture(scope="module")
def ray_sets(mixed):
    return bm.ray_sets(mixed)


# --------------------------------------------------------------------------------------------------------- sweeps ---
@pytest.fixture(scope="module")
def sweeps(mixed):
    """(sweeps, the mirror's answers, rows of the ties with their expected index, rows of the contact chain)."""
    rec, mats = mixed.rec, mixed.mats
    strict = bm.strict_sweeps(mixed)
    ties, want = bm.tie_sweeps(mixed)
    contact = bm.contact_sweeps(mixed, lambda x: sr.answers(rec, mats, x))[0]
    q = np.concatenate([strict, ties, contact])
    assert len(contact) <= 300 and len(q) % 64
    ans = sr.answers(rec, mats, q)
    assert np.array_equal(ans["prim"][len(strict):len(strict) + len(ties)], want)
    return q, ans, len(strict)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_sweeps_strict_equal_the_mirror(qctx, mixed, sweeps, builder):
    q, want, n_strict = sweeps
    assert np.any(want["prim"] >= 0) and np.any(want["prim"] < 0) and np.any(want["start_overlap"] == 1)
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        resident(qctx, builder)
        for kname, k in POINT_KERNELS.items():
            if kname == "brute" and builder == "device":
                continue
            hits, st = qctx.sweep(q, rtow.F64_STRICT, k, want_stats=True)
            assert hits.tobytes() == want.tobytes(), (builder, kname, sr.diff_fields(hits, want))
            assert st.kernel_used == (rtow.KERNEL_BRUTE if kname == "brute" else rtow.KERNEL_BVH), (kname, st.kernel_used)
            assert st.segments == len(q)
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_sweeps_fast_within_the_band(qctx, mixed, sweeps, builder):
    """The fast build against the exact segment distances (sweep_ref.Checker at K_fast): the placed sweeps, 300 of the
    random ones and the ties, then a contact chain from the fast build's OWN centres."""
    q, _, n_strict = sweeps
    rec, mats = mixed.rec, mixed.mats
    fixed = len(sweep_cases.placed_sweeps()) + len(sweep_cases.skipped_sweeps())
    rnd = sweep_cases.thin((q[fixed:n_strict],), 300)[0]
    part = np.concatenate([q[:fixed], rnd, q[n_strict:n_strict + 3]])
    part = part[~sr.skipped(part)]
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        resident(qctx, builder)
        ck = sr.Checker(rec, mats, part)
        for kname in ("brute", "bvh", "grid") if builder == "host" else ("bvh", "grid"):
            hits, st = qctx.sweep(part, rtow.F64_FAST, WALKS[kname], want_stats=True)
            assert st.kernel_used == (rtow.KERNEL_BRUTE if kname == "brute" else rtow.KERNEL_BVH)
            s = ck.check(hits, "fast", ("big_mixed", builder, kname))
            print("big_mixed", builder, kname, sr.stats_line(s))
            assert s["open"] <= 0.02 * len(part), (kname, s["open"])
        own = lambda x: qctx.sweep(x, rtow.F64_FAST, rtow.KERNEL_BVH)  # noqa: E731
        cq, rest, into = bm.contact_sweeps(mixed, own, 150)
        hits = own(cq)
        s = sr.Checker(rec, mats, cq).check(hits, "fast", ("big_mixed contact", builder))
        print("big_mixed contact", builder, sr.stats_line(s))
        assert np.all(hits["prim"][into] >= 0) and into.sum() > 15 and s["hits"] > 0.5 * len(cq)
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------------ radiance, camera rays, guides, render ---
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_radiance(qctx, mixed, builder):
    """Strict: the in-order sums of the frame's primaries equal the oracle image bit for bit, the segment counter equals
    the log's length and the per-ray results do not depend on the walk; fast: test_gpu_radiance.test_fast_against_strict's
    three assertions, under BVH and GRID."""
    w, h, spp, depth, seed = bm.FRAME
    rays, ids = primaries(mixed.log)
    assert len(rays) == w * h * spp
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        resident(qctx, builder)
        per_ray = {}
        for wname, walk in WALKS.items():
            if wname == "brute" and builder == "device":
                continue
            rgb, st = qctx.radiance(rays, 1, depth, seed, ids, 0, rtow.F64_STRICT, walk, want_stats=True)
            assert st.kernel_used == USED[wname], (wname, st.kernel_used)
            got = sum_in_order(rgb, spp)
            bad = int((got.view(np.uint64) != mixed.image.view(np.uint64)).any(axis=1).sum())
            assert bad == 0, (builder, wname, bad)
            assert st.segments == len(mixed.log) and st.samples == len(rays)
            per_ray[wname] = rgb
        for wname, rgb in per_ray.items():
            assert same_bits(rgb, per_ray["bvh"]), wname
        strict = sum_in_order(per_ray["bvh"], spp)
        for wname in ("bvh", "grid"):
            rgb, st = qctx.radiance(rays, 1, depth, seed, ids, 0, rtow.F64_FAST, WALKS[wname], want_stats=True)
            assert st.kernel_used == USED[wname]
            fast = sum_in_order(rgb, spp)
            mean = np.abs(fast - strict).mean() / spp
            close = np.isclose(fast, strict, rtol=1e-9, atol=1e-12).all(axis=-1).mean()
            print(f"big_mixed {builder} {wname}: mean |fast - strict| per sample {mean:.3e}, close fraction {close:.4f}")
            assert np.isfinite(fast).all()
            assert mean <= 2e-3
            assert close > 0.97, close
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_strict_render_equals_the_oracle(qctx, mixed, builder):
    """The trace kernels on the same frame: BRUTE, BVH, GRID, AUTO and REFTREE equal the oracle image and its segment count."""
    w, h, spp, depth, seed = bm.FRAME
    want = mixed.image.reshape(h, w, 3)
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        resident(qctx, builder)
        buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        for kname, k in dict(KERNELS, auto=rtow.KERNEL_AUTO).items():
            if kname == "bvh4" or (kname == "brute" and builder == "device"):
                continue  # (a mixed scene has no 4-wide image)
            buf.zero_()
            st = qctx.render_device(mixed.config(kernel=k), buf.data_ptr(), 0, True)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (builder, kname, int((got != want).sum()))
            assert st.segments == len(mixed.log), (builder, kname, st.segments, len(mixed.log))
            assert kname == "auto" or st.kernel_used == k, (kname, st.kernel_used)
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


@pytest.fixture(scope="module")
def two_materials():
    """(Case of the variant whose equal spheres keep the hand scene's two materials, the pixels whose oracle paths touch them)."""
    c = bm.Case(bm.geometry(two_twin_materials=True))
    log, twin = c.log, c.view.sph[bm.TWINS[0]]
    p = log[:, 3:6] + np.where(np.isfinite(log[:, 10:11]), log[:, 10:11], 0.0) * log[:, 6:9]
    on = np.isfinite(log[:, 10]) & (np.abs(np.linalg.norm(p - twin[:3], axis=1) - twin[3]) < 1e-6)
    assert on.sum() >= 5
    return c, np.unique(log[on, 0]).astype(np.int64)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_strict_render_of_an_exact_tie_between_two_materials(qctx, two_materials, builder):
    """The equal spheres with two materials (big_mixed's docstring): REFTREE, which walks the oracle's tree, equals the
    oracle image and segment count bit for bit; BRUTE, BVH, GRID and AUTO report the other sphere of the tie, all the
    same one — they equal one another bit for bit, and differ from the oracle only in pixels whose oracle paths touch
    the equal spheres."""
    c, tied = two_materials
    w, h, spp, depth, seed = bm.FRAME
    want = c.image.reshape(h, w, 3)
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(c.hs.c)
        resident(qctx, builder)
        buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        got = {}
        for kname in ("reftree", "bvh", "grid", "auto") + (("brute",) if builder == "host" else ()):
            buf.zero_()
            st = qctx.render_device(c.config(kernel=dict(KERNELS, auto=rtow.KERNEL_AUTO)[kname]), buf.data_ptr(), 0, True)
            torch.cuda.synchronize()
            got[kname] = (buf.cpu().numpy(), st.segments)
        assert same_bits(got["reftree"][0], want) and got["reftree"][1] == len(c.log)
        for kname in set(got) - {"reftree", "bvh"}:
            assert same_bits(got[kname][0], got["bvh"][0]) and got[kname][1] == got["bvh"][1], (builder, kname)
        bad = np.nonzero((got["bvh"][0] != want).any(axis=2).reshape(-1))[0]
        print(f"\nbig_mixed, two materials, {builder}: {len(bad)} pixels differ from the oracle, {len(tied)} touch the equal spheres; "
              f"segments {got['bvh'][1]} (oracle {len(c.log)})")
        assert len(bad) > 0 and set(bad.tolist()) <= set(tied.tolist()), (builder, bad, tied)
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------- strict answers do not depend on the walk ---
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_strict_ray_queries_do_not_depend_on_the_walk_or_the_batch(qctx, mixed, ray_sets, builder):
    """Closest hit, any hit and first k hits: the BVH and GRID records equal BRUTE's bit for bit, and the batch sliced to
    n = 1, 63 and 65 equals those rows of the whole batch.  (Closest point, k nearest and sweeps equal their mirrors bit
    for bit under every walk; ambient, path step, radiance and the guides compare their strict walks with BRUTE in their
    own tests, and the next test slices the first three.)"""
    rays = np.concatenate([ray_sets[n][0] for n in ("logged", "random", "handmade", "tangent")])
    brute = {}
    for bname, walks in (("host", ("brute",)), (builder, ("bvh", "grid"))):  # (the brute force does not depend on the builder)
        qctx.set_builder(BUILDERS[bname])
        try:
            qctx.upload(mixed.hs.c)
            resident(qctx, bname)
            for wname in walks:
                h, st = qctx.intersect(rays, rtow.F64_STRICT, WALKS[wname], want_stats=True)
                assert st.kernel_used == USED[wname]
                got = {"hits": h, "occluded": qctx.occluded(rays, rtow.F64_STRICT, WALKS[wname])}
                got["first"], got["counts"] = qctx.first_hits(rays, 8, rtow.F64_STRICT, WALKS[wname])
                if wname == "brute":
                    brute = got
                    continue
                assert_hits_equal(got["hits"], brute["hits"], (builder, wname))
                assert np.array_equal(got["occluded"], brute["occluded"]) and np.array_equal(got["counts"], brute["counts"])
                assert_hits_equal(got["first"].reshape(-1), brute["first"].reshape(-1), (builder, wname, "first hits"))
                for n in (1, 63, 65):
                    part = rays[200:200 + n]
                    assert_hits_equal(qctx.intersect(part, rtow.F64_STRICT, WALKS[wname]), got["hits"][200:200 + n], (wname, n))
                    assert np.array_equal(qctx.occluded(part, rtow.F64_STRICT, WALKS[wname]), got["occluded"][200:200 + n])
                    fh, fc = qctx.first_hits(part, 8, rtow.F64_STRICT, WALKS[wname])
                    assert np.array_equal(fc, got["counts"][200:200 + n])
                    assert_hits_equal(fh.reshape(-1), got["first"][200:200 + n].reshape(-1), (wname, n, "first hits"))
        finally:
            qctx.set_builder(rtow.BUILDER_AUTO)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_ambient_path_step_and_radiance_do_not_depend_on_the_batch(qctx, mixed, builder):
    """The queries whose per-ray outputs are keyed by a Philox identity: under BVH and GRID, in both builds, the batch
    sliced to n = 1, 63 and 65 equals those rows of the whole batch, every output bit for bit.  (The guides take their
    batch from a config, not a count.)"""
    w, h, spp, depth, seed = bm.FRAME
    pts, pids = bm.ambient_points(mixed)
    rows = bm.scatter_case(mixed)
    bounce = int(np.bincount(rows.bounce).argmax())  # (the depth most rows have)
    first = np.nonzero(rows.bounce == bounce)[0]
    srays, sids = rows.rays[first], rows.ids[first]
    rrays, rids = primaries(mixed.log)
    assert min(len(pts), len(srays), len(rrays)) >= 165
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        resident(qctx, builder)
        for wname in ("bvh", "grid"):
            walk = WALKS[wname]
            for prec in (rtow.F64_STRICT, rtow.F64_FAST):
                amb = lambda s: qctx.ambient(pts[s], 4, bm.FRAME[4], pids[s], 0, prec, walk, want_rays=True, want_stats=True)  # noqa: E731, B023
                step = lambda s: qctx.path_step(srays[s], bounce, seed, sids[s], 0, prec, walk, want_stats=True)  # noqa: E731, B023
                rad = lambda s: qctx.radiance(rrays[s], 1, depth, seed, rids[s], 0, prec, walk, want_stats=True)  # noqa: E731, B023
                every = slice(None)
                whole = {"ambient": amb(every), "path step": step(every), "radiance": rad(every)}
                for kind, out in whole.items():
                    assert out[-1].kernel_used == USED[wname], (kind, wname, out[-1].kernel_used)
                for n in (1, 63, 65):
                    s = slice(100, 100 + n)
                    for kind, part in (("ambient", amb(s)), ("path step", step(s)), ("radiance", rad(s))):
                        for x, y in zip(part[:-1], whole[kind][:-1]):
                            assert same_bits(x, y[s]), (kind, builder, wname, prec, n)
    finally:
        qctx.set_builder(rtow.BUILDER_AUTO)


# ----------------------------------------------------------------------------------------------- after a refit ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("motion", ["jitter", "translate"])
def test_refit_keeps_both_images_beyond_lds(qctx, fresh, mixed, motion, builder):
    """Both images stay above 160 KiB, pass the ray-independent image checker on the NEW geometry, and the grid the device
    rebuilt is byte-identical to a fresh upload's."""
    new = bm.refitted(motion)
    for c in (qctx, fresh):
        c.set_builder(BUILDERS[builder])
    try:
        qctx.upload(mixed.hs.c)
        qctx.refit(new.hs.c)
        fresh.upload(new.hs.c)
        sizes = resident(qctx, builder)
        assert sizes[1] == resident(fresh, builder)[1]  # (a fresh upload builds its own tree: only the grids compare)
        print(f"\nbig_mixed after {motion}, {builder} builder: BVH image {sizes[0]} bytes, grid image {sizes[1]} bytes")
        imgs, ref = resident_images(qctx), resident_images(fresh)
        ai.check_resident(imgs, new.G)
        assert imgs[1] == ref[1] and imgs[3] == ref[3], (motion, builder, len(imgs[1]), len(ref[1]))
        ri = qctx.refit_info()
        assert ri.refits == 1 and ri.grid_resident
    finally:
        for c in (qctx, fresh):
            c.set_builder(rtow.BUILDER_AUTO)


@pytest.mark.parametrize("motion", ["jitter", "translate"])
def test_sweeps_after_a_refit(qctx, mixed, motion):
    new = bm.refitted(motion)
    rec, mats = new.rec, new.mats
    q = sweep_cases.random_sweeps(rec, 400, 19, finite=False, radii=bm.SWEEP_RADII)
    want = sr.answers(rec, mats, q)
    live = q[~sr.skipped(q)][:150]
    ck = sr.Checker(rec, mats, live)
    for bname, builder in BUILDERS.items():
        qctx.set_builder(builder)
        try:
            qctx.upload(mixed.hs.c)
            qctx.refit(new.hs.c)
            resident(qctx, bname)
            for kname in ("brute", "bvh", "grid", "auto") if bname == "host" else ("bvh", "grid", "auto"):
                hits, st = qctx.sweep(q, rtow.F64_STRICT, POINT_KERNELS[kname], want_stats=True)
                assert hits.tobytes() == want.tobytes(), (motion, bname, kname, sr.diff_fields(hits, want))
                assert st.kernel_used == (rtow.KERNEL_BRUTE if kname == "brute" else rtow.KERNEL_BVH)
            s = ck.check(qctx.sweep(live, rtow.F64_FAST, rtow.KERNEL_BVH), "fast", (motion, bname))
            print("big_mixed refit", motion, bname, sr.stats_line(s))
            assert s["open"] <= 0.02 * len(live)
        finally:
            qctx.set_builder(rtow.BUILDER_AUTO)
