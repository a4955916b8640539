"""Swept-sphere queries (rtow_sweep / rtow_sweep_device) on the GPU.

The strict build's whole record is compared bit for bit with the numpy mirror of the kernel's formulas (sweep_ref.py)
under BRUTE, BVH, GRID (answered by BVH), BVH4 and AUTO with both builders — on the hand scene and its triangles alone, the
cover scene with moving spheres, suzanne (4-wide image whole in LDS) and the 96,800-triangle mesh (binary16 planes, the top
of the tree in LDS, stack spill) — for batches of 1, 63, 64, 65 and 4,097 sweeps, after a refit, and against an actual
strict rtow_closest_point for start_overlap.  The fast build is checked against the exact segment distances within its band
(sweep_ref.check_answers).  Then the sweeps that start at contact (sweep_cases.contact_sets: chained from the centres of
earlier answers, aimed at every piece, hand-made and pinned rests, far copies of the hand scene): the strict build against
the mirror under every walk and builder and after a refit, a chain formed on the device from the device's own records, the
fast build against the exact distances on chains from its OWN centres, walk by walk, and the unbounded rows.  The
contracts close the file.
"""
import math

import numpy as np
import pytest

import accel_images as ai
import point_ref as pr
import rtow
import sweep_cases as sc
import sweep_ref as sr
from support_fixtures import pctx  # noqa: F401
from support_scenes import SMALL, deform, scene_of, suzanne_tris
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu

KERNELS = dict(WALKS, auto=rtow.KERNEL_AUTO)
SCENES = ["hand", "hand_mesh", "cover_moving", "suzanne"]
_CACHE = {}


def case(name):
    """(scene to upload, records, material per insertion index, is a triangle mesh), built once per name."""
    if name not in _CACHE:
        keep = []
        if name in ("hand", "hand_mesh") or name in sc.FAR_OFFSETS:
            hs = sc.hand_scene(name == "hand_mesh", sc.FAR_OFFSETS.get(name))
            rec, mats = sc.hand_records(name == "hand_mesh", sc.FAR_OFFSETS.get(name))
            _CACHE[name] = (hs.c, rec, mats, name == "hand_mesh", [hs])
        else:
            G = ai.mesh_geometry(suzanne_tris(10)) if name == "mesh96k" else SMALL[name]
            _CACHE[name] = (scene_of(G, keep), pr.make_records(G.sph, G.mov, G.tri), G.pmat, G.ns + G.nm == 0, keep)
    return _CACHE[name][:4]


def expected(name, key, make):
    """The mirror's answers to a sweep set of a scene, computed once: (sweeps, records)."""
    if (name, key) not in _CACHE:
        _, rec, mats, _ = case(name)
        q = make(rec)
        _CACHE[(name, key)] = (q, sr.answers(rec, mats, q))
    return _CACHE[(name, key)]


def upload(ctx, name, builder=rtow.BUILDER_HOST_SAH):
    ctx.set_builder(builder)
    ctx.upload(case(name)[0])


def used(kernel, mesh):
    b4 = rtow.KERNEL_BVH4 if mesh else rtow.KERNEL_BVH
    return {rtow.KERNEL_GRID: rtow.KERNEL_BVH, rtow.KERNEL_AUTO: b4, rtow.KERNEL_BVH4: b4}.get(kernel, kernel)


def assert_same(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, sr.diff_fields(got, want))


def strict_sets(rec):
    """4,097 sweeps: the hand-placed ones (they reach every scene: the origins are around the origin), every skipped
    kind, and random ones with finite, infinite and zero tmax."""
    return sc.strict_sets(rec)


# ------------------------------------------------------------------------------------------------- strict build ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_strict_equals_the_mirror_every_kernel(pctx, name, builder):
    _, rec, mats, mesh = case(name)
    q, want = expected(name, "strict", strict_sets)
    assert np.any(want["prim"] >= 0) and np.any(want["prim"] < 0) and np.any(want["start_overlap"] == 1)
    upload(pctx, name, BUILDERS[builder])
    for kname, k in KERNELS.items():
        hits, st = pctx.sweep(q, rtow.F64_STRICT, k, want_stats=True)
        assert_same(hits, want, (name, builder, kname))
        assert st.segments == len(q) and st.kernel_used == used(k, mesh), (name, kname, st.kernel_used)
        assert st.prim_tests > 0 and (st.node_tests > 0) == (st.kernel_used != rtow.KERNEL_BRUTE)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mesh_strict(pctx, builder):
    _, rec, mats, _ = case("mesh96k")
    lo, hi, ext = sc.extent(rec)
    q, want = expected("mesh96k", "strict", lambda r: np.concatenate([
        sc.random_sweeps(r, 1500, 9, finite=True, radii=(0.0, 0.01, 0.05)),
        sc.random_sweeps(r, 29, 10, finite=False, radii=(0.0, 0.01))]))
    assert np.any(want["prim"] >= 0) and np.any(want["prim"] < 0)
    upload(pctx, "mesh96k", BUILDERS[builder])
    for kname in ("bvh", "bvh4", "auto"):
        hits, st = pctx.sweep(q, rtow.F64_STRICT, KERNELS[kname], want_stats=True)
        assert_same(hits, want, ("mesh96k", builder, kname))
        assert st.prim_tests / len(q) < 0.2 * rec.n  # the walks prune


def test_batches_slices_and_canaries(pctx):
    import torch

    q, want = expected("cover_moving", "strict", strict_sets)
    upload(pctx, "cover_moving")
    pad = 4096
    dq = torch.full((pad + len(q) * 80 + pad,), 0xAB, dtype=torch.uint8, device="cuda")
    dq[pad:pad + len(q) * 80] = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    dh = torch.empty(pad + len(q) * 80 + pad, dtype=torch.uint8, device="cuda")
    before = dq.cpu().numpy().copy()
    for n in (1, 63, 64, 65, 4097):
        for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
            dh.fill_(0xCD)
            pctx.sweep_device(dq.data_ptr() + pad, n, dh.data_ptr() + pad, rtow.F64_STRICT, k)
            torch.cuda.synchronize()
            g = dh.cpu().numpy()
            assert g[pad:pad + n * 80].tobytes() == want[:n].tobytes(), (n, k)  # a slice of the batch equals the batch
            assert np.all(g[:pad] == 0xCD) and np.all(g[pad + n * 80:] == 0xCD), (n, k)
    assert np.array_equal(dq.cpu().numpy(), before)
    # a slice from the middle, through the tensor form of Context.sweep
    mid = torch.from_numpy(q[1000:1321].view(np.uint8).copy()).cuda()
    got = pctx.sweep(mid, rtow.F64_STRICT, rtow.KERNEL_BVH).cpu().numpy().view(sr.HIT_DTYPE).reshape(-1)
    assert_same(got, want[1000:1321], "tensor slice")


def test_start_overlap_is_the_strict_closest_point(pctx):
    for name in ("hand", "suzanne"):
        q, want = expected(name, "strict", strict_sets)
        upload(pctx, name)
        live = ~sr.skipped(q)
        pq = rtow.make_point_queries(q["origin"][live], q["time"][live], q["radius"][live])
        near = pctx.closest_point(pq, rtow.F64_STRICT, rtow.KERNEL_BVH)
        hits = pctx.sweep(q, rtow.F64_STRICT, rtow.KERNEL_BVH)
        assert np.array_equal(hits["start_overlap"][live] == 1, near["prim"] >= 0), name
        assert np.all(hits["t"][hits["start_overlap"] == 1] == 0.0) and np.all(hits["start_overlap"][~live] == 0)


def test_skipped_queries_give_the_miss_record(pctx):
    upload(pctx, "hand")
    q = sc.skipped_sweeps()
    for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            h, st = pctx.sweep(q[:-1], prec, k, want_stats=True)
            assert np.all(np.isinf(h["t"])) and np.all(np.isinf(h["dist"])) and np.all(h["centre"] == 0) and np.all(h["point"] == 0)
            assert np.all(h["prim"] == -1) and np.all(h["kind"] == -1) and np.all(h["material"] == -1)
            assert np.all(h["start_overlap"] == 0) and st.prim_tests == 0 and st.node_tests == 0
            assert pctx.sweep(q[-1:], prec, k)["prim"][0] >= 0  # the valid sweep they were made from


def test_refit_equals_the_mirror(pctx):
    G = ai.mesh_geometry(suzanne_tris(1))
    keep = []
    for builder in BUILDERS.values():
        pctx.set_builder(builder)
        pctx.upload(scene_of(G, keep))
        H = deform(G, lambda p: p * np.array([1.2, 0.9, 1.0]) + np.array([0.1, -0.2, 0.3]))
        pctx.refit(scene_of(H, keep))
        rec = pr.make_records(H.sph, H.mov, H.tri)
        if "refit" not in _CACHE:
            q = sc.random_sweeps(rec, 1000, 19, finite=False)
            _CACHE["refit"] = (q, sr.answers(rec, H.pmat, q))
        q, want = _CACHE["refit"]
        for kname in ("brute", "bvh", "bvh4", "auto"):
            assert_same(pctx.sweep(q, rtow.F64_STRICT, KERNELS[kname]), want, ("refit", builder, kname))


# --------------------------------------------------------------------------------------------------- fast build ---
FAST = {"hand": 1500, "cover_moving": 600, "suzanne": 600, "mesh96k": 150}


@pytest.mark.parametrize("name", list(FAST))
def test_fast_build_within_its_band(pctx, name):
    _, rec, mats, mesh = case(name)
    q = sc.random_sweeps(rec, FAST[name], 31, finite=True, radii=(0.0, 0.01, 0.05) if name == "mesh96k" else (0.0, 0.002, 0.01, 0.05, 0.2))
    if name == "hand":
        q = np.concatenate([sc.placed_sweeps(), q])
    upload(pctx, name)
    ck = sr.Checker(rec, mats, q)
    for kname in ("bvh", "bvh4") if name == "mesh96k" else ("brute", "bvh", "bvh4"):
        hits = pctx.sweep(q, rtow.F64_FAST, KERNELS[kname])
        s = ck.check(hits, "fast", (name, kname))
        print(name, kname, sr.stats_line(s))
        assert s["open"] <= 0.02 * len(q), (name, kname, s["open"])


# ------------------------------------------------------------------------------- sweeps that start at contact ---
MESH_RADII = (0.0, 0.01, 0.05)  # of the 96,800-triangle mesh: a larger ball holds hundreds of triangles


def contact_expected(name):
    """(sweeps, the mirror's answers) of the contact set of a scene, chained from the mirror's own answers."""
    _, rec, mats, _ = case(name)
    big = name == "mesh96k"
    return expected(name, "contact", lambda r: sc.contact_sets(
        name, r, lambda x: sr.answers(r, mats, x), 100 if big else None, MESH_RADII if big else sc.RADII)[0])


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES + list(sc.FAR_OFFSETS) + ["mesh96k"])
def test_strict_equals_the_mirror_at_contact(pctx, name, builder):
    _, rec, mats, mesh = case(name)
    q, want = contact_expected(name)
    assert len(q) <= 100 or name != "mesh96k"
    assert np.any(want["prim"] >= 0) and np.any(want["prim"] < 0)
    if name == "hand":  # a rest the overlap test does not see answers t = 0 without the flag
        assert np.any((want["t"] == 0.0) & (want["start_overlap"] == 0) & (want["prim"] >= 0))
    upload(pctx, name, BUILDERS[builder])
    for kname, k in KERNELS.items():
        if name == "mesh96k" and kname == "brute":
            continue
        hits, st = pctx.sweep(q, rtow.F64_STRICT, k, want_stats=True)
        assert_same(hits, want, (name, builder, kname))
        assert st.kernel_used == used(k, mesh), (name, kname, st.kernel_used)


def refit_case():
    """(undeformed geometry, deformed geometry, its records) of test_refit_equals_the_mirror."""
    if "refit_geometry" not in _CACHE:
        G = ai.mesh_geometry(suzanne_tris(1))
        H = deform(G, lambda p: p * np.array([1.2, 0.9, 1.0]) + np.array([0.1, -0.2, 0.3]))
        _CACHE["refit_geometry"] = (G, H, pr.make_records(H.sph, H.mov, H.tri))
    return _CACHE["refit_geometry"]


def test_refit_equals_the_mirror_at_contact(pctx):
    G, H, rec = refit_case()
    keep = []
    if "refit_contact" not in _CACHE:
        q = sc.contact_set(rec, sc.random_sweeps(rec, 200, 19), lambda x: sr.answers(rec, H.pmat, x), 4)[0]
        _CACHE["refit_contact"] = (q, sr.answers(rec, H.pmat, q))
    q, want = _CACHE["refit_contact"]
    for builder in BUILDERS.values():
        pctx.set_builder(builder)
        pctx.upload(scene_of(G, keep))
        pctx.refit(scene_of(H, keep))
        for kname in ("brute", "bvh", "bvh4", "auto"):
            assert_same(pctx.sweep(q, rtow.F64_STRICT, KERNELS[kname]), want, ("refit at contact", builder, kname))


def test_a_chain_formed_on_the_device(pctx):
    """Stage 2 from the device's own stage-1 records: the origin is copied from `centre` on the device, and both
    launches are enqueued on the same stream with nothing read back in between.  Strict: equal to the host-built chain."""
    import torch

    for name in ("hand", "suzanne"):
        _, rec, mats, _ = case(name)
        first = sc.random_sweeps(rec, 600, 3)
        if name == "hand":
            first = np.concatenate([sc.aimed_sweeps(1), first])
        q2, d, tmax = sc.chain_all(first, sr.answers(rec, mats, first), 8)
        want = sr.answers(rec, mats, q2)
        assert (q2["tmax"] > 0).sum() > 100 and np.any(want["prim"] >= 0)
        upload(pctx, name)
        d_first = torch.from_numpy(first.view(np.uint8).reshape(-1, 80).copy()).cuda()
        d_dir, d_tmax = torch.from_numpy(d).cuda(), torch.from_numpy(tmax).cuda()
        for kname in ("brute", "bvh", "auto"):
            h1 = pctx.sweep(d_first, rtow.F64_STRICT, KERNELS[kname])          # uint8 [n, 80], on the current stream
            f, prim = h1.view(torch.float64), h1.view(torch.int32)[:, 16]      # t, dist, centre[3], point[3] | prim ...
            q = d_first.view(torch.float64).clone()                            # origin[3], time, direction[3], tmax, radius
            q[:, 0:3], q[:, 4:7] = f[:, 2:5], d_dir
            q[:, 7] = torch.where((prim >= 0) & (f[:, 0] > 0.0), d_tmax, torch.full_like(d_tmax, -1.0))
            h2 = pctx.sweep(q.view(torch.uint8), rtow.F64_STRICT, KERNELS[kname])
            got = h2.cpu().numpy().view(sr.HIT_DTYPE).reshape(-1)
            assert_same(got, want, ("device chain", name, kname))
            assert q.cpu().numpy().tobytes() == q2.tobytes(), (name, kname)


FAST_CONTACT = {"hand": 300, "cover_moving": 200, "suzanne": 200, "mesh96k": 60, "far1e5": 300, "far1e7": 300}


def fast_chain_check(ctx, name, rec, mats, walks, limit, first=None):
    """For each walk: the contact set chained from the fast build's OWN answers under that walk, answered by it and
    checked against the exact segment distances with a reference of its own (the centres differ in the last bits
    between walks).  Every "into" sweep must come back a hit."""
    radii = MESH_RADII if name == "mesh96k" else sc.RADII
    for kname in walks:
        own = lambda x: ctx.sweep(x, rtow.F64_FAST, KERNELS[kname])  # noqa: E731, B023
        if first is None:
            q, rest, into = sc.contact_sets(name, rec, own, limit, radii)
        else:
            q, rest, into = sc.thin(sc.contact_set(rec, first, own, 4), limit)
        hits = own(q)
        s = sr.Checker(rec, mats, q).check(hits, "fast", (name, kname))
        print(name, kname, sr.stats_line(s))
        assert np.all(hits["prim"][into] >= 0), (name, kname)
        assert s["hits"] > 0.5 * len(q) and into.sum() > 0.1 * min(len(q), limit or len(q))


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(FAST_CONTACT))
def test_fast_build_at_contact_within_its_band(pctx, name, builder):
    _, rec, mats, _ = case(name)
    upload(pctx, name, BUILDERS[builder])
    fast_chain_check(pctx, name, rec, mats, ("bvh", "bvh4") if name == "mesh96k" else ("brute", "bvh", "bvh4"), FAST_CONTACT[name])


def test_fast_build_at_contact_after_a_refit(pctx):
    G, H, rec = refit_case()
    keep = []
    for builder in BUILDERS.values():
        pctx.set_builder(builder)
        pctx.upload(scene_of(G, keep))
        pctx.refit(scene_of(H, keep))
        fast_chain_check(pctx, "refit", rec, H.pmat, ("brute", "bvh", "bvh4"), 200, first=sc.random_sweeps(rec, 200, 19))


@pytest.mark.parametrize("name", list(FAST))
def test_fast_build_on_unbounded_sweeps(pctx, name):
    """The tmax = +inf rows of the strict sets: a miss is checked up to the horizon where the sweep has left the scene."""
    _, rec, mats, _ = case(name)
    q = expected(name, "strict", strict_sets)[0] if name != "mesh96k" else np.concatenate([
        sc.random_sweeps(rec, 1500, 9, finite=True, radii=MESH_RADII), sc.random_sweeps(rec, 29, 10, finite=False, radii=(0.0, 0.01))])
    q = q[np.isinf(q["tmax"]) & ~sr.skipped(q)]
    assert len(q) > (3 if name == "mesh96k" else 400)
    upload(pctx, name)
    ck = sr.Checker(rec, mats, q)
    for kname in ("bvh", "bvh4") if name == "mesh96k" else ("brute", "bvh4"):
        s = ck.check(pctx.sweep(q, rtow.F64_FAST, KERNELS[kname]), "fast", (name, kname))
        print(name, kname, sr.stats_line(s))


# ---------------------------------------------------------------------------------------------------- contracts ---
def test_refusals_residency_and_stats():
    import torch

    scene, rec, mats, _ = case("cover_moving")
    q = sc.random_sweeps(rec, 200, 37)
    want = sr.answers(rec, mats, q)
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.sweep(q, rtow.F64_STRICT)
        hs = rtow.HostScene.cover(11, 1.5, True)
        c.render(hs, rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST))  # lean upload: the grid only
        h, st = c.sweep(q, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0 and st.prim_tests == len(q) * rec.n
        for k in (rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
                c.sweep(q, rtow.F64_STRICT, k)
        hs.close()
        c.upload(scene)
        for prec, k in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_STRICT, rtow.KERNEL_REFTREE),
                        (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, rtow.KERNEL_AUTO), (rtow.F64_STRICT, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.sweep(q, prec, k)
        dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
        dh = torch.empty(len(q) * 80, dtype=torch.uint8, device="cuda")
        bad = ((dq.data_ptr() + 8, 4, dh.data_ptr()), (dq.data_ptr(), 4, dh.data_ptr() + 8), (0, 4, dh.data_ptr()),
               (dq.data_ptr(), 4, 0), (dq.data_ptr(), -1, dh.data_ptr()), (dq.data_ptr(), (1 << 31) - 63, dh.data_ptr()))
        for a, n, b in bad:
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.sweep_device(a, n, b, rtow.F64_STRICT, rtow.KERNEL_BVH)
        st = c.sweep_device(0, 0, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)  # n == 0 launches nothing
        assert st.segments == 0 and st.prim_tests == 0 and st.node_tests == 0 and st.kernel_ms == 0.0
        st = c.sweep_device(dq.data_ptr(), len(q), dh.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_BVH, want_stats=True)
        assert_same(dh.cpu().numpy().view(sr.HIT_DTYPE).reshape(-1), want, "device form")
        assert st.segments == len(q) and st.samples == 0 and st.kernel_used == rtow.KERNEL_BVH
        assert 0 < st.prim_tests < len(q) * rec.n and st.node_tests > 0 and 0.0 < st.kernel_ms <= st.total_ms
    finally:
        c.close()


def test_sweeps_leave_the_render_untouched():
    hs = rtow.HostScene.cover(11, 1.5, True)
    G = ai.Geometry.of_scene(hs.c)
    q = sc.random_sweeps(pr.make_records(G.sph, G.mov, G.tri), 300, 41)
    cfg = rtow.make_config(48, 32, 2, 1, 10, seed=5, precision=rtow.F64_STRICT)
    c = rtow.Context(0)
    try:
        before, _ = c.render(hs, cfg)
        c.upload(hs.c)
        for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_AUTO):
            c.sweep(q, rtow.F64_STRICT, k)
            c.sweep(q, rtow.F64_FAST, k)
        after, _ = c.render(hs, cfg)
        assert np.array_equal(before, after)
    finally:
        c.close()
        hs.close()
