"""Box-overlap queries (rtow_overlap / rtow_overlap_device) on the GPU.

The strict build's counts and ids are compared bit for bit with the numpy mirror of the kernel's predicate
(overlap_ref.py) under BRUTE, BVH, GRID (answered by BVH), BVH4 and AUTO with both builders — on the hand scene, the cover
scene with moving spheres, suzanne (4-wide image whole in LDS), the 96,800-triangle mesh (binary16 planes, image beyond
LDS, stack spill) and big_mixed's scene (the global-memory BVH kernels on spheres and moving spheres) — and after a refit.
The fast build is checked against the exact reference within its band (overlap_ref.check_answers); the lattice set gives
the exact closed-set answer in both builds; a box around everything counts every primitive once and paging returns all of
them; then the batch shapes, the voxelisation of suzanne, the argument errors in their order and the statistics.
"""
import ctypes as C

import numpy as np
import pytest

import accel_images as ai
import big_mixed as bm
import overlap_cases as oc
import overlap_ref as ov
import point_ref as pr
import rtow
import sweep_cases as sc
from support_fixtures import pctx  # noqa: F401
from support_scenes import SMALL, deform, scene_of, suzanne_tris
from support_tables import BUILDERS, WALKS

pytestmark = pytest.mark.gpu

KERNELS = dict(WALKS, auto=rtow.KERNEL_AUTO)
SCENES = ["hand", "cover_moving", "suzanne"]
BIG_SIZES = (0.004, 0.02, 0.08)  # box edges on the big scenes, x the extent: a larger box holds thousands of primitives
_CACHE = {}


def case(name):
    """(scene to upload, records, is a triangle mesh), built once per name."""
    if name not in _CACHE:
        keep = []
        if name == "hand":
            hs = sc.hand_scene()
            _CACHE[name] = (hs.c, sc.hand_records()[0], False, [hs])
        elif name == "lattice":
            hs = oc.lattice_scene()
            _CACHE[name] = (hs.c, oc.lattice_records(), False, [hs])
        elif name == "big_mixed":
            c = bm.case()
            _CACHE[name] = (c.hs.c, c.rec, False, [c])
        else:
            G = ai.mesh_geometry(suzanne_tris(10)) if name == "mesh96k" else SMALL[name]
            _CACHE[name] = (scene_of(G, keep), pr.make_records(G.sph, G.mov, G.tri), G.ns + G.nm == 0, keep)
    return _CACHE[name][:3]


def boxes_of(name):
    rec = case(name)[1]
    if name == "mesh96k":
        return np.concatenate([oc.placed_boxes()[0], oc.skipped_boxes(), oc.random_boxes(rec, 500, 9, BIG_SIZES)])
    if name == "big_mixed":
        return np.concatenate([oc.placed_boxes()[0], oc.min_prim_boxes(rec.n), oc.random_boxes(rec, 900, 7, BIG_SIZES)])
    return oc.strict_set(rec)


def expected(name):
    """(boxes, the mirror's full sets, counts, ids at max_ids = 8) of a scene, computed once."""
    if (name, "strict") not in _CACHE:
        rec = case(name)[1]
        q = boxes_of(name)
        sets = ov.full_sets(rec, q)
        _CACHE[(name, "strict")] = (q, sets) + ov.answers(rec, q, 8, sets)
    return _CACHE[(name, "strict")]


def classified(name):
    if (name, "exact") not in _CACHE:
        _CACHE[(name, "exact")] = ov.Classified(case(name)[1], expected(name)[0])
    return _CACHE[(name, "exact")]


def upload(ctx, name, builder=rtow.BUILDER_HOST_SAH):
    ctx.set_builder(builder)
    ctx.upload(case(name)[0])


def used(kernel, mesh):
    b4 = rtow.KERNEL_BVH4 if mesh else rtow.KERNEL_BVH
    return {rtow.KERNEL_GRID: rtow.KERNEL_BVH, rtow.KERNEL_AUTO: b4, rtow.KERNEL_BVH4: b4}.get(kernel, kernel)


def assert_same(got, want, what):
    counts, ids = got
    assert np.array_equal(counts, want[0]), (what, "counts", np.nonzero(counts != want[0])[0][:8])
    assert np.array_equal(ids, want[1]), (what, "ids", np.nonzero(np.any(ids != want[1], axis=1))[0][:8])


# ------------------------------------------------------------------------------------------------- strict build ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_strict_equals_the_mirror_every_kernel(pctx, name, builder):
    _, rec, mesh = case(name)
    q, sets, counts, ids = expected(name)
    assert len(q) == 4097 and counts.max() > 8 and np.any(counts == 0) and np.any((counts > 0) & (counts <= 8))
    upload(pctx, name, BUILDERS[builder])
    for kname, k in KERNELS.items():
        c, i, st = pctx.overlap(q, 8, rtow.F64_STRICT, k, want_stats=True)
        assert_same((c, i), (counts, ids), (name, builder, kname))
        assert st.segments == len(q) and st.kernel_used == used(k, mesh), (name, kname, st.kernel_used)
        assert st.prim_tests > 0 and (st.node_tests > 0) == (st.kernel_used != rtow.KERNEL_BRUTE)
        c1, none = pctx.overlap(q, 8, rtow.F64_STRICT, k, want_ids=False)
        assert none is None and np.array_equal(c1, counts), (name, builder, kname, "counts only")


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mesh_strict(pctx, builder):
    _, rec, _ = case("mesh96k")
    q, sets, counts, ids = expected("mesh96k")
    assert counts.max() > 8 and np.any(counts == 0)
    upload(pctx, "mesh96k", BUILDERS[builder])
    assert pctx.build_info().bvh4_nodes > 0 and len(pctx.debug_image(4)) > bm.LDS_LIMIT
    small = np.arange(len(q)) >= len(q) - 500  # the random boxes
    for kname in ("bvh", "bvh4", "auto"):
        c, i = pctx.overlap(q, 8, rtow.F64_STRICT, KERNELS[kname])
        assert_same((c, i), (counts, ids), ("mesh96k", builder, kname))
        st = pctx.overlap(q[small], 8, rtow.F64_STRICT, KERNELS[kname], want_stats=True)[2]
        assert st.prim_tests / small.sum() < 0.02 * rec.n  # the walks prune


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mixed_strict_beyond_lds(pctx, builder):
    _, rec, _ = case("big_mixed")
    q, sets, counts, ids = expected("big_mixed")
    assert counts.max() > 8 and np.any(counts == 0)
    upload(pctx, "big_mixed", BUILDERS[builder])
    bm.resident(pctx, builder)
    for kname in ("brute", "bvh", "grid", "bvh4", "auto"):
        c, i, st = pctx.overlap(q, 8, rtow.F64_STRICT, KERNELS[kname], want_stats=True)
        assert_same((c, i), (counts, ids), ("big_mixed", builder, kname))
        assert st.kernel_used == (rtow.KERNEL_BRUTE if kname == "brute" else rtow.KERNEL_BVH)


def refit_case():
    """(undeformed geometry, deformed geometry, its records, boxes, the mirror's answers): the sweep tests' refit."""
    if "refit" not in _CACHE:
        G = ai.mesh_geometry(suzanne_tris(1))
        H = deform(G, lambda p: p * np.array([1.2, 0.9, 1.0]) + np.array([0.1, -0.2, 0.3]))
        rec = pr.make_records(H.sph, H.mov, H.tri)
        q = oc.random_boxes(rec, 1000, 19)
        _CACHE["refit"] = (G, H, rec, q, ov.answers(rec, q, 8))
    return _CACHE["refit"]


def test_refit_equals_the_mirror(pctx):
    G, H, rec, q, want = refit_case()
    keep = []
    assert want[0].max() > 8
    for builder in BUILDERS.values():
        pctx.set_builder(builder)
        pctx.upload(scene_of(G, keep))
        pctx.refit(scene_of(H, keep))
        for kname in ("brute", "bvh", "bvh4", "auto"):
            assert_same(pctx.overlap(q, 8, rtow.F64_STRICT, KERNELS[kname]), want, ("refit", builder, kname))
        ck = ov.Classified(rec, q) if "refit_exact" not in _CACHE else _CACHE["refit_exact"]
        _CACHE["refit_exact"] = ck
        for kname in ("brute", "bvh4"):
            c, i = pctx.overlap(q, 8, rtow.F64_FAST, KERNELS[kname])
            ov.check_answers(ck, c, i, 8, "fast", ("refit", builder, kname))


# --------------------------------------------------------------------------------------------------- fast build ---
@pytest.mark.parametrize("name", SCENES + ["mesh96k", "big_mixed"])
def test_fast_build_within_its_band(pctx, name):
    q = expected(name)[0]
    ck = classified(name)
    upload(pctx, name)
    walks = ("bvh", "bvh4") if name == "mesh96k" else ("brute", "bvh", "bvh4")
    for kname in walks:
        for max_ids in (8, 3):
            c, i = pctx.overlap(q, max_ids, rtow.F64_FAST, KERNELS[kname])
            free = ov.check_answers(ck, c, i, max_ids, "fast", (name, kname, max_ids))
        c, _ = pctx.overlap(q, 8, rtow.F64_FAST, KERNELS[kname], want_ids=False)
        ov.check_answers(ck, c, None, 8, "fast", (name, kname, "counts only"))
        print(name, kname, "pairs the fast build was free in:", free)
    # ... and the strict build meets its own, narrower band
    c, i = pctx.overlap(q, 8, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    ov.check_answers(ck, c, i, 8, "strict", (name, "strict"))


# ------------------------------------------------------------------------------------------------ exact inputs ---
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_lattice_gives_the_closed_set_answer(pctx, builder):
    _, rec, _ = case("lattice")
    q = oc.lattice_boxes()
    if "lattice_exact" not in _CACHE:
        _CACHE["lattice_exact"] = ov.Classified(rec, q)
    ck = _CACHE["lattice_exact"]
    want = ov.answers(rec, q, 8, ck.closed_sets())
    assert np.sum(ck.r == 0.0) > 100  # faces, edges and vertices ON the geometry: gaps of exactly 0
    upload(pctx, "lattice", BUILDERS[builder])
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        for kname, k in KERNELS.items():
            assert_same(pctx.overlap(q, 8, prec, k), want, ("lattice", builder, prec, kname))


# ------------------------------------------------------------------------------------ each primitive counted once ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["hand", "cover_moving", "suzanne", "mesh96k"])
def test_every_primitive_is_counted_once(pctx, name, builder):
    _, rec, mesh = case(name)
    lo, hi, ext = oc.extent(rec)
    mp = np.array([0, -3, 1, rec.n // 3, rec.n - 1, rec.n], dtype=np.int32)
    q = ov.make_boxes(np.tile(np.minimum(lo, -50.0) - ext, (len(mp), 1)), np.tile(np.maximum(hi, 50.0) + ext, (len(mp), 1)), 0.5, mp)
    upload(pctx, name, BUILDERS[builder])
    for kname, k in KERNELS.items():
        if name == "mesh96k" and kname == "brute":
            continue
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            c, i = pctx.overlap(q, 8, prec, k)
            assert np.array_equal(c, rec.n - np.maximum(mp, 0)), (name, builder, kname, c)
            for row, m in zip(i, np.maximum(mp, 0)):
                assert np.array_equal(row, np.where(m + np.arange(8) < rec.n, m + np.arange(8), -1)), (name, kname, row)
        if rec.n < 1000:
            everything = pctx.overlap_all(q[:1], rtow.F64_STRICT, k)
            assert len(everything) == 1 and np.array_equal(everything[0], np.arange(rec.n)), (name, builder, kname)


def test_paging_returns_the_whole_sets(pctx):
    _, rec, _ = case("hand")
    q, sets, counts, ids = expected("hand")
    sel = np.concatenate([np.nonzero(counts > 8)[0], np.nonzero(counts <= 8)[0][:200]])
    upload(pctx, "hand")
    for max_ids in (8, 5, 1):
        for k in (rtow.KERNEL_BVH, rtow.KERNEL_BRUTE):
            got = pctx.overlap_all(q[sel], rtow.F64_STRICT, k, max_ids=max_ids)
            assert all(np.array_equal(g, sets[j]) for g, j in zip(got, sel)), (max_ids, k)
    # by hand, as the contract says it: min_prim = ids[max_ids - 1] + 1 while counts > max_ids
    j = int(np.argmax(counts))
    one, seen = q[j:j + 1].copy(), []
    while True:
        c, i = pctx.overlap(one, 8, rtow.F64_STRICT)
        seen += list(i[0, :min(int(c[0]), 8)])
        if c[0] <= 8:
            break
        one["min_prim"] = i[0, 7] + 1
    assert np.array_equal(seen, sets[j]) and len(seen) > 16


# ------------------------------------------------------------------------------------------------- batch shapes ---
def test_batches_guards_and_forms(pctx):
    import torch

    q, sets, counts, ids8 = expected("cover_moving")
    rec = case("cover_moving")[1]
    upload(pctx, "cover_moving")
    pad = 4096
    dq = torch.full((pad + len(q) * 64 + pad,), 0xAB, dtype=torch.uint8, device="cuda")
    dq[pad:pad + len(q) * 64] = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    before = dq.cpu().numpy().copy()
    for max_ids in (1, 8):
        want_ids = ov.answers(rec, q, max_ids, sets)[1]
        dc = torch.empty(pad // 4 + len(q) + pad // 4, dtype=torch.int32, device="cuda")
        di = torch.empty(pad // 4 + len(q) * max_ids + pad // 4, dtype=torch.int32, device="cuda")
        for n in (1, 63, 64, 65, 4097):
            for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
                for with_ids in (True, False):
                    dc.fill_(0x5A5A5A5A), di.fill_(0x5A5A5A5A)
                    pctx.overlap_device(dq.data_ptr() + pad, n, dc.data_ptr() + pad, di.data_ptr() + pad if with_ids else 0,
                                        max_ids, rtow.F64_STRICT, k)
                    torch.cuda.synchronize()
                    gc, gi = dc.cpu().numpy(), di.cpu().numpy()
                    o = pad // 4
                    assert np.array_equal(gc[o:o + n], counts[:n]), (n, k, max_ids)  # a slice of the batch equals the batch
                    assert np.all(gc[:o] == 0x5A5A5A5A) and np.all(gc[o + n:] == 0x5A5A5A5A), (n, k, "guards behind counts")
                    if with_ids:
                        assert np.array_equal(gi[o:o + n * max_ids].reshape(n, max_ids), want_ids[:n]), (n, k, max_ids)
                        assert np.all(gi[:o] == 0x5A5A5A5A) and np.all(gi[o + n * max_ids:] == 0x5A5A5A5A), (n, k, "guards behind ids")
                    else:
                        assert np.all(gi == 0x5A5A5A5A), (n, k, "ids written without a buffer")
    assert np.array_equal(dq.cpu().numpy(), before)
    # the tensor form of Context.overlap equals the host form, a slice from the middle
    mid = torch.from_numpy(q[1000:1321].view(np.uint8).copy()).cuda()
    c, i = pctx.overlap(mid, 8, rtow.F64_STRICT, rtow.KERNEL_BVH)
    assert c.dtype == torch.int32 and i.shape == (321, 8)
    assert_same((c.cpu().numpy(), i.cpu().numpy()), (counts[1000:1321], ids8[1000:1321]), "tensor slice")
    c, i = pctx.overlap(mid, 8, rtow.F64_STRICT, rtow.KERNEL_BVH, want_ids=False)
    assert i is None and np.array_equal(c.cpu().numpy(), counts[1000:1321])


def test_skipped_queries_walk_nothing(pctx):
    upload(pctx, "hand")
    q = oc.skipped_boxes()
    for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            c, i, st = pctx.overlap(q[:-1], 8, prec, k, want_stats=True)
            assert np.all(c == 0) and np.all(i == -1) and st.prim_tests == 0 and st.node_tests == 0
            assert pctx.overlap(q[-1:], 8, prec, k)[0][0] > 0  # the valid box they were made from


# ------------------------------------------------------------------------------------------------ voxelisation ---
def test_voxelisation_of_suzanne(pctx):
    _, rec, _ = case("suzanne")
    lo, hi = pr.scene_box(rec)
    q = oc.voxel_grid(lo, hi, 8)
    ck = ov.Classified(rec, q)
    k = ov.K["fast"]
    yes = np.array([np.any(ck.r[ck.cut[i]:ck.cut[i + 1]] < -k) for i in range(len(q))])
    maybe = np.array([np.any(np.abs(ck.r[ck.cut[i]:ck.cut[i + 1]]) <= k) for i in range(len(q))])
    # (the mesh is symmetric and the grid has a face in its seam: pairs touch there, but every voxel that touches a
    # triangle also holds one)
    assert not np.any(maybe & ~yes)  # no undecided voxel on this input
    assert 100 < yes.sum() < 400
    want = ov.answers(rec, q, 8)[0]
    upload(pctx, "suzanne")
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        for kname, kk in KERNELS.items():
            c, _ = pctx.overlap(q, 8, prec, kk, want_ids=False)
            assert np.array_equal(c > 0, yes), (prec, kname)
            if prec == rtow.F64_STRICT:
                assert np.array_equal(c, want), kname
            ov.check_answers(ck, c, None, 8, "fast", (prec, kname))


# ---------------------------------------------------------------------------------------------------- contracts ---
def _message(call):
    with pytest.raises(rtow.RtowError) as e:
        call()
    return str(e.value)


def test_argument_errors_in_their_order():
    import torch

    scene, rec, _ = case("cover_moving")
    q = oc.random_boxes(rec, 200, 37)
    L = rtow.lib()
    c = rtow.Context(0)
    dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    dc = torch.empty(len(q) + 4, dtype=torch.int32, device="cuda")
    di = torch.empty(len(q) * 8 + 4, dtype=torch.int32, device="cuda")
    Q, Cn, I = dq.data_ptr(), dc.data_ptr(), di.data_ptr()

    def dev(ctx=c, prec=rtow.F64_STRICT, k=rtow.KERNEL_BVH, q_=Q, n=4, max_ids=8, counts=Cn, ids=I):
        h = ctx._h if ctx is not None else None
        return lambda: rtow.check(L.rtow_overlap_device(h, prec, k, C.c_void_p(q_), n, max_ids, C.c_void_p(counts),
                                                        C.c_void_p(ids), None, None), "rtow_overlap_device")

    def host(ctx=c, prec=rtow.F64_STRICT, k=rtow.KERNEL_BVH, n=4, max_ids=8, q_=True, counts=True):
        h = ctx._h if ctx is not None else None
        cn, ids = np.empty(max(n, 1), np.int32), np.empty((max(n, 1), 8), np.int32)
        return lambda: rtow.check(L.rtow_overlap(h, prec, k, q.ctypes.data_as(C.c_void_p) if q_ else None, n, max_ids,
                                                 cn.ctypes.data_as(C.c_void_p) if counts else None,
                                                 ids.ctypes.data_as(C.c_void_p), None), "rtow_overlap")

    try:
        # every later error is present in each call: the earliest one in the order is the one reported
        assert "(-1)" in _message(dev(ctx=None, max_ids=0, n=-1)) and "ctx is NULL" in _message(dev(ctx=None, max_ids=0, n=-1))
        assert "ctx is NULL" in _message(host(ctx=None, max_ids=9))
        for m in (0, 9, -1):
            assert "max_ids" in _message(dev(max_ids=m, n=-1, counts=0, prec=rtow.F32))
            assert "max_ids" in _message(host(max_ids=m, n=-1, counts=False, prec=rtow.F32))
        for n in (-1, (1 << 31) - 63):
            assert "outside [0, 2^31 - 64]" in _message(dev(n=n, counts=0, q_=Q + 8, prec=rtow.F32))
            assert "outside [0, 2^31 - 64]" in _message(host(n=n, counts=False, prec=rtow.F32))
        assert "NULL query or count buffer" in _message(dev(counts=0, q_=Q + 8, prec=rtow.F32))
        assert "NULL query or count buffer" in _message(dev(q_=0, counts=Cn + 2, prec=rtow.F32))
        assert "NULL query or count array" in _message(host(counts=False, prec=rtow.F32))
        assert "NULL query or count array" in _message(host(q_=False, k=rtow.KERNEL_REFTREE))
        assert "query buffer must be 16-byte aligned" in _message(dev(q_=Q + 8, counts=Cn + 2, prec=rtow.F32))
        assert "count buffer must be 4-byte aligned" in _message(dev(counts=Cn + 2, ids=I + 1, prec=rtow.F32))
        assert "ids buffer must be 4-byte aligned" in _message(dev(ids=I + 1, prec=rtow.F32))
        assert "RTOW_F32" in _message(dev(prec=rtow.F32, k=9))
        assert "unknown precision" in _message(dev(prec=7, k=9))
        assert "unknown kernel" in _message(dev(k=9)) and "unknown kernel" in _message(dev(k=-1))
        # no scene yet: before the strategy is looked at (the host form stages nothing for a context without a scene)
        for call in (dev(k=rtow.KERNEL_REFTREE), host(k=rtow.KERNEL_REFTREE), dev(), host(), host(prec=rtow.F32)):
            assert "(-4)" in _message(call)
        hs = rtow.HostScene.cover(11, 1.5, True)
        c.render(hs, rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST))  # lean upload: the grid only
        q0 = q.copy()  # (the host scene has its own insertion order: counts without min_prim do not depend on it)
        q0["min_prim"] = 0
        cn, ids, st = c.overlap(q0, 8, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0 and st.prim_tests == len(q) * rec.n
        assert np.array_equal(cn, ov.answers(rec, q0, 8)[0]) and cn.max() > 0, "lean upload, AUTO"
        for k in (rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            assert "(-4)" in _message(lambda k=k: c.overlap(q, 8, rtow.F64_STRICT, k))
        hs.close()
        c.upload(scene)
        assert "RTOW_F32" in _message(host(prec=rtow.F32, k=9)) and "unknown precision" in _message(host(prec=7, k=9))
        assert "unknown kernel" in _message(host(k=9))
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            assert "(-1)" in _message(dev(prec=prec, k=rtow.KERNEL_REFTREE)) and "REFTREE" in _message(host(prec=prec, k=rtow.KERNEL_REFTREE))
        st = c.overlap_device(0, 0, 0, 0, 8, rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)  # n == 0 launches nothing
        assert st.segments == 0 and st.prim_tests == 0 and st.node_tests == 0 and st.kernel_ms == 0.0
    finally:
        c.close()


def test_stats(pctx):
    _, rec, _ = case("mesh96k")
    q = oc.random_boxes(rec, 256, 43, (0.004,))
    upload(pctx, "mesh96k")
    for kname, k in KERNELS.items():
        if kname == "brute":
            continue
        st = pctx.overlap(q, 8, rtow.F64_FAST, k, want_stats=True)[2]
        assert st.kernel_used == used(k, True) and st.segments == len(q) and st.samples == 0
        assert 0 < st.node_tests < 0.01 * len(q) * rec.n  # a small box in a big mesh: far fewer nodes than primitives exist
        assert 0 < st.prim_tests < 0.01 * len(q) * rec.n and 0.0 < st.kernel_ms <= st.total_ms
    _, rec, _ = case("cover_moving")
    q = np.concatenate([oc.skipped_boxes(), oc.random_boxes(rec, 300, 44)])
    upload(pctx, "cover_moving")
    active = int((~ov.skipped(q)).sum())
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        st = pctx.overlap(q, 8, prec, rtow.KERNEL_BRUTE, want_stats=True)[2]
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0 and st.prim_tests == active * rec.n
        st = pctx.overlap(q, 8, prec, rtow.KERNEL_GRID, want_stats=True)[2]
        assert st.kernel_used == rtow.KERNEL_BVH and 0 < st.prim_tests < active * rec.n and st.node_tests > 0


def test_overlaps_leave_the_render_untouched():
    hs = rtow.HostScene.cover(11, 1.5, True)
    G = ai.Geometry.of_scene(hs.c)
    q = oc.random_boxes(pr.make_records(G.sph, G.mov, G.tri), 300, 41)
    cfg = rtow.make_config(48, 32, 2, 1, 10, seed=5, precision=rtow.F64_STRICT)
    c = rtow.Context(0)
    try:
        before, _ = c.render(hs, cfg)
        c.upload(hs.c)
        for k in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_AUTO):
            c.overlap(q, 8, rtow.F64_STRICT, k)
            c.overlap(q, 8, rtow.F64_FAST, k)
        after, _ = c.render(hs, cfg)
        assert np.array_equal(before, after)
    finally:
        c.close()
        hs.close()
