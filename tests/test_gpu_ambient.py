"""Ambient (hemisphere visibility) queries (rtow_ambient / rtow_ambient_device) on the GPU.

The strict build is checked against the numpy mirror of the definition (ambient_ref.py): the exported rays bit for bit,
and the record as the mirror's in-order fold of rtow_occluded's answers on those rays, under every strategy and both
builders.  Both builds are checked for sample additivity and batch independence, and for the skipped points; the fast
build against fast rtow_occluded on its own exported rays and against the strict build outside the rounding band of the
existing occlusion test.  The contracts close the file.
"""
import ctypes as C
import math

import numpy as np
import pytest

import ambient_ref
import rtow
from ambient_cases import handmade_points, scene_extent
from support_fixtures import big_mesh, logged  # noqa: F401
from support_oracle import FAST_CASES, LOGGED, rays_of
from support_scenes import SceneView, handmade_scene
from support_tables import BUILDERS, KERNELS, WALKS

pytestmark = pytest.mark.gpu

SEED = 20261021
N_POINTS = 4000


@pytest.fixture(scope="module")
def actx():
    c = rtow.Context(0)
    yield c
    c.close()


def points_of_log(ctx, view, log, n, seed):
    """Hit points and hit normals of logged rays (strict closest hit on the resident scene) at the log's times: half with
    max_dist = 5 % of the scene's extent, half unbounded."""
    hits = ctx.intersect(rays_of(log), rtow.F64_STRICT, rtow.KERNEL_AUTO)
    ok = np.nonzero(np.isfinite(hits["t"]))[0]
    g = np.random.default_rng(seed)
    idx = np.sort(g.choice(ok, size=min(n, len(ok)), replace=False))
    md = np.where(g.random(len(idx)) < 0.5, 0.05 * scene_extent(view), math.inf)
    return rtow.make_surface_points(hits["point"][idx], hits["normal"][idx], time=log[idx, 9], max_dist=md)


@pytest.fixture(scope="module")
def cases(actx, logged, big_mesh):
    """name -> (scene, view, points, ids): the point sets of the module, made once."""
    out = {}
    for j, (name, (scene, view, log)) in enumerate(list(logged.items()) + [("mesh96k", big_mesh)]):
        actx.upload(scene)
        pts = points_of_log(actx, view, log, N_POINTS, seed=31 + j)
        g = np.random.default_rng(100 + j)
        ids = np.stack([g.integers(0, 1 << 32, len(pts)), g.integers(0, 1 << 32, len(pts))], axis=1).astype(np.uint32)
        out[name] = (scene, view, pts, ids)
    hs = handmade_scene()
    out["handmade"] = (hs, SceneView(hs), handmade_points(), None)
    return out


def upload(ctx, scene):
    ctx.upload(scene.c if not isinstance(scene, rtow.HostScene) else scene)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. strict: every kernel and both builders ---
def strict_against_mirror(ctx, pts, ids, kernels, what):
    answers = {}
    for samples in (1, 7):
        want_rays = ambient_ref.rays(pts, samples, SEED, ids, sample_first=3)
        for kn, k in kernels.items():
            out, rays, st = ctx.ambient(pts, samples, SEED, ids, 3, rtow.F64_STRICT, k, want_rays=True, want_stats=True)
            assert same_bytes(rays, want_rays), (what, kn, samples, int((rays != want_rays).sum()))
            occ = ctx.occluded(rays.reshape(-1), rtow.F64_STRICT, k)
            want = ambient_ref.fold(pts, rays, occ)
            assert same_bytes(out, want), (what, kn, samples, np.nonzero(out != want)[0][:5])
            assert st.segments == len(pts) * samples == st.samples and st.prim_tests > 0
            total = len(pts) * samples
            assert 0 < out["open"].sum() < total, (what, kn, samples)
            if kn != "reftree":
                answers[(kn, samples)] = out
    for (kn, samples), out in answers.items():
        assert same_bytes(out, answers[("bvh", samples)]), (what, kn, samples)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(LOGGED) + ["handmade"])
def test_strict_equals_the_mirror_folded_over_occluded(actx, cases, name, builder):
    """samples 1 and 7: the exported rays are the mirror's bit for bit; the record is the mirror's fold of strict
    rtow_occluded (same kernel) on them, bit for bit; BRUTE, BVH, GRID and BVH4 give the same bytes; open and closed
    samples both occur."""
    scene, view, pts, ids = cases[name]
    actx.set_builder(BUILDERS[builder])
    try:
        upload(actx, scene)
        strict_against_mirror(actx, pts, ids, KERNELS, (name, builder))
    finally:
        actx.set_builder(rtow.BUILDER_AUTO)


def test_strict_on_the_large_mesh(actx, cases):
    scene, view, pts, ids = cases["mesh96k"]
    upload(actx, scene)
    strict_against_mirror(actx, pts, ids, {k: KERNELS[k] for k in ("bvh", "bvh4", "grid")}, "mesh96k")


# ------------------------------------------- 2. sample additivity and batch independence, both builds ---
@pytest.mark.parametrize("precision", [rtow.F64_STRICT, rtow.F64_FAST], ids=["strict", "fast"])
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_samples_add_up_and_batches_do_not_matter(actx, cases, name, precision):
    """samples = 5 equals the in-order sum of five one-sample calls at sample_first + j; slices of a batch with explicit
    ids equal the whole batch; nothing is written beyond n records and n x samples rays."""
    import torch

    scene, view, pts, ids = cases[name]
    upload(actx, scene)
    pts, ids = pts[:200], ids[:200]
    samples = 5
    for k in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH):
        whole, whole_rays = actx.ambient(pts, samples, SEED, ids, 40, precision, k, want_rays=True)
        acc = np.zeros(len(pts), dtype=rtow.AMBIENT_DTYPE)
        for j in range(samples):
            one, one_rays = actx.ambient(pts, 1, SEED, ids, 40 + j, precision, k, want_rays=True)
            assert same_bytes(one_rays[:, 0], whole_rays[:, j]), (name, k, j)
            for f in ("open", "bent", "sky", "samples"):
                acc[f] = acc[f] + one[f]
        assert same_bytes(acc, whole), (name, k)
        assert 0 < whole["open"].sum() < samples * len(pts)

        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to("cuda:0")
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).to("cuda:0")
        for n in (1, 63, 64, 65, 200):
            d_out = torch.full(((n + 2) * 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
            d_rays = torch.full(((n * samples + 2) * 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
            st = actx.ambient_device(d_pts.data_ptr(), n, d_ids.data_ptr(), d_out.data_ptr() + 64, samples,
                                     d_rays.data_ptr() + 64, SEED, 40, precision, k, 0, True)
            assert st.segments == n * samples
            o, r = d_out.cpu().numpy(), d_rays.cpu().numpy()
            assert np.all(o[:64] == 0xAB) and np.all(o[-64:] == 0xAB), n
            assert np.all(r[:64] == 0xCD) and np.all(r[-64:] == 0xCD), n
            assert o[64:-64].tobytes() == whole[:n].tobytes(), (name, k, n)
            assert r[64:-64].tobytes() == whole_rays[:n].tobytes(), (name, k, n)
            # without the export: the same records, nothing else
            d_out.fill_(0xAB)
            actx.ambient_device(d_pts.data_ptr(), n, d_ids.data_ptr(), d_out.data_ptr() + 64, samples, 0, SEED, 40,
                                precision, k, 0, True)
            o = d_out.cpu().numpy()
            assert np.all(o[:64] == 0xAB) and np.all(o[-64:] == 0xAB), n
            assert o[64:-64].tobytes() == whole[:n].tobytes(), (name, k, n)


# ------------------------------------------------------------------------------------------ 3. skipped points ---
@pytest.mark.parametrize("precision", [rtow.F64_STRICT, rtow.F64_FAST], ids=["strict", "fast"])
def test_skipped_points_give_zero_records_and_leave_their_neighbours_alone(actx, cases, precision):
    scene, view, pts, ids = cases["cover_static"]
    upload(actx, scene)
    good, ids = pts[:130].copy(), ids[:130]
    good[71]["normal"] = [0.0, 2e-154, 0.0]  # (live: its squared length, 4e-308, is a normal binary64)
    bad = good.copy()
    where = {0: ("normal", [0.0, 0.0, 0.0]), 5: ("normal", [math.nan, 1.0, 0.0]), 63: ("normal", [0.0, math.inf, 0.0]),
             64: ("max_dist", math.nan), 100: ("max_dist", 0.0009), 129: ("max_dist", -1.0), 7: ("normal", [0.0, -0.0, 0.0]),
             65: ("normal", [1e200, 0.0, 0.0]), 66: ("normal", [1e-200, 0.0, 0.0]),
             # a subnormal normal . normal: too few bits to normalise by
             67: ("normal", [1e-155, 0.0, 0.0]), 68: ("normal", [0.0, -1e-158, 0.0]), 69: ("normal", [0.0, 0.0, 1e-160]),
             70: ("normal", [-1e-161, 0.0, 0.0])}
    for i, (field, value) in where.items():
        bad[i][field] = value
    skip = np.zeros(len(bad), dtype=bool)
    skip[list(where)] = True
    assert np.array_equal(ambient_ref.skipped(bad), skip)
    for kn, k in WALKS.items():
        ref, ref_rays = actx.ambient(good, 3, SEED, ids, 0, precision, k, want_rays=True)
        out, rays = actx.ambient(bad, 3, SEED, ids, 0, precision, k, want_rays=True)
        assert same_bytes(out[~skip], ref[~skip]) and same_bytes(rays[~skip], ref_rays[~skip]), kn
        assert not out[skip].view(np.uint8).any(), kn  # (eight doubles of +0.0)
        dead = rays[skip].copy()
        assert np.all(dead["tmax"] == -1.0), kn
        dead["tmax"] = 0.0
        assert not dead.view(np.uint8).any(), kn
        assert np.all(out["samples"][~skip] == 3.0)
        assert np.abs(np.sqrt((rays["direction"][71] ** 2).sum(axis=1)) - 1.0).max() <= 2e-8, kn


# ---------------------------------------------------------------------------------------------- 4. fast build ---
def fast_against_occluded(ctx, pts, ids, k, what):
    out_f, rays_f = ctx.ambient(pts, 1, SEED, ids, 9, rtow.F64_FAST, k, want_rays=True)
    out_s, rays_s = ctx.ambient(pts, 1, SEED, ids, 9, rtow.F64_STRICT, k, want_rays=True)
    rays_f, rays_s = rays_f.reshape(-1), rays_s.reshape(-1)
    assert np.abs(rays_f["direction"] - rays_s["direction"]).max() <= 1e-12, what
    for f in ("origin", "time", "tmax"):
        assert same_bytes(rays_f[f], rays_s[f]), (what, f)
    occ_f = ctx.occluded(rays_f, rtow.F64_FAST, k)
    inf_f, inf_s = rays_f.copy(), rays_s.copy()
    inf_f["tmax"] = inf_s["tmax"] = math.inf
    tf_all = ctx.intersect(inf_f, rtow.F64_FAST, k)["t"]
    ts_all = ctx.intersect(inf_s, rtow.F64_STRICT, k)["t"]
    tmax = rays_f["tmax"]
    with np.errstate(invalid="ignore"):
        # (an unbounded ray has no band: no t is near max_dist = inf, though inf <= 1e-9 * inf would say so)
        tol = np.where(np.isfinite(tmax), 1e-9 * np.maximum(1.0, tmax), 0.0)
        band_f = np.isfinite(tmax) & (np.abs(tf_all - tmax) <= tol)
        band_s = np.isfinite(tmax) & (np.abs(ts_all - tmax) <= tol)
    open_f, open_s = out_f["open"], out_s["open"]
    assert set(np.unique(open_f)) <= {0.0, 1.0}
    bad = np.nonzero(((1.0 - open_f) != occ_f) & ~band_f)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5])
    assert band_f.mean() < 0.01 and band_s.mean() < 0.01, (what, band_f.mean(), band_s.mean())
    split = np.isfinite(tf_all) != np.isfinite(ts_all)
    assert split.mean() <= 1e-4, (what, int(split.sum()))
    keep = ~band_f & ~band_s & ~split
    assert np.array_equal(open_f[keep], open_s[keep]), (what, int((open_f != open_s)[keep].sum()))
    assert 0 < open_f.sum() < len(open_f), what
    print(f"\n{what}: band {int(band_f.sum())} of {len(rays_f)}, split {int(split.sum())}, "
          f"fast != strict {int((open_f != open_s).sum())}")


@pytest.mark.parametrize("name,kernel", FAST_CASES)
def test_fast_build_equals_fast_occluded_on_its_own_rays(actx, cases, name, kernel):
    """One sample per point, so `open` is per ray: the exported directions are within 1e-12 of the strict ones, 1 - open
    is fast rtow_occluded on the exported rays outside the band |t_fast - tmax| <= 1e-9 max(1, tmax), the band holds
    under 1 % of the rays, and fast and strict agree outside the band and the closest hits' hit / miss split."""
    scene, view, pts, ids = cases[name]
    upload(actx, scene)
    fast_against_occluded(actx, pts, ids, WALKS[kernel], (name, kernel))


# ------------------------------------------------------------------------------------------------ 5. contracts ---
def test_zero_points_launch_nothing(actx, cases):
    import torch

    scene, view, pts, ids = cases["cover_static"]
    upload(actx, scene)
    d_out = torch.full((256,), 0xAB, dtype=torch.uint8, device="cuda:0")
    st = actx.ambient_device(0, 0, 0, d_out.data_ptr(), 4, 0, SEED, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
    assert st.segments == 0 and st.samples == 0 and st.prim_tests == 0 and st.node_tests == 0 and st.kernel_ms == 0.0
    assert np.all(d_out.cpu().numpy() == 0xAB)
    prm = rtow.AmbientParams(1, 4, 0)
    assert rtow.lib().rtow_ambient_device(actx._h, 0, 0, C.byref(prm), None, 0, None, None, None, None, None) == rtow.RTOW_OK
    out = actx.ambient(np.empty(0, dtype=rtow.SURFACE_POINT_DTYPE), 4, precision=rtow.F64_STRICT)
    assert out.shape == (0,)


def test_refusals(actx, cases):
    import torch

    scene, view, pts, ids = cases["cover_static"]
    upload(actx, scene)
    few = pts[:100]
    for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, 0), (0, 9)):
        with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
            actx.ambient(few, 4, precision=prec, kernel=kern)
    for samples in (0, -3, rtow.MAX_AMBIENT_SAMPLES + 1):
        with pytest.raises(rtow.RtowError, match=r"\(-1\).*samples"):
            actx.ambient(few, samples, precision=rtow.F64_STRICT)
        with pytest.raises(rtow.RtowError, match=r"\(-1\).*samples"):
            actx.ambient(few, samples, precision=rtow.F64_STRICT, want_rays=True)
    out, st = actx.ambient(few[:2], rtow.MAX_AMBIENT_SAMPLES, precision=rtow.F64_STRICT, want_stats=True)
    assert np.all(out["samples"] == rtow.MAX_AMBIENT_SAMPLES) and st.segments == 2 * rtow.MAX_AMBIENT_SAMPLES
    assert np.all(out["open"] <= rtow.MAX_AMBIENT_SAMPLES)
    L = rtow.lib()
    d_pts = torch.from_numpy(few.view(np.uint8).copy()).to("cuda:0")
    d_out = torch.zeros(len(few) * 64 + 64, dtype=torch.uint8, device="cuda:0")
    d_rays = torch.zeros(len(few) * 2 * 64 + 64, dtype=torch.uint8, device="cuda:0")
    d_ids = torch.zeros(len(few) * 2 + 2, dtype=torch.int32, device="cuda:0")
    prm = rtow.AmbientParams(1, 2, 0)
    P, I, O, R = d_pts.data_ptr(), d_ids.data_ptr(), d_out.data_ptr(), d_rays.data_ptr()
    v = lambda a: C.c_void_p(a) if a else None  # noqa: E731
    call = lambda p, n, i, o, r, prm=prm: L.rtow_ambient_device(actx._h, 0, 0, C.byref(prm) if prm else None, v(p), n,  # noqa: E731
                                                                v(i), v(o), v(r), None, None)
    assert call(P, 4, I, O, R) == rtow.RTOW_OK
    for args in ((P + 8, 4, I, O, R), (P, 4, I + 4, O, R), (P, 4, I, O + 8, R), (P, 4, I, O, R + 8)):
        assert call(*args) == rtow.RTOW_EINVAL, args
        assert b"aligned" in L.rtow_last_error()
    assert call(P, 4, I, O, R, prm=None) == rtow.RTOW_EINVAL and b"params" in L.rtow_last_error()
    for n, p, o in ((-1, None, None), (1, None, None), (1, P, None), ((1 << 31) - 63, 16, 16)):
        assert call(p, n, None, o, None) == rtow.RTOW_EINVAL, n
    # n * samples beyond 2^31 - 64 is refused with an export only (nothing is launched: the pointers are never read)
    big = rtow.AmbientParams(1, 65536, 0)
    assert call(16, 1 << 16, None, 16, 16, prm=big) == rtow.RTOW_EINVAL and b"n * samples" in L.rtow_last_error()
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy()[4 * 64:].any()


def test_lean_upload_residency_and_kernel_used(cases):
    scene, view, pts, ids = cases["cover_moving"]
    few = pts[:500]
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.ambient(few, 2, precision=rtow.F64_STRICT)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        out, st = c.ambient(few, 2, precision=rtow.F64_FAST, kernel=rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and st.segments == 2 * len(few) == st.samples
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
            c.ambient(few, 2, precision=rtow.F64_FAST, kernel=rtow.KERNEL_BVH)
        c.upload(scene)
        for prec in (rtow.F64_STRICT, rtow.F64_FAST):
            for k in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
                a, st = c.ambient(few, 3, SEED, precision=prec, kernel=k, want_stats=True)
                b = c.ambient(few, 3, SEED, precision=prec, kernel=k)
                assert same_bytes(a, b), (prec, k)
                # the render's fallbacks: AUTO walks the grid on a sphere scene, BVH4 is for triangle meshes only
                want = {rtow.KERNEL_AUTO: rtow.KERNEL_GRID, rtow.KERNEL_BVH4: rtow.KERNEL_BVH}.get(k, k)
                assert st.kernel_used == want, (prec, k)
                assert st.node_tests > 0 and st.prim_tests > 0 and st.segments == 3 * len(few)
        hs, _, hp, _ = cases["handmade"]
        c.upload(hs.c)
        _, st = c.ambient(hp, 2, precision=rtow.F64_STRICT, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0 and st.prim_tests > 0
    finally:
        c.close()


def test_side_stream_right_after_upload_on_a_fresh_context(cases):
    import torch

    scene, view, pts, ids = cases["suzanne"]
    ref_ctx = rtow.Context(0)
    try:
        ref_ctx.upload(scene)
        ref = ref_ctx.ambient(pts, 4, SEED, ids, precision=rtow.F64_STRICT)
    finally:
        ref_ctx.close()
    side = torch.cuda.Stream(device="cuda:0")
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to("cuda:0")
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to("cuda:0")
    d_out = torch.zeros(len(pts) * 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for builder in BUILDERS.values():
        c = rtow.Context(0)
        try:
            c.set_builder(builder)
            c.upload(scene)  # no wait: the query on the side stream must find the scene complete
            c.ambient_device(d_pts.data_ptr(), len(pts), d_ids.data_ptr(), d_out.data_ptr(), 4, 0, SEED, 0,
                             rtow.F64_STRICT, rtow.KERNEL_AUTO, side.cuda_stream, False)
            side.synchronize()
            assert d_out.cpu().numpy().tobytes() == ref.tobytes(), builder
        finally:
            c.close()


def test_ambient_leaves_the_render_and_the_occlusion_query_untouched(cases):
    """A render and an rtow_occluded call before and after ten ambient calls: bit-identical, and the profile ring counts
    render launches only."""
    import torch

    scene, view, pts, ids = cases["cover_moving"]
    c = rtow.Context(0)
    try:
        c.upload(scene)
        cfg = rtow.make_config(120, 80, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((80, 120, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        probe = ambient_ref.rays(pts, 2, SEED, ids).reshape(-1)
        occ_before = c.occluded(probe, rtow.F64_STRICT, rtow.KERNEL_BVH)
        assert c.profile_collect()[1] == 1
        for k in range(10):
            c.ambient(pts[:1000], 1 + k % 3, SEED, precision=rtow.F64_STRICT if k % 2 else rtow.F64_FAST,
                      kernel=[0, 1, 2, 3, 5][k % 5] if k % 2 else [0, 1, 2, 3][k % 4], want_rays=bool(k % 4 == 0))
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
        assert c.occluded(probe, rtow.F64_STRICT, rtow.KERNEL_BVH).tobytes() == occ_before.tobytes()
    finally:
        c.close()
