"""Any-hit (occlusion) ray queries (rtow_occluded / rtow_occluded_device) on the GPU.

The strict build is checked against the oracle's log (the expected bits come from the logged t_hit, not from the GPU),
against the closest-hit query on shadow and AO rays under every strategy, and against an any-hit brute force over the
oracle's hit tests on the hand-made scene.  The fast build is checked against the fast closest hit and the strict
answer outside a rounding band around tmax.  The contracts (ragged counts, ordering, residency, errors, no side effect
on the render or the closest-hit query) close the file.
"""
import ctypes as C
import math

import numpy as np
import pytest

import rtow
from support_fixtures import big_mesh, logged, octx  # noqa: F401
from support_oracle import LOGGED, rays_of
from support_scenes import SceneView, handmade_rays, handmade_scene
from support_tables import BUILDERS, KERNELS as STRICT_KERNELS, WALKS

pytestmark = pytest.mark.gpu


def expected_from_log(log, tmax):
    t = log[:, 10]
    return np.isfinite(t) & (t <= tmax)


def scene_box(view):
    """Box of the scene's small primitives (not the cover scene's ground sphere): (lo, hi)."""
    pts = []
    small = view.sph[np.abs(view.sph[:, 3]) < 100.0]
    if len(small):
        pts += [small[:, :3] - np.abs(small[:, 3:4]), small[:, :3] + np.abs(small[:, 3:4])]
    if len(view.mov):
        pts += [view.mov[:, 0:3] - view.mov[:, 6:7], view.mov[:, 3:6] + view.mov[:, 6:7]]
    if len(view.tri):
        pts.append(view.tri.reshape(-1, 3))
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def shadow_and_ao_rays(view, log, n, seed):
    """From the hit points of logged segments: shadow rays toward a point light above the scene (d = L - p, tmax = 1)
    and AO rays along seeded uniform directions with tmax = 5 % of the scene's extent."""
    hit = log[np.isfinite(log[:, 10])]
    g = np.random.default_rng(seed)
    rows = hit[g.choice(len(hit), size=min(n, len(hit)), replace=False)]
    p = rows[:, 3:6] + rows[:, 10:11] * rows[:, 6:9]
    lo, hi = scene_box(view)
    ext = float(np.max(hi - lo))
    light = 0.5 * (lo + hi) + np.array([0.2 * ext, 1.5 * ext, 0.1 * ext])
    shadow = rtow.make_rays(p, light[None, :] - p, time=rows[:, 9], tmax=1.0)
    u = g.normal(size=(len(p), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ao = rtow.make_rays(p, u, time=rows[:, 9], tmax=0.05 * ext)
    return shadow, ao


# ------------------------------------------------------------------------------------ 1. logged rays, strict ---
@pytest.mark.parametrize("kernel", list(STRICT_KERNELS))
@pytest.mark.parametrize("name", list(LOGGED))
def test_logged_rays_strict_every_kernel(octx, logged, name, kernel):
    """Every segment of an oracle render with tmax = inf, t_hit, nextafter(t_hit, 0), 0.000999, a random fraction of
    t_hit and a value beyond it: the answer is the log's `t_hit <= tmax`, under every strategy."""
    scene, view, log = logged[name]
    octx.upload(scene)
    k = STRICT_KERNELS[kernel]
    t = log[:, 10]
    hit = np.isfinite(t)
    g = np.random.default_rng(17)
    tf = np.where(hit, t, g.uniform(0.01, 30.0, len(t)))  # (miss rays: some finite tmax)
    cases = {
        "inf": np.full(len(t), math.inf),
        "t_hit": tf,
        "below": np.nextafter(tf, 0.0),
        "short": np.full(len(t), 0.000999),
        "fraction": tf * g.random(len(t)),
        "beyond": tf * (1.0 + g.random(len(t))),
    }
    for what, tmax in cases.items():
        occ, st = octx.occluded(rays_of(log, tmax=tmax), rtow.F64_STRICT, k, want_stats=True)
        want = expected_from_log(log, tmax)
        assert occ.dtype == np.bool_ and len(occ) == len(log)
        bad = np.nonzero(occ != want)[0]
        assert len(bad) == 0, (name, kernel, what, len(bad), bad[:5])
        assert st.segments == len(log) and st.samples == 0
    assert np.array_equal(octx.occluded(rays_of(log, tmax=math.inf), rtow.F64_STRICT, k), hit)


# ------------------------------------------------------------------------------ 2. shadow and AO rays, strict ---
SHADOW_CASES = [(n, b) for n in list(LOGGED) + ["mesh96k"] for b in BUILDERS]


@pytest.mark.parametrize("name,builder", SHADOW_CASES)
def test_shadow_and_ao_rays_strict_equal_closest_hit(octx, logged, big_mesh, name, builder):
    """occluded == (intersect(rays).t <= tmax) under the same strategy, and the same answer under BRUTE, BVH, GRID and
    BVH4 (REFTREE: against its own closest hit; not on the 96.8k mesh, nor BRUTE there: 96,800 tests per ray)."""
    scene, view, log = big_mesh if name == "mesh96k" else logged[name]
    octx.set_builder(BUILDERS[builder])
    try:
        octx.upload(scene)
        shadow, ao = shadow_and_ao_rays(view, log, 60000, seed=3)
        kernels = dict(WALKS, reftree=rtow.KERNEL_REFTREE) if name != "mesh96k" else {"bvh": rtow.KERNEL_BVH,
                                                                                     "grid": rtow.KERNEL_GRID,
                                                                                     "bvh4": rtow.KERNEL_BVH4}
        for set_name, rays in (("shadow", shadow), ("ao", ao)):
            answers = {}
            for kn, k in kernels.items():
                occ, st = octx.occluded(rays, rtow.F64_STRICT, k, want_stats=True)
                hits = octx.intersect(rays, rtow.F64_STRICT, k)
                want = np.isfinite(hits["t"]) & (hits["t"] <= rays["tmax"])
                assert np.array_equal(occ, want), (name, builder, set_name, kn, int((occ != want).sum()))
                assert st.segments == len(rays) and st.prim_tests > 0
                if kn != "reftree":
                    answers[kn] = occ
            share = float(answers["bvh"].mean())
            assert 0.0 < share < 1.0, (name, set_name, share)  # (both answers occur)
            for kn, occ in answers.items():
                assert np.array_equal(occ, answers["bvh"]), (name, builder, set_name, kn)
    finally:
        octx.set_builder(rtow.BUILDER_AUTO)


# ------------------------------------------------------------------------------ 3. hand-made scene, strict ---
def any_hit_brute_force(view, rays):
    out = np.zeros(len(rays), dtype=bool)
    for j, r in enumerate(rays):
        for p in range(len(view.kind)):
            if view.oracle_hit(p, r["origin"], r["direction"], r["time"], tmax=r["tmax"]) is not None:
                out[j] = True
                break
    return out


@pytest.mark.parametrize("kernel", list(WALKS))
def test_handmade_rays_strict_equal_any_hit_brute_force(octx, kernel):
    """Axis-parallel rays with +-0 components, rays from inside the glass shell and the hollow sphere, rays in a
    triangle's plane, the moving sphere at three shutter times: with infinite tmax and with seeded finite ones, the
    answer equals `some primitive's oracle hit test accepts in [0.001, tmax]`.  (REFTREE is left out as in
    test_gpu_query.py: the reference's tree misses negative-radius spheres by design.)"""
    scene = handmade_scene()
    view = SceneView(scene)
    octx.upload(scene.c)
    rays = handmade_rays()
    assert np.signbit(rays["direction"]).any()
    g = np.random.default_rng(11)
    finite = rays.copy()
    finite["tmax"] = g.choice([0.0005, 0.3, 1.0, 2.5, 6.0, 50.0], size=len(rays)) * g.random(len(rays)) * 2.0
    for what, rs in (("inf", rays), ("finite", finite)):
        want = any_hit_brute_force(view, rs)
        got = octx.occluded(rs, rtow.F64_STRICT, WALKS[kernel])
        assert np.array_equal(got, want), (kernel, what, np.nonzero(got != want)[0][:5])
        if what == "finite":
            assert 0 < want.sum() < len(want)


@pytest.mark.parametrize("kernel", list(WALKS))
def test_axis_parallel_rays_with_signed_zeros(octx, logged, kernel):
    """Directions along the axes (-e has -0.0 components) on the cover scene (the grid walk's sphere lists) and on
    suzanne: the answer equals the closest-hit query's under the same strategy and BRUTE's."""
    for name in ("cover_static", "suzanne"):
        scene, view, log = logged[name]
        octx.upload(scene)
        lo, hi = scene_box(view)
        g = np.random.default_rng(2)
        o, d = [], []
        for a in range(3):
            for s in (1.0, -1.0):
                e = s * np.eye(3)[a]
                for _ in range(300):
                    p = lo + (hi - lo) * g.random(3)
                    p[a] = (lo[a] - 1.0) if s > 0 else (hi[a] + 1.0)
                    o.append(p), d.append(e)
        rays = rtow.make_rays(np.array(o), np.array(d), time=0.0)
        rays["tmax"] = np.where(g.random(len(rays)) < 0.5, math.inf, float(np.max(hi - lo)) * g.random(len(rays)))
        assert np.signbit(rays["direction"]).sum() > len(rays)
        got = octx.occluded(rays, rtow.F64_STRICT, WALKS[kernel])
        hits = octx.intersect(rays, rtow.F64_STRICT, WALKS[kernel])
        assert np.array_equal(got, np.isfinite(hits["t"])), (name, kernel)
        assert np.array_equal(got, octx.occluded(rays, rtow.F64_STRICT, rtow.KERNEL_BRUTE)), (name, kernel)
        assert 0 < got.sum() < len(got)


# ---------------------------------------------------------------------------------------------- 4. fast build ---
FAST_CASES = [(n, k) for n in list(LOGGED) + ["mesh96k"] for k in WALKS if (n, k) != ("mesh96k", "brute")]


@pytest.mark.parametrize("name,kernel", FAST_CASES)
def test_fast_build_outside_the_rounding_band(octx, logged, big_mesh, name, kernel):
    """Fast occlusion == fast `intersect.t <= tmax` and == strict occlusion, except for rays whose t lies within
    1e-9 * max(1, tmax) of tmax; that band holds a small share of the rays."""
    scene, view, log = big_mesh if name == "mesh96k" else logged[name]
    octx.upload(scene)
    shadow, ao = shadow_and_ao_rays(view, log, 40000, seed=5)
    g = np.random.default_rng(6)
    lg = rays_of(log[:40000], tmax=np.where(np.isfinite(log[:40000, 10]), log[:40000, 10], 1.0) * 2 * g.random(
        min(40000, len(log))))
    k = WALKS[kernel]
    for set_name, rays in (("shadow", shadow), ("ao", ao), ("logged", lg)):
        tol = 1e-9 * np.maximum(1.0, rays["tmax"])
        fast = octx.occluded(rays, rtow.F64_FAST, k)
        strict = octx.occluded(rays, rtow.F64_STRICT, k)
        tf = octx.intersect(rays, rtow.F64_FAST, k)["t"]
        ts = octx.intersect(rays, rtow.F64_STRICT, k)["t"]
        # (the closest-hit query post-filters by tmax; with tmax = inf it gives the unfiltered t)
        inf_rays = rays.copy()
        inf_rays["tmax"] = math.inf
        tf_all = octx.intersect(inf_rays, rtow.F64_FAST, k)["t"]
        ts_all = octx.intersect(inf_rays, rtow.F64_STRICT, k)["t"]
        band_f = np.abs(tf_all - rays["tmax"]) <= tol
        band_s = np.abs(ts_all - rays["tmax"]) <= tol
        want_f = np.isfinite(tf) & (tf <= rays["tmax"])
        assert np.array_equal(fast[~band_f], want_f[~band_f]), (name, kernel, set_name)
        # against the strict build: outside the band, and where the two builds' closest hits agree on hit / miss (they
        # may not at a grazing hit, test_gpu_query.py::test_fast_agrees_with_strict: >= 99.99 % of the rays)
        split = np.isfinite(tf_all) != np.isfinite(ts_all)
        assert split.mean() <= 1e-4, (name, kernel, set_name, int(split.sum()))
        keep = ~band_s & ~split
        assert np.array_equal(fast[keep], strict[keep]), (name, kernel, set_name)
        assert np.array_equal(strict, np.isfinite(ts)), (name, kernel, set_name)
        assert band_s.mean() < 0.01 and band_f.mean() < 0.01, (name, kernel, set_name, band_s.mean())
        print(f"\n{name}/{kernel}/{set_name}: band {int(band_s.sum())} of {len(rays)}, split {int(split.sum())}, "
              f"fast != strict {int((fast != strict).sum())}")


# ------------------------------------------------------------------------------------------------ 5. contracts ---
def test_zero_rays_launch_nothing(octx, logged):
    import torch

    scene, view, log = logged["cover_static"]
    octx.upload(scene)
    d_out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda:0")
    st = octx.occluded_device(0, 0, d_out.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
    assert st.segments == 0 and st.prim_tests == 0 and st.node_tests == 0 and st.kernel_ms == 0.0
    assert np.all(d_out.cpu().numpy() == 0xAB)
    assert rtow.lib().rtow_occluded_device(octx._h, 0, 0, None, 0, None, None, None) == rtow.RTOW_OK
    occ = octx.occluded(np.empty(0, dtype=rtow.RAY_DTYPE), rtow.F64_STRICT)
    assert occ.shape == (0,)


def test_ragged_counts_match_one_batch_and_write_nothing_beyond(octx, logged):
    import torch

    scene, view, log = logged["cover_static"]
    octx.upload(scene)
    shadow, _ = shadow_and_ao_rays(view, log, 20000, seed=8)
    total = 64 * 211 + 1
    rays = np.concatenate([shadow] * (-(-total // len(shadow))))[:total]
    whole = octx.occluded(rays, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    for n in (1, 63, 64, 65, 64 * 211 + 1):
        pad = 192
        d_out = torch.full((1 + n + pad,), 0xAB, dtype=torch.uint8, device="cuda:0")
        st = octx.occluded_device(d_rays.data_ptr(), n, d_out.data_ptr() + 1, rtow.F64_STRICT, rtow.KERNEL_AUTO, 0,
                                  True)  # (an odd address: the result has no alignment)
        assert st.segments == n
        out = d_out.cpu().numpy()
        assert out[0] == 0xAB and np.all(out[1 + n:] == 0xAB), n
        assert set(np.unique(out[1:1 + n])) <= {0, 1}
        assert np.array_equal(out[1:1 + n].view(np.bool_), whole[:n]), n
    # a torch.bool tensor as the result
    b = torch.zeros(total, dtype=torch.bool, device="cuda:0")
    octx.occluded_device(d_rays.data_ptr(), total, b.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
    assert np.array_equal(b.cpu().numpy(), whole)


def test_side_stream_right_after_upload_on_a_fresh_context(logged):
    import torch

    scene, view, log = logged["suzanne"]
    shadow, _ = shadow_and_ao_rays(view, log, 50000, seed=9)
    ref_ctx = rtow.Context(0)
    try:
        ref_ctx.upload(scene)
        ref = ref_ctx.occluded(shadow, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    finally:
        ref_ctx.close()
    side = torch.cuda.Stream(device="cuda:0")
    d_rays = torch.from_numpy(shadow.view(np.uint8).copy()).to("cuda:0")
    d_out = torch.zeros(len(shadow), dtype=torch.bool, device="cuda:0")
    torch.cuda.synchronize()
    for builder in BUILDERS.values():
        c = rtow.Context(0)
        try:
            c.set_builder(builder)
            c.upload(scene)  # no wait: the query on the side stream must find the scene complete
            c.occluded_device(d_rays.data_ptr(), len(shadow), d_out.data_ptr(), rtow.F64_STRICT, rtow.KERNEL_AUTO,
                              side.cuda_stream, False)
            side.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), ref), builder
        finally:
            c.close()


def test_lean_upload_residency_and_argument_errors(logged):
    import torch

    scene, view, log = logged["cover_static"]
    shadow, _ = shadow_and_ao_rays(view, log, 1000, seed=10)
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.occluded(shadow, rtow.F64_STRICT)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(scene, cfg)  # lean upload: the grid only
        occ, st = c.occluded(shadow, rtow.F64_FAST, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and st.segments == len(shadow)
        with pytest.raises(rtow.RtowError) as q:
            c.occluded(shadow, rtow.F64_FAST, rtow.KERNEL_BVH)
        with pytest.raises(rtow.RtowError) as i:
            c.intersect(shadow, rtow.F64_FAST, rtow.KERNEL_BVH)
        assert "(-4)" in str(q.value) and str(q.value).split(": ", 1)[1] == str(i.value).split(": ", 1)[1]
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, 0), (0, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.occluded(shadow, prec, kern)
        L = rtow.lib()
        d_rays = torch.from_numpy(shadow.view(np.uint8).copy()).to("cuda:0")
        d_out = torch.zeros(len(shadow) + 16, dtype=torch.uint8, device="cuda:0")
        assert L.rtow_occluded_device(c._h, 1, 0, C.c_void_p(d_rays.data_ptr() + 8), 4, C.c_void_p(d_out.data_ptr()),
                                      None, None) == rtow.RTOW_EINVAL  # misaligned rays
        assert b"aligned" in L.rtow_last_error()
        for n, pr, po in ((-1, None, None), (1, None, None), ((1 << 31) - 63, 16, 16)):
            assert L.rtow_occluded_device(c._h, 0, 0, pr, n, po, None, None) == rtow.RTOW_EINVAL, n
        assert np.all(d_out.cpu().numpy() == 0)
    finally:
        c.close()


def test_two_calls_identical_and_kernel_used_follows_fallbacks(octx, logged):
    import torch

    scene, view, log = logged["cover_moving"]
    octx.upload(scene)
    shadow, ao = shadow_and_ao_rays(view, log, 30000, seed=12)
    rays = np.concatenate([shadow, ao])
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    a = torch.zeros(len(rays), dtype=torch.uint8, device="cuda:0")
    b = torch.full((len(rays),), 7, dtype=torch.uint8, device="cuda:0")
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        for k in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):
            octx.occluded_device(d_rays.data_ptr(), len(rays), a.data_ptr(), prec, k)
            st = octx.occluded_device(d_rays.data_ptr(), len(rays), b.data_ptr(), prec, k, 0, True)
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (prec, k)
            # the render's fallbacks: AUTO walks the grid on a sphere scene, BVH4 is for triangle meshes only
            want = {rtow.KERNEL_AUTO: rtow.KERNEL_GRID, rtow.KERNEL_BVH4: rtow.KERNEL_BVH}.get(k, k)
            assert st.kernel_used == want, (prec, k)
            assert st.node_tests > 0 and st.prim_tests > 0
    scene_h = handmade_scene()
    octx.upload(scene_h.c)
    _, st = octx.occluded(handmade_rays(), rtow.F64_STRICT, rtow.KERNEL_AUTO, want_stats=True)
    assert st.kernel_used == rtow.KERNEL_BRUTE and st.node_tests == 0 and st.prim_tests > 0


def test_occlusion_leaves_the_render_and_the_closest_hit_query_untouched(logged):
    """A render before and after ten occlusion calls: bit-identical, the profile ring counts render launches only; the
    closest-hit query gives the same bytes before and after."""
    import torch

    scene, view, log = logged["cover_moving"]
    shadow, ao = shadow_and_ao_rays(view, log, 50000, seed=13)
    c = rtow.Context(0)
    try:
        c.upload(scene)
        cfg = rtow.make_config(120, 80, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((80, 120, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        hits_before = c.intersect(shadow, rtow.F64_STRICT, rtow.KERNEL_BVH)
        assert c.profile_collect()[1] == 1
        for k in range(10):
            c.occluded(ao if k % 3 else shadow, rtow.F64_STRICT if k % 2 else rtow.F64_FAST,
                       [0, 1, 2, 3, 5][k % 5] if k % 2 else [0, 1, 2, 3][k % 4])
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
        assert c.intersect(shadow, rtow.F64_STRICT, rtow.KERNEL_BVH).tobytes() == hits_before.tobytes()
    finally:
        c.close()
