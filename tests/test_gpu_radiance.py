"""Radiance queries (rtow_radiance / rtow_radiance_device) on the GPU.

The strict build is checked against the oracle IMAGE: a single-threaded oracle render logs every segment
(orc_set_raylog); its segment-0 rows are the W*H*spp primaries in pixel-major, sample-minor order with their exact origin,
direction and shutter time.  Queried with the identity (pixel, sample), the render's seed and depth, and added over the
samples of a pixel in order from zero, the per-ray results must equal orc.render's sums bit for bit — under every
strategy and either builder — and the device's segment counter must equal the log's length.  The other tests pin the
sample loop, the independence of the schedule, the fast build's distance from the strict one, -0.0 directions, refits
and the contracts.
"""
import ctypes as C

import numpy as np
import pytest

import rtow
from support_fixtures import qctx  # noqa: F401
from support_oracle import expected_kernel, logged_render, primaries, same_bits, sum_in_order
from support_scenes import cover, cover_moving, suzanne
from support_tables import KERNELS

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- fixtures ---
RENDERS = {
    # name: (scene, width, height, spp, max_child_rays, seed)
    "cover_d50": (cover, 48, 32, 4, 50, 21),
    "cover_d3": (cover, 48, 32, 4, 3, 21),
    "cover_moving_d50": (cover_moving, 48, 32, 4, 50, 22),
    "suzanne_d20": (suzanne, 48, 27, 4, 20, 23),
    "suzanne_d2": (suzanne, 48, 27, 4, 2, 23),
}
DEEP = ("cover_d50", "cover_moving_d50", "suzanne_d20")


class Logged:
    def __init__(self, name):
        mk, w, h, self.spp, self.depth, self.seed = RENDERS[name]
        self.scene = mk()
        cfg = rtow.make_config(w, h, self.spp, 1, self.depth, seed=self.seed, precision=rtow.F64_STRICT)
        self.image, self.log = logged_render(self.scene, cfg)
        self.rays, self.ids = primaries(self.log)
        assert len(self.rays) == w * h * self.spp
        # pixel-major, sample-minor
        assert np.array_equal(self.ids[:, 0], np.repeat(np.arange(w * h), self.spp))
        assert np.array_equal(self.ids[:, 1], np.tile(np.arange(self.spp), w * h))

    def query(self, ctx, precision, kernel=rtow.KERNEL_AUTO, **kw):
        return ctx.radiance(self.rays, 1, self.depth, self.seed, self.ids, 0, precision, kernel, **kw)


@pytest.fixture(scope="module")
def logged():
    """name -> the five small oracle renders (computed once, never changed)."""
    return {name: Logged(name) for name in RENDERS}


@pytest.fixture(scope="module")
def strict_cover(qctx, logged):
    """Strict and fast per-ray results of the 6,144 cover primaries in the module's context (uncapped launch)."""
    lg = logged["cover_d50"]
    qctx.set_builder(rtow.BUILDER_HOST_SAH)
    qctx.upload(lg.scene)
    return lg.query(qctx, rtow.F64_STRICT), lg.query(qctx, rtow.F64_FAST)


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("builder", [rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH], ids=["host", "device"])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(RENDERS))
def test_strict_equals_the_oracle_image(qctx, logged, name, kernel, builder):
    """1. The primaries of an oracle render, queried with their identities: the in-order sums equal the oracle's image
    bit for bit and the segment counter equals the log's length, under every strategy and either builder.  The depth-3
    and depth-2 renders end 348 and 186 paths on a hit with no child rays left; the depth-50 cover renders hold
    51-segment paths, glass (both faces, the hollow sphere) and metal."""
    lg = logged[name]
    qctx.set_builder(builder)
    try:
        qctx.upload(lg.scene)
        rgb, st = lg.query(qctx, rtow.F64_STRICT, KERNELS[kernel], want_stats=True)
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)
    want = expected_kernel(lg.scene, KERNELS[kernel])
    if want is not None:
        assert st.kernel_used == want
    got = sum_in_order(rgb, lg.spp)
    bad = int((got.view(np.uint64) != lg.image.view(np.uint64)).any(axis=1).sum())
    print(f"{name} {kernel}: {bad} of {len(got)} pixels differ; segments {st.segments} (log {len(lg.log)})")
    assert bad == 0
    assert st.segments == len(lg.log)
    assert st.samples == len(lg.rays) and st.local_rows == 0


@pytest.mark.parametrize("precision", [rtow.F64_STRICT, rtow.F64_FAST], ids=["strict", "fast"])
def test_many_samples_per_ray(qctx, logged, strict_cover, precision):
    """2. Five samples per ray = the in-order sum of five one-sample queries with the consecutive sample indices, bit for
    bit; ids = None is (arange(n), 0)."""
    lg = logged["cover_d50"]
    rays = lg.rays[::len(lg.rays) // 257][:257]
    n = len(rays)
    assert n == 257
    rng = np.random.default_rng(5)
    ids = np.stack([rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)],
                   axis=1).astype(np.uint32)
    ids[0, 1] = 0xfffffffe  # the sample index wraps mod 2^32
    five = qctx.radiance(rays, 5, lg.depth, lg.seed, ids, 3, precision)
    want = np.zeros((n, 3))
    for j in range(5):
        one_ids = ids.copy()
        one_ids[:, 1] += np.uint32(3 + j)
        want = want + qctx.radiance(rays, 1, lg.depth, lg.seed, one_ids, 0, precision)
    assert same_bits(five, want)
    assert np.isfinite(five).all() and (five > 0).any()
    no_ids = qctx.radiance(rays, 2, lg.depth, lg.seed, None, 0, precision)
    arange = np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.uint32)
    assert same_bits(no_ids, qctx.radiance(rays, 2, lg.depth, lg.seed, arange, 0, precision))


def test_result_does_not_depend_on_the_schedule(logged, strict_cover, monkeypatch):
    """3. One workgroup for 6,144 rays (every lane takes several items): bit-identical to the uncapped launch in both
    builds; two fast runs agree; n = 1, 63 and 65 equal the same rays inside the large batch."""
    lg = logged["cover_d50"]
    strict, fast = strict_cover
    monkeypatch.setenv("RTOW_RADIANCE_BLOCKS", "1")
    c = rtow.Context(0)
    try:
        c.upload(lg.scene)
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_BRUTE):
            assert same_bits(lg.query(c, rtow.F64_STRICT, kernel), strict), kernel
        f1, st = lg.query(c, rtow.F64_FAST, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID
        assert same_bits(f1, fast)
        assert same_bits(lg.query(c, rtow.F64_FAST), f1)
        for n in (1, 63, 65):
            for prec, whole in ((rtow.F64_STRICT, strict), (rtow.F64_FAST, fast)):
                part = c.radiance(lg.rays[100:100 + n], 1, lg.depth, lg.seed, lg.ids[100:100 + n], 0, prec)
                assert same_bits(part, whole[100:100 + n]), (n, prec)
    finally:
        c.close()


@pytest.mark.parametrize("name", DEEP)
def test_fast_against_strict(qctx, logged, name):
    """4. The thresholds of test_gpu_parity.py::test_fast_build_within_tolerance on the per-pixel sums of the same rays:
    finite, mean |fast - strict| per sample <= 2e-3, more than 97 % of the pixels isclose(rtol=1e-9, atol=1e-12).
    Measured on one MI355X: mean 1.5e-14 (cover), 1.1e-14 (moving cover), 9.0e-18 (suzanne); close
    fraction 1.0000 on all three."""
    lg = logged[name]
    qctx.upload(lg.scene)
    strict = sum_in_order(lg.query(qctx, rtow.F64_STRICT), lg.spp)
    fast = sum_in_order(lg.query(qctx, rtow.F64_FAST), lg.spp)
    mean = np.abs(fast - strict).mean() / lg.spp
    close = np.isclose(fast, strict, rtol=1e-9, atol=1e-12).all(axis=-1).mean()
    print(f"{name}: mean |fast - strict| per sample {mean:.3e}, close fraction {close:.4f}")
    assert np.isfinite(fast).all()
    assert mean <= 2e-3
    assert close > 0.97, close


def test_negative_zero_directions(qctx, logged):
    """5. Axis-parallel caller rays whose zero components are -0.0: strict GRID equals strict BRUTE bit for bit."""
    lg = logged["cover_d50"]
    qctx.upload(lg.scene)
    u = np.linspace(-6.0, 6.0, 24)
    gx, gz = [a.ravel() for a in np.meshgrid(u, u)]
    down = rtow.make_rays(np.stack([gx, np.full_like(gx, 9.0), gz], axis=1), np.tile(-np.array([0.0, 1.0, 0.0]), (len(gx), 1)))
    along_z = rtow.make_rays(np.stack([u, np.full_like(u, 0.2), np.full_like(u, 14.0)], axis=1),
                             np.tile(-np.array([0.0, 0.0, 1.0]), (len(u), 1)))
    along_x = rtow.make_rays(np.stack([np.full_like(u, 14.0), np.full_like(u, 0.2), u], axis=1),
                             np.tile(-np.array([1.0, 0.0, 0.0]), (len(u), 1)))
    rays = np.concatenate([down, along_z, along_x])
    assert np.signbit(rays["direction"]).sum() == 3 * len(rays)  # every component carries a sign bit: -0.0 or -1.0
    grid, st = qctx.radiance(rays, 2, 50, 7, None, 0, rtow.F64_STRICT, rtow.KERNEL_GRID, want_stats=True)
    assert st.kernel_used == rtow.KERNEL_GRID
    brute = qctx.radiance(rays, 2, 50, 7, None, 0, rtow.F64_STRICT, rtow.KERNEL_BRUTE)
    assert same_bits(grid, brute)
    assert st.samples == 2 * len(rays) and st.segments > st.samples  # (the rays straight down all hit: the ground at least)


def test_after_a_refit(logged):
    """6. The moving cover scene refitted with changed geometry: strict radiance on a fresh log of the new scene equals
    that oracle render."""
    lg = logged["cover_moving_d50"]
    moved = cover_moving()
    sc = moved.c
    for i in range(1, sc.n_spheres):  # (sphere 0 is the ground)
        sc.sphere_geom[4 * i + 0] += 0.05 * ((i % 5) - 2)
        sc.sphere_geom[4 * i + 1] += 0.02 * (i % 3)
    for i in range(sc.n_moving):
        sc.moving_geom[8 * i + 1] += 0.03 * (i % 4)
        sc.moving_geom[8 * i + 4] += 0.03 * (i % 4) + 0.1
    _, w, h, spp, depth, seed = RENDERS["cover_moving_d50"]
    cfg = rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=rtow.F64_STRICT)
    image, log = logged_render(moved, cfg)
    assert not same_bits(image, lg.image)
    rays, ids = primaries(log)
    c = rtow.Context(0)
    try:
        c.upload(lg.scene)
        c.refit(moved)
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH):
            rgb, st = c.radiance(rays, 1, depth, seed, ids, 0, rtow.F64_STRICT, kernel, want_stats=True)
            assert same_bits(sum_in_order(rgb, spp), image), kernel
            assert st.segments == len(log)
    finally:
        c.close()


def test_render_is_untouched_by_radiance_queries(logged):
    """7a. A strict render before and after a batch of radiance queries is bit-identical; the profile ring sees the
    render's launches only."""
    import torch

    lg = logged["cover_moving_d50"]
    c = rtow.Context(0)
    try:
        c.upload(lg.scene)
        cfg = rtow.make_config(96, 64, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((64, 96, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        assert c.profile_collect()[1] == 1
        for k in range(6):
            lg.query(c, rtow.F64_STRICT if k % 2 else rtow.F64_FAST, [0, 1, 2, 3, 5][k % 5] if k % 2 else 0)
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
    finally:
        c.close()


def test_side_stream_is_ordered_behind_the_upload(qctx, logged):
    """7b. On a torch side stream, right after an upload on a fresh context, the query finds the scene complete."""
    import torch

    lg = logged["suzanne_d20"]
    qctx.upload(lg.scene)
    ref = lg.query(qctx, rtow.F64_STRICT)
    side = torch.cuda.Stream(device="cuda:0")
    d_rays = torch.from_numpy(lg.rays.view(np.uint8).copy()).to("cuda:0")
    d_ids = torch.from_numpy(lg.ids.view(np.int32).copy()).to("cuda:0")
    d_rgb = torch.zeros((len(lg.rays), 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for builder in (rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH):
        c = rtow.Context(0)
        try:
            c.set_builder(builder)
            c.upload(lg.scene)  # no wait
            c.radiance_device(d_rays.data_ptr(), len(lg.rays), d_ids.data_ptr(), d_rgb.data_ptr(), 1, lg.depth, lg.seed, 0,
                              rtow.F64_STRICT, rtow.KERNEL_AUTO, side.cuda_stream, False)
            side.synchronize()
            assert same_bits(d_rgb.cpu().numpy(), ref), builder
        finally:
            c.close()


def test_errors_residency_and_bounds(logged):
    """7c. Argument errors, RTOW_ENOSCENE without a scene and after a lean upload, n = 0, guard words."""
    import torch

    lg = logged["cover_d50"]
    rays, ids = lg.rays[:1000], lg.ids[:1000]
    L = rtow.lib()
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.radiance(rays, 1, 50, 1, ids)
        cfg = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(lg.scene, cfg)  # lean upload: the grid only
        rgb, st = c.radiance(rays, 1, 50, lg.seed, ids, 0, rtow.F64_FAST, rtow.KERNEL_AUTO, want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and st.samples == len(rays) and np.isfinite(rgb).all()
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
            c.radiance(rays, 1, 50, 1, ids, 0, rtow.F64_FAST, rtow.KERNEL_BVH)
        c.upload(lg.scene)
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, 0), (0, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.radiance(rays, 1, 50, 1, ids, 0, prec, kern)
        with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
            c.radiance(rays, 0, 50, 1, ids)
        with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
            c.radiance(rays, 1, -1, 1, ids)

        n = 1000
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).to("cuda:0")
        guard = 64
        d_rgb = torch.full((n * 3 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        prm = rtow.RadianceParams(lg.seed, 1, lg.depth, 0, 0)

        def call(pr, count, pi, po, p=prm):
            return L.rtow_radiance_device(c._h, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(p) if p is not None else None,
                                          pr, count, pi, po, None, None)

        pr, pi, po = d_rays.data_ptr(), d_ids.data_ptr(), d_rgb.data_ptr()
        assert call(pr + 8, n, pi, po) == rtow.RTOW_EINVAL      # rays not 16-byte aligned
        assert call(pr, n, pi + 4, po) == rtow.RTOW_EINVAL      # ids not 8-byte aligned
        assert call(pr, n, pi, po + 4) == rtow.RTOW_EINVAL      # result not 8-byte aligned
        assert call(pr, -1, pi, po) == rtow.RTOW_EINVAL
        assert call(pr, (1 << 31) - 63, pi, po) == rtow.RTOW_EINVAL
        assert call(None, 1, None, po) == rtow.RTOW_EINVAL
        assert call(pr, 1, None, None) == rtow.RTOW_EINVAL
        assert call(pr, n, pi, po, None) == rtow.RTOW_EINVAL     # NULL params
        torch.cuda.synchronize()
        assert np.all(d_rgb.cpu().numpy() == -7.0)               # nothing was launched
        assert call(None, 0, None, None) == rtow.RTOW_OK         # n = 0: OK, no launch
        assert call(pr, 0, pi, po) == rtow.RTOW_OK
        torch.cuda.synchronize()
        assert np.all(d_rgb.cpu().numpy() == -7.0)

        st = c.radiance_device(pr, n, pi, po, 1, lg.depth, lg.seed, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
        out = d_rgb.cpu().numpy()
        assert np.all(out[n * 3:] == -7.0)                       # guard words
        assert same_bits(out[:n * 3].reshape(n, 3), lg.query(c, rtow.F64_STRICT)[:n])
        assert st.samples == n
    finally:
        c.close()
