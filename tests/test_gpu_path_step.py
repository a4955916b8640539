"""Path-step queries (rtow_path_step / rtow_path_step_device) on the GPU.

The strict build is checked against the oracle's ray LOG: a single-threaded oracle render logs every segment of every
path (orc_set_raylog) with its exact origin, direction, shutter time and hit parameter.  Stepping the rows of segment b
with bounce = b and the identity (pixel, sample) must give the rows of segment b + 1 bit for bit, under every strategy and
either builder; stepping the primaries depth + 1 times in place and folding the attenuations on the host must give
rtow_radiance's per-ray colours and the oracle's image bit for bit.  The other tests pin the hit record against
rtow_intersect, the absorbed branch, the independence of the batch shape, the fast build's distance from the strict one
and the contracts.
"""
import ctypes as C
import math

import numpy as np
import pytest

import orc
import rtow
from support_fixtures import qctx  # noqa: F401
from support_oracle import (assert_hits_equal, expected_kernel, logged_render, primaries, rays_of, same_bits,
                            seeded_finite_tmax, sum_in_order)
from support_scenes import cover, cover_moving, random_scene, suzanne
from support_tables import BUILDERS, KERNELS

pytestmark = pytest.mark.gpu

MISS, SCATTERED, ABSORBED, SKIPPED = rtow.STEP_MISS, rtow.STEP_SCATTERED, rtow.STEP_ABSORBED, rtow.STEP_SKIPPED


# ------------------------------------------------------------------------------------------------- fixtures ---
RENDERS = {
    # name: (scene, width, height, spp, max_child_rays, seed) — the seeds of test_gpu_radiance.py
    "cover_d50": (cover, 48, 32, 4, 50, 21),
    "cover_d3": (cover, 48, 32, 4, 3, 21),
    "cover_moving_d50": (cover_moving, 48, 32, 4, 50, 22),
    "suzanne_d20": (suzanne, 48, 27, 4, 20, 23),
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
        # the log by segment: rows, and for every row the index of its path's next row in the next segment (or -1)
        seg = self.log[:, 2].astype(np.int64)
        assert seg.max() <= self.depth
        self.segments = []
        for b in range(int(seg.max()) + 1):
            rows = self.log[seg == b]
            nxt = self.log[seg == b + 1]
            key = rows[:, 0].astype(np.int64) * self.spp + rows[:, 1].astype(np.int64)
            nkey = nxt[:, 0].astype(np.int64) * self.spp + nxt[:, 1].astype(np.int64)
            assert len(np.unique(key)) == len(key)
            order = np.argsort(nkey)
            pos = np.searchsorted(nkey[order], key)
            pos = np.minimum(pos, max(len(nkey) - 1, 0))
            found = (nkey[order][pos] == key) if len(nkey) else np.zeros(len(key), dtype=bool)
            follow = np.where(found, order[pos] if len(nkey) else 0, -1)
            self.segments.append((rows, nxt, follow))

    def radiance(self, ctx, precision, kernel=rtow.KERNEL_AUTO):
        return ctx.radiance(self.rays, 1, self.depth, self.seed, self.ids, 0, precision, kernel)


@pytest.fixture(scope="module")
def logged():
    """name -> the four small oracle renders (computed once, never changed)."""
    return {name: Logged(name) for name in RENDERS}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def is_dead(nxt):
    """The dead ray: every field 0 and tmax = -1."""
    return ((nxt["origin"] == 0).all(axis=1) & (nxt["direction"] == 0).all(axis=1) & (nxt["time"] == 0)
            & (nxt["tmax"] == -1.0))


def sky_of(d):
    """The strict build's background for direction d, operation by operation in binary64."""
    dot = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    t = 0.5 * (d[:, 1] * (1.0 / np.sqrt(dot)) + 1.0)
    return np.stack([(1.0 - t) * 1.0 + t * k for k in (0.5, 0.7, 1.0)], axis=1)


def fold(status, atten):
    """The colour of every path from its per-bounce status and attenuation ([depth + 1, n] and [depth + 1, n, 3]):
    a_0 * (a_1 * (... * sky)) from the end; 0 for an absorbed path and for a hit at the last depth."""
    c = np.zeros(atten.shape[1:])
    for b in range(len(status) - 1, -1, -1):
        s = status[b][:, None]
        c = np.where(s == SCATTERED, atten[b] * c, np.where(s == MISS, atten[b], 0.0))
    return c


def chain(ctx, lg, precision, kernel=rtow.KERNEL_AUTO):
    """The primaries stepped depth + 1 times IN PLACE on the device: (status [depth + 1, n], atten [depth + 1, n, 3])."""
    import torch

    n, steps = len(lg.rays), lg.depth + 1
    d_rays = torch.from_numpy(lg.rays.view(np.uint8).copy()).to("cuda:0")
    d_ids = torch.from_numpy(lg.ids.view(np.int32).copy()).to("cuda:0")
    d_att = torch.full((steps, n, 3), -7.0, dtype=torch.float64, device="cuda:0")
    d_st = torch.full((steps, n), -7, dtype=torch.int32, device="cuda:0")
    for b in range(steps):
        ctx.path_step_device(d_rays.data_ptr(), n, d_ids.data_ptr(), d_rays.data_ptr(), d_att[b].data_ptr(),
                             d_st[b].data_ptr(), 0, b, lg.seed, 0, precision, kernel)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_att.cpu().numpy()


def same_step(a, b):
    """Two path_step results (status, next, atten, hits) with the same bits."""
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(a[:4], b[:4]))


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(RENDERS))
def test_every_logged_segment_strict(qctx, logged, name, kernel, builder):
    """1. The rows of segment b, stepped with bounce = b and their (pixel, sample): hit.t is the row's t_hit, the next
    ray is the path's row of segment b + 1 (origin, direction and time bit for bit, tmax = +inf), a hit the log does not
    continue is ABSORBED when child rays were left, a miss is MISS with a dead next ray."""
    lg = logged[name]
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(lg.scene)
        want = expected_kernel(lg.scene, KERNELS[kernel])
        n_scat = n_abs = 0
        for b, (rows, nxt_rows, follow) in enumerate(lg.segments):
            status, nxt, atten, hits, st = qctx.path_step(rays_of(rows), b, lg.seed, rows[:, 0:2].astype(np.uint32), 0,
                                                          rtow.F64_STRICT, KERNELS[kernel], want_stats=True)
            if want is not None:
                assert st.kernel_used == want
            assert st.segments == len(rows)
            assert np.array_equal(bits(hits["t"]), bits(rows[:, 10])), (b, "t_hit")
            missed = np.isinf(rows[:, 10])
            assert np.all(status[missed] == MISS), b
            assert np.all(is_dead(nxt[missed])), b
            cont = follow >= 0
            assert not np.any(cont & missed)
            assert np.all(status[cont] == SCATTERED), (b, np.unique(status[cont]))
            f = nxt_rows[follow[cont]]
            assert np.array_equal(bits(nxt["origin"][cont]), bits(f[:, 3:6])), (b, "origin")
            assert np.array_equal(bits(nxt["direction"][cont]), bits(f[:, 6:9])), (b, "direction")
            assert np.array_equal(bits(nxt["time"][cont]), bits(f[:, 9])), (b, "time")
            assert np.all(nxt["tmax"][cont] == math.inf), b
            ended = ~cont & ~missed
            if b < lg.depth:
                assert np.all(status[ended] == ABSORBED), b
                assert np.all(is_dead(nxt[ended])) and np.all(atten[ended] == 0.0), b
                n_abs += int(ended.sum())
            else:  # a hit with no child rays left: the caller's to paint black; the step scatters it like any other
                assert np.all((status[ended] == SCATTERED) | (status[ended] == ABSORBED)), b
            n_scat += int(cont.sum())
        print(f"{name} {kernel} {builder}: {len(lg.segments)} launches, {n_scat} scattered rows continued, {n_abs} absorbed")
        assert n_scat == len(lg.log) - len(lg.rays)
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)


@pytest.mark.parametrize("name", list(RENDERS))
def test_closure_with_radiance_strict(qctx, logged, name):
    """2. camera rays, then depth + 1 steps in place, folded on the host, IS rtow_radiance — per ray, bit for bit — and,
    summed per pixel in sample order, the oracle's image.  The depth-3 render ends paths on a hit with no child rays
    left."""
    lg = logged[name]
    qctx.upload(lg.scene)
    status, atten = chain(qctx, lg, rtow.F64_STRICT)
    assert np.all((status >= 0) & (status <= 3)) and np.all(atten >= 0.0)
    colour = fold(status, atten)
    last_hit = int(np.isin(status[lg.depth], (SCATTERED, ABSORBED)).sum())
    print(f"{name}: {last_hit} paths hit at bounce == depth; {int((status == ABSORBED).sum())} absorbed")
    if name == "cover_d3":
        assert last_hit > 0
    assert same_bits(colour, lg.radiance(qctx, rtow.F64_STRICT))
    assert same_bits(sum_in_order(colour, lg.spp), lg.image)


def _check_against_intersect(ctx, rays, kernel, seed=5):
    """Strict step against strict rtow_intersect on `rays` under `kernel`: hits, status classes, sky, dead rays."""
    hits_ref = ctx.intersect(rays, rtow.F64_STRICT, kernel)
    status, nxt, atten, hits = ctx.path_step(rays, 0, seed, None, 0, rtow.F64_STRICT, kernel)
    assert_hits_equal(hits, hits_ref, kernel)
    skipped = np.isnan(rays["tmax"]) | (rays["tmax"] < 0.001)
    missed = ~skipped & np.isinf(hits_ref["t"])
    hit = ~skipped & ~missed
    assert np.all(status[skipped] == SKIPPED) and np.all(status[missed] == MISS)
    assert np.all((status[hit] == SCATTERED) | (status[hit] == ABSORBED))
    assert np.all(np.isinf(hits["t"][skipped])) and np.all(hits["prim"][skipped] == -1)
    assert np.all(atten[skipped] == 0.0)
    assert same_bits(atten[missed], sky_of(rays["direction"][missed]))
    assert np.all(is_dead(nxt[skipped | missed]))
    sc = status == SCATTERED
    assert same_bits(nxt["origin"][sc], hits["point"][sc]) and same_bits(nxt["time"][sc], rays["time"][sc])
    assert np.all(nxt["tmax"][sc] == math.inf)
    # a dead ray fed back stays dead
    s2, n2, a2, h2 = ctx.path_step(nxt, 1, seed, None, 0, rtow.F64_STRICT, kernel)
    dead = ~sc
    assert np.all(s2[dead] == SKIPPED) and np.all(is_dead(n2[dead])) and np.all(a2[dead] == 0.0)
    assert np.all(np.isinf(h2["t"][dead]))
    # without hit records: the same other outputs
    s3, n3, a3, h3 = ctx.path_step(rays, 0, seed, None, 0, rtow.F64_STRICT, kernel, want_hits=False)
    assert h3 is None and same_step((s3, n3, a3, None), (status, nxt, atten, None))
    return status, skipped, missed


def test_hits_agree_with_intersect(logged):
    """3. Strict hits are strict rtow_intersect's on the first-segment rays and on rays with finite, tiny and NaN tmax;
    a miss is MISS with the strict radiance query's sky and a dead next ray; NaN or tmax < 0.001 is SKIPPED; once more
    after a refit, where the whole result equals a fresh upload's."""
    lg = logged["cover_moving_d50"]
    c, fresh = rtow.Context(0), rtow.Context(0)
    try:
        c.upload(lg.scene)
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH):
            status, skipped, missed = _check_against_intersect(c, lg.rays, kernel)
            assert not skipped.any() and missed.any() and (status == SCATTERED).any()
            # the sky is the one strict radiance adds (depth 0: a miss is the sky, a hit is black)
            sky = c.radiance(lg.rays, 1, 0, 5, None, 0, rtow.F64_STRICT, kernel)
            atten = c.path_step(lg.rays, 0, 5, None, 0, rtow.F64_STRICT, kernel)[2]
            assert same_bits(atten[missed], sky[missed]) and np.all(sky[~missed] == 0.0)
            finite = seeded_finite_tmax(lg.rays)
            status, skipped, missed = _check_against_intersect(c, finite, kernel)
            assert skipped[:2].all() and not skipped[2] and skipped.sum() > 10
            unbounded = np.isinf(c.intersect(lg.rays, rtow.F64_STRICT, kernel)["t"])
            assert (missed & ~unbounded).any()  # (hits beyond tmax reported as misses)

        sl = logged["suzanne_d20"]
        fresh.upload(sl.scene)
        _check_against_intersect(fresh, seeded_finite_tmax(sl.rays), rtow.KERNEL_AUTO)

        moved = cover_moving()
        sc = moved.c
        for i in range(1, sc.n_spheres):  # (sphere 0 is the ground)
            sc.sphere_geom[4 * i + 0] += 0.05 * ((i % 5) - 2)
            sc.sphere_geom[4 * i + 1] += 0.02 * (i % 3)
        for i in range(sc.n_moving):
            sc.moving_geom[8 * i + 1] += 0.03 * (i % 4)
            sc.moving_geom[8 * i + 4] += 0.03 * (i % 4) + 0.1
        before = c.path_step(lg.rays, 0, 5, None, 0, rtow.F64_STRICT)
        c.refit(moved)
        fresh.upload(moved)
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH):
            _check_against_intersect(c, seeded_finite_tmax(lg.rays), kernel)
            after = c.path_step(lg.rays, 0, 5, None, 0, rtow.F64_STRICT, kernel)
            assert same_step(after, fresh.path_step(lg.rays, 0, 5, None, 0, rtow.F64_STRICT, kernel)), kernel
            assert not same_step(after, before)
    finally:
        c.close()
        fresh.close()


def test_absorbed_is_reachable():
    """4. A Lambertian triangle whose e1 x e2 IS the ball point the bounce draws: normal - rnd is below 1e-8 in every
    component, scatter returns nothing, the step says ABSORBED with the hit filled, and strict radiance of the ray is 0."""
    L = orc.lib()
    seed, pixel, sample = 77, 1234, 2
    rnd = np.array([L.orc_philox_request(seed, pixel, sample, 1, 2, k) for k in range(3)])
    assert np.all(rnd >= 0.0) and np.linalg.norm(rnd) > 1e-2, rnd
    # e1 perpendicular to rnd, e2 = (rnd x e1) / |e1|^2: e1 x e2 = rnd
    e1 = np.cross(rnd, [0.0, 0.0, 1.0] if abs(rnd[2]) < 0.9 * np.linalg.norm(rnd) else [1.0, 0.0, 0.0])
    e2 = np.cross(rnd, e1) / np.dot(e1, e1)
    a = np.array([0.25, -0.5, 0.125])
    tri = np.concatenate([a, a + e1, a + e2])
    n = np.cross(tri[3:6] - tri[0:3], tri[6:9] - tri[0:3])
    assert np.abs(n - rnd).max() < 1e-12, (n, rnd)
    d = -rnd / np.dot(rnd, rnd)  # det = -d . n = 1 >= 1e-6: the side the cut accepts
    assert -np.dot(d, n) >= 1e-6
    centroid = (tri[0:3] + tri[3:6] + tri[6:9]) / 3.0
    ray = rtow.make_rays([centroid - d], [d], time=0.5)
    ids = np.array([[pixel, sample]], dtype=np.uint32)

    keep = []
    sc = random_scene(1, 0, 0, 1, keep)  # one triangle, Lambertian
    assert sc.n_prims == 1 and sc.n_triangles == 1
    keep[3][0, :] = tri

    ctx = rtow.Context(0)
    try:
        ctx.upload(sc)
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BRUTE, rtow.KERNEL_BVH):
            status, nxt, atten, hits = ctx.path_step(ray, 0, seed, ids, 0, rtow.F64_STRICT, kernel)
            assert status[0] == ABSORBED, (kernel, status)
            assert hits["prim"][0] == 0 and hits["kind"][0] == rtow.PRIM_TRIANGLE and abs(hits["t"][0] - 1.0) < 1e-9
            assert np.abs(hits["normal"][0] - rnd).max() < 1e-12
            assert np.all(atten == 0.0) and is_dead(nxt)[0]
            assert np.all(ctx.radiance(ray, 1, 50, seed, ids, 0, rtow.F64_STRICT, kernel) == 0.0)
            # (another sample of the same pixel draws another point: the same hit scatters)
            other = ctx.path_step(ray, 0, seed, ids, 1, rtow.F64_STRICT, kernel)
            assert other[0][0] == SCATTERED and same_bits(other[3], hits)
        assert ctx.path_step(ray, 0, seed, ids, 0, rtow.F64_FAST)[0][0] == ABSORBED
    finally:
        ctx.close()


def test_schedule_and_shape(qctx, logged):
    """5. n = 1, 63 and 65 equal the same rays inside the 6,144-ray batch in both builds; out of place equals in place;
    ids = None is (arange(n), 0); sample_first = s with ids (p, q) is ids (p, q + s), wrapping at 2^32; axis-parallel
    rays with -0.0 components: strict GRID equals strict BRUTE."""
    import torch

    lg = logged["cover_d50"]
    qctx.upload(lg.scene)
    n_all = len(lg.rays)
    assert n_all == 6144
    for prec in (rtow.F64_STRICT, rtow.F64_FAST):
        whole = qctx.path_step(lg.rays, 0, lg.seed, lg.ids, 0, prec)
        assert len(np.unique(whole[0])) >= 2
        for n in (1, 63, 65):
            part = qctx.path_step(lg.rays[100:100 + n], 0, lg.seed, lg.ids[100:100 + n], 0, prec)
            assert same_step(part, tuple(x[100:100 + n] for x in whole)), (n, prec)

        # the device form out of place and in place against the host form
        d_rays = torch.from_numpy(lg.rays.view(np.uint8).copy()).to("cuda:0")
        d_ids = torch.from_numpy(lg.ids.view(np.int32).copy()).to("cuda:0")
        d_next = torch.zeros_like(d_rays)
        d_att = torch.zeros((2, n_all, 3), dtype=torch.float64, device="cuda:0")
        d_st = torch.zeros((2, n_all), dtype=torch.int32, device="cuda:0")
        d_hits = torch.zeros((2, n_all * 72), dtype=torch.uint8, device="cuda:0")
        qctx.path_step_device(d_rays.data_ptr(), n_all, d_ids.data_ptr(), d_next.data_ptr(), d_att[0].data_ptr(),
                              d_st[0].data_ptr(), d_hits[0].data_ptr(), 0, lg.seed, 0, prec)
        qctx.path_step_device(d_rays.data_ptr(), n_all, d_ids.data_ptr(), d_rays.data_ptr(), d_att[1].data_ptr(),
                              d_st[1].data_ptr(), d_hits[1].data_ptr(), 0, lg.seed, 0, prec)
        torch.cuda.synchronize()
        for k, d_n in ((0, d_next), (1, d_rays)):
            got = (d_st[k].cpu().numpy(), d_n.cpu().numpy().view(rtow.RAY_DTYPE), d_att[k].cpu().numpy(),
                   d_hits[k].cpu().numpy().view(rtow.HIT_DTYPE))
            assert same_step(got, whole), (k, prec)

        rays = lg.rays[::len(lg.rays) // 257][:257]
        n = len(rays)
        arange = np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.uint32)
        assert same_step(qctx.path_step(rays, 2, lg.seed, None, 0, prec), qctx.path_step(rays, 2, lg.seed, arange, 0, prec))
        rng = np.random.default_rng(5)
        ids = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
        ids[0, 1] = 0xfffffffe  # the sample index wraps mod 2^32
        shifted = ids.copy()
        shifted[:, 1] += np.uint32(3)
        assert shifted[0, 1] == 1
        a = qctx.path_step(rays, 1, lg.seed, ids, 3, prec)
        assert same_step(a, qctx.path_step(rays, 1, lg.seed, shifted, 0, prec))
        assert not same_step(a, qctx.path_step(rays, 1, lg.seed, ids, 0, prec))  # (the identity matters)
        assert not same_step(a, qctx.path_step(rays, 2, lg.seed, ids, 3, prec))  # (and so does the bounce)

    u = np.linspace(-6.0, 6.0, 24)
    gx, gz = [a.ravel() for a in np.meshgrid(u, u)]
    down = rtow.make_rays(np.stack([gx, np.full_like(gx, 9.0), gz], axis=1), np.tile(-np.array([0.0, 1.0, 0.0]), (len(gx), 1)))
    along_z = rtow.make_rays(np.stack([u, np.full_like(u, 0.2), np.full_like(u, 14.0)], axis=1),
                             np.tile(-np.array([0.0, 0.0, 1.0]), (len(u), 1)))
    along_x = rtow.make_rays(np.stack([np.full_like(u, 14.0), np.full_like(u, 0.2), u], axis=1),
                             np.tile(-np.array([1.0, 0.0, 0.0]), (len(u), 1)))
    rays = np.concatenate([down, along_z, along_x])
    assert np.signbit(rays["direction"]).sum() == 3 * len(rays)  # every component carries a sign bit: -0.0 or -1.0
    grid = qctx.path_step(rays, 0, 7, None, 0, rtow.F64_STRICT, rtow.KERNEL_GRID, want_stats=True)
    assert grid[4].kernel_used == rtow.KERNEL_GRID
    assert same_step(grid, qctx.path_step(rays, 0, 7, None, 0, rtow.F64_STRICT, rtow.KERNEL_BRUTE))
    assert np.all(grid[0][:len(down)] != MISS)  # (the rays straight down all hit: the ground at least)


@pytest.mark.parametrize("name", DEEP)
def test_fast_against_strict(qctx, logged, name):
    """6. The thresholds of test_gpu_parity.py::test_fast_build_within_tolerance (test_gpu_radiance.py test 4).  On the
    logged first- and second-segment rays the status agrees on more than 97 % of the rays and, where both builds
    scatter, more than 97 % of the rays have next and atten isclose(rtol=1e-9, atol=1e-12); the fast chain against fast
    rtow_radiance: mean |difference| per ray <= 2e-3 and more than 97 % of the rays close.
    Measured on one MI355X: status agreement 1.0000 on both segments of all three renders; close
    fraction on segment 0 / 1: 0.9998 / 1.0000 (cover), 0.9994 / 1.0000 (moving cover), 1.0000 / 1.0000 (suzanne); chain
    against radiance: mean 2.7e-19 (cover), 1.8e-19 (moving cover), 0 (suzanne), close fraction 1.0000 on all three."""
    lg = logged[name]
    qctx.upload(lg.scene)
    for b in (0, 1):
        rows = lg.segments[b][0]
        rays, ids = rays_of(rows), rows[:, 0:2].astype(np.uint32)
        s_st, s_nx, s_at, _ = qctx.path_step(rays, b, lg.seed, ids, 0, rtow.F64_STRICT)
        f_st, f_nx, f_at, _ = qctx.path_step(rays, b, lg.seed, ids, 0, rtow.F64_FAST)
        agree = (s_st == f_st).mean()
        both = (s_st == SCATTERED) & (f_st == SCATTERED)
        close = np.ones(len(rays), dtype=bool)
        for f in ("origin", "direction", "time", "tmax"):
            x, y = s_nx[f][both].reshape(both.sum(), -1), f_nx[f][both].reshape(both.sum(), -1)
            close[both] &= np.isclose(y, x, rtol=1e-9, atol=1e-12).all(axis=1)
        close[both] &= np.isclose(f_at[both], s_at[both], rtol=1e-9, atol=1e-12).all(axis=1)
        frac = close[both].mean()
        print(f"{name} segment {b}: status agreement {agree:.4f}, close fraction {frac:.4f} of {int(both.sum())} rays")
        assert both.sum() > 100
        assert agree > 0.97, agree
        assert frac > 0.97, frac
        assert np.isfinite(f_at).all()
    status, atten = chain(qctx, lg, rtow.F64_FAST)
    colour = fold(status, atten)
    fast = lg.radiance(qctx, rtow.F64_FAST)
    mean = np.abs(colour - fast).mean()
    close = np.isclose(colour, fast, rtol=1e-9, atol=1e-12).all(axis=-1).mean()
    print(f"{name}: mean |chain - fast radiance| per ray {mean:.3e}, close fraction {close:.4f}")
    assert np.isfinite(colour).all()
    assert mean <= 2e-3
    assert close > 0.97, close


def test_contracts(logged):
    """7. Argument errors, RTOW_ENOSCENE without a scene, n = 0, guard words, stats; a render and a radiance query after
    the steps are bit-identical to ones before, and the profile ring sees the render's launches only."""
    import torch

    lg = logged["cover_moving_d50"]
    n = 1000
    rays, ids = lg.rays[:n], lg.ids[:n]
    L = rtow.lib()
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.path_step(rays, 0, 1, ids)
        c.upload(lg.scene)
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (rtow.F64_FAST, rtow.KERNEL_REFTREE), (7, 0), (0, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.path_step(rays, 0, 1, ids, 0, prec, kern)
        with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
            c.path_step(rays, -1, 1, ids)

        cfg = rtow.make_config(96, 64, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((64, 96, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(cfg, buf.data_ptr(), 0, True)
        image_before = buf.cpu().numpy().copy()
        assert c.profile_collect()[1] == 1
        radiance_before = lg.radiance(c, rtow.F64_STRICT)
        hits_before = c.intersect(lg.rays, rtow.F64_STRICT)

        guard = 64
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).to("cuda:0")
        d_next = torch.full((n * 8 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        d_att = torch.full((n * 3 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        d_st = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda:0")
        d_hits = torch.full((n * 9 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        prm = rtow.StepParams(lg.seed, 0, 0)

        def call(pr, count, pi, pn, pa, ps, ph, p=prm, prec=rtow.F64_STRICT):
            return L.rtow_path_step_device(c._h, prec, rtow.KERNEL_AUTO, C.byref(p) if p is not None else None, pr, count,
                                           pi, pn, pa, ps, ph, None, None)

        pr, pi, pn, pa, ps, ph = (t.data_ptr() for t in (d_rays, d_ids, d_next, d_att, d_st, d_hits))
        assert call(pr + 8, n, pi, pn, pa, ps, ph) == rtow.RTOW_EINVAL   # rays not 16-byte aligned
        assert call(pr, n, pi + 4, pn, pa, ps, ph) == rtow.RTOW_EINVAL   # ids not 8-byte aligned
        assert call(pr, n, pi, pn + 8, pa, ps, ph) == rtow.RTOW_EINVAL   # next not 16-byte aligned
        assert call(pr, n, pi, pn, pa + 4, ps, ph) == rtow.RTOW_EINVAL   # atten not 8-byte aligned
        assert call(pr, n, pi, pn, pa, ps + 2, ph) == rtow.RTOW_EINVAL   # status not 4-byte aligned
        assert call(pr, n, pi, pn, pa, ps, ph + 4) == rtow.RTOW_EINVAL   # hits not 8-byte aligned
        assert call(pr, n, pi, pn, pa, None, ph) == rtow.RTOW_EINVAL     # NULL status with n > 0
        assert call(pr, n, pi, None, pa, ps, ph) == rtow.RTOW_EINVAL     # NULL next
        assert call(pr, n, pi, pn, None, ps, ph) == rtow.RTOW_EINVAL     # NULL atten
        assert call(None, 1, None, pn, pa, ps, ph) == rtow.RTOW_EINVAL   # NULL rays
        assert call(pr, -1, pi, pn, pa, ps, ph) == rtow.RTOW_EINVAL
        assert call(pr, (1 << 31) - 63, pi, pn, pa, ps, ph) == rtow.RTOW_EINVAL
        assert call(pr, n, pi, pn, pa, ps, ph, None) == rtow.RTOW_EINVAL  # NULL params
        assert call(pr, n, pi, pn, pa, ps, ph, rtow.StepParams(lg.seed, -1, 0)) == rtow.RTOW_EINVAL  # bounce < 0
        assert call(pr, n, pi, pn, pa, ps, ph, prec=rtow.F32) == rtow.RTOW_EINVAL
        assert call(None, 0, None, None, None, None, None) == rtow.RTOW_OK  # n = 0: OK, no launch
        assert call(pr, 0, pi, pn, pa, ps, ph) == rtow.RTOW_OK
        torch.cuda.synchronize()
        for t in (d_next, d_att, d_st, d_hits):
            assert np.all(t.cpu().numpy() == -7)  # nothing was launched

        st = c.path_step_device(pr, n, pi, pn, pa, ps, ph, 0, lg.seed, 0, rtow.F64_STRICT, rtow.KERNEL_AUTO, 0, True)
        assert st.segments == n and st.kernel_used > 0 and st.prim_tests > 0 and st.kernel_ms > 0
        want = c.path_step(rays, 0, lg.seed, ids, 0, rtow.F64_STRICT)
        for t, count, ref in ((d_next, n * 8, want[1]), (d_att, n * 3, want[2]), (d_st, n, want[0]), (d_hits, n * 9, want[3])):
            out = t.cpu().numpy()
            assert np.all(out[count:] == -7)  # guard words
            assert np.array_equal(out[:count].view(np.uint8), np.ascontiguousarray(ref).view(np.uint8).reshape(-1))
        empty = c.path_step(rays[:0], 0, lg.seed, None)
        assert len(empty[0]) == 0 and len(empty[1]) == 0

        for k in range(6):  # steps in both builds and under every strategy, with and without hit records
            c.path_step(lg.rays, k, lg.seed, lg.ids, 0, rtow.F64_STRICT if k % 2 else rtow.F64_FAST,
                        [0, 1, 2, 3, 5][k % 5] if k % 2 else 0, want_hits=k < 3)
        assert c.profile_collect()[1] == 0
        assert same_bits(lg.radiance(c, rtow.F64_STRICT), radiance_before)
        assert same_bits(c.intersect(lg.rays, rtow.F64_STRICT), hits_before)
        buf.zero_()
        c.render_device(cfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), image_before)
    finally:
        c.close()
