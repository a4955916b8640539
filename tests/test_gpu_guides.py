"""The camera stage on the GPU: the primaries of the resident camera (rtow_camera_rays*) and the first-hit guide buffers
(rtow_guides*).

The oracle renders are logged with max_child_rays = 0 (orc_set_raylog): every log row is then a primary with its exact
origin, direction, shutter time, t_hit and class index, and the oracle's image is the sky summed over the misses.  The
strict primaries must equal the log bit for bit; the strict guides must equal, bit for bit, the numpy fold
(guides_ref.fold_guides: csrc/rtow_guides.h's written operand order) of pieces that are each pinned to the oracle — the
strict closest hits of the logged primaries (t and class index = the log's), their strict depth-0 radiance (summed = the
oracle's image) and the scene's material table.  The other tests pin the partition, the sample set, the closure
render == sum of radiance(camera_rays), schedule independence, the fast build's distance, refits and the contracts.
"""
import ctypes as C

import numpy as np
import pytest

import orc
import rtow
from guides_ref import (SCENES, Logged, attenuations, camera_ray_scales, fold_guides, guide_values, logged,  # noqa: F401
                        moved_cover, row_list)
from support_fixtures import qctx  # noqa: F401
from support_oracle import expected_kernel, same_bits, sum_in_order
from support_scenes import cover
from support_tables import BUILDERS, KERNELS

pytestmark = pytest.mark.gpu

# Fast camera rays against strict ones: |fast - strict| <= K_CAMERA * 2^-53 * S per component, S the sum of the absolute
# values of the component's terms (test_fast_camera_rays_against_strict).  Measured on one MI355X over the three scenes'
# primaries: max |fast - strict| / (2^-53 S) = 32.79 (origin), 2.47 (direction), 0 (time).  The origin's maximum is suzanne's
# y component: that camera's origin has y = 0, so the component is the lens offset alone and shows the fast build's lens
# sample as it is (second-order square root, 4e-15 relative, and the contracted sine polynomial); on the cover cameras the
# origin's own term dominates S and the ratio is 1.99.  Rounded up to a power of two, 64, times 4 for other cameras and
# image sizes.
K_CAMERA = 256.0


@pytest.fixture(scope="module")
def pieces(qctx, logged):
    """name -> (hits, sky, attenuations, expected guides): the pinned pieces of the fold and the fold itself, once."""
    out = {}
    qctx.set_builder(rtow.BUILDER_HOST_SAH)
    for name, lg in logged.items():
        qctx.upload(lg.scene)
        hits = qctx.intersect(lg.rays, rtow.F64_STRICT)
        sky = qctx.radiance(lg.rays, 1, 0, lg.seed, lg.ids, 0, rtow.F64_STRICT)
        att = attenuations(lg.scene)
        out[name] = (hits, sky, att, fold_guides(lg.rays, hits, sky, att, lg.spp))
    return out


def check_rays_against_log(rays, ids, lg, what):
    assert np.array_equal(ids, lg.ids), what
    for f in ("origin", "direction", "time"):
        assert same_bits(rays[f], lg.rays[f]), (what, f, int((rays[f] != lg.rays[f]).sum()))
    assert np.all(np.isposinf(rays["tmax"])), what


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(SCENES))
def test_primaries_equal_the_oracles(qctx, logged, name, builder):
    """1. Strict camera_rays: origin, direction and time carry the bits of the log's rows, matched by (pixel, sample);
    ids are the log's identities; tmax is +inf.  The cover scenes' origins vary with the lens sample, the moving
    cover's times with the shutter sample."""
    lg = logged[name]
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(lg.scene)
        rays, ids = qctx.camera_rays(lg.cfg)
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)
    check_rays_against_log(rays, ids, lg, name)
    if name != "suzanne":
        assert len(np.unique(rays["origin"][:, 0])) > len(rays) // 2  # a lens
    if name == "cover_moving":
        assert len(np.unique(rays["time"])) > len(rays) // 2          # a shutter


def test_primaries_of_an_image_smaller_than_a_wave(qctx):
    """1b. 5 x 3 pixels at 3 spp: 45 rays, fewer than one wave and no multiple of 64."""
    lg = Logged(cover, 5, 3, 3, 5)
    qctx.upload(lg.scene)
    rays, ids = qctx.camera_rays(lg.cfg)
    assert len(rays) == 45
    check_rays_against_log(rays, ids, lg, "5x3x3")
    g = qctx.guides(lg.cfg)
    assert g.shape == (3, 5) and np.isfinite(guide_values(g)).all()


def test_partition_and_sample_set(qctx, logged):
    """2. Three ranks with strips of 4 rows (H = 27), put together by rtow_local_row_list, equal the one-rank output:
    rays, ids and guides.  spp 5 over 2 streams traces samples 0..3; stream 1 of 2 traces samples 2, 3 with the bits of
    the full call's."""
    lg = logged["suzanne"]
    qctx.upload(lg.scene)
    rays, ids = qctx.camera_rays(lg.cfg)
    guides = qctx.guides(lg.cfg)
    rays3, ids3 = rays.reshape(lg.h, lg.w, lg.spp), ids.reshape(lg.h, lg.w, lg.spp, 2)
    seen = np.zeros(lg.h, dtype=int)
    for rank in range(3):
        cfg = lg.config(rank=rank, nranks=3, tile_rows=4)
        rows = row_list(cfg)
        seen[rows] += 1
        r, i = qctx.camera_rays(cfg)
        assert same_bits(r.reshape(len(rows), lg.w, lg.spp), rays3[rows]), rank
        assert np.array_equal(i.reshape(len(rows), lg.w, lg.spp, 2), ids3[rows]), rank
        g, st = qctx.guides(cfg, want_stats=True)
        assert g.shape == (len(rows), lg.w) and st.local_rows == len(rows)
        assert st.samples == st.segments == len(rows) * lg.w * lg.spp
        assert same_bits(g, guides[rows]), rank
    assert np.all(seen == 1)

    r5, i5 = qctx.camera_rays(lg.config(spp=5, nstreams=2))
    assert same_bits(r5, rays) and np.array_equal(i5, ids)  # samples 0..3
    assert same_bits(qctx.guides(lg.config(spp=5, nstreams=2)), guides)
    r1, i1 = qctx.camera_rays(lg.config(nstreams=2, stream_first=1, stream_count=1))
    assert same_bits(r1.reshape(lg.h, lg.w, 2), rays3[:, :, 2:]) and np.array_equal(i1.reshape(lg.h, lg.w, 2, 2), ids3[:, :, 2:])
    # the guides of the two halves are sums over disjoint samples: hits add up exactly (small integers)
    g0 = qctx.guides(lg.config(nstreams=2, stream_first=0, stream_count=1))
    g1 = qctx.guides(lg.config(nstreams=2, stream_first=1, stream_count=1))
    assert np.array_equal(g0["hits"] + g1["hits"], guides["hits"])


@pytest.mark.parametrize("name,depth", [("cover", 50), ("suzanne", 20)])
def test_render_is_the_sum_of_radiance_over_camera_rays(qctx, logged, name, depth):
    """3. Closure without the oracle: radiance(camera_rays(cfg), ids) added per pixel in sample order equals
    render_device(cfg) bit for bit (strict, one stream)."""
    import torch

    lg = logged[name]
    qctx.upload(lg.scene)
    cfg = rtow.make_config(lg.w, lg.h, lg.spp, 1, depth, seed=lg.seed, precision=rtow.F64_STRICT)
    buf = torch.zeros((lg.h, lg.w, 3), dtype=torch.float64, device="cuda:0")
    qctx.render_device(cfg, buf.data_ptr(), 0, True)
    image = buf.cpu().numpy().reshape(-1, 3)
    rays, ids = qctx.camera_rays(cfg)
    rgb = qctx.radiance(rays, 1, depth, lg.seed, ids, 0, rtow.F64_STRICT)
    assert same_bits(sum_in_order(rgb, lg.spp), image)
    assert np.isfinite(image).all() and (image > 0).any()


@pytest.mark.parametrize("name", list(SCENES))
def test_the_pieces_of_the_fold_are_pinned_to_the_oracle(logged, pieces, name):
    """4a. The strict hits of the logged primaries carry the log's t and class index; their depth-0 radiance, added per
    pixel, is the oracle's image (the sky over the misses)."""
    lg = logged[name]
    hits, sky, att, _ = pieces[name]
    assert same_bits(hits["t"], lg.log[:, 10])
    hit = np.isfinite(hits["t"])
    assert 0 < hit.sum() < len(hit)
    index = orc.scene_arrays(lg.scene.c)["prim_index"]
    assert np.array_equal(index[hits["prim"][hit]], lg.log[hit, 11].astype(np.int32))
    assert np.all(hits["prim"][~hit] == -1)
    assert same_bits(sum_in_order(sky, lg.spp), lg.image)
    assert np.all(sky[hit] == 0.0)
    assert att.min() >= 0.0 and att.max() <= 1.0


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(SCENES))
def test_strict_guides_equal_the_fold(qctx, logged, pieces, name, kernel, builder):
    """4b. All eight doubles of every pixel equal the numpy fold bit for bit, under every strategy and either builder;
    kernel_used follows the render's fallbacks; segments = pixels x spp."""
    lg = logged[name]
    want = pieces[name][3]
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(lg.scene)
        g, st = qctx.guides(lg.config(kernel=KERNELS[kernel]), want_stats=True)
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)
    used = expected_kernel(lg.scene, KERNELS[kernel])
    if used is not None:
        assert st.kernel_used == used
    got, exp = guide_values(g).reshape(-1, 8), guide_values(want)
    bad = (got.view(np.uint64) != exp.view(np.uint64))
    print(f"{name} {kernel} {builder}: {int(bad.any(axis=1).sum())} of {len(got)} pixels differ, per field {bad.sum(axis=0)}")
    assert not bad.any()
    assert st.segments == st.samples == lg.w * lg.h * lg.spp and st.local_rows == lg.h
    assert st.prim_tests > 0 and st.kernel_ms > 0
    # coverage and the unit normals: sane values
    cov = got[:, 7]
    assert cov.min() == 0 and cov.max() == lg.spp
    full = cov == lg.spp
    assert np.all(np.linalg.norm(got[full, 3:6], axis=1) <= lg.spp * (1 + 1e-12))


def test_result_does_not_depend_on_the_schedule(qctx, logged, monkeypatch):
    """5. One workgroup (RTOW_GUIDES_BLOCKS=1: every lane takes many pixels) gives the bits of the uncapped launch, in
    both builds.  (The rank split: test_partition_and_sample_set.)"""
    runs = [(name, prec, kern) for name in SCENES for prec in (rtow.F64_STRICT, rtow.F64_FAST)
            for kern in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_BRUTE)]
    free = {}
    for name in SCENES:
        qctx.upload(logged[name].scene)
        for n, prec, kern in runs:
            if n == name:
                free[(n, prec, kern)] = qctx.guides(logged[n].config(prec, kern), want_stats=True)
    monkeypatch.setenv("RTOW_GUIDES_BLOCKS", "1")
    c = rtow.Context(0)
    try:
        for name in SCENES:
            c.upload(logged[name].scene)
            for n, prec, kern in runs:
                if n == name:
                    g, st = c.guides(logged[n].config(prec, kern), want_stats=True)
                    assert st.kernel_used == free[(n, prec, kern)][1].kernel_used
                    assert same_bits(g, free[(n, prec, kern)][0]), (n, prec, kern)
    finally:
        c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_fast_guides_against_strict(qctx, logged, name):
    """6a. The thresholds of test_gpu_parity.py::test_fast_build_within_tolerance on the eight guide values (depth divided
    by the strict depth where the pixel has hits): finite, mean |fast - strict| per sample <= 2e-3, more than 97 % of the
    pixels isclose(rtol=1e-9, atol=1e-12) in all eight.  Measured on one MI355X: mean 5.5e-14 (cover),
    4.0e-14 (moving cover), 3.0e-17 (suzanne); close fraction 1.0000, 0.9993 (one pixel of 1,536) and 1.0000.
    Every pixel of the fast guides is held to its exact first hits in tests/test_gpu_exact_guides.py."""
    lg = logged[name]
    qctx.upload(lg.scene)
    strict =guide_values(qctx.guides(lg.config(rtow.F64_STRICT))).reshape(-1, 8).copy()
    fast = guide_values(qctx.guides(lg.config(rtow.F64_FAST))).reshape(-1, 8).copy()
    assert np.isfinite(fast).all() and np.isfinite(strict).all()
    scale = np.where(strict[:, 7] > 0, strict[:, 6], 1.0)
    assert np.all(scale > 0)
    fast[:, 6] /= scale
    strict[:, 6] /= scale
    mean = np.abs(fast - strict).mean() / lg.spp
    close = np.isclose(fast, strict, rtol=1e-9, atol=1e-12).all(axis=-1).mean()
    print(f"{name}: guides mean |fast - strict| per sample {mean:.3e}, close fraction {close:.4f}")
    assert mean <= 2e-3
    assert close > 0.97, close


def test_fast_camera_rays_against_strict(qctx, logged):
    """6b. |fast - strict| <= K_CAMERA 2^-53 S per component over the three scenes' primaries (K_CAMERA above)."""
    u = 2.0 ** -53
    worst = {"origin": 0.0, "direction": 0.0, "time": 0.0}
    for name, lg in logged.items():
        qctx.upload(lg.scene)
        strict, ids = qctx.camera_rays(lg.cfg)
        fast, fids = qctx.camera_rays(lg.config(rtow.F64_FAST))
        assert np.array_equal(ids, fids) and np.all(np.isposinf(fast["tmax"]))
        s_org, s_dir, s_time = camera_ray_scales(lg.scene, strict)
        for f, s in (("origin", s_org), ("direction", s_dir), ("time", s_time)):
            err = np.abs(fast[f] - strict[f])
            assert np.all(err[s == 0] == 0), (name, f)
            ratio = float((err[s > 0] / (u * s[s > 0])).max()) if (s > 0).any() else 0.0
            print(f"{name} {f}: max |fast - strict| / (2^-53 S) = {ratio:.3f}")
            worst[f] = max(worst[f], ratio)
    print("worst:", worst)
    for f, r in worst.items():
        assert r <= K_CAMERA, (f, r)


def test_after_a_refit(logged):
    """7. The camera and the spheres moved with Context.refit: strict camera_rays and guides equal those of a fresh
    context that uploaded the moved scene, and differ from the unmoved scene's."""
    lg = logged["cover_moving"]
    moved = moved_cover()
    a, b = rtow.Context(0), rtow.Context(0)
    try:
        a.upload(lg.scene)
        r0, _ = a.camera_rays(lg.cfg)
        g0 = a.guides(lg.cfg)
        a.refit(moved)
        b.upload(moved)
        ra, ia = a.camera_rays(lg.cfg)
        rb, ib = b.camera_rays(lg.cfg)
        assert same_bits(ra, rb) and np.array_equal(ia, ib)
        assert not same_bits(ra["origin"], r0["origin"])
        for kernel in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_BRUTE):
            ga, gb = a.guides(lg.config(kernel=kernel)), b.guides(lg.config(kernel=kernel))
            assert same_bits(ga, gb), kernel
            assert not same_bits(ga, g0)
    finally:
        a.close()
        b.close()


def test_contracts(logged):
    """8. Refused arguments, RTOW_ENOSCENE without a scene and after a lean upload (guides only), alignment, guard words,
    and a render that neither call disturbs."""
    import torch

    lg = logged["cover"]
    L = rtow.lib()
    c = rtow.Context(0)
    try:
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):  # no scene yet
            c.camera_rays(lg.cfg)
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
            c.guides(lg.cfg)
        lean = rtow.make_config(60, 40, 2, 1, 10, seed=3, precision=rtow.F64_FAST)
        c.render(lg.scene, lean)  # lean upload: the grid only
        g, st = c.guides(lg.config(rtow.F64_FAST), want_stats=True)
        assert st.kernel_used == rtow.KERNEL_GRID and np.isfinite(guide_values(g)).all()
        with pytest.raises(rtow.RtowError, match=r"\(-4\)"):
            c.guides(lg.config(rtow.F64_FAST, rtow.KERNEL_BVH))
        rays, ids = c.camera_rays(lg.config(rtow.F64_STRICT, rtow.KERNEL_BVH))  # needs no walk: fine after a lean upload
        assert same_bits(rays["direction"], lg.rays["direction"]) and np.array_equal(ids, lg.ids)

        c.upload(lg.scene)
        for prec, kern in ((rtow.F32, rtow.KERNEL_AUTO), (7, 0), (rtow.F64_STRICT, 9)):
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.camera_rays(lg.config(prec, kern))
            with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
                c.guides(lg.config(prec, kern))
        with pytest.raises(rtow.RtowError, match=r"\(-1\)"):
            c.guides(lg.config(rtow.F64_FAST, rtow.KERNEL_REFTREE))
        c.camera_rays(lg.config(rtow.F64_FAST, rtow.KERNEL_REFTREE))  # the kernel is not read beyond its range

        n, npix, guard = len(lg.rays), lg.w * lg.h, 64
        d_rays = torch.full((n * 8 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        d_ids = torch.full((n * 2 + guard,), -7, dtype=torch.int32, device="cuda:0")
        d_g = torch.full((npix * 8 + guard,), -7.0, dtype=torch.float64, device="cuda:0")
        pr, pi, pg = d_rays.data_ptr(), d_ids.data_ptr(), d_g.data_ptr()
        cfg = C.byref(lg.cfg)
        assert L.rtow_camera_rays_device(c._h, cfg, pr + 8, pi, None) == rtow.RTOW_EINVAL   # rays not 16-byte aligned
        assert L.rtow_camera_rays_device(c._h, cfg, pr, pi + 4, None) == rtow.RTOW_EINVAL   # ids not 8-byte aligned
        assert L.rtow_guides_device(c._h, cfg, pg + 8, None, None) == rtow.RTOW_EINVAL      # guides not 16-byte aligned
        assert L.rtow_camera_rays_device(c._h, cfg, None, pi, None) == rtow.RTOW_EINVAL
        assert L.rtow_guides_device(c._h, cfg, None, None, None) == rtow.RTOW_EINVAL
        assert L.rtow_camera_rays_device(c._h, None, pr, pi, None) == rtow.RTOW_EINVAL      # NULL cfg
        assert L.rtow_guides_device(c._h, None, pg, None, None) == rtow.RTOW_EINVAL
        none = lg.config(spp=1, nstreams=2)                                                  # no effective samples
        assert L.rtow_camera_rays_device(c._h, C.byref(none), None, None, None) == rtow.RTOW_OK
        torch.cuda.synchronize()
        assert np.all(d_rays.cpu().numpy() == -7.0) and np.all(d_ids.cpu().numpy() == -7) and np.all(d_g.cpu().numpy() == -7.0)

        c.profile_collect()  # (empties the ring: the lean upload above rendered once)
        # a strict render before ...
        rcfg = rtow.make_config(96, 64, 4, 2, 50, seed=9, precision=rtow.F64_STRICT)
        buf = torch.zeros((64, 96, 3), dtype=torch.float64, device="cuda:0")
        c.render_device(rcfg, buf.data_ptr(), 0, True)
        before = buf.cpu().numpy().copy()
        assert c.profile_collect()[1] == 1
        # ... a batch of both calls, on device buffers with guard words behind them ...
        c.camera_rays_device(lg.cfg, pr, 0)                  # NULL ids: no id is written
        torch.cuda.synchronize()
        assert np.all(d_ids.cpu().numpy() == -7)
        c.camera_rays_device(lg.cfg, pr, pi)
        st = c.guides_device(lg.cfg, pg, 0, True)
        for k in range(4):
            c.guides(lg.config(rtow.F64_FAST if k % 2 else rtow.F64_STRICT, [0, 1, 2, 3][k]))
            c.camera_rays(lg.config(rtow.F64_FAST if k % 2 else rtow.F64_STRICT))
        rays_out, ids_out, g_out = d_rays.cpu().numpy(), d_ids.cpu().numpy(), d_g.cpu().numpy()
        assert np.all(rays_out[n * 8:] == -7.0) and np.all(ids_out[n * 2:] == -7) and np.all(g_out[npix * 8:] == -7.0)
        assert same_bits(rays_out[:n * 8].reshape(n, 8)[:, [0, 1, 2]], lg.rays["origin"])
        assert same_bits(rays_out[:n * 8].reshape(n, 8)[:, [4, 5, 6]], lg.rays["direction"])
        assert np.array_equal(ids_out[:n * 2].reshape(n, 2).astype(np.uint32), lg.ids)
        assert same_bits(g_out[:npix * 8].reshape(lg.h, lg.w, 8), guide_values(c.guides(lg.cfg)))
        assert st.samples == n and st.local_rows == lg.h
        # ... and after: the same bits, and the profile ring saw the renders only
        assert c.profile_collect()[1] == 0
        buf.zero_()
        c.render_device(rcfg, buf.data_ptr(), 0, True)
        assert c.profile_collect()[1] == 1
        assert np.array_equal(buf.cpu().numpy(), before)
    finally:
        c.close()
