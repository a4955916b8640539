"""In-place refit of the resident scene (rtow_scene_refit / rtow_refit_info) on the GPU.

The refit keeps the trees' topology and recomputes everything derived from geometry on the device, by the host builder's
own rules.  So: an unchanged refit after a host-builder upload leaves every image byte-identical; a deformed refit passes
the ray-independent image checker (tests/accel_images.py) against the NEW geometry; in the strict build renders equal the
oracle's render of the new scene and queries equal those after a fresh upload of it, bit for bit, under every strategy;
grid presence follows the new scene; and the API contracts (shape checks, residency, ordering) hold.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import accel_images as ai
import orc
import rtow
from support_fixtures import fresh, rctx  # noqa: F401
from support_oracle import assert_hits_equal, block_means
from support_scenes import (SMALL, _copy, _set_order, motions, rays_for, resident_images, scene_of, wave,
                            write_mesh_obj)
from support_tables import BUILDERS, KERNELS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh96k(tmp_path_factory):
    hs = rtow.HostScene.obj(write_mesh_obj(tmp_path_factory.mktemp("mesh")), 16 / 9)
    G = ai.Geometry.of_scene(hs.c)
    hs.close()
    assert G.nt == 96800
    return G


def frame_of(ctx, cfg, stream=0):
    rows = rtow.lib().rtow_local_rows(C.byref(cfg))
    buf = torch.zeros((rows, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    ctx.render_device(cfg, buf.data_ptr(), stream, False)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


# ------------------------------------------------------------------------------- 1. unchanged refit, host builder ---
@pytest.mark.parametrize("name", list(SMALL) + ["mesh96k"])
def test_unchanged_refit_is_byte_identical_host_builder(rctx, mesh96k, name):
    G = mesh96k if name == "mesh96k" else SMALL[name]
    keep = []
    sc = scene_of(_copy(G), keep)
    rctx.set_builder(rtow.BUILDER_HOST_SAH)
    rctx.upload(sc)
    before = resident_images(rctx)
    assert rctx.refit_info().refits == 0 and rctx.refit_info().bvh_area_ratio == 1.0
    rctx.refit(sc)
    after = resident_images(rctx)
    for w in range(6):
        assert after[w] == before[w], (name, w, len(before[w]), len(after[w]))
    ri = rctx.refit_info()
    assert ri.refits == 1 and ri.bvh_area_ratio == 1.0
    assert ri.grid_resident == (len(after[1]) > 0)
    assert ri.refit_ms > 0 and ri.device_ms > 0


# -------------------------------------------------------------------------- 2. deformed refits pass the checker ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(SMALL) + ["mesh96k"])
def test_deformed_refit_images_enclose_the_new_geometry(rctx, mesh96k, name, builder):
    G = mesh96k if name == "mesh96k" else SMALL[name]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    todo = motions(G)
    if name == "mesh96k":
        todo = {k: todo[k] for k in ("translate", "jitter", "scale1000", "flatten")}
    for mname, (H, shift) in todo.items():
        rctx.upload(scene_of(_copy(G), keep))
        rctx.refit(scene_of(H, keep, cam_shift=shift))
        try:
            ai.check_resident(resident_images(rctx), H)
        except AssertionError as e:
            raise AssertionError(f"{name} / {mname}: {e}") from None
    assert rctx.refit_info().refits == 1


# ----------------------------------------------------------------------------------------- 3. strict renders ---
RENDER_SCENES = ["cover_moving", "suzanne", "sph_far_moving", "edge_n17"]
RENDER_KERNELS = dict(KERNELS, auto=rtow.KERNEL_AUTO)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", RENDER_SCENES)
def test_strict_render_after_refit_equals_the_oracle(rctx, name, builder):
    G = SMALL[name]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    todo = motions(G)
    cases = [("translate", todo["translate"][0], None, None), ("jitter", todo["jitter"][0], None, None),
             ("camera_shutter", todo["camera"][0], todo["camera"][1], (0.2, 0.7))]
    if "moving_c1" in todo:
        cases.append(("moving_c1", todo["moving_c1"][0], None, None))
    for mname, H, shift, shutter in cases:
        B = scene_of(H, keep, cam_shift=shift, shutter=shutter)
        cfg = rtow.make_config(40, 26, 2, 1, 8, seed=3, precision=rtow.F64_STRICT)
        ref, _ = orc.render(B, cfg, orc.RNG_PHILOX, nthreads=4)
        rctx.upload(scene_of(_copy(G), keep))
        rctx.refit(B)
        for kn, k in RENDER_KERNELS.items():
            cfg.kernel = k
            got = frame_of(rctx, cfg)
            assert np.array_equal(got, ref), (name, mname, kn, int((got != ref).sum()))


# ----------------------------------------------------------------------------------------- 4. strict queries ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["cover_moving", "suzanne", "suz1400", "edge_coincident", "sph_negative_radius",
                                  "mesh96k"])
def test_strict_queries_after_refit_equal_a_fresh_upload(rctx, fresh, mesh96k, name, builder):
    G = mesh96k if name == "mesh96k" else SMALL[name]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    fresh.set_builder(BUILDERS[builder])
    todo = motions(G)
    kernels = KERNELS if name != "mesh96k" else {k: KERNELS[k] for k in ("bvh", "grid", "bvh4")}
    for mname in ("rotate", "jitter", "camera"):
        H, shift = todo[mname]
        B = scene_of(H, keep, cam_shift=shift)
        rctx.upload(scene_of(_copy(G), keep))
        rctx.refit(B)
        fresh.upload(B)
        rays = rays_for(H, 4000 if name == "mesh96k" else 3000, seed=7)
        for kn, k in kernels.items():
            a, sa = rctx.intersect(rays, rtow.F64_STRICT, k, want_stats=True)
            b, sb = fresh.intersect(rays, rtow.F64_STRICT, k, want_stats=True)
            assert sa.kernel_used == sb.kernel_used, (name, mname, kn)
            assert_hits_equal(a, b, (name, mname, kn))
            oa = rctx.occluded(rays, rtow.F64_STRICT, k)
            ob = fresh.occluded(rays, rtow.F64_STRICT, k)
            assert np.array_equal(oa, ob), (name, mname, kn, int((oa != ob).sum()))
            assert np.isfinite(a["t"]).any()


# -------------------------------------------------------------------------------------------- 5. identifiers ---
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_duplicated_triangles_separated_by_the_refit_keep_their_ids(rctx, fresh, builder):
    base = ai.unit_mesh(300, 4)
    tris = np.concatenate([base, base[:80]])  # 80 exact duplicates at upload
    G = ai.mesh_geometry(tris, cam=(0.5, 0.5, -3.0))
    moved = tris.copy()
    moved[300:] += np.array([0.0, 0.0, -0.6])  # the second copies move toward the camera
    H = ai.mesh_geometry(moved, cam=(0.5, 0.5, -3.0))
    keep = []
    rctx.set_builder(BUILDERS[builder])
    fresh.set_builder(BUILDERS[builder])
    rctx.upload(scene_of(G, keep))
    rctx.intersect(rays_for(G, 10, 1), rtow.F64_STRICT, rtow.KERNEL_BVH4)  # (an id table of the upload exists)
    B = scene_of(H, keep)
    rctx.refit(B)
    fresh.upload(B)
    ctr = moved[300:].mean(axis=1)
    o = np.repeat(np.array([[0.5, 0.5, -3.0]]), len(ctr), 0)
    rays = np.concatenate([rtow.make_rays(o, ctr - o), rays_for(H, 2000, 3)])
    for kn, k in KERNELS.items():
        a = rctx.intersect(rays, rtow.F64_STRICT, k)
        b = fresh.intersect(rays, rtow.F64_STRICT, k)
        assert_hits_equal(a, b, (builder, kn))
        assert (a["prim"][:80] >= 300).sum() >= 30, kn  # the moved copies are what the centre rays hit


def _permuted_scene(G, keep, perm):
    return _set_order(scene_of(G, keep), G, keep, perm)


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_permuted_insertion_order_ids_equal_a_fresh_upload(rctx, fresh, builder):
    sp = SMALL["sph_same_centre"]
    tri = ai.unit_mesh(120, 9) * 2.0 - 1.0
    G = ai.Geometry(sp.sph, np.zeros((0, 8)), tri.reshape(-1, 9), np.zeros(sp.ns + len(tri), np.int32), sp.mats, sp.cam)
    perm = np.random.default_rng(2).permutation(G.np)
    H, _ = motions(G)["jitter"]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    fresh.set_builder(BUILDERS[builder])
    rctx.upload(_permuted_scene(G, keep, perm))
    B = _permuted_scene(H, keep, perm)
    rctx.refit(B)
    fresh.upload(B)
    rays = rays_for(H, 3000, 5)
    for kn, k in KERNELS.items():
        assert_hits_equal(rctx.intersect(rays, rtow.F64_STRICT, k), fresh.intersect(rays, rtow.F64_STRICT, k), (kn,))
    # a different permutation is another insertion order: refused
    with pytest.raises(rtow.RtowError, match="insertion order"):
        rctx.refit(_permuted_scene(H, keep, np.roll(perm, 1)))


# ------------------------------------------------------------------------------------------ 6. grid presence ---
def _grid_cases():
    g = np.random.default_rng(21)
    spread = np.c_[g.uniform(-4, 4, size=(300, 3)) * [1, 0.3, 1], np.full(300, 0.05)]
    crowded = spread.copy()
    crowded[:, 0:3] = crowded[:, 0:3] * 1e-4 + np.array([0.5, 0.2, -0.3])  # 300 spheres in one cell: lists > 255
    big = spread.copy()
    big[:70, 3] = 3.0  # 70 large spheres (against the median diagonal): more than 64
    return {"crowd": (ai.sphere_geometry(spread), ai.sphere_geometry(crowded)),
            "enlarge": (ai.sphere_geometry(spread), ai.sphere_geometry(big))}


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("case", ["crowd", "enlarge"])
def test_grid_presence_follows_the_new_scene(rctx, fresh, case, builder):
    A, B = _grid_cases()[case]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    fresh.set_builder(BUILDERS[builder])
    for src, dst in ((A, B), (B, A)):  # grid lost, then grid regained
        rctx.upload(scene_of(_copy(src), keep))
        had = len(rctx.debug_image(1)) > 0
        sc = scene_of(_copy(dst), keep)
        rctx.refit(sc)
        fresh.upload(sc)
        imgs, ref = resident_images(rctx), resident_images(fresh)
        assert (len(imgs[1]) > 0) == (len(ref[1]) > 0) and had != (len(imgs[1]) > 0), (case, had)
        assert rctx.refit_info().grid_resident == (len(imgs[1]) > 0)
        assert imgs[1] == ref[1] and imgs[3] == ref[3]
        ai.check_resident(imgs, dst)
        rays = rays_for(dst, 500, 1)
        for k in (rtow.KERNEL_AUTO, rtow.KERNEL_GRID):
            a, sa = rctx.intersect(rays, rtow.F64_STRICT, k, want_stats=True)
            b, sb = fresh.intersect(rays, rtow.F64_STRICT, k, want_stats=True)
            assert sa.kernel_used == sb.kernel_used
            assert_hits_equal(a, b, (case, k))


# --------------------------------------------------------------------------------------------- 7. contracts ---
def test_shape_mismatch_is_einval_and_leaves_the_scene(rctx):
    G = SMALL["cover_moving"]
    keep = []
    rctx.set_builder(rtow.BUILDER_HOST_SAH)
    rctx.upload(scene_of(_copy(G), keep))
    cfg = rtow.make_config(32, 20, 2, 1, 6, seed=4, precision=rtow.F64_STRICT)
    before = frame_of(rctx, cfg)
    fewer = ai.Geometry(G.sph[:-1], G.mov, G.tri, G.pmat[1:], G.mats, G.cam)
    more_mats = ai.Geometry(G.sph, G.mov, G.tri, G.pmat, list(G.mats) + [ai.LAMBERTIAN_GREY], G.cam)
    unordered = scene_of(motions(G)["translate"][0], keep)
    unordered.prim_kind, unordered.prim_index = None, None
    bad = {"count": scene_of(fewer, keep), "materials": scene_of(more_mats, keep), "order": unordered}
    L = rtow.lib()
    for what, sc in bad.items():
        rc = L.rtow_scene_refit(rctx._h, C.byref(sc))
        assert rc == rtow.RTOW_EINVAL, what
        assert L.rtow_last_error(), what
        assert np.array_equal(frame_of(rctx, cfg), before), what
    assert L.rtow_scene_refit(rctx._h, None) == rtow.RTOW_EINVAL
    assert b"NULL" in L.rtow_last_error()
    assert rctx.refit_info().refits == 0


def test_without_a_scene_is_enoscene():
    c = rtow.Context(0)
    try:
        keep = []
        L = rtow.lib()
        assert L.rtow_scene_refit(c._h, C.byref(scene_of(_copy(SMALL["suzanne"]), keep))) == rtow.RTOW_ENOSCENE
        assert L.rtow_refit_info(c._h, C.byref(rtow.RefitInfo())) == rtow.RTOW_ENOSCENE
    finally:
        c.close()


@pytest.mark.parametrize("name,kernel,other", [("cover_moving", rtow.KERNEL_GRID, rtow.KERNEL_BVH),
                                               ("suzanne", rtow.KERNEL_BVH4, rtow.KERNEL_BVH)])
def test_lean_render_upload_refits_what_it_built(name, kernel, other):
    G = SMALL[name]
    H, _ = motions(G)["jitter"]
    keep = []
    c = rtow.Context(0)
    try:
        cfg = rtow.make_config(40, 26, 2, 1, 8, seed=6, precision=rtow.F64_STRICT, kernel=kernel)
        c.render(scene_of(_copy(G), keep), cfg)  # the lean upload: what this kernel reads
        B = scene_of(H, keep)
        c.refit(B)
        ref, _ = orc.render(B, cfg, orc.RNG_PHILOX, nthreads=4)
        assert np.array_equal(frame_of(c, cfg), ref)
        cfg.kernel = other
        with pytest.raises(rtow.RtowError) as e:
            frame_of(c, cfg)
        assert f"({rtow.RTOW_ENOSCENE})" in str(e.value)
    finally:
        c.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_render_on_a_nonblocking_stream_sees_the_refit(rctx, builder):
    G = SMALL["suzanne"]
    H, _ = motions(G)["translate"]
    keep = []
    cfg = rtow.make_config(40, 26, 2, 1, 8, seed=8, precision=rtow.F64_STRICT)
    B = scene_of(H, keep)
    ref, _ = orc.render(B, cfg, orc.RNG_PHILOX, nthreads=4)
    side = torch.cuda.Stream(device="cuda:0")
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    rctx.set_builder(BUILDERS[builder])
    rctx.upload(scene_of(_copy(G), keep))
    torch.cuda.synchronize()
    rctx.refit(B)  # no host wait before the render
    rctx.render_device(cfg, buf.data_ptr(), side.cuda_stream, False)
    side.synchronize()
    assert np.array_equal(buf.cpu().numpy(), ref)


def test_profile_ring_is_not_touched_by_refits(rctx):
    G = SMALL["cover_moving"]
    keep = []
    rctx.upload(scene_of(_copy(G), keep))
    rctx.profile_collect()
    cfg = rtow.make_config(32, 20, 2, 1, 6, seed=4, precision=rtow.F64_STRICT)
    frame_of(rctx, cfg)
    rctx.refit(scene_of(motions(G)["jitter"][0], keep))
    rctx.refit(scene_of(motions(G)["rotate"][0], keep))
    ms, n = rctx.profile_collect()
    assert n == 1 and ms > 0
    assert rctx.profile_collect() == (0.0, 0)


# --------------------------------------------------------------------------------------------- 8. animation ---
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_twenty_refits_then_the_strict_frame_equals_the_oracle(rctx, builder):
    G = SMALL["suzanne"]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    rctx.upload(scene_of(_copy(G), keep))
    cfg = rtow.make_config(40, 26, 2, 1, 8, seed=12, precision=rtow.F64_STRICT)
    for f in range(1, 21):
        B = scene_of(wave(G, f), keep)
        rctx.refit(B)
        rctx.occluded(rays_for(G, 200, f), rtow.F64_STRICT)
    ref, _ = orc.render(B, cfg, orc.RNG_PHILOX, nthreads=4)
    assert np.array_equal(frame_of(rctx, cfg), ref)
    ri = rctx.refit_info()
    assert ri.refits == 20 and ri.bvh_area_ratio > 0.5


# --------------------------------------------------------------------------------------- 9. fast and f32 builds ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["cover_moving", "suzanne"])
def test_fast_and_f32_after_refit_match_a_fresh_upload(rctx, fresh, name, builder):
    G = SMALL[name]
    H, _ = motions(G)["jitter"]
    keep = []
    rctx.set_builder(BUILDERS[builder])
    fresh.set_builder(BUILDERS[builder])
    rctx.upload(scene_of(_copy(G), keep))
    B = scene_of(H, keep)
    rctx.refit(B)
    fresh.upload(B)
    rays = rays_for(H, 4000, 9)
    for k in (rtow.KERNEL_AUTO, rtow.KERNEL_BVH, rtow.KERNEL_GRID):
        a = rctx.intersect(rays, rtow.F64_FAST, k)
        b = fresh.intersect(rays, rtow.F64_FAST, k)
        ha, hb = np.isfinite(a["t"]), np.isfinite(b["t"])
        assert (ha == hb).mean() >= 0.9999
        same = ha & hb & (a["prim"] == b["prim"])
        assert np.all(np.abs(a["t"][same] - b["t"][same]) <= 1e-9 * np.maximum(b["t"][same], 1.0))
        assert (ha & hb & (a["prim"] != b["prim"])).sum() <= max(2, int(1e-4 * len(rays)))
    spp = 8
    cfg = rtow.make_config(64, 40, spp, 1, 10, seed=13, precision=rtow.F32)
    x, y = frame_of(rctx, cfg) / spp, frame_of(fresh, cfg) / spp
    assert np.abs(x.mean(axis=(0, 1)) - y.mean(axis=(0, 1))).max() <= 0.05 / 255.0  # the f32 tests' T2b, T2c
    assert np.abs(block_means(x) - block_means(y)).max() <= 2.0 / 255.0
