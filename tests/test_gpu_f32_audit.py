"""GPU: the binary32 build (RTOW_F32) sample by sample against exact hits — the per-sample bar of that build
(tests/f32_audit.py; tests/test_gpu_f32.py holds the full-depth, statistical one).

Each case renders the one-sample frames of a frame in RTOW_F32 at max_child_rays 0 and 1 and runs both layers of the
audit: on every kept sample the primary's any-hit decision (layer P) and the scattered ray's (layer S) must be the exact
one and the colour within its first-order bound — zero exceptions.  The kernel that ran is asserted, and so is what the
audit assumes about it: the spheres it takes as tested in binary64 are in the resident grid image's large list (GRID),
or the kernel tests every sphere in binary64 (STREAM, BVH).

Measured on the MI355X: see DESIGN.md section 4.4 (kept and left-out shares, worst |q| / band, worst colour error over
its tolerance, per case).
"""
import numpy as np
import pytest

import accel_images as ai
import exact_hits as ex
import f32_audit as fa
import rtow
import sample_audit as sa

pytestmark = pytest.mark.gpu

STREAM, BVH, GRID = rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_GRID


@pytest.fixture(scope="module")
def actx():
    c = rtow.Context(0)
    yield c
    c.close()


def _c(scene):
    return scene.c if hasattr(scene, "c") else scene


def _frames_resident(ctx, cfg):
    """The one-sample frames of `cfg` of the RESIDENT scene: (c [spp, H, W, 3], kernel_used)."""
    import torch

    out, used = [], set()
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    for j in range(rtow.spp_effective(cfg)):
        buf.zero_()
        st = ctx.render_device(sa.sample_cfg(cfg, j), buf.data_ptr(), 0, True)
        torch.cuda.synchronize()
        assert st.samples == cfg.image_height * cfg.image_width
        out.append(buf.cpu().numpy().copy())
        used.add(st.kernel_used)
    assert len(used) == 1, used
    return np.stack(out), used.pop()


def _check_assumed_large(ctx, au, used):
    if used in (STREAM, BVH):
        return  # (closest_hit_stream and closest_hit_bvh test every sphere in binary64)
    assert used == GRID and not au.all_f64, (used, au.name)
    G = ai.Geometry.of_scene(_c(au.scene))
    blob = ctx.debug_image(1)
    assert blob, "no resident grid image"
    P = ai.parse_grid(blob, G)
    ids = np.frombuffer(blob, np.int32, P["n_cell_ids"] + P["n_large"], P["off_ids"])
    large = set(int(i) for i in ids[P["n_cell_ids"]:])
    base = {ex.SPHERE: 0, ex.MOVING: G.ns}
    for cls, i in au.large:
        assert base[cls] + i in large, f"{au.name}: sphere {(cls, i)} is taken as tested in binary64, the grid lists it in cells"


def run_audit(ctx, name, kernel, want, upload=None, refit=None):
    au = fa.audit(name)
    fa.check_conditions(au)
    ctx.upload(_c(upload if upload is not None else au.scene))
    if refit is not None:
        ctx.refit(_c(refit))
    got = []
    for depth in (0, 1):
        c, used = _frames_resident(ctx, fa.shallow_cfg(au.cfg, depth, rtow.F32, kernel))
        assert used in want, (name, kernel, used)
        got.append(c)
    _check_assumed_large(ctx, au, used)
    p, s = au.check(got[0], got[1], f"{name} (kernel {kernel}, used {used})")
    sh = au.shares()
    print(f"\n{name} kernel {kernel} (used {used}): layer P kept {p['kept']} of {sh['samples']} ({p['kept_hits']} hits), worst "
          f"colour error {p['worst_err_over_tol']:.3f} of its tolerance; layer S kept {s['kept']} of {sh['S_lm_hits']} decided "
          f"hits ({s['kept_black']} black), worst colour error {s['worst_err_over_tol']:.3f} of its tolerance")


CASES = [
    ("cover_static", rtow.KERNEL_AUTO, (GRID,)),   # binary32 cell spheres, binary64 large list
    ("cover_static", rtow.KERNEL_BVH, (BVH,)),
    ("cover_moving", rtow.KERNEL_AUTO, (GRID,)),   # binary32 moving records, shutter time
    ("cover_moving", rtow.KERNEL_BVH, (BVH,)),
    ("cover0", rtow.KERNEL_AUTO, (STREAM,)),       # binary64 tests on the widened ray
    ("suzanne", rtow.KERNEL_BVH, (BVH,)),          # binary32 triangles
    ("suzanne", rtow.KERNEL_GRID, (GRID,)),
    ("handmade", rtow.KERNEL_AUTO, (STREAM, BVH)),  # negative radius, triangles inserted first
    ("cover_far", rtow.KERNEL_AUTO, (GRID,)),      # far from the origin: binary32 loses a digit and a half
]


@pytest.mark.parametrize("name,kernel,want", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_f32_samples_against_exact_hits(actx, name, kernel, want):
    run_audit(actx, name, kernel, want)


@pytest.mark.parametrize("builder", [rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH])
def test_f32_samples_with_either_builder(actx, builder):
    actx.set_builder(builder)
    try:
        run_audit(actx, "cover_moving", rtow.KERNEL_BVH, (BVH,))
        assert actx.build_info().builder == builder
    finally:
        actx.set_builder(rtow.BUILDER_AUTO)


def test_f32_samples_after_a_refit(actx):
    """The moving cover scene is uploaded, then refitted to the same scene turned about the vertical axis (the `rotate`
    motion of support_scenes.motions); the audit is of the turned scene."""
    run_audit(actx, "cover_refit", rtow.KERNEL_AUTO, (GRID, BVH), upload=fa.FRAMES["cover_moving"][0](),
              refit=fa.audit("cover_refit").scene)


@pytest.mark.parametrize("name,kernel", [("cover_small", rtow.KERNEL_AUTO), ("suzanne_small", rtow.KERNEL_BVH)])
def test_f32_full_depth_census_is_reported(actx, name, kernel):
    """Full depth, reported only: the census (sample_audit.census) of the F32 one-sample frames against the strict
    build's.  Only finiteness and the range [0, 1 + 1e-6] are asserted: at full depth every bounce multiplies the
    bands of the ones before it, and a count cap taken from bands would be so wide that it could not fail; T2
    (tests/test_gpu_f32.py) stays the full-depth bar."""
    scene, cfg = sa.frame(name, rtow.F32, kernel)
    stacks = {}
    for prec in (rtow.F32, rtow.F64_STRICT):
        c, seg = [], 0
        for j in range(rtow.spp_effective(cfg)):
            img, st = actx.render(scene, sa.sample_cfg(sa.copy_cfg(cfg, precision=prec), j))
            c.append(img)
            seg += st.segments
        stacks[prec] = (np.stack(c), seg)
    a, seg_a = stacks[rtow.F32]
    b, seg_b = stacks[rtow.F64_STRICT]
    assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 + 1e-6, (float(a.min()), float(a.max()))
    cen = sa.census(a, b)
    print(f"\n{name}: {cen.n} samples; equal {cen.equal / cen.n:.4f}, tight {cen.tight / cen.n:.4f}, loose "
          f"{cen.loose / cen.n:.5f} ({cen.loose}), max |diff| {cen.max_abs:.3g}; segments F32 {seg_a}, strict {seg_b}")
