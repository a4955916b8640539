"""GPU: the specialised GRID trace kernels, which take the walk's per-scene constants from the host's block
(TraceParams::walk, csrc/rtow_walk_consts.h), against the generic instantiation, which reads the image header itself.

RTOW_NO_SPEC selects the generic kernel: it is the reference inside the build.  Both must visit the same cells and test
the same primitives: images and the three work counters (segments, node tests = cells read, primitive tests) are equal
bit for bit, in the strict and in the fast build, on the static and the moving cover scene (one layer of cells in y: the
two-axis walk), on a 3-D cloud of spheres (the 3D walk of the class kernel), and on the cover scene after a refit that
moves the slab of small spheres — the block must follow the header of the image that is resident NOW.  64 x 48 pixels,
4 samples, 8 bounces.  Knobs are read when a context is created: one context per setting."""
import functools
import os

import numpy as np
import pytest
import torch

import accel_images as ai
import rtow
from support_scenes import look_at, sphere_scene, to_scene

pytestmark = pytest.mark.gpu

FLAT = rtow.SPEC_FLAT_Y
PRECISIONS = {"strict": rtow.F64_STRICT, "fast": rtow.F64_FAST}
_KEEP = []


def config(precision):
    return rtow.make_config(64, 48, 4, 2, 8, seed=13, precision=precision, kernel=rtow.KERNEL_GRID)


@pytest.fixture(scope="module")
def pair():
    """(context with the class kernels, context under RTOW_NO_SPEC)."""
    spec = rtow.Context(0)
    old = os.environ.get("RTOW_NO_SPEC")
    os.environ["RTOW_NO_SPEC"] = "1"
    try:
        generic = rtow.Context(0)
    finally:
        if old is None:
            os.environ.pop("RTOW_NO_SPEC", None)
        else:
            os.environ["RTOW_NO_SPEC"] = old
    yield spec, generic
    spec.close()
    generic.close()


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, expected class of the specialised kernel): made once, shared, never modified."""
    if name in ("cover_static", "cover_moving"):
        hs = rtow.HostScene.cover(11, 1.5, name == "cover_moving")
        _KEEP.append(hs)
        return hs.c, (rtow.SPEC_MOVING_SPHERES if name == "cover_moving" else rtow.SPEC_STATIC_SPHERES) | FLAT
    assert name == "cloud"
    g = np.random.default_rng(3)
    centres = g.uniform([-4.0, 0.3, -4.0], [4.0, 3.3, 4.0], size=(260, 3))
    return (sphere_scene(centres, 0.18, look_at((0.0, 2.5, 9.0), (0.0, 1.5, 0.0), (0, 1, 0)), _KEEP),
            rtow.SPEC_STATIC_SPHERES)


def grid_header(ctx):
    img = ctx.debug_image(1)
    assert len(img) >= 64, "no grid image resident"
    return img[:64]


def counters(st):
    return (st.segments, st.node_tests, st.prim_tests)


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", ["cover_static", "cover_moving", "cloud"])
def test_class_kernels_walk_like_the_generic_kernel(pair, name, precision):
    spec, generic = pair
    sc, cls = scene(name)
    cfg = config(PRECISIONS[precision])
    img, st = spec.render(sc, cfg)
    assert st.kernel_used == rtow.KERNEL_GRID and spec.last_spec() == cls
    ny = int(np.frombuffer(grid_header(spec)[40:44], "<i4")[0])
    assert (ny == 1) == bool(cls & FLAT), ny  # the covers: one layer; the cloud: a 3-D grid
    gimg, gst = generic.render(sc, cfg)
    assert gst.kernel_used == rtow.KERNEL_GRID and generic.last_spec() == rtow.SPEC_GENERIC
    print(name, precision, "class", counters(st), "generic", counters(gst))
    assert st.segments > 0 and st.node_tests > 0 and st.prim_tests > 0
    assert counters(st) == counters(gst)
    assert np.array_equal(img, gimg), int((img != gimg).sum())


def _frame(ctx, cfg):
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    st = ctx.render_device(cfg, buf.data_ptr(), 0, True)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_block_follows_the_header_after_a_refit_that_moves_the_slab(pair, precision):
    spec, generic = pair
    hs = rtow.HostScene.cover(11, 1.5, False)
    G = ai.Geometry.of_scene(hs.c)
    hs.close()
    H = ai.Geometry(G.sph.copy(), G.mov.copy(), G.tri.copy(), G.pmat.copy(), list(G.mats), G.cam.copy())
    small = np.abs(H.sph[:, 3]) < 0.5  # the slab of r = 0.2 spheres: up, and sideways by more than a cell
    assert 100 < small.sum() < G.ns
    H.sph[small, 0:3] += np.array([1.25, 0.6, -0.75])
    keep = []
    before, after = to_scene(G, keep), to_scene(H, keep)
    cfg = config(PRECISIONS[precision])
    out = {}
    for label, ctx in (("class", spec), ("generic", generic)):
        ctx.upload(before)
        first, _ = _frame(ctx, cfg)
        h0 = grid_header(ctx)
        ctx.refit(after)
        img, st = _frame(ctx, cfg)
        h1 = grid_header(ctx)
        assert h1[0:12] != h0[0:12], "the refit moved the grid's corner"
        assert not np.array_equal(img, first)
        out[label] = (img, counters(st), h1, ctx.last_spec())
    print(precision, "class", out["class"][1], "generic", out["generic"][1])
    assert out["class"][3] == rtow.SPEC_STATIC_SPHERES | FLAT and out["generic"][3] == rtow.SPEC_GENERIC
    assert out["class"][2] == out["generic"][2]  # the same resident header
    assert out["class"][1] == out["generic"][1]
    assert np.array_equal(out["class"][0], out["generic"][0]), int((out["class"][0] != out["generic"][0]).sum())
