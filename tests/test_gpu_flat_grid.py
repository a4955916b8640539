"""GPU: the two-axis walk of the GRID trace kernel (kSpecFlatY, csrc/rtow_dda_step.h) on grids with one layer of cells in y.

The flat instantiation must be TAKEN where the resident grid header says n[1] == 1 (and reported: Context.last_spec),
never elsewhere, and it must visit exactly the cells the 3D walk visits, in the same order: strict images are the
oracle's bit for bit, fast and f32 images are those of RTOW_NO_FLAT and RTOW_NO_SPEC bit for bit, and the three work
counters (segments, node tests = cells read, primitive tests) are those of RTOW_NO_FLAT in every build.  Knobs are read
when a context is created: one context per setting.  Every render here goes through a synchronising entry point, which
turns a non-zero sticky `dropped` word into RTOW_EHIP: a render that returns has dropped nothing."""
import functools
import os

import numpy as np
import pytest

import orc
import rtow
from support_scenes import look_at, sphere_scene

pytestmark = pytest.mark.gpu

FLAT = rtow.SPEC_FLAT_Y
CAPS = {"cap_default": {}, "cap_off": {"RTOW_WALK_CAP": "off"}, "cap_3_64": {"RTOW_WALK_CAP": "3,64"}}


@pytest.fixture(scope="module")
def contexts():
    """get(**env): the context created under that environment (created once, closed at the end of the module)."""
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[key] = rtow.Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return made[key]

    yield get
    for c in made.values():
        c.close()


def grid_dims(ctx):
    img = ctx.debug_image(1)
    assert len(img) >= 64, "no grid image resident"
    return tuple(int(v) for v in np.frombuffer(img[36:48], "<i4"))


def counters(st):
    return (st.segments, st.node_tests, st.prim_tests)


# ---- scenes ------------------------------------------------------------------------------------------------------------

def lattice(layers):
    """Small spheres (r = 0.2) on integer (x, z) in [-5, 5]^2, `layers` of them one unit apart in y from y = 0.2."""
    g = np.arange(-5, 6, dtype=float)
    return np.array([[x, 0.2 + y, z] for y in range(layers) for z in g for x in g])


# the slab of the one-layer lattice is y in [0, 0.4], the grid's bounds are x, z in [-5.2, 5.2] (plus the padding)
CAMERAS = {
    "down": ((0.3, 6.0, 0.2), (0.3, 0.0, 0.2), (0, 0, -1)),          # straight down from above the slab
    "along_x": ((-5.15, 0.2, 0.5), (5.0, 0.2, 0.5), (0, 1, 0)),     # inside the slab, across the whole grid: many resumes
    "diagonal": ((-4.5, 0.2, -4.5), (4.5, 0.2, 4.5), (0, 1, 0)),    # inside the slab along x = z from a symmetric origin
    "away": ((0.0, 0.2, 8.0), (0.0, 0.2, 20.0), (0, 1, 0)),         # outside the bounds looking away: no walk
    "up": ((0.3, -0.6, 0.2), (0.3, 3.0, 0.25), (0, 0, -1)),         # below the slab looking up through it
}
_KEEP = []


@functools.lru_cache(maxsize=None)
def lattice_case(cam_name):
    """(scene, strict config, the oracle's image and segment count): made once, shared, never modified."""
    scene = sphere_scene(lattice(1), 0.2, look_at(*CAMERAS[cam_name]), _KEEP)
    cfg = rtow.make_config(96, 64, 4, 2, 8, seed=7, precision=rtow.F64_STRICT, kernel=rtow.KERNEL_GRID)
    ref, ost = orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=4)
    ref.setflags(write=False)
    return scene, cfg, ref, ost.segments


@functools.lru_cache(maxsize=None)
def cover_case(moving):
    scene = rtow.HostScene.cover(11, 1.5, moving)
    cfg = rtow.make_config(240, 160, 8, 2, 50, seed=3 if moving else 6, precision=rtow.F64_STRICT)
    ref, ost = orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=16, accel=True)
    ref.setflags(write=False)
    return scene, cfg, ref, ost.segments


# ---- 1. the path is taken, and reported ----------------------------------------------------------------------------------

def test_flat_path_is_taken_and_reported(contexts):
    fcfg = rtow.make_config(96, 64, 4, 2, 8, seed=2, precision=rtow.F64_FAST)
    keep = []
    stacked = sphere_scene(lattice(4), 0.2, look_at((0.0, 2.0, 9.0), (0.0, 1.5, 0.0), (0, 1, 0)), keep)
    flat_one = sphere_scene(lattice(1), 0.2, look_at((0.0, 2.0, 9.0), (0.0, 0.2, 0.0), (0, 1, 0)), keep)
    gcfg = rtow.make_config(96, 64, 4, 2, 8, seed=2, precision=rtow.F64_FAST, kernel=rtow.KERNEL_GRID)
    c, noflat, nospec = contexts(), contexts(RTOW_NO_FLAT="1"), contexts(RTOW_NO_SPEC="1")
    for moving, cls in ((False, rtow.SPEC_STATIC_SPHERES), (True, rtow.SPEC_MOVING_SPHERES)):
        scene = rtow.HostScene.cover(11, 1.5, moving)
        _, st = c.render(scene, fcfg)
        assert st.kernel_used == rtow.KERNEL_GRID and grid_dims(c)[1] == 1
        assert c.last_spec() == cls | FLAT
        noflat.render(scene, fcfg)
        assert noflat.last_spec() == cls  # the class, without the bit
        nospec.render(scene, fcfg)
        assert nospec.last_spec() == rtow.SPEC_GENERIC
        # the strict and f32 builds: the class kernels exist in the binary64 builds only
        c.render(scene, rtow.make_config(96, 64, 4, 2, 8, seed=2, precision=rtow.F64_STRICT))
        assert c.last_spec() == cls | FLAT
        c.render(scene, rtow.make_config(96, 64, 4, 2, 8, seed=2, precision=rtow.F32))
        assert c.last_spec() == rtow.SPEC_GENERIC
    # several layers in y: the class kernel with the 3D walk
    c.render(stacked, gcfg)
    assert grid_dims(c)[1] > 1 and c.last_spec() == rtow.SPEC_STATIC_SPHERES
    # ... and the bit follows the header of whatever is resident NOW: a new upload, then refits both ways
    c.render(flat_one, gcfg)
    assert grid_dims(c)[1] == 1 and c.last_spec() == rtow.SPEC_STATIC_SPHERES | FLAT
    import torch

    buf = torch.zeros((64, 96, 3), dtype=torch.float64, device="cuda:0")
    squashed = lattice(4)
    squashed[:, 1] = 0.2  # the stacked scene's spheres, same count and order, pressed into one layer
    squashed[:, 0] += np.repeat(np.arange(4), 121) * 0.25
    for builder in (rtow.BUILDER_HOST_SAH, rtow.BUILDER_DEVICE_LBVH):
        c.set_builder(builder)
        try:
            c.upload(stacked)
            c.render_device(gcfg, buf.data_ptr())
            torch.cuda.synchronize()
            assert grid_dims(c)[1] > 1 and c.last_spec() == rtow.SPEC_STATIC_SPHERES
            c.refit(sphere_scene(squashed, 0.2, stacked.camera, keep))
            c.render_device(gcfg, buf.data_ptr())
            torch.cuda.synchronize()
            assert grid_dims(c)[1] == 1 and c.last_spec() == rtow.SPEC_STATIC_SPHERES | FLAT, builder
            c.refit(stacked)
            c.render_device(gcfg, buf.data_ptr())
            torch.cuda.synchronize()
            assert grid_dims(c)[1] > 1 and c.last_spec() == rtow.SPEC_STATIC_SPHERES, builder
        finally:
            c.set_builder(rtow.BUILDER_AUTO)
    c.render(flat_one, gcfg)  # (synchronising: nothing was dropped on the way)


# ---- 2. the cover scenes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [rtow.F64_STRICT, rtow.F64_FAST, rtow.F32], ids=["strict", "fast", "f32"])
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_cover_scenes_same_image_same_cells(contexts, moving, precision):
    scene, scfg, ref, ref_segments = cover_case(moving)
    c, noflat, nospec = contexts(), contexts(RTOW_NO_FLAT="1"), contexts(RTOW_NO_SPEC="1")
    if precision == rtow.F64_STRICT:
        cfg = scfg
    else:
        cfg = rtow.make_config(240, 160, 24, 2, 50, seed=5, precision=precision)
    img, st = c.render(scene, cfg)
    if precision != rtow.F32:
        assert c.last_spec() & FLAT
    nimg, nst = noflat.render(scene, cfg)
    assert not noflat.last_spec() & FLAT
    print("flat", counters(st), "no_flat", counters(nst))
    assert counters(st) == counters(nst)  # the same cells in the same order
    if precision == rtow.F64_STRICT:
        assert st.segments == ref_segments
        assert np.array_equal(img, ref), int((img != ref).sum())
        assert np.array_equal(nimg, ref)
    else:
        gimg, gst = nospec.render(scene, cfg)
        assert nospec.last_spec() == rtow.SPEC_GENERIC
        assert np.array_equal(img, nimg), int((img != nimg).sum())
        assert np.array_equal(img, gimg), int((img != gimg).sum())
        assert st.segments == gst.segments


# ---- 3. walk shapes the cover camera never makes ----------------------------------------------------------------------------

@pytest.mark.parametrize("cap", list(CAPS))
@pytest.mark.parametrize("cam_name", list(CAMERAS))
def test_lattice_walks_match_the_oracle_and_the_3d_walk(contexts, cam_name, cap):
    scene, scfg, ref, ref_segments = lattice_case(cam_name)
    c, noflat = contexts(**CAPS[cap]), contexts(RTOW_NO_FLAT="1", **CAPS[cap])
    fcfg = rtow.make_config(96, 64, 4, 2, 8, seed=9, precision=rtow.F64_FAST, kernel=rtow.KERNEL_GRID)
    for cfg in (scfg, fcfg):
        img, st = c.render(scene, cfg)
        assert grid_dims(c)[1] == 1  # one layer: from the header of the resident image
        assert c.last_spec() == rtow.SPEC_STATIC_SPHERES | FLAT
        nimg, nst = noflat.render(scene, cfg)
        assert noflat.last_spec() == rtow.SPEC_STATIC_SPHERES
        print(cam_name, cap, "flat", counters(st), "no_flat", counters(nst))
        assert counters(st) == counters(nst)
        assert np.array_equal(img, nimg), int((img != nimg).sum())
        if cfg is scfg:
            assert st.segments == ref_segments
            assert np.array_equal(img, ref), int((img != ref).sum())
