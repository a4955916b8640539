"""GPU: the trace kernels' wave votes as lane masks (rtow_trace_math.h `lanemask`; rtow_trace_body.h).

The trip keeps its lanes' flags — done, need_sample, pending_hit, helping, holding — as scalar lane masks of the wave,
formed from votes on the comparisons that define them; the walks vote on their own thresholds (queued cells, walking
lanes, the resume cap).  All of that is scheduling and control only: which trip does what may depend on the vote
thresholds, the image, the statistics and the dropped-samples word may not.  A wrong mask shows where few lanes vote, so
the renders here are SMALL: fewer pixels than a wave has lanes per level, queues
shorter than the launch (the fetch quorum, the empty-queue path and the end-of-launch sample donation all run), a width
that is no multiple of the 8-pixel tile, one sample per pixel and twenty, the moving cover (scene class 2), a lattice of
four layers (a grid that is not flat: the 3D walk) and the small scenes of support_scenes.CASES (suzanne: the BVH4 trip
kernel shares the trip).

Per case and build (fast, strict), under every knob setting — the defaults and the extremes of RTOW_LEAF_VOTES (1, 64),
RTOW_FETCH_VOTES (1, 64) and RTOW_WALK_CAP (3,64 and off), read when a context is created:
  * the class kernel without statistics, the class kernel with them (RTOW_COUNT_ALWAYS=1) and the generic kernel
    (RTOW_NO_SPEC) render the same bits, and those are the bits of the default setting;
  * the counting class kernel and the generic kernel report the same segments, node tests and primitive tests, and every
    setting the same samples and segments;
  * the strict image and its segment count are the oracle's;
  * no launch dropped a sample (rtow_profile_collect raises on the dropped-samples word).
"""
import functools
import os

import numpy as np
import pytest
import torch

import orc
import rtow
from support_scenes import CASES, look_at, make_scene, sphere_scene

pytestmark = pytest.mark.gpu

PRECISIONS = {"fast": rtow.F64_FAST, "strict": rtow.F64_STRICT}
KNOBS = {
    "default": {},
    "leaf_votes_1": {"RTOW_LEAF_VOTES": "1"},
    "leaf_votes_64": {"RTOW_LEAF_VOTES": "64"},
    "fetch_votes_1": {"RTOW_FETCH_VOTES": "1"},
    "fetch_votes_64": {"RTOW_FETCH_VOTES": "64"},
    "walk_cap_3_64": {"RTOW_WALK_CAP": "3,64"},
    "walk_cap_off": {"RTOW_WALK_CAP": "off"},
}
_KEEP = []


def _cover(moving):
    return lambda: rtow.HostScene.cover(11, 1.5, moving)


def _stacked():
    """Spheres on integer (x, z) in [-5, 5]^2 in four layers one unit apart: a grid with more than one layer in y."""
    g = np.arange(-5, 6, dtype=float)
    centres = np.array([[x, 0.2 + y, z] for y in range(4) for z in g for x in g])
    return sphere_scene(centres, 0.2, look_at((0.0, 2.0, 9.0), (0.0, 1.5, 0.0), (0, 1, 0)), _KEEP)


def _small(name):
    kind, args = CASES[name][0], CASES[name][1]
    return lambda: make_scene(kind, args)


def _small_shape(name):
    _, _, width, aspect, spp, nstreams, depth, seed = CASES[name]
    return width, int(width / aspect), spp, nstreams, depth, seed


RENDERS = {
    # name: (scene, width, height, spp, nstreams, max_child_rays, seed)
    "cover_24x16_1spp": (_cover(False), 24, 16, 1, 1, 50, 31),
    "cover_24x16_20spp": (_cover(False), 24, 16, 20, 1, 50, 32),
    "cover_40x24_3spp": (_cover(False), 40, 24, 3, 1, 50, 33),
    "cover_40x24_20spp_2streams": (_cover(False), 40, 24, 20, 2, 50, 34),
    "cover_44x24_20spp": (_cover(False), 44, 24, 20, 1, 50, 35),  # 5.5 tiles across
    "moving_24x16_3spp": (_cover(True), 24, 16, 3, 1, 50, 36),
    "moving_44x24_20spp": (_cover(True), 44, 24, 20, 2, 50, 37),
    "stacked_40x24_3spp": (_stacked, 40, 24, 3, 1, 12, 38),
    "stacked_24x16_20spp": (_stacked, 24, 16, 20, 1, 12, 39),
}
RENDERS.update({"small_" + n: (_small(n),) + _small_shape(n) for n in CASES})


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return RENDERS[name][0]()


def config(name, precision):
    _, w, h, spp, ns, depth, seed = RENDERS[name]
    return rtow.make_config(w, h, spp, ns, depth, seed=seed, precision=PRECISIONS[precision])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(image, segments) of the oracle's render of the strict configuration: made once, shared, never modified."""
    ref, ost = orc.render(scene_of(name), config(name, "strict"), orc.RNG_PHILOX, nthreads=8)
    ref.setflags(write=False)
    return ref, ost.segments


def _context(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return rtow.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def contexts():
    """knob setting -> (class kernels, class kernels with RTOW_COUNT_ALWAYS=1, generic kernel)."""
    made = {k: (_context(**env), _context(RTOW_COUNT_ALWAYS="1", **env), _context(RTOW_NO_SPEC="1", **env))
            for k, env in KNOBS.items()}
    yield made
    for group in made.values():
        for c in group:
            c.close()


def frame(ctx, cfg, want_stats):
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    st = ctx.render_device(cfg, buf.data_ptr(), 0, want_stats)
    torch.cuda.synchronize()
    ctx.profile_collect()  # raises if the launch dropped a sample
    return buf.cpu().numpy(), st


def work(st):
    return (st.samples, st.segments, st.node_tests, st.prim_tests)


def expected_spec(name):
    """(kernel, specialisation of the class contexts) the render must take."""
    if name.endswith("suzanne"):
        return rtow.KERNEL_BVH4, None
    if name.startswith("stacked"):
        return rtow.KERNEL_GRID, rtow.SPEC_STATIC_SPHERES  # four layers: the 3D walk
    if name.startswith("moving") or name == "small_cover_moving":
        return rtow.KERNEL_GRID, rtow.SPEC_MOVING_SPHERES | rtow.SPEC_FLAT_Y
    if name.startswith("cover") or name == "small_cover_static":
        return rtow.KERNEL_GRID, rtow.SPEC_STATIC_SPHERES | rtow.SPEC_FLAT_Y
    return None, None  # (three spheres: whatever the render's rule picks)


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(RENDERS))
def test_votes_change_the_schedule_and_nothing_else(contexts, name, precision):
    cfg = config(name, precision)
    scene = scene_of(name)
    kernel, spec = expected_spec(name)
    first = None  # the default setting's image and (samples, segments)
    for knob, (plain, always, generic) in contexts.items():
        for c in (plain, always, generic):
            c.upload(scene)
        img, none = frame(plain, cfg, False)
        counted, st = frame(always, cfg, True)
        ref, gst = frame(generic, cfg, True)
        assert none is None and always.last_counted() is True and generic.last_counted() is True
        print(name, precision, knob, "class", work(st), "generic", work(gst), "kernel", st.kernel_used, plain.last_spec())
        if kernel is not None:
            assert st.kernel_used == kernel and gst.kernel_used == kernel
        if spec is not None:
            assert plain.last_counted() is False  # the instantiation without the counters ran
            assert plain.last_spec() == spec and always.last_spec() == spec
            assert generic.last_spec() == rtow.SPEC_GENERIC
        assert np.array_equal(img, ref), (knob, int((img != ref).sum()))
        assert np.array_equal(counted, ref), (knob, int((counted != ref).sum()))
        assert work(st) == work(gst), (knob, work(st), work(gst))
        assert st.samples == cfg.image_width * cfg.image_height * cfg.samples_per_pixel
        if first is None:
            first = (ref, st.segments)
        assert np.array_equal(ref, first[0]), (knob, int((ref != first[0]).sum()))
        assert st.segments == first[1], (knob, st.segments, first[1])
    if precision == "strict":
        want, segments = oracle(name)
        assert np.array_equal(first[0], want), int((first[0] != want).sum())
        assert first[1] == segments
