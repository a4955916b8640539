"""GPU: the trace kernels' two instantiations, with and without statistics.

A render that returns no statistics (stats == NULL) launches an instantiation of the trace kernel without the three
per-lane work counters where the kernel has one: the GRID scene-class kernels and the BVH4 trip kernels of the binary64
builds.  RTOW_COUNT_ALWAYS=1 (read at rtow_ctx_create) keeps the counting instantiation.  The image does not depend on
which one ran; the statistics of a counting launch are those of the generic kernel (RTOW_NO_SPEC), which always counts;
no-stats launches in between leave nothing behind in the counters; the sticky dropped-samples word is reported after a
no-stats launch as before.

Scenes: cover static and cover moving at 96 x 64, 20 spp, 2 streams, depth 50; suzanne at 64 x 36, 16 spp.  Builds: fast
and strict.  Tile order on and off.  Knobs are read when a context is created: one context per setting, made once."""
import os

import numpy as np
import pytest
import torch

import rtow
from support_scenes import cover, cover_moving, suzanne

pytestmark = pytest.mark.gpu

PRECISIONS = {"strict": rtow.F64_STRICT, "fast": rtow.F64_FAST}
SCENES = {
    # name: (maker, width, height, spp, nstreams, depth)
    "cover_static": (cover, 96, 64, 20, 2, 50),
    "cover_moving": (cover_moving, 96, 64, 20, 2, 50),
    "suzanne": (suzanne, 64, 36, 16, 2, 20),
}
_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = SCENES[name][0]()
    return _SCENES[name]


def config(name, precision):
    _, w, h, spp, ns, depth = SCENES[name]
    return rtow.make_config(w, h, spp, ns, depth, seed=29, precision=PRECISIONS[precision])


def context(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
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
    """tile order -> (default, RTOW_COUNT_ALWAYS=1, RTOW_NO_SPEC)."""
    made = {}
    for tiles in (1, 0):
        made[tiles] = (context(RTOW_TILE_ORDER=tiles), context(RTOW_TILE_ORDER=tiles, RTOW_COUNT_ALWAYS=1),
                       context(RTOW_TILE_ORDER=tiles, RTOW_NO_SPEC=1))
    yield made
    for group in made.values():
        for c in group:
            c.close()


def frame(ctx, cfg, want_stats):
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    st = ctx.render_device(cfg, buf.data_ptr(), 0, want_stats)
    torch.cuda.synchronize()
    ctx.profile_collect()  # (reports a dropped sample of a no-stats launch)
    return buf.cpu().numpy(), st


def work(st):
    return (st.samples, st.segments, st.node_tests, st.prim_tests)


@pytest.mark.parametrize("tiles", [1, 0], ids=["tile_order", "row_order"])
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(SCENES))
def test_counting_and_non_counting_kernels_render_the_same_frame(contexts, name, precision, tiles):
    default, always, generic = contexts[tiles]
    cfg = config(name, precision)
    for c in (default, always, generic):
        c.upload(scene(name))
    with_stats, st1 = frame(default, cfg, True)
    assert default.last_counted() is True  # a stats pointer: the counting kernel
    kernel = st1.kernel_used
    assert kernel == (rtow.KERNEL_BVH4 if name == "suzanne" else rtow.KERNEL_GRID)
    if kernel == rtow.KERNEL_GRID:
        assert default.last_spec() & 3 == (rtow.SPEC_MOVING_SPHERES if name == "cover_moving" else rtow.SPEC_STATIC_SPHERES)
    without, none = frame(default, cfg, False)
    assert none is None and default.last_counted() is False  # no stats pointer: the kernel without the counters
    forced, none = frame(always, cfg, False)
    assert none is None and always.last_counted() is True  # ... unless RTOW_COUNT_ALWAYS=1
    forced_stats, st3 = frame(always, cfg, True)
    assert always.last_counted() is True
    assert np.array_equal(with_stats, without), int((with_stats != without).sum())
    assert np.array_equal(with_stats, forced), int((with_stats != forced).sum())
    assert np.array_equal(with_stats, forced_stats)
    ref, gst = frame(generic, cfg, True)
    assert generic.last_counted() is True
    if kernel == rtow.KERNEL_GRID:
        assert generic.last_spec() == rtow.SPEC_GENERIC
    _, none = frame(generic, cfg, False)
    assert generic.last_counted() is (kernel == rtow.KERNEL_GRID)  # the generic GRID kernel always counts
    print(name, precision, tiles, "default", work(st1), "always", work(st3), "generic", work(gst))
    assert st1.segments > 0 and st1.node_tests > 0 and st1.prim_tests > 0
    assert work(st1) == work(st3) == work(gst)
    assert np.array_equal(with_stats, ref), int((with_stats != ref).sum())


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_interleaved_stats_and_no_stats_calls_keep_the_statistics_right(contexts, precision):
    """One context, calls with and without statistics in turn, two configurations: every stats call reports what the
    first one of its configuration reported — a launch that does not count adds nothing and leaves nothing behind."""
    ctx = contexts[1][0]
    ctx.upload(scene("cover_static"))
    a = config("cover_static", precision)
    b = rtow.make_config(64, 48, 6, 2, 12, seed=5, precision=PRECISIONS[precision])
    img_a, st_a = frame(ctx, a, True)
    img_b, st_b = frame(ctx, b, True)
    assert work(st_a) != work(st_b)
    for cfg, img, st, want_stats in ((a, img_a, st_a, False), (b, img_b, st_b, True), (b, img_b, st_b, False),
                                     (a, img_a, st_a, True), (a, img_a, st_a, False), (a, img_a, st_a, False),
                                     (b, img_b, st_b, True), (a, img_a, st_a, True)):
        got, gst = frame(ctx, cfg, want_stats)
        assert ctx.last_counted() is want_stats
        assert np.array_equal(got, img)
        if want_stats:
            assert work(gst) == work(st), (work(gst), work(st))


def test_dropped_samples_are_reported_after_a_no_stats_launch():
    """RTOW_TAIL_BOUND (tests only) shrinks the structural trip bound of the end-of-launch protocol, so waves give up
    samples.  The dropped-samples words are no statistics: the kernel without the counters still writes them, and the
    asynchronous entry point reports them at rtow_profile_collect; with the default bound nothing is dropped."""
    hs = scene("cover_static")
    cfg = rtow.make_config(240, 160, 20, 2, 50, seed=3, precision=rtow.F64_FAST)
    bad, good = context(RTOW_TAIL_BOUND=2), context()
    try:
        buf = torch.zeros((160, 240, 3), dtype=torch.float64, device="cuda:0")
        bad.upload(hs)
        bad.render_device(cfg, buf.data_ptr(), 0, False)
        assert bad.last_counted() is False
        with pytest.raises(rtow.RtowError, match="end-of-launch bound"):
            bad.profile_collect()
        bad.profile_collect()  # the word was cleared by the report
        good.upload(hs)
        good.render_device(cfg, buf.data_ptr(), 0, False)
        assert good.last_counted() is False
        good.profile_collect()  # nothing dropped
    finally:
        bad.close()
        good.close()
