"""GPU: the head of the always-test (large-primitive) list from the host's block (csrc/rtow_walk_consts.h).

The host puts the first (up to four) static spheres of the large list — ids and record offsets — into the walk's
constants block for every resident grid image.  The GRID trace kernels of the class with moving spheres test those from
wave-uniform values and the rest of the list through the id section; the class of static spheres reads the ids as the
generic kernel (RTOW_NO_SPEC) does, which tests all of the list that way and is the reference inside the build.  Same
tests in the same order: images and the three work counters are equal bit for bit, in the fast and the strict build, and
the strict image is the oracle's.  Scenes (tests/support_large_lists.py), 64 x 48 pixels, 8 samples: large lists of 0, 1,
3, 4, 5 and 7 entries — a block that is unused, partly used, exactly full and overflowing into the id section — in both
classes, a moving scene whose large list mixes a static and a moving sphere, and a scene refitted in place so that other
spheres are the large ones: the block must follow the image that is resident NOW (after a refit: an image built on the
device, whose list the host reads back).  The block itself is compared with the resident image's header and id section.
Knobs are read when a context is created: one context per setting."""
import functools
import os

import numpy as np
import pytest
import torch

import accel_images as ai
import orc
import rtow
import support_large_lists as sl
from support_scenes import scene_of

pytestmark = pytest.mark.gpu

PRECISIONS = {"strict": rtow.F64_STRICT, "fast": rtow.F64_FAST}
_KEEP = []


def config(precision):
    return rtow.make_config(64, 48, 8, 2, 8, seed=17, precision=PRECISIONS[precision], kernel=rtow.KERNEL_GRID)


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
def cases():
    """name -> (Geometry, scene, large-list entries, entries the block serves): made once, shared, never modified."""
    return {name: (G, scene_of(G, _KEEP), n_large, n_fast) for name, (G, n_large, n_fast) in sl.scenes().items()}


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """The oracle's image and segment count of the strict configuration, once per scene."""
    img, st = orc.render(cases()[name][1], config("strict"), orc.RNG_PHILOX, nthreads=4)
    return img, st.segments


def frame(ctx, cfg, want_stats=True):
    buf = torch.zeros((cfg.image_height, cfg.image_width, 3), dtype=torch.float64, device="cuda:0")
    st = ctx.render_device(cfg, buf.data_ptr(), 0, want_stats)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st


def counters(st):
    return (st.samples, st.segments, st.node_tests, st.prim_tests)


def check_block(ctx, G, n_large, n_fast):
    """The resident block's large-list words against the resident image."""
    blob = ctx.debug_image(1)
    assert len(blob) > 64, "no grid image resident"
    P = ai.parse_grid(blob, G)
    assert P["n_large"] == n_large, P["n_large"]
    w = ctx.walk_consts()
    want_fast, want_rec, want_id = sl.block_of_image(blob, G.ns)
    assert int(w[16]) == n_large and int(w[40]) == want_fast == n_fast, (w[16], w[40], want_fast, n_fast)
    assert [int(x) for x in w[32:36]] == want_rec and [int(x) for x in w[36:40]] == want_id, (w[32:41], want_rec, want_id)
    assert not w[25:32].any() and not w[41:48].any()


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(sl.scenes()))
def test_class_kernels_test_the_large_list_like_the_generic_kernel(pair, name, precision):
    spec, generic = pair
    G, sc, n_large, n_fast = cases()[name]
    cfg = config(precision)
    spec.upload(sc)
    generic.upload(sc)
    check_block(spec, G, n_large, n_fast)
    img, st = frame(spec, cfg)
    cls = rtow.SPEC_MOVING_SPHERES if G.nm else rtow.SPEC_STATIC_SPHERES
    assert st.kernel_used == rtow.KERNEL_GRID and spec.last_spec() & 3 == cls and spec.last_counted() is True
    quiet, _ = frame(spec, cfg, want_stats=False)  # the instantiation without statistics reads the same block
    assert spec.last_counted() is False
    gimg, gst = frame(generic, cfg)
    assert gst.kernel_used == rtow.KERNEL_GRID and generic.last_spec() == rtow.SPEC_GENERIC
    print(name, precision, "class", counters(st), "generic", counters(gst))
    assert st.segments > 0 and st.node_tests > 0 and (st.prim_tests > 0 or n_large == 0)
    assert counters(st) == counters(gst)
    assert np.array_equal(img, gimg), int((img != gimg).sum())
    assert np.array_equal(img, quiet), int((img != quiet).sum())
    if precision == "strict":
        ref, segments = oracle_frame(name)
        assert np.array_equal(img, ref), int((img != ref).sum())
        assert st.segments == segments


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_block_follows_a_refit_that_changes_the_large_list(pair, precision):
    """Same counts and order, other sizes: two of the big spheres shrink to small ones and two small spheres grow, so the
    refit's grid image (built on the device) has another large list, and the host refills the block from it."""
    spec, generic = pair
    G, before, n_large, n_fast = cases()["moving_large5"]
    H = ai.Geometry(G.sph.copy(), G.mov.copy(), G.tri.copy(), G.pmat.copy(), list(G.mats), G.cam.copy())
    big = np.flatnonzero((H.sph[:, 3] > 1.0) & (H.sph[:, 3] < 100.0))
    small = np.flatnonzero(H.sph[:, 3] < 1.0)
    assert len(big) == 4
    for i in big[:2]:
        H.sph[i, 1] = H.sph[i, 3] = 0.2
    for i, (x, z) in zip(small[[3, 110]], ((2.0, 2.0), (-2.5, -3.0))):
        H.sph[i] = [x, 1.25, z, 1.25]
    after = scene_of(H, _KEEP)
    cfg = config(precision)
    out = {}
    for label, ctx in (("class", spec), ("generic", generic)):
        ctx.upload(before)
        first, _ = frame(ctx, cfg)
        ids0 = large_ids(ctx, G)
        ctx.refit(after)
        if label == "class":
            check_block(ctx, H, 5, 4)
        img, st = frame(ctx, cfg)
        ids1 = large_ids(ctx, H)
        assert ids1 != ids0 and len(ids1) == 5, (ids0, ids1)
        assert not np.array_equal(img, first)
        out[label] = (img, counters(st), ctx.last_spec())
    assert out["class"][2] & 3 == rtow.SPEC_MOVING_SPHERES and out["generic"][2] == rtow.SPEC_GENERIC
    assert out["class"][1] == out["generic"][1]
    assert np.array_equal(out["class"][0], out["generic"][0]), int((out["class"][0] != out["generic"][0]).sum())
    spec.upload(after)  # a fresh upload of the refitted geometry: the same frame
    check_block(spec, H, 5, 4)
    fresh, fst = frame(spec, cfg)
    assert np.array_equal(fresh, out["class"][0]) and counters(fst)[:2] == out["class"][1][:2]
    if precision == "strict":
        ref, ost = orc.render(after, cfg, orc.RNG_PHILOX, nthreads=4)
        assert np.array_equal(out["class"][0], ref) and out["class"][1][1] == ost.segments


def large_ids(ctx, G):
    blob = ctx.debug_image(1)
    P = ai.parse_grid(blob, G)
    return [int(i) for i in np.frombuffer(blob, np.uint32, P["n_large"], P["off_large"])]
