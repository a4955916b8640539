"""The guide buffers of both builds against exact first hits, pixel by pixel (GPU; the construction is
tests/guides_exact.py).

Every call under test is checked against the fast (strict) camera_rays of the SAME config: each sample's exact closest
hit gives the material's attenuation, the unit normal, the depth or the sky, and a decided pixel's eight sums must be
the in-order sums of those within the derived bounds (hits and an all-hit albedo bit for bit).  The fast build runs under
every walk and either builder, through the queue's three batch sizes, a rank's strips with dropped border positions, a
stream range, and after a refit.  Per case the undecided pixels (at most 1 %: guides_ref.CAP) and the worst error / bound ratio per
field are printed; DESIGN.md §4.13 records them.
"""
import numpy as np
import pytest

import big_mixed as bm
import guides_exact as gx
import rtow
from guides_ref import SCENES, Logged, Parts, guide_values, logged, moved_cover, row_list, within_cap  # noqa: F401
from support_fixtures import qctx  # noqa: F401
from support_oracle import expected_kernel, primaries, same_bits
from support_tables import BUILDERS, WALKS as KERNELS

pytestmark = pytest.mark.gpu

PRECISION = {gx.STRICT: rtow.F64_STRICT, gx.FAST: rtow.F64_FAST}


# ---------------------------------------------------------------------------------------------------- helpers ---
_refs = {}


def checked(ctx, parts, cfg, build, key, want_kernel=None):
    """guides(cfg) against the reference of camera_rays(cfg); references are shared by `key` (the rays must be the
    same bits) and the walk's triangle cut.  Returns (guides, stats of the call, ids)."""
    rays, ids = ctx.camera_rays(cfg)
    g, st = ctx.guides(cfg, want_stats=True)
    if want_kernel is not None:
        assert st.kernel_used == want_kernel, (key, st.kernel_used)
    spp = len(rays) // g.size
    assert spp * g.size == len(rays) and st.samples == len(rays)
    unit_cut = build == gx.FAST and st.kernel_used == rtow.KERNEL_GRID and len(parts.exact.tri) > 0
    k = (key, build, unit_cut)
    if k not in _refs:
        _refs[k] = parts.reference(rays, ids, spp, build, unit_cut)
    ref = _refs[k]
    assert same_bits(rays, ref.rays) and np.array_equal(ids.reshape(-1, spp, 2), ref.ids), key
    within_cap((key, build, f"kernel {st.kernel_used}"), ref.check(guide_values(g).reshape(-1, 8), (key, build)))
    return g, st, ids


@pytest.fixture(scope="module")
def parts(logged):
    return {name: Parts(lg.scene) for name, lg in logged.items()}


# ---------------------------------------------------------------------------------------------------- tests ---
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", list(SCENES))
def test_fast_guides_under_every_walk(qctx, logged, parts, name, kernel, builder):
    """The fast guides of the three scenes under BRUTE, BVH, GRID and BVH4 with either builder; kernel_used follows the
    render's fallbacks and chooses the triangle cut of the reference."""
    lg = logged[name]
    qctx.set_builder(BUILDERS[builder])
    try:
        qctx.upload(lg.scene)
        checked(qctx, parts[name], lg.config(rtow.F64_FAST, KERNELS[kernel]), gx.FAST, name,
                expected_kernel(lg.scene, KERNELS[kernel]))
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)


@pytest.mark.parametrize("name,kernel", [("cover", "grid"), ("cover_moving", "bvh"), ("suzanne", "bvh4")])
def test_strict_guides(qctx, logged, parts, name, kernel):
    """The checker's own check beside test_strict_guides_equal_the_fold: strict guides against strict rays."""
    lg = logged[name]
    qctx.upload(lg.scene)
    checked(qctx, parts[name], lg.config(rtow.F64_STRICT, KERNELS[kernel]), gx.STRICT, name, KERNELS[kernel])


@pytest.mark.parametrize("spp", [1, 20])
def test_queue_batch_sizes(qctx, parts, spp):
    """pos_batch_max: 1024 positions per atomic at 1 spp and 64 at 20 spp (256 at the 4 spp of the other tests), on a
    24 x 16 image whose 384 positions are fewer than one batch at 1 spp."""
    p = parts["cover"]
    qctx.upload(p.scene)
    cfg = rtow.make_config(24, 16, spp, max_child_rays=0, seed=31, precision=rtow.F64_FAST, nstreams=1)
    g, st, _ = checked(qctx, p, cfg, gx.FAST, f"cover 24x16x{spp}")
    assert g.shape == (16, 24) and st.samples == 24 * 16 * spp


def test_a_rank_with_dropped_border_positions(qctx, logged, parts):
    """Ranks 1 and 0 of 3 with strips of 4 rows on suzanne (27 rows).  Rank 1 holds 8 rows in two strips (4-7, 16-19):
    one row of 8 x 8 tiles whose halves are different strips.  Rank 0 holds 11: its second tile row has 3 rows, and the
    positions of the other 5 are taken and dropped.  The pixels are those of rtow_local_row_list, in order."""
    lg = logged["suzanne"]
    qctx.upload(lg.scene)
    for rank in (1, 0):
        cfg = lg.config(rtow.F64_FAST, rank=rank, nranks=3, tile_rows=4)
        rows = row_list(cfg)
        g, st, ids = checked(qctx, parts["suzanne"], cfg, gx.FAST, f"suzanne rank {rank} of 3")
        assert g.shape == (len(rows), lg.w) and st.local_rows == len(rows)
        want = (rows[:, None].astype(np.int64) * lg.w + np.arange(lg.w)[None, :]).reshape(-1)
        assert np.array_equal(ids.reshape(-1, lg.spp, 2)[:, 0, 0], want)


def test_a_stream_range(qctx, logged, parts):
    """nstreams = 2, stream 1 alone: the call traces samples 2 and 3 of every pixel, and the checker holds it to them."""
    lg = logged["cover_moving"]
    qctx.upload(lg.scene)
    cfg = lg.config(rtow.F64_FAST, nstreams=2, stream_first=1, stream_count=1)
    g, st, ids = checked(qctx, parts["cover_moving"], cfg, gx.FAST, "cover_moving stream 1 of 2")
    assert np.array_equal(np.unique(ids[:, 1]), [2, 3]) and st.samples == lg.w * lg.h * 2


@pytest.fixture(scope="module")
def moved():
    return Parts(moved_cover())


@pytest.mark.parametrize("kernel", ["grid", "bvh", "brute"])
def test_fast_guides_after_a_refit(logged, moved, kernel):
    """The motion of test_gpu_guides.test_after_a_refit, refitted over the unmoved scene: the fast guides are those of
    the moved geometry and the moved camera."""
    lg = logged["cover_moving"]
    c = rtow.Context(0)
    try:
        c.upload(lg.scene)
        c.refit(moved.scene)
        checked(c, moved, lg.config(rtow.F64_FAST, KERNELS[kernel]), gx.FAST, "cover_moving refitted", KERNELS[kernel])
    finally:
        c.close()


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_big_mixed(qctx, builder):
    """The fast guides under every walk; the strict ones under BRUTE (the host builder's: the brute force reads no tree),
    BVH and GRID, each through the checker and BVH's and GRID's equal to BRUTE's bit for bit; the strict camera rays are the
    oracle's primaries."""
    c = bm.case()
    if "big_mixed" not in _refs:
        _refs["big_mixed"] = Parts(c.hs)
    parts, used = _refs["big_mixed"], bm.used()
    strict = lambda wname: c.config(rtow.F64_STRICT, max_child_rays=0, kernel=KERNELS[wname])  # noqa: E731
    try:
        if "big_mixed strict brute" not in _refs:
            qctx.set_builder(rtow.BUILDER_HOST_SAH)
            qctx.upload(c.hs.c)
            _refs["big_mixed strict brute"] = checked(qctx, parts, strict("brute"), gx.STRICT, "big_mixed", used["brute"])[0]
        brute = _refs["big_mixed strict brute"]
        qctx.set_builder(BUILDERS[builder])
        qctx.upload(c.hs.c)
        bm.resident(qctx, builder)
        rays, ids = qctx.camera_rays(c.config(max_child_rays=0))
        want_rays, want_ids = primaries(c.log)
        assert same_bits(rays, want_rays) and np.array_equal(ids, want_ids)
        for wname, walk in KERNELS.items():
            if wname == "brute" and builder == "device":
                continue
            checked(qctx, parts, c.config(rtow.F64_FAST, max_child_rays=0, kernel=walk), gx.FAST, "big_mixed", used[wname])
        for wname in ("bvh", "grid"):
            g = checked(qctx, parts, strict(wname), gx.STRICT, "big_mixed", used[wname])[0]
            assert same_bits(g, brute), (builder, wname, int((guide_values(g) != guide_values(brute)).any(axis=-1).sum()))
    finally:
        qctx.set_builder(rtow.BUILDER_HOST_SAH)
