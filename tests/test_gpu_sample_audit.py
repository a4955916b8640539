"""Every pixel of a render against its own samples, sample by sample (GPU; the construction is tests/sample_audit.py).

A. The frame is the fold of its own samples.  One full frame and spp_eff one-sample frames (nstreams = spp_eff, stream j
   alone: one level of one sample in every build, so the same kernel instantiation traces it with the full render's
   sample index and random numbers).  The full frame must be the fixed-order fold of those colours over the levels of
   rtow_debug_schedule — bits compared, every pixel, no exceptions — the segment counts must add up and every one-sample
   frame must count one sample per pixel.  A sample traced under a wrong index, traced twice, added out of order or a
   level sum written to another level's slot all break this, whatever the knobs; the cases cover the scheduling
   machinery of the fast build (two levels, the ragged last level, 64-pixel tiles with more empty tiles than one wave,
   the empty segment bought 16 levels at a time, partitions, an untiled image, a launch that is almost all tail).
B. Each fast sample against the strict sample of the same identity: counted, against caps taken from the reference side
   (the contracted oracle against the oracle, computed here on the CPU) — never from the code under test.
C. The fast radiance query of the render's own primaries against the fast render, per sample, under the same caps.
"""
import numpy as np
import pytest

import rtow
import sample_audit as sa
from support_oracle import tile_order

pytestmark = pytest.mark.gpu

KERNEL_NAMES = {rtow.KERNEL_BRUTE: "brute", rtow.KERNEL_BVH: "bvh", rtow.KERNEL_GRID: "grid", rtow.KERNEL_BVH4: "bvh4"}


# ---------------------------------------------------------------------------------------------------- helpers ---
def gpu_samples(ctx, scene, cfg):
    """(c [spp_eff, rows, W, 3], total segments, kernel_used): the one-sample frames of `cfg`."""
    c, segments, used = [], 0, set()
    for j in range(rtow.spp_effective(cfg)):
        img, st = ctx.render(scene, sa.sample_cfg(cfg, j))
        assert st.samples == img.shape[0] * img.shape[1], (j, st.samples)
        c.append(img)
        segments += st.segments
        used.add(st.kernel_used)
    assert len(used) == 1
    return np.stack(c), segments, used.pop()


_stacks = {}


def frame_samples(ctx, name, precision, kernel=rtow.KERNEL_AUTO):
    """The one-sample frames of sa.FRAMES[name] in the module's context: rendered once, shared, read-only."""
    key = (name, precision, kernel)
    if key not in _stacks:
        scene, cfg = sa.frame(name, precision, kernel)
        c, seg, used = gpu_samples(ctx, scene, cfg)
        c.setflags(write=False)
        _stacks[key] = (c, seg, used)
    return _stacks[key]


def audit(ctx, scene, cfg, samples=None, want_levels=None, want_kernel=None):
    """A: the frame of `cfg` is the fold of its samples (bits), the segments add up, the kernel is the one meant.
    Returns (full, c)."""
    full, st = ctx.render(scene, cfg)  # (the scene is resident from here on: the schedule is its class's)
    lv = sa.levels(ctx, cfg)
    if want_levels is not None:
        assert lv == want_levels, lv
    c, seg, used = samples if samples is not None else gpu_samples(ctx, scene, cfg)
    assert used == st.kernel_used
    if want_kernel is not None:
        assert st.kernel_used == want_kernel, st.kernel_used
    assert st.samples == full.shape[0] * full.shape[1] * rtow.spp_effective(cfg)
    sa.check_fold(full, lv, c, f"levels {lv}")
    assert seg == st.segments, (seg, st.segments)
    return full, c


def tiled_with_empty_tiles(scene, cfg, more_than):
    table, empty, ne, tw, th = tile_order(scene, cfg)
    assert len(table) > 0 and tw + th == 6, "the launch is not tiled"
    assert ne > more_than, f"{ne} empty tiles"
    return ne


# ------------------------------------------------------------------------------------------ A: frame = fold ---
@pytest.mark.parametrize("spp,want", [(24, [(0, 12), (12, 12)]), (23, [(0, 10), (10, 13)]),
                                      (37, [(0, 10), (10, 10), (20, 17)])])
def test_fast_frame_is_the_fold_of_its_samples(ctx, spp, want):
    """Static cover, 240x160, the fast build under AUTO (the grid walk): two levels of 12; 10 + 13 (ragged); and 10 + 10 +
    17 — with two levels g = s_1 + (s_0 + 0) is symmetric in the level sums, so only three or more levels can tell a
    level sum in another level's slot.  600 tiles, more than 64 of them empty: the empty segment is bought in more
    batches than one wave takes."""
    scene, cfg = sa.frame("cover")
    cfg.samples_per_pixel = spp
    tiled_with_empty_tiles(scene, cfg, 64)
    audit(ctx, scene, cfg, frame_samples(ctx, "cover", rtow.F64_FAST) if spp == 24 else None, want, rtow.KERNEL_GRID)


def test_f32_frame_is_the_fold_of_its_samples(ctx):
    """The binary32 build: the pixel sums are binary64 in every build."""
    scene, cfg = sa.frame("cover", rtow.F32)
    audit(ctx, scene, cfg, None, [(0, 12), (12, 12)])


def test_strict_frame_is_the_fold_of_its_samples_and_each_sample_is_the_oracles(ctx):
    """F64_STRICT, nstreams = 3: the levels are the streams.  Every one-sample frame equals the oracle's frame of the
    same sample config bit for bit: "sample j" is the oracle's sample j."""
    scene, cfg = sa.frame("cover", rtow.F64_STRICT)
    cfg.nstreams = 3
    full, c = audit(ctx, scene, cfg, frame_samples(ctx, "cover", rtow.F64_STRICT), [(0, 8), (8, 8), (16, 8)])
    ref, seg = sa.oracle_stack("cover")
    bad = sa.differing_pixels(c, ref)
    assert not bad.any(), (f"{int(bad.sum())} samples differ from the oracle's; first (sample, row, column) "
                           f"{np.argwhere(bad)[:5].tolist()}")
    assert frame_samples(ctx, "cover", rtow.F64_STRICT)[1] == seg


@pytest.mark.parametrize("kernel", [rtow.KERNEL_BVH, rtow.KERNEL_BRUTE], ids=["bvh", "brute"])
def test_moving_cover_frame_is_the_fold_of_its_samples(ctx, kernel):
    scene, cfg = sa.frame("cover_moving", rtow.F64_FAST, kernel)
    audit(ctx, scene, cfg, None, [(0, 12), (12, 12)], kernel)


@pytest.mark.parametrize("spp,want", [(32, [(0, 16), (16, 16)]), (35, [(0, 16), (16, 19)]),
                                      (51, [(0, 17), (17, 17), (34, 17)])])
def test_mesh_frame_is_the_fold_of_its_samples(ctx, spp, want):
    """suzanne, 320x180, the 4-wide walk (resumable walks, items of 16 samples): 2 x 16, 16 + 19 (ragged) and 3 x 17
    (three levels: their order shows)."""
    scene, cfg = sa.frame("suzanne", rtow.F64_FAST, rtow.KERNEL_BVH4)
    cfg.samples_per_pixel = spp
    audit(ctx, scene, cfg, None, want, rtow.KERNEL_BVH4)


@pytest.mark.parametrize("tile_rows", [8, 4])
def test_partition_frame_is_the_fold_of_its_samples(ctx, tile_rows):
    """Rank 1 of 3: strips of 8 rows (8x8 tiles) and of 4 rows (16x4 tiles)."""
    scene, cfg = sa.frame("cover")
    cfg.nranks, cfg.rank, cfg.tile_rows = 3, 1, tile_rows
    tiled_with_empty_tiles(scene, cfg, 0)
    full, _ = audit(ctx, scene, cfg, None, [(0, 12), (12, 12)])
    assert full.shape[0] == len(rtow.local_rows(cfg)) < 160


def test_untiled_frame_is_the_fold_of_its_samples(ctx):
    """50x37: no tile shape divides the width; plain row-major order."""
    scene = rtow.HostScene.cover(11, 50 / 37, False)
    cfg = rtow.make_config(50, 37, 24, 1, 50, seed=7, precision=rtow.F64_FAST)
    table, _, _, tw, th = tile_order(scene, cfg)
    assert len(table) == 0 and (tw, th) == (0, 0)
    audit(ctx, scene, cfg, None, [(0, 12), (12, 12)])


def test_many_levels_per_empty_batch(monkeypatch):
    """RTOW_EMPTY_LEVELS=16 and 60 spp: all six levels of an empty tile are bought at once."""
    monkeypatch.setenv("RTOW_EMPTY_LEVELS", "16")
    c16 = rtow.Context(0)
    try:
        scene, cfg = sa.frame("cover")
        cfg.samples_per_pixel = 60
        tiled_with_empty_tiles(scene, cfg, 64)
        audit(c16, scene, cfg, None, [(10 * k, 10) for k in range(6)], rtow.KERNEL_GRID)
    finally:
        c16.close()


@pytest.mark.parametrize("precision", [rtow.F64_FAST, rtow.F64_STRICT], ids=["fast", "strict"])
def test_a_launch_that_is_almost_all_tail(monkeypatch, precision):
    """RTOW_SCHED_CHUNK=0 (one item per stream), one stream, 16x8 pixels, 120 spp: 128 items of 120 samples for a
    queue that is empty at once, so the launch is almost all tail and the slow pixels' samples are donated.  The fold is
    the plain sequential sum; the strict frame is also the oracle's."""
    monkeypatch.setenv("RTOW_SCHED_CHUNK", "0")
    c0 = rtow.Context(0)
    try:
        scene = rtow.HostScene.cover(11, 2.0, False)
        cfg = rtow.make_config(16, 8, 120, 1, 50, seed=7, precision=precision)
        full, c = audit(c0, scene, cfg, None, [(0, 120)])
        s = np.zeros_like(full)
        for j in range(120):
            s = s + c[j]
        assert sa.bits(full).tolist() == sa.bits(s).tolist()
        if precision == rtow.F64_STRICT:
            ref, ost = sa.oracle_render(scene, cfg)
            assert not sa.differing_pixels(full, ref).any()
    finally:
        c0.close()


# ------------------------------------------------------------------------- B: fast samples against strict ones ---
def _capped(what, got, ref, n, seg_got, seg_ref, a, b):
    """The caps of B on a census `got` of a (fast) against b, given the reference-side census `ref` of the same frame."""
    print(f"{what}: {got.n} samples; equal bits {got.equal} ({got.equal / got.n:.4f}), tight {got.tight} "
          f"(reference side {ref.tight}, cap {4 * ref.tight + 16}), loose {got.loose} (cap {int(1e-5 * n)}), "
          f"max |d| {got.max_abs:.3g}; segments {seg_got} against {seg_ref}")
    if got.loose:
        print(sa.describe_loose(got, a, b))
    assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 + 1e-12, (a.min(), a.max())
    assert ref.loose == 0
    assert got.tight <= 4 * ref.tight + 16
    assert got.loose <= 1e-5 * n
    assert abs(seg_got - seg_ref) <= 1e-5 * seg_ref


@pytest.mark.parametrize("name,kernel,want", [
    ("cover", rtow.KERNEL_AUTO, rtow.KERNEL_GRID), ("cover_moving", rtow.KERNEL_AUTO, None),
    ("cover", rtow.KERNEL_BVH, rtow.KERNEL_BVH), ("suzanne", rtow.KERNEL_BVH4, rtow.KERNEL_BVH4)],
    ids=["cover-auto", "cover_moving-auto", "cover-bvh", "suzanne-bvh4"])
def test_fast_samples_against_strict_samples(ctx, name, kernel, want):
    """Sample for sample, 921,600 of them per frame: every fast value finite and in [0, 1]; tight differences at most
    4 x the contracted oracle's against the oracle's on this frame, + 16 (tests/exact_hits.py: the fast build's rounding
    band per decision is 34 u against the strict build's 18 u — about twice, doubled; + 16 for counts near zero); loose
    differences — flipped decisions — at most 1e-5 of the samples, and the segment totals within 1e-5 (the project's
    bound on flipped decisions); the reference side has none."""
    fast, fseg, fused = frame_samples(ctx, name, rtow.F64_FAST, kernel)
    strict, sseg, sused = frame_samples(ctx, name, rtow.F64_STRICT, kernel)
    if want is not None:
        assert fused == sused == want
    ref, oseg, _ = sa.reference_census(name)
    assert sseg == oseg  # (the strict build's paths are the oracle's)
    _capped(f"{name} {KERNEL_NAMES.get(fused, fused)}", sa.census(fast, strict), ref,
            fast.shape[0] * fast.shape[1] * fast.shape[2], fseg, sseg, fast, strict)


# --------------------------------------------------------------------- C: the fast query against the fast render ---
@pytest.mark.parametrize("name", ["cover_small", "suzanne_small"])
def test_fast_radiance_queries_against_the_fast_render(ctx, name):
    """120x80x24: radiance(camera_rays(cfg)) with one sample per ray, against the one-sample frames of the render, both
    in the fast build — the caps of B.  The share of samples with equal bits is printed, not asserted: the query kernel
    restates the shading expression for expression, but contraction may differ between two kernels."""
    scene, cfg = sa.frame(name)
    c, seg, used = gpu_samples(ctx, scene, cfg)
    ctx.upload(scene)
    rays, ids = ctx.camera_rays(cfg)
    spp, (rows, w) = cfg.samples_per_pixel, c.shape[1:3]
    assert len(rays) == rows * w * spp
    assert np.array_equal(ids[:, 0], np.repeat(np.arange(rows * w), spp))  # pixel-major, a pixel's samples ascending
    assert np.array_equal(ids[:, 1], np.tile(np.arange(spp), rows * w))
    rgb, st = ctx.radiance(rays, 1, cfg.max_child_rays, cfg.seed, ids, 0, rtow.F64_FAST, want_stats=True)
    assert st.samples == len(rays)
    q = np.ascontiguousarray(rgb.reshape(rows, w, spp, 3).transpose(2, 0, 1, 3))
    ref, _, _ = sa.reference_census(name)
    _capped(f"{name} query {KERNEL_NAMES.get(st.kernel_used, st.kernel_used)} / render {KERNEL_NAMES.get(used, used)}",
            sa.census(q, c), ref, q.shape[0] * rows * w, st.segments, seg, q, c)
