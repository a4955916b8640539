"""The sample audit's own ground (no GPU): tests/sample_audit.py against the oracle.

The fold of the oracle's one-sample frames must be the oracle's frame bit for bit; the schedules the GPU tests rely on
must be what rtow_debug_schedule says; the fold check must reject planted sample-identity faults; and the contracted
oracle (the reference under FMA contraction) gives the reference-side count of samples that rounding alone moves.
"""
import numpy as np
import pytest

import rtow
import sample_audit as sa


def _streams(cfg):
    spt = cfg.samples_per_pixel // cfg.nstreams
    return [(k * spt, spt) for k in range(cfg.nstreams)]


# ------------------------------------------------------------------------------------------------- oracle fold ---
@pytest.mark.parametrize("name", ["cover", "cover_moving"])
def test_the_oracle_frame_is_the_fold_of_the_oracle_samples(name):
    """240x160, 24 spp, depth 50: for nstreams = 1, 2, 3 and spp the oracle's frame equals the fold of its 24 one-sample
    frames over its streams, every bit of every pixel, and the segments add up.  (The sample frames do not depend on
    nstreams: sample j is sample j.)"""
    c, seg = sa.oracle_stack(name)
    scene, base = sa.frame(name, rtow.F64_STRICT)
    assert len(c) == base.samples_per_pixel == 24
    for ns in (1, 2, 3, 24):
        cfg = sa.copy_cfg(base, nstreams=ns)
        lv = sa.levels(None, cfg)
        assert lv == _streams(cfg)  # strict: the levels are the reference's streams
        full, st = sa.oracle_render(scene, cfg)
        sa.check_fold(full, lv, c, f"{name} nstreams {ns}")
        assert st.segments == seg and st.samples == 240 * 160 * 24


def test_an_effective_sample_count_below_spp():
    """spp 25 with 3 streams is 24 samples: sample_cfg counts the effective ones."""
    scene, base = sa.frame("cover", rtow.F64_STRICT)
    cfg = sa.copy_cfg(base, samples_per_pixel=25, nstreams=3)
    c, _ = sa.oracle_stack("cover")
    one = sa.sample_cfg(cfg, 23)
    assert (one.samples_per_pixel, one.nstreams, one.stream_first, one.stream_count) == (24, 24, 23, 1)
    full, _ = sa.oracle_render(scene, cfg)
    sa.check_fold(full, _streams(sa.copy_cfg(cfg, samples_per_pixel=24)), c)


# --------------------------------------------------------------------------------------------------- schedules ---
def _fast(spp, nstreams=1, **kw):
    return rtow.make_config(240, 160, spp, nstreams, 50, seed=7, precision=rtow.F64_FAST, **kw)


def test_schedules_the_gpu_tests_rely_on(monkeypatch):
    """Preconditions of tests/test_gpu_sample_audit.py, from the library (a new context's table)."""
    for knob in ("RTOW_SCHED_CHUNK", "RTOW_SCHED_CHUNK_MESH"):
        monkeypatch.delenv(knob, raising=False)
    assert sa.levels(None, _fast(24)) == [(0, 12), (12, 12)]
    assert sa.levels(None, _fast(23)) == [(0, 10), (10, 13)]  # ragged
    assert sa.levels(None, _fast(37)) == [(0, 10), (10, 10), (20, 17)]  # ragged, three levels
    assert sa.levels(None, _fast(60)) == [(10 * k, 10) for k in range(6)]
    assert sa.levels(None, _fast(24, 3)) == [(0, 12), (12, 12)]  # fast: not the streams
    assert sa.levels(None, sa.copy_cfg(_fast(24, 3), precision=rtow.F64_STRICT)) == [(0, 8), (8, 8), (16, 8)]
    assert sa.levels(None, sa.copy_cfg(_fast(24), precision=rtow.F32)) == [(0, 12), (12, 12)]
    # a triangle mesh aims at 16 samples per item (the context-free table takes its length from RTOW_SCHED_CHUNK)
    monkeypatch.setenv("RTOW_SCHED_CHUNK", "16")
    assert sa.levels(None, _fast(32)) == [(0, 16), (16, 16)]
    assert sa.levels(None, _fast(35)) == [(0, 16), (16, 19)]  # ragged
    assert sa.levels(None, _fast(51)) == [(0, 17), (17, 17), (34, 17)]
    # one item per stream
    monkeypatch.setenv("RTOW_SCHED_CHUNK", "0")
    assert sa.levels(None, _fast(120)) == [(0, 120)]


@pytest.mark.parametrize("chunk", [None, "16", "0", "1"])
@pytest.mark.parametrize("precision", [rtow.F64_STRICT, rtow.F64_FAST, rtow.F32], ids=["strict", "fast", "f32"])
def test_a_sample_config_is_one_level_of_one_sample(monkeypatch, precision, chunk):
    if chunk is None:
        monkeypatch.delenv("RTOW_SCHED_CHUNK", raising=False)
    else:
        monkeypatch.setenv("RTOW_SCHED_CHUNK", chunk)
    for spp, ns in ((24, 1), (23, 1), (25, 3), (120, 1), (1, 1)):
        cfg = sa.copy_cfg(_fast(spp, ns, rank=1, nranks=3, tile_rows=4), precision=precision)
        eff = spp // ns * ns
        for j in range(eff):
            one = sa.sample_cfg(cfg, j)
            assert sa.levels(None, one) == [(j, 1)], (spp, ns, j)
            assert (one.image_width, one.image_height, one.max_child_rays, one.precision, one.kernel, one.rank, one.nranks,
                    one.tile_rows, one.seed, one.accumulate) == (240, 160, 50, precision, cfg.kernel, 1, 3, 4, 7, 0)


# ------------------------------------------------------------------------------------------------ planted faults ---
def test_the_fold_check_rejects_planted_faults():
    """The oracle's frame of the static cover scene at nstreams = 3 (levels 3 x 8) passes against its own samples; each
    alteration of the sample stack is applied across the frame and must be caught in at least one pixel."""
    c, _ = sa.oracle_stack("cover")
    scene, base = sa.frame("cover", rtow.F64_STRICT)
    cfg = sa.copy_cfg(base, nstreams=3)
    lv = sa.levels(None, cfg)
    assert lv == [(0, 8), (8, 8), (16, 8)]
    full, _ = sa.oracle_render(scene, cfg)
    sa.check_fold(full, lv, c)

    def rejected(what, stack):
        with pytest.raises(sa.AuditError) as e:
            sa.check_fold(full, lv, stack, what)
        print(str(e.value)[:160])
        assert "pixels are not the fold" in str(e.value)

    dropped = c.copy()
    dropped[5] = 0.0  # sample 5 never traced
    rejected("one sample dropped", dropped)
    twice = c.copy()
    twice[8] = c[7]  # a level's last sample traced again as the next level's first
    rejected("one sample duplicated over its neighbour", twice)
    swapped = c.copy()
    swapped[7], swapped[8] = c[8], c[7]  # across the boundary of levels 0 and 1: the multiset of colours is unchanged
    rejected("two samples of a pixel swapped across a level boundary", swapped)
    exchanged = c.copy()
    exchanged[3] = np.roll(c[3], 1, axis=1)  # sample 3 of every pixel is its left neighbour's
    rejected("two pixels' samples exchanged", exchanged)
    with pytest.raises(sa.AuditError) as e:  # a frame whose level sums were added last level first
        sa.check_fold(sa.fold(lv[::-1], c), lv, c, "the levels added in reverse order")
    print(str(e.value)[:160])
    assert "pixels are not the fold" in str(e.value)
    with pytest.raises(sa.AuditError):  # (and the same samples cut into other levels)
        sa.check_fold(full, [(0, 12), (12, 12)], c)
    ulp = c.copy()
    ulp[11] = np.nextafter(c[11], 2.0)
    rejected("one sample 1 ulp off", ulp)
    # the sums alone would not tell: dropped-and-duplicated frames keep their sample count, and the swap keeps every colour
    assert np.allclose(sa.fold(lv, swapped), full, rtol=1e-12)


def test_the_census_classes():
    b = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    a = b.copy()
    a[1, 2] = np.nextafter(0.5, 1)  # other bits, still close
    a[2, 0] = 0.5 * (1 + 1e-8)      # tight, not loose
    a[3, 1] = 2e-3                  # tight and loose
    a[4, 2] = np.nan                # tight and loose
    cen = sa.census(a, b)
    assert (cen.n, cen.equal, cen.tight, cen.loose) == (5, 1, 3, 2)
    assert cen.tight_mask.tolist() == [False, False, True, True, True]
    assert cen.loose_mask.tolist() == [False, False, False, True, True]
    assert sa.census(np.array([[-0.0, 0, 0]]), np.zeros((1, 3))).equal == 0  # bits, not values


# ------------------------------------------------------------------------------------------ contraction census ---
@pytest.mark.parametrize("name", ["cover", "cover_moving", "suzanne"])
def test_contraction_alone_moves_no_sample_far(name):
    """The contracted oracle against the oracle, sample by sample, on the frames of the GPU comparison (seed 7): FMA
    contraction with no other change moves some samples of the cover scene beyond rtol 1e-9 — amplification through
    specular bounces — and none beyond 1e-3; the segment totals are the same.  Measured (g++ -O3): static cover 70
    tight of 921,600, moving cover 83, suzanne 0; largest |difference| 9.7e-8."""
    cen, seg, fseg = sa.reference_census(name)
    print(f"{name}: {cen.n} samples, equal bits {cen.equal}, tight {cen.tight}, loose {cen.loose}, "
          f"max |d| {cen.max_abs:.3g}, segments {seg} / {fseg}")
    assert cen.n == 921_600
    assert cen.loose == 0
    assert cen.equal < cen.n  # the second build is contracted: it is not the oracle again
    assert abs(fseg - seg) <= 1e-5 * seg


def test_no_fma_is_an_error_not_a_skip(monkeypatch):
    monkeypatch.setattr(sa, "host_has_fma", lambda: False)
    monkeypatch.setattr(sa, "_contracted", None)
    with pytest.raises(RuntimeError, match="FMA"):
        sa.contracted_oracle()
