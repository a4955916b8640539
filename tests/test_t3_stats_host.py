"""Self-tests of the device T3's statistic (tests/t3_stats.py), no GPU: the proof that the checker passes what it must
and can fail.

Null cases, on the three scenes at 60x40 (tests/t3_ref.py): the Philox oracle at 16 x 1024 spp against the reference's
mt19937 stream at 16 x 256, and a second mt19937 set against the first.  Mutants: seven planted faults on the Philox
oracle's batches, each refused with the condition that is meant to see it.  The measured figures are printed (-s).
The mt19937 batches are computed once per scene (t3_ref.mt_stream caches them); the whole module takes about two minutes.
"""
import numpy as np
import pytest

import orc
import t3_ref as tr
import t3_stats as ts


def null(kind, which):
    if which == "philox":
        return tr.philox_batches(kind), tr.ORACLE_SPP
    return tr.mt_second(kind), tr.MT_SPP


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("which", ["philox", "mt_second"])
def test_null_cases_pass(kind, which):
    dev, spp = null(kind, which)
    fig = ts.check(tr.mt_batches(kind), dev, f"{kind}, {which} against mt19937", tr.MT_SPP, spp)
    print(ts.describe(f"{kind} {which}", fig))
    assert fig["det_share"] <= ts.DET_CAP
    # the batches' variances are in the ratio of their sample counts (a loose check of the set-up, not of the estimator:
    # the pooled ratio of 6,000+ variances of 15 degrees of freedom each is good to a few per cent)
    assert 0.85 < fig["r"] * spp / tr.MT_SPP < 1.15, fig["r"]


def test_the_second_mt19937_set_starts_where_the_first_ended():
    """mt_second burns the number of doubles the first set's renders report: the stream is then at the double the first
    set would have drawn next — the two sets share no draw."""
    _, draws, nxt = tr.mt_stream("static")
    tr.oracle_scene("static", draws)
    assert orc.lib().orc_mt_random_double(0.0, 1.0) == nxt


def test_a_displaced_stream_is_refused_once_it_meets_the_first():
    """What the lower band is for, found with it: the moving cover's stream displaced by 12,345 draws meets the first
    one in batch 11 and repeats it from there on."""
    kind = "moving"
    a = tr.mt_batches(kind)
    b = tr.mt_stream(kind, 12345)[0]
    same = [bool(np.array_equal(a[i], b[i])) for i in range(tr.B)]
    assert same == [False] * 12 + [True] * 4
    with pytest.raises(ts.T3Error) as e:
        ts.check(a, b, "moving, displaced stream", tr.MT_SPP, tr.MT_SPP)
    assert "mean F low" in e.value.conditions, e.value


def refused(kind, dev, name, want):
    with pytest.raises(ts.T3Error) as e:
        ts.check(tr.mt_batches(kind), dev, f"{kind}, {name}", tr.MT_SPP, tr.ORACLE_SPP)
    err = e.value
    print(f"{kind}, {name}: refused by {sorted(set(err.conditions))}; mean F {err.figures['mean_f']:.3f}, max F "
          f"{err.figures['max_f']:.1f}, |diff| / SE {[f'{v:.1f}' for v in err.figures['ratio']]}")
    assert want in err.conditions, (want, str(err))
    assert f"{kind}, {name}" in str(err) and want in str(err)
    return err


def typical_pixel(ref, dev, bound):
    """The pixel of median sensitivity, pixels ranked by the F that x 1.05 alone gives their most sensitive channel; and
    the share of pixels where that F is beyond `bound`."""
    se2 = ref.var(axis=0, ddof=1) / ts.B + dev.var(axis=0, ddof=1) / ts.B
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.nan_to_num((0.05 * dev.mean(axis=0)) ** 2 / se2, posinf=np.inf).max(axis=-1)
    order = np.argsort(f, axis=None)
    return np.unravel_index(order[order.size // 2], f.shape), float((f > bound).mean())


@pytest.mark.parametrize("kind", tr.KINDS)
def test_mutants_are_refused(kind):
    ref, dev = tr.mt_batches(kind), tr.philox_batches(kind)
    fig = ts.check(ref, dev, kind, tr.MT_SPP, tr.ORACLE_SPP)
    # the whole image 0.1 % too bright: 9-12 SE on the image means
    refused(kind, dev * (1.0 + 1e-3), "image x (1 + 1e-3)", "image mean")
    z = dev.copy()
    z[..., 0] += 0.1 / 255
    err = refused(kind, z, "red + 0.1 / 255", "image mean (absolute)")
    assert all("channel R" in part for part in str(err).split("; ") if part.startswith("image mean"))
    z = dev.copy()
    z[:, 24:31, 20:27] *= 1.03
    err = refused(kind, z, "a 7 x 7 block x 1.03", "mean F high")
    (i, j), share = typical_pixel(ref, dev, fig["max_f_bound"])
    print(f"{kind}: x 1.05 on one pixel alone is beyond the largest-F bound on {share:.2f} of the pixels; the median "
          f"pixel is ({i}, {j})")
    z = dev.copy()
    z[:, i, j] *= 1.05
    err = refused(kind, z, "one pixel x 1.05", "max F")
    assert f"pixel (row {i}, column {j})" in str(err)
    # a term without spread on either side, moved by 1e-6
    tol = ts.FLOOR * np.maximum(np.abs(ref.mean(axis=0)), ts.FLOOR_SCALE)
    quiet = np.argwhere((np.ptp(ref, axis=0) < tol) & (np.ptp(dev, axis=0) < tol))
    assert len(quiet) >= 80
    i, j, c = quiet[len(quiet) // 2]
    z = dev.copy()
    z[:, i, j, c] += 1e-6
    err = refused(kind, z, "one deterministic term + 1e-6", "deterministic")
    assert f"pixel (row {i}, column {j}) channel {ts.CHANNELS[c]}" in str(err) and err.conditions == ["deterministic"]
    # closer than independent samples can be: the reference itself, and half of it
    err = refused(kind, ref, "the reference as the device image", "mean F low")
    assert err.conditions == ["mean F low"]
    refused(kind, 0.5 * (ref + dev), "the mean of reference and device", "mean F low")
    # sixteen copies of one batch: the device's variance is gone, its noise is not
    refused(kind, np.repeat(dev[:1], ts.B, axis=0), "sixteen copies of one batch", "mean F high")


def test_odd_samples_in_a_term_the_reference_saw_none_in():
    """Condition 1b: a device batch may hold samples the reference's 4,096 never showed, up to the bound — and not beyond."""
    kind = "static"
    ref, dev = tr.mt_batches(kind), tr.philox_batches(kind)
    fig = ts.check(ref, dev, kind, tr.MT_SPP, tr.ORACLE_SPP)
    assert fig["odd_terms"] > 0 and fig["odd_max"] < fig["odd_bound"]  # (the cover has such silhouette pixels)
    bound = ts.odd_sample_bound(16 * 256, 16 * 1024, 7200)
    assert fig["odd_bound"] == bound and 7.0e-3 < bound < 7.5e-3
    assert 5.5e-3 < ts.odd_sample_bound(4096, 65536, 7200) < 5.7e-3
    tol = ts.FLOOR * np.maximum(np.abs(ref.mean(axis=0)), ts.FLOOR_SCALE)
    i, j, c = np.argwhere((np.ptp(ref, axis=0) < tol) & (np.ptp(dev, axis=0) < tol))[0]
    z = dev.copy()
    z[3, i, j, c] -= 16 * 0.9 * bound  # one batch off: the device mean moves by 0.9 of the bound
    ts.check(ref, z, kind, tr.MT_SPP, tr.ORACLE_SPP)
    z[3, i, j, c] -= 16 * 0.2 * bound
    with pytest.raises(ts.T3Error) as e:
        ts.check(ref, z, kind, tr.MT_SPP, tr.ORACLE_SPP)
    assert e.value.conditions == ["deterministic (odd samples)"]


def test_the_checker_refuses_what_it_has_no_quantile_for():
    a = np.zeros((16, 40, 61, 3))
    with pytest.raises(ValueError):
        ts.check(a, a, "61 columns", 1, 1)
    with pytest.raises(ValueError):
        ts.check(a[:8, :, :60], a[:8, :, :60], "8 batches", 1, 1)


def test_quantiles_are_scipys():
    st = pytest.importorskip("scipy.stats")
    assert ts.Z == pytest.approx(st.norm.isf(ts.ALPHA / 2), rel=1e-12)
    for k, nu in enumerate(ts.NU):
        assert ts.T_MEANS[k] == pytest.approx(st.t.isf(ts.ALPHA / 3 / 2, nu), abs=1e-6)
        assert ts.T_MAXF[k] == pytest.approx(st.t.isf(ts.ALPHA / ts.T_MAXF_TERMS / 2, nu), abs=1e-6)
        assert ts.T_MAXF[k] ** 2 == pytest.approx(st.f.isf(ts.ALPHA / ts.T_MAXF_TERMS, 1, nu), rel=1e-6)
    # between the table's entries: linear interpolation is within 1e-3, on the generous side
    for nu in np.arange(15.25, 30.0, 0.25):
        for table, p in ((ts.T_MEANS, ts.ALPHA / 6), (ts.T_MAXF, ts.ALPHA / ts.T_MAXF_TERMS / 2)):
            got, want = ts.t_quantile(table, nu), st.t.isf(p, nu)
            assert want * (1 - 1e-6) <= got <= want * (1 + 1e-3), (nu, got, want)
    # the moments of F(1, nu)
    for nu in (15.0, 16.9, 22.1, 30.0):
        e, v = ts.f_moments(nu)
        assert e == pytest.approx(st.f.mean(1, nu), rel=1e-12) and v == pytest.approx(st.f.var(1, nu), rel=1e-12)
