"""Self-tests of the guide-buffer checker (tests/guides_exact.py), no GPU.

The buffer under test is the oracle's: the logged primaries of the three guide scenes (support_oracle.logged_render /
primaries), the oracle's own hit test on them (the hittable list's closest hit: the log's t_hit, with the record of
support_scenes.SceneView.oracle_hit; support_oracle.brute_force on a sample of the rays confirms the shortcut below), the
oracle's sky (summed, the oracle's image bit for bit), folded by guides_ref.fold_guides.  The checker must accept it under
STRICT and under FAST with the widened band, stay inside the 1 % cap on undecided pixels, and reject every planted fault
with the right pixel and field.
"""
import math

import numpy as np
import pytest

import guides_exact as gx
import rtow
from guides_ref import CAP, SCENES, Logged, Parts, fold_guides, guide_values, within_cap
from support_oracle import brute_force, same_bits, sky_of_strict, sum_in_order
from support_scenes import SceneView

BUILDS = [gx.STRICT, gx.FAST]


def oracle_hits(view, lg):
    """The oracle's closest hit of every logged primary as HIT_DTYPE records.  The log holds the hittable list's answer
    (t_hit and the class index of the primitive); the record comes from the oracle's hit test on the at most three
    inserted primitives with that class index, the interval shrinking as in brute_force, and must reproduce t_hit."""
    out = np.zeros(len(lg.rays), dtype=rtow.HIT_DTYPE)
    out["t"], out["prim"], out["kind"], out["material"] = math.inf, -1, -1, -1
    by_index = {}
    for p, i in enumerate(view.index):
        by_index.setdefault(int(i), []).append(p)
    t_log, cls = lg.log[:, 10], lg.log[:, 11]
    for j in np.nonzero(np.isfinite(t_log))[0]:
        r = lg.rays[j]
        best, tmax = None, math.inf
        for p in by_index[int(cls[j])]:
            h = view.oracle_hit(p, r["origin"], r["direction"], r["time"], tmax=tmax)
            if h is not None:
                best, tmax = (p, h), h[0]
        assert best is not None and same_bits(best[1][0], t_log[j]), j
        p, (t, pt, n, front) = best
        out[j] = (t, pt, n, p, view.kind[p], view.prim_mat[p], front)
    return out


def oracle_sky(rays):
    """ray_color's miss branch in binary64, the oracle's operand order: unit = d * (1 / sqrt(d.d))."""
    return sky_of_strict(rays["direction"])


class Case:
    def __init__(self, name):
        self.lg = lg = Logged(*SCENES[name])
        self.parts = Parts(lg.scene)
        view = SceneView(lg.scene)
        self.hits = oracle_hits(view, lg)
        self.hit = np.isfinite(self.hits["t"])
        self.sky_all = oracle_sky(lg.rays)
        # the pieces are the oracle's: the image is the sky over the misses, a sample of the rays is the brute force's
        assert same_bits(sum_in_order(self.sky(self.hit), lg.spp), lg.image)
        some = np.random.default_rng(3).choice(len(lg.rays), 12, replace=False)
        want = brute_force(view, lg.rays[some])
        for f in rtow.HIT_DTYPE.names:
            assert same_bits(self.hits[f][some].astype(np.float64), want[f].astype(np.float64)), f
        self.refs = {b: self.parts.reference(lg.rays, lg.ids, lg.spp, b) for b in BUILDS}

    def sky(self, hit):
        return np.where(hit[:, None], 0.0, self.sky_all)

    def fold(self, hits=None, rays=None):
        hits = self.hits if hits is None else hits
        g = fold_guides(self.lg.rays if rays is None else rays, hits, self.sky(np.isfinite(hits["t"])), self.parts.att,
                        self.lg.spp)
        return guide_values(g).reshape(-1, 8).copy()

    def quiet_pixels(self, ref):
        """Decided pixels all of whose samples hit, both neighbours in the row included, with a depth bound far below
        1e-9 of the depth: where every mutant below must show."""
        spp, w = self.lg.spp, self.lg.w
        dec = ref.decided.reshape(-1, spp).all(axis=1) & ref.hit.reshape(-1, spp).all(axis=1)
        tight = (ref.bound[:, 6] < 1e-11 * ref.value[:, 6]).reshape(-1, spp).all(axis=1)
        ok = dec & tight
        both = ok & np.roll(ok, -1) & (np.arange(len(ok)) % w < w - 1)
        return np.nonzero(both)[0]


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracles_buffer_passes_within_the_cap(name, build):
    c = case(name)
    ref = c.refs[build]
    stats = ref.check(c.fold(), (name, build))
    within_cap((name, build), stats)
    n_pix, und_pix, und_samples, share = ref.counts()
    # the logged primaries stay far inside the cap, and the exact hit / miss answers are the oracle's
    assert und_pix <= CAP * n_pix and und_samples <= CAP * len(c.lg.rays)
    assert np.array_equal(ref.hit[ref.decided], c.hit[ref.decided])
    assert 0.5 < share < 0.99


def passes_the_distance_test(fast, strict, spp):
    """The thresholds of test_gpu_guides.test_fast_guides_against_strict, `strict` in the strict build's place."""
    fast, strict = fast.copy(), strict.copy()
    if not (np.isfinite(fast).all() and np.isfinite(strict).all()):
        return False
    scale = np.where(strict[:, 7] > 0, strict[:, 6], 1.0)
    fast[:, 6] /= scale
    strict[:, 6] /= scale
    mean = np.abs(fast - strict).mean() / spp
    return bool(mean <= 2e-3 and np.isclose(fast, strict, rtol=1e-9, atol=1e-12).all(axis=-1).mean() > 0.97)


def rejected(ref, buf, pixels, field, clean=None):
    """The checker rejects `buf`; every failure is in `pixels` and one of them names `field`.  clean: the unmutated
    buffer — the distance test of the fast guides against the strict ones does not see the fault."""
    if clean is not None:
        assert passes_the_distance_test(buf, clean, ref.spp)
    with pytest.raises(gx.CheckError) as e:
        ref.check(buf, "mutant")
    got = [(f["pixel"], f["field"]) for f in e.value.failures]
    assert all(p in pixels for p, _ in got), (got, pixels)
    assert any(f == field for _, f in got), (got, field)
    assert "got" in str(e.value) and "expected" in str(e.value) and "bound" in str(e.value)
    return got


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_planted_faults_are_rejected(name, build):
    c = case(name)
    ref, lg = c.refs[build], c.lg
    spp = lg.spp
    quiet = c.quiet_pixels(ref)
    assert len(quiet) > 20
    p = int(quiet[len(quiet) // 2])  # (the full image, one rank: the global pixel is the buffer's index)
    assert int(lg.ids[p * spp, 0]) == p
    i = p * spp + 1                  # its second sample
    clean = c.fold()

    def rej(buf, pixels, field):  # (... and the fast-against-strict distance test would let every one of them pass)
        return rejected(ref, buf, pixels, field, clean)

    # one sample's hit turned into a miss
    h = c.hits.copy()
    h[i] = (math.inf, (0, 0, 0), (0, 0, 0), -1, -1, -1, 0)
    got = rej(c.fold(h), {p}, "hits")
    assert {f for _, f in got} >= {"hits"}

    # one hit's albedo taken from another material
    h = c.hits.copy()
    other = [m for m in range(len(c.parts.att)) if not np.array_equal(c.parts.att[m], c.parts.att[h["material"][i]])]
    if other:  # (suzanne has one material)
        h["material"][i] = other[0]
        rej(c.fold(h), {p}, "albedo")
    else:
        buf = c.fold()
        buf[p, 0:3] = buf[p, 0:3] - c.parts.att[h["material"][i]] + np.array([0.25, 0.5, 0.75])
        rej(buf, {p}, "albedo")

    # one normal negated (a sphere's on the cover scenes, a triangle's on suzanne)
    h = c.hits.copy()
    h["normal"][i] = -h["normal"][i]
    assert (h["kind"][i] == rtow.PRIM_TRIANGLE) == (name == "suzanne")
    rej(c.fold(h), {p}, "normal")

    # one depth scaled by 1 + 1e-9
    h = c.hits.copy()
    h["t"][i] *= 1 + 1e-9
    got = rej(c.fold(h), {p}, "depth")
    assert {f for _, f in got} == {"depth"}

    # the values of two neighbouring pixels swapped
    buf = c.fold()
    buf[[p, p + 1]] = buf[[p + 1, p]]
    got = rej(buf, {p, p + 1}, "depth")  # (two pixels of one flat triangle share the normal)
    assert {q for q, _ in got} == {p, p + 1}

    # one pixel's samples folded with a sample of the next pixel
    h, r = c.hits.copy(), lg.rays.copy()
    h[i], r[i] = c.hits[i + spp], lg.rays[i + spp]
    rej(c.fold(h, r), {p}, "depth")

    # hits off by one
    for delta in (1.0, -1.0):
        buf = c.fold()
        buf[p, 7] += delta
        got = rej(buf, {p}, "hits")
        assert {f for _, f in got} == {"hits"}


def test_an_undecided_sample_gets_the_weak_checks_only():
    """A pixel with an undecided sample: any hit count the band allows passes, whatever the sums; a count outside it, a
    non-finite value, a negative depth or an albedo above spp does not."""
    c = case("cover")
    ref = c.parts.reference(c.lg.rays, c.lg.ids, c.lg.spp, gx.FAST)
    p = int(c.quiet_pixels(ref)[0])
    spp = c.lg.spp
    ref.decided = ref.decided.copy()
    ref.decided[p * spp] = False
    buf = c.fold()
    buf[p, 3:6] *= 0.9
    buf[p, 6] *= 1.01
    assert ref.check(buf)["undecided_pixels"] == ref.counts()[1] >= 1
    for col, v, field in ((7, spp - 2.0, "hits"), (7, spp - 0.5, "hits"), (6, -1.0, "depth"), (6, math.nan, "depth"),
                          (1, spp + 0.5, "albedo"), (4, 2.0 * spp, "normal")):
        bad = buf.copy()
        bad[p, col] = v
        rejected(ref, bad, {p}, field)
