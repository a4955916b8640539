"""Swept-sphere queries, host side (no GPU): the entry points and layouts, the argument errors that need no device, and
the numpy mirror of the kernel's formulas (sweep_ref.py) against the exact segment distances through check_answers — on
hand-placed sweeps around one primitive of each class, on 2,000 random sweeps against the hand scene and its triangles
alone, on suzanne — with the measured worst residual in units of u S (the figure of DESIGN §4.19), the cap on open
queries, start_overlap against point_ref's mirror, the tie rule, and corrupted answers, each of which the checker must
reject.  Then the sweeps that START AT CONTACT (the next stage of a continuous-collision loop: sweep_cases.contact_sets),
the far copies of the hand scene and the unbounded rows: the mirror is refused nowhere, each "starts outside" guard of
the earlier rule put back alone (sweep_ref.GUARDS) is refused somewhere, every "into" sweep is decided by the exact
distance alone, and the two wrong answers the earlier rule gave are rejected."""
import functools
import ctypes as C
import re

import numpy as np
import pytest

import point_ref as pr
import rtow
import sweep_cases as sc
import sweep_ref as sr
from conftest import REPO
from support_scenes import SMALL


def test_sweep_symbols_are_exported_and_declared():
    L = rtow.lib()
    header = (REPO / "include" / "rtow.h").read_text()
    for name in ("rtow_sweep", "rtow_sweep_device"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert L.rtow_abi_version() == 9


def test_layouts_match_the_header():
    assert C.sizeof(rtow.SweepQuery) == 80 and C.sizeof(rtow.SweepHit) == 80
    want_q = {"origin": 0, "time": 24, "direction": 32, "tmax": 56, "radius": 64, "pad_": 72}
    want_h = {"t": 0, "dist": 8, "centre": 16, "point": 40, "prim": 64, "kind": 68, "material": 72, "start_overlap": 76}
    for cls, dts, want in ((rtow.SweepQuery, (rtow.SWEEP_QUERY_DTYPE, sr.QUERY_DTYPE), want_q),
                           (rtow.SweepHit, (rtow.SWEEP_HIT_DTYPE, sr.HIT_DTYPE), want_h)):
        for dt in dts:
            assert dt.itemsize == 80 and set(dt.names) == set(want)
            for name, off in want.items():
                assert getattr(cls, name).offset == off and dt.fields[name][1] == off, name
    q = rtow.make_sweeps([[1, 2, 3]], [[0, 0, 1]], 0.5, time=0.25, tmax=2.0)
    assert q.tobytes() == sr.make_sweeps([[1, 2, 3]], [[0, 0, 1]], 0.5, 0.25, 2.0).tobytes()


def test_argument_errors_that_need_no_device():
    L = rtow.lib()
    q = rtow.make_sweeps([[0, 0, 0]], [[0, 0, 1]], 0.1)
    out = np.zeros(1, dtype=rtow.SWEEP_HIT_DTYPE)
    out["t"] = 7.0
    rc = L.rtow_sweep(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, q.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p), None)
    assert rc == rtow.RTOW_EINVAL and b"NULL" in L.rtow_last_error() and out["t"][0] == 7.0
    assert L.rtow_sweep_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, None, 0, None, None, None) == rtow.RTOW_EINVAL


# ---------------------------------------------------------------------------------- the mirror against the exact ---
CONTACT = ("hand", "hand_mesh", "suzanne", "far1e5", "far1e7")  # the scenes of the sets "<scene>_contact"
UNBOUNDED = ("hand", "hand_mesh", "suzanne")                     # ... and of "<scene>_unbounded"
EXTRA = {}  # set name -> (resting id per sweep, decided "into" rows) of a contact set


@functools.lru_cache(maxsize=None)
def _sets():
    """name -> (records, materials, sweeps): the hand-placed sweeps, the random sets, the sweeps at contact and the
    unbounded (tmax = +inf) rows of the sets the GPU tests hold the strict build to."""
    hand, mesh = sc.hand_records(), sc.hand_records(True)
    G = SMALL["suzanne"]
    suz = pr.make_records(G.sph, G.mov, G.tri)
    out = {"placed": hand + (sc.placed_sweeps(),), "hand": hand + (sc.random_sweeps(hand[0], 2000, 3),),
           "hand_mesh": mesh + (sc.random_sweeps(mesh[0], 2000, 3),), "suzanne": (suz, G.pmat, sc.random_sweeps(suz, 600, 31))}
    scenes = {"hand": hand, "hand_mesh": mesh, "suzanne": (suz, G.pmat)}
    scenes.update({k: sc.hand_records(False, off) for k, off in sc.FAR_OFFSETS.items()})
    for name in CONTACT:
        rec, mats = scenes[name]
        q, rest, into = sc.contact_sets(name, rec, lambda x: sr.answers(rec, mats, x))  # noqa: B023
        out[name + "_contact"] = (rec, mats, q)
        EXTRA[name + "_contact"] = (rest, into)
    for name in UNBOUNDED:
        rec, mats = scenes[name]
        q = sc.strict_sets(rec)
        out[name + "_unbounded"] = (rec, mats, q[np.isinf(q["tmax"]) & ~sr.skipped(q)])
    return out


_DONE = {}


def _mirror_case(name):
    """The mirror's answers to a set pass check_answers at the strict band (once per set); the figures are printed.
    Returns (answers, statistics, worst contact residual in u S)."""
    if name not in _DONE:
        rec, mats, q = _sets()[name]
        h = sr.answers(rec, mats, q)
        assert not any(np.isnan(h[f]).any() for f in ("t", "dist", "centre", "point"))
        ck = sr.Checker(rec, mats, q)
        s = ck.check(h, "strict", name)
        worst = s["worst_contact"] * sr.K["strict"]
        print(f"{name}: {sr.stats_line(s)}; worst contact residual {worst:.2f} u S")
        assert s["filter_worst"] <= sr.FILTER_U
        _DONE[name] = (h, s, worst, ck)
    return _DONE[name]


def test_mirror_on_the_hand_placed_sweeps():
    h, s = _mirror_case("placed")[:2]
    assert s["hits"] == s["queries"]  # (what passes everything else reaches the inner side of the large sphere)
    assert s["open"] <= 8  # (only the exact tangencies are open, by construction)


@pytest.mark.parametrize("name", ["hand", "hand_mesh", "suzanne"])
def test_mirror_on_random_sweeps(name):
    h, s = _mirror_case(name)[:2]
    assert 0.2 * s["queries"] < s["hits"] < s["queries"]
    assert s["open"] <= 0.02 * s["queries"], (name, s["open"])  # the cap on open queries


def test_the_band_leaves_a_factor_four_over_the_measured_worst():
    """K_strict >= 4 x the mirror's worst residual over all the sets; K_fast = 2 K_strict."""
    names = ("placed", "hand", "hand_mesh", "suzanne") + tuple(n + "_contact" for n in CONTACT) + tuple(n + "_unbounded" for n in UNBOUNDED)
    worst = max(_mirror_case(name)[2] for name in names)
    print(f"worst contact residual of the mirror over all sets: {worst:.2f} u S; K_strict = {sr.K['strict']}")
    assert sr.K["strict"] >= 4.0 * worst and sr.K["fast"] == 2 * sr.K["strict"]


def test_start_overlap_is_the_point_mirror_at_the_origin():
    rec, mats = sc.hand_records()
    q = np.concatenate([sc.placed_sweeps(), sc.random_sweeps(rec, 2000, 3, finite=False)])
    h = sr.answers(rec, mats, q)
    dmin = pr.nearest(rec, q["origin"], q["time"])[0]
    live = ~sr.skipped(q)
    assert np.array_equal(h["start_overlap"][live] == 1, dmin[live] <= q["radius"][live])
    assert np.all(h["t"][h["start_overlap"] == 1] == 0.0) and h["start_overlap"].sum() > 50


def test_skipped_sweeps_get_the_miss_record():
    rec, mats = sc.hand_records()
    q = sc.skipped_sweeps()
    assert np.array_equal(sr.skipped(q), np.arange(len(q)) < len(q) - 1)
    h = sr.answers(rec, mats, q)
    assert np.all(h["prim"][:-1] == -1) and np.all(np.isinf(h["t"][:-1])) and h["prim"][-1] >= 0
    finite = q.copy()
    finite["tmax"] = np.where(np.isfinite(q["tmax"]), q["tmax"], 5.0)
    sr.check_answers(rec, mats, finite, sr.answers(rec, mats, finite), "strict", "skipped")


def test_the_tie_rule_names_the_lowest_insertion_index():
    for rec, mats, q, want in sc.tie_cases():
        h = sr.answers(rec, mats, q)
        assert np.all(h["prim"] == want), (h["prim"], want)
        assert np.all(h["t"] > 0) and np.all(h["start_overlap"] == 0)
        full = sr.pair_times(rec, q)
        for i in range(len(q)):  # (a real tie: two primitives at exactly the winning t)
            assert (full[2][full[0] == i] == h["t"][i]).sum() == 2, i


def test_the_checker_rejects_corrupted_answers():
    rec, mats = sc.hand_records()
    q = sc.random_sweeps(rec, 300, 7)
    good = sr.answers(rec, mats, q)
    ck = sr.Checker(rec, mats, q)
    ck.check(good, "fast", "good")
    hit = np.nonzero((good["prim"] >= 0) & (good["t"] > 0))[0]
    miss = np.nonzero(good["prim"] < 0)[0]
    assert len(hit) > 20 and len(miss) > 20

    def corrupt(i, **fields):
        bad = good.copy()
        for f, v in fields.items():
            bad[f][i] = v
        with pytest.raises(AssertionError):
            ck.check(bad, "fast", "corrupted")

    i, j = int(hit[0]), int(hit[1])
    later = good[i].copy()
    corrupt(i, t=good["t"][i] * (1 + 1e-9), centre=q["origin"][i] + q["direction"][i] * (good["t"][i] * (1 + 1e-9)))
    corrupt(i, t=good["t"][i] * (1 - 1e-9), centre=q["origin"][i] + q["direction"][i] * (good["t"][i] * (1 - 1e-9)))
    corrupt(i, t=np.inf, dist=np.inf, centre=0.0, point=0.0, prim=-1, kind=-1, material=-1)  # a hit turned into a miss
    corrupt(i, point=good["point"][i] + 1e-9)
    corrupt(i, dist=good["dist"][i] * (1 + 1e-9))
    corrupt(i, kind=(good["kind"][i] + 1) % 3)
    corrupt(i, start_overlap=1)
    corrupt(int(miss[0]), t=0.5 * q["tmax"][miss[0]], dist=q["radius"][miss[0]], prim=good["prim"][j],
            kind=good["kind"][j], material=good["material"][j],
            centre=q["origin"][miss[0]] + q["direction"][miss[0]] * (0.5 * q["tmax"][miss[0]]))  # a miss turned into a hit
    corrupt(int(miss[0]), start_overlap=1)
    assert later.tobytes() == good[i].tobytes()


# --------------------------------------------------------------------------------- sweeps that start at contact ---
@pytest.mark.parametrize("name", [n + "_contact" for n in CONTACT])
def test_mirror_on_sweeps_that_start_at_contact(name):
    """No refusal on any chained, aimed, hand-made, pinned or far sweep.  `open` is large here by construction (a
    primitive is at rho from the start of every segment) and relaxes nothing, so it has no cap."""
    h, s = _mirror_case(name)[:2]
    rest, into = EXTRA[name]
    assert 0.5 * s["queries"] < s["hits"] and len(rest) == len(into) == s["queries"] and into.sum() >= 80
    if name == "hand_contact":  # the contract's t == 0 without the overlap flag occurs: a rest the overlap test did not see
        assert np.any((h["t"] == 0.0) & (h["start_overlap"] == 0) & (h["prim"] >= 0))


@pytest.mark.parametrize("name", [n + "_unbounded" for n in UNBOUNDED])
def test_mirror_on_unbounded_sweeps(name):
    """The tmax = +inf rows of the strict sets of test_gpu_sweep.py: a miss is checked up to the horizon T."""
    h, s = _mirror_case(name)[:2]
    rec, mats, q = _sets()[name]
    miss = np.nonzero(h["prim"] < 0)[0]
    assert s["queries"] > 400 and (len(miss) > 20 or name == "hand_unbounded")  # (inside the R = 40 sphere nothing escapes)
    ck = _mirror_case(name)[3]
    for i in miss[:50]:  # the horizon is a power of two, beyond the box on the axis it names, and no smaller one is
        T, k = ck.horizon(int(i), "strict")
        lo, hi, _ = ck.scene_bounds(float(q["time"][i]))
        o, d = q["origin"][i], q["direction"][i]
        end = sr._F(o[k]) + T * sr._F(d[k])
        assert end > hi[k] + sr._F(q["radius"][i]) if d[k] > 0 else end < lo[k] - sr._F(q["radius"][i])
        half = sr._F(o[k]) + T / 2 * sr._F(d[k])
        assert not (half > hi[k] + sr._F(q["radius"][i]) + 1 if d[k] > 0 else half < lo[k] - sr._F(q["radius"][i]) - 1)


@pytest.mark.parametrize("guard", sr.GUARDS)
def test_each_guard_of_the_earlier_rule_is_refused(guard):
    """The earlier rule's "starts outside" test of one piece put back into the mirror (sweep_ref.GUARDS): at least one
    sweep of the committed contact sets is then answered in a way the exact checker refuses — the piece the sweep rests
    on is dropped and it passes through, or meets the same primitive later through another piece."""
    refused, differ, shapes = 0, 0, set()
    for name in (n + "_contact" for n in CONTACT):
        rec, mats, q = _sets()[name]
        good, _, _, ck = _mirror_case(name)
        mut = sr.answers(rec, mats, q, old=(guard,))
        for i in np.nonzero([good[j].tobytes() != mut[j].tobytes() for j in range(len(q))])[0]:
            differ += 1
            bad = good.copy()
            bad[i] = mut[i]
            try:
                ck.check(bad, "strict", guard)
            except AssertionError as e:
                refused += 1
                shapes.add(str(e).rsplit("('", 1)[-1].split("'")[0])
    print(f"guard {guard}: {differ} answers differ, {refused} refused: {sorted(shapes)}")
    assert refused >= 1, (guard, differ)


def test_every_into_sweep_is_decided_by_the_exact_distance():
    """On the reference alone: from a rest, a sweep towards the contact point comes closer than rho - band (the fast
    build's, the wider) to the primitive it rests on within [o, p(tmax)], so neither a miss nor a hit beyond that can be
    excused as open — and the mirror answers every one with a hit."""
    total = 0
    for name in (n + "_contact" for n in CONTACT):
        rec, mats, q = _sets()[name]
        good, _, _, ck = _mirror_case(name)
        rest, into = EXTRA[name]
        for i in np.nonzero(into)[0]:
            i, c = int(i), int(rest[i])
            o, d, tmax = sr._fr3(q["origin"][i]), sr._fr3(q["direction"][i]), sr._F(q["tmax"][i])
            D, e = ck.seg(i, c, ("tmax", "decided"), [o[k] + tmax * d[k] for k in range(3)])
            band = sr.K["fast"] * sr._F(sr.U) * ck.scale(i, float(q["tmax"][i]), c)
            assert D + e < sr._F(q["radius"][i]) - band, (name, i, float(D), float(q["radius"][i]))
            assert good["prim"][i] >= 0, (name, i)
            total += 1
    assert total > 800, total


def test_the_checker_rejects_the_two_wrong_answers_at_contact():
    """The shapes the earlier rule produced on a chained "into" sweep: the resting primitive replaced by a later hit on
    another primitive, and a miss."""
    rec, mats, q = _sets()["hand_contact"]
    good, _, _, ck = _mirror_case("hand_contact")
    rest, into = EXTRA["hand_contact"]
    qi, cid, t, ov = sr.pair_times(rec, q)
    done = 0
    for i in np.nonzero(into)[0]:
        m = (qi == i) & (t <= q["tmax"][i]) & (t > good["t"][i] + 0.05) & (cid != rest[i])
        if rec.ins2cls[good["prim"][i]] != rest[i] or not m.any():
            continue
        j = np.nonzero(m)[0][np.argmin(t[m])]
        later = good.copy()
        centre = q["origin"][i] + q["direction"][i] * t[j]
        dist, point = pr.prim_point(rec, cid[j:j + 1], centre[None], q["time"][i:i + 1])
        ins = rec.cls2ins[cid[j]]
        later[i] = (t[j], dist[0], centre, point[0], ins, rec.kind_of(cid[j]), mats[ins], 0)
        miss = good.copy()
        miss[i] = (np.inf, np.inf, 0.0, 0.0, -1, -1, -1, 0)
        for bad in (later, miss):
            with pytest.raises(AssertionError, match="within rho - band of the travelled segment"):
                ck.check(bad, "fast", "corrupted")
        done += 1
        if done == 5:
            break
    assert done == 5
