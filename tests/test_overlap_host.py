"""The box-overlap references against each other, without a GPU: the numpy mirror of the kernel's predicate equals the
exact Fraction reference on every decided pair of every set the GPU tests use, few pairs are undecided, K_strict covers
the mirror's worst residual, paging through the mirror reproduces the full sets, the checker rejects wrong answers, and
the Python side exports what the header declares."""
import re

import numpy as np
import pytest

import overlap_cases as oc
import overlap_ref as ov
import sweep_cases as sc
from conftest import REPO

_CACHE = {}


def records(name):
    if name not in _CACHE:
        if name == "hand":
            _CACHE[name] = sc.hand_records()[0]
        elif name == "lattice":
            _CACHE[name] = oc.lattice_records()
        else:
            import accel_images as ai
            import point_ref as pr
            from support_scenes import SMALL, suzanne_tris

            if name == "big_mixed":
                import big_mixed as bm

                _CACHE[name] = bm.case().rec
            else:
                G = ai.mesh_geometry(suzanne_tris(10)) if name == "mesh96k" else SMALL[name]
                _CACHE[name] = pr.make_records(G.sph, G.mov, G.tri)
    return _CACHE[name]


BIG_SIZES = (0.004, 0.02, 0.08)  # test_gpu_overlap.py's


def random_set(name):
    """The random boxes of the set the GPU tests put to scene `name` (test_gpu_overlap.boxes_of)."""
    rec = records(name)
    if name == "mesh96k":
        return oc.random_boxes(rec, 500, 9, BIG_SIZES)
    if name == "big_mixed":
        return oc.random_boxes(rec, 900, 7, BIG_SIZES)
    fixed = len(oc.placed_boxes()[0]) + len(oc.skipped_boxes()) + len(oc.min_prim_boxes(rec.n))
    return oc.random_boxes(rec, 4097 - fixed, 5)


def both(name, q):
    rec = records(name)
    sets = ov.full_sets(rec, q)
    return rec, sets, ov.Classified(rec, q)


@pytest.mark.parametrize("name", ["hand", "cover_moving", "suzanne", "mesh96k", "big_mixed"])
def test_mirror_equals_the_exact_reference_on_random_boxes(name):
    q = random_set(name)
    rec, sets, ck = both(name, q)
    counts, ids = ov.answers(rec, q, 8, sets)
    for prec in ("strict", "fast"):
        ov.check_answers(ck, counts, ids, 8, prec, (name, prec))
        ov.check_answers(ck, counts, None, 8, prec, (name, prec))
    # the cap: the check above is free in the undecided pairs only, and those are few — of the pairs whose boxes meet
    near = len(ck.r)
    und = ck.undecided(ov.K["fast"])
    print(name, "boxes", len(q), "pairs", ck.n_pairs, "boxes meet", near, "reported", int(counts.sum()), "exact", ck.n_exact, "undecided", und)
    assert counts.sum() > 100 and und <= 0.01 * near and und <= 0.01 * counts.sum()


def test_mirror_equals_the_exact_reference_on_the_placed_boxes():
    q, names = oc.placed_boxes()
    q = np.concatenate([q, oc.skipped_boxes(), oc.min_prim_boxes(40)])
    rec, sets, ck = both("hand", q)
    counts, ids = ov.answers(rec, q, 8, sets)
    ov.check_answers(ck, counts, ids, 8, "strict", "placed")
    got = dict(zip(names, (list(s) for s in sets)))
    ins = rec.cls2ins
    glass, hollow, big, quad = ins[0], ins[1], ins[5], sorted(ins[rec.ns + rec.nm:rec.ns + rec.nm + 2])
    assert got["inside the hollow glass sphere"] == [] and got["inside the glass shell"] == []
    assert got["contains the glass pair"] == sorted([glass, hollow]) == got["crosses the glass surfaces"]
    assert got["touches the glass sphere at a face"] == [glass] == got["a point on the glass sphere"]
    assert big in got["touches the R = 40 sphere with its far corner"] and big not in got["far corner one ulp short of R = 40"]
    assert got["pierced by a triangle, no vertex inside"] == [ins[rec.ns + rec.nm + 2]]
    assert got["in a triangle's bounding box, beside it"] == [] and got["beside the sliver"] == []
    assert got["the sliver"] == [ins[rec.ns + rec.nm + 7]]
    assert got["the collinear triangle"] == [ins[rec.ns + rec.nm + 8]] == got["a point of the collinear triangle"]
    assert got["the point triangle"] == [ins[rec.ns + rec.nm + 9]] == got["the point triangle's point"]
    for name in ("a rectangle in the quad's plane", "a segment in the quad's plane along its diagonal's box", "a point on the quad",
                 "a point on the quad's shared edge"):
        assert got[name] == quad, name
    assert got["a point off the quad"] == [] and len(got["beside the quad's diagonal, in one triangle only"]) == 1
    assert got["crosses R = 40 far out"] == [big] and got["far from the origin 1e7"] == [] == got["far from the origin 1e12"]
    assert len(got["a huge box around everything"]) == rec.n and len(got["a box around the scene inside R = 40"]) == rec.n - 1
    mov = ins[rec.ns]
    for t, start, above, touch in ((0.0, True, False, False), (0.5, True, False, True), (1.0, True, True, True)):
        assert (mov in got[f"the first moving sphere's start, time {t}"]) == start, t
        assert (mov in got[f"above the first moving sphere, time {t}"]) == above, t
        assert (mov in got[f"touches the first moving sphere from above at time 0.5, time {t}"]) == touch, t
    # skipped boxes answer nothing; min_prim cuts the list from below
    n_placed, n_skip = len(names), len(oc.skipped_boxes())
    assert all(len(s) == 0 for s in sets[n_placed:n_placed + n_skip - 1]) and len(sets[n_placed + n_skip - 1]) > 0
    mp = q["min_prim"][n_placed + n_skip:]
    whole = sets[n_placed + n_skip + 2]
    for m, s in zip(mp, sets[n_placed + n_skip:]):
        assert np.array_equal(s, whole[whole >= max(int(m), 0)]), m
    assert len(whole) == rec.n - 1 and len(sets[-2]) == 0 and len(sets[-1]) == len(whole)


def test_lattice_is_exact_in_the_mirror():
    q = oc.lattice_boxes()
    rec, sets, ck = both("lattice", q)
    closed = ck.closed_sets()
    assert all(np.array_equal(a, b) for a, b in zip(sets, closed))
    assert np.sum(ck.r == 0.0) > 300 and ck.n_exact > 500  # touching pairs: exempt from the cap, answered exactly instead
    assert sum(len(s) for s in sets) > 1000


def test_k_covers_the_mirrors_worst_residual():
    worst = {}
    for name in ("hand", "cover_moving", "suzanne", "big_mixed"):
        worst[name] = ov.mirror_residual(records(name), random_set(name)[:1500], 300)
    far, _ = oc.placed_boxes()
    worst["placed"] = ov.mirror_residual(records("hand"), far, 300)
    print("mirror residuals in u E_L:", {k: round(v, 3) for k, v in worst.items()})
    assert 0.5 < max(worst.values()) <= ov.K["strict"] - 1  # (the mirror's gap has one rounding more than the kernel's comparison)
    assert ov.K["fast"] == 2 * ov.K["strict"]


def test_paging_through_the_mirror_reproduces_the_full_sets():
    rec = records("hand")
    q = np.concatenate([oc.placed_boxes()[0], oc.min_prim_boxes(rec.n), oc.random_boxes(rec, 200, 3)])
    sets = ov.full_sets(rec, q)
    assert max(len(s) for s in sets) > 16
    for max_ids in (1, 3, 8):
        pages = ov.paged(rec, q, max_ids)
        assert all(np.array_equal(a, b) for a, b in zip(pages, sets)), max_ids


def test_the_checker_rejects_wrong_answers():
    rec = records("hand")
    q = oc.random_boxes(rec, 300, 3, (0.25, 0.5))
    sets = ov.full_sets(rec, q)
    ck = ov.Classified(rec, q)
    counts, ids = ov.answers(rec, q, 8, sets)
    ov.check_answers(ck, counts, ids, 8, "strict")
    i = int(np.nonzero((counts >= 2) & (counts <= 8))[0][0])
    j = int(np.nonzero(counts > 8)[0][0])

    def bad(fn):
        c, d = counts.copy(), ids.copy()
        fn(c, d)
        with pytest.raises(AssertionError):
            ov.check_answers(ck, c, d, 8, "strict")

    def drop(c, d):
        c[i] -= 1
        d[i, c[i]] = -1

    def swap(c, d):
        d[i, [0, 1]] = d[i, [1, 0]]

    def repeat(c, d):
        d[i, 1] = d[i, 0]

    def stranger(c, d):
        missing = np.setdiff1d(np.arange(rec.n), sets[i])
        d[i, :c[i]] = np.sort(np.concatenate([d[i, 1:c[i]], missing[:1]]))

    def skip_one(c, d):  # a full list that leaves out one of the lowest ids
        d[j] = sets[j][1:9]

    for fn in (drop, swap, repeat, stranger, skip_one, lambda c, d: c.__setitem__(j, 8), lambda c, d: d.__setitem__((i, 7), 0)):
        bad(fn)
    q2 = q.copy()  # an id below the query's min_prim
    q2["min_prim"][i] = sets[i][0] + 1
    with pytest.raises(AssertionError):
        ov.check_answers(ov.Classified(rec, q2), counts, ids, 8, "strict")


def test_exports_and_layout():
    import rtow

    header = (REPO / "include" / "rtow.h").read_text()
    for name in ("rtow_overlap_device", "rtow_overlap"):
        assert name in rtow.EXPORTS and re.search(rf"\bint {name}\(", header), name
    assert rtow.MAX_OVERLAP_IDS == 8 == int(re.search(r"#define RTOW_MAX_OVERLAP_IDS (\d+)", header).group(1))
    d = rtow.BOX_QUERY_DTYPE
    assert d.itemsize == 64 and d == ov.BOX_DTYPE
    assert [d.fields[f][1] for f in ("lo", "hi", "time", "min_prim", "pad_")] == [0, 24, 48, 56, 60]
    body = re.search(r"typedef struct rtow_box_query_t \{(.*?)\} rtow_box_query_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [m for m in re.findall(r"\b(lo|hi|time|min_prim|pad_)\b(?=[\[;,])", body)] == ["lo", "hi", "time", "min_prim", "pad_"]
    q = rtow.make_boxes([[0, 1, 2]], [[3, 4, 5]], 0.5, 7)
    assert q.tobytes() == ov.make_boxes([[0, 1, 2]], [[3, 4, 5]], 0.5, 7).tobytes()
    for name in ("overlap", "overlap_device", "overlap_all"):
        assert callable(getattr(rtow.Context, name))
    text = (REPO / "DESIGN.md").read_text()
    assert "K_strict = 10" in text and "K_fast = 20" in text
