"""The `big_mixed` scene (tests/big_mixed.py) and its query sets, host side (no GPU): the scene is what it claims to be,
the grid's two rules leave it a grid (before and after the refits the GPU tests make), and every query set is admissible —
each kind's exact checker, fed with the reference side alone (the oracle or the numpy mirror the strict build is pinned
to bit for bit), accepts it within the caps the GPU tests assert.  The measured shares and the worst residuals in band
units are printed.  The image sizes themselves need the device: test_gpu_big_mixed.py asserts them.
"""
import numpy as np
import pytest

import ambient_cases as ac
import ambient_exact as ax
import ambient_ref
import big_mixed as bm
import exact_hits as ex
import first_hits_ref as fr
import nearest_cases as nc
import nearest_ref as nr
import point_ref as pr
import rtow
import scatter_cases as sc
import scatter_exact as sx
import sweep_cases
import sweep_ref as sr
from exact_cases import SHARE
from support_scenes import motions


@pytest.fixture(scope="module")
def case():
    return bm.case()


# ------------------------------------------------------------------------------------------------- scene facts ---
def test_counts_classes_materials_and_order(case):
    G, view = case.G, case.view
    hsph, hmov, htri, hkind, hindex, hmat = sweep_cases.hand_geometry()
    assert (len(hsph), len(hmov), len(htri)) == (bm.N_CORE_SPH, bm.N_CORE_MOV, bm.N_CORE_TRI)
    assert (G.ns, G.nm, G.nt) == (len(hsph) + bm.N_SPH, len(hmov) + bm.N_MOV, len(htri) + bm.N_TRI)
    assert G.np <= 4096 and len(view.kind) == G.np  # (small enough for the brute force of the run_case helpers)
    # the core: the hand scene's primitives under the hand scene's insertion and class indices, bit for bit
    assert np.array_equal(view.kind[:bm.N_CORE], hkind) and np.array_equal(view.index[:bm.N_CORE], hindex)
    assert np.array_equal(view.sph[:len(hsph)], hsph) and np.array_equal(view.mov[:len(hmov)], hmov)
    assert np.array_equal(view.tri[:len(htri)], htri)
    hand_mats = np.array([hmat[k][i] for k, i in zip(hkind, hindex)])
    differs = np.nonzero(view.prim_mat[:bm.N_CORE] != hand_mats)[0]
    assert sorted((int(view.kind[i]), int(view.index[i])) for i in differs) == [(0, bm.TWINS[1]), (0, bm.ENCLOSING)]  # (see big_mixed)
    assert (view.sph[:, 3] < 0).sum() == 1 and np.array_equal(view.sph[3], view.sph[4])  # hollow glass, equal spheres
    # every class and every material kind; Lambertian and metal on the filler's triangles
    kinds = np.array([m[0] for m in bm.MATS])
    by_class = {k: set(kinds[view.prim_mat[view.kind == k]]) for k in range(3)}
    assert by_class[0] == by_class[1] == {bm.LAMBERTIAN, bm.METAL, bm.DIELECTRIC}
    filler_tri = view.prim_mat[bm.N_CORE:][view.kind[bm.N_CORE:] == 2]
    assert set(kinds[filler_tri]) == {bm.LAMBERTIAN, bm.METAL}
    # insertion order is not class-major, in the core and in the filler
    for part in (view.kind[:bm.N_CORE], view.kind[bm.N_CORE:]):
        assert np.any(np.diff(part) < 0)
    assert set(view.kind[bm.N_CORE:bm.N_CORE + 64]) == {0, 1, 2}  # (a wave's worth of the filler already mixes classes)
    # beside the core, inside its R = 40 sphere, and no round coordinates
    fill = view.tri[len(htri):].reshape(-1, 3)
    assert fill[:, 0].min() > 4.5 and np.linalg.norm(fill, axis=1).max() < 30
    for a in (view.tri[len(htri):], view.sph[len(hsph):], view.mov[len(hmov):, :7]):
        m, e = np.frexp(a)
        assert np.all(m * 2.0 ** 20 != np.round(m * 2.0 ** 20))


def test_the_filler_mixes_classes_in_space(case):
    """Every filler sphere and moving sphere lies within 0.5 of a filler triangle's centroid: leaves and cells hold
    triangles beside them."""
    view = case.view
    ctr = view.tri[bm.N_CORE_TRI:].reshape(-1, 3, 3).mean(axis=1)
    for c in (view.sph[bm.N_CORE_SPH:, :3], view.mov[bm.N_CORE_MOV:, :3]):
        d = np.sqrt(((c[:, None, :] - ctr[None]) ** 2).sum(axis=2)).min(axis=1)
        assert d.max() < 0.5, d.max()


@pytest.mark.parametrize("motion", [None, "jitter", "translate"])
def test_the_grid_stays_resident(case, motion):
    """At most 64 large primitives and no cell list above 255 entries (csrc/rtow_grid.h), before and after the refits."""
    G = case.G if motion is None else bm.moved(case.G, motions(case.G)[motion][0])
    n_large, longest, n = bm.grid_rules(G)
    print(f"\n{motion}: {n_large} large primitives, longest cell list {longest}, {n} cells")
    assert n_large <= 64 and longest <= 255


# -------------------------------------------------------------------------------- rays: closest hit and first k ---
@pytest.fixture(scope="module")
def ray_sets(case):
    return bm.ray_sets(case)


@pytest.mark.parametrize("name", bm.RAY_SETS)
def test_ray_sets_against_the_exact_reference(case, ray_sets, name):
    """Undecided rays of each build's reference (and the fast GRID walk's unit cut); the strict mirror of first_hits (the
    strict build's bits) passes check and check_sequences."""
    rays, share = ray_sets[name]
    refs = {"strict": ex.Reference(case.exact, rays, ex.STRICT), "fast": ex.Reference(case.exact, rays, ex.FAST),
            "fast, unit cut": ex.Reference(case.exact, rays, ex.FAST, unit_cut=True)}
    for what, r in refs.items():
        und = int((~r.decided).sum())
        print(f"\n{name} {what}: {len(rays)} rays, {und} undecided ({und / len(rays):.2e}), {r.n_exact} exact pairs")
        if share is not None:
            assert und <= share * len(rays), (name, what, und)
    h8, c8 = fr.reference(case.view, rays, 8)
    s = ex.check(refs["strict"], np.ascontiguousarray(h8[:, 0]), c8 > 0, (name, "mirror"))
    print(f"{name} mirror: worst t err {s['worst_t_err']:.3f} of bound")
    assert 0.05 < refs["strict"].occ.mean()
    if name in bm.SEQUENCE_SETS:
        rays, share = bm.sequence_sets(case, ray_sets)[name]
        refs = {b: ex.Reference(case.exact, rays, b) for b in (ex.STRICT, ex.FAST)}
        h8, c8 = fr.reference(case.view, rays, 8)
        for k in (8, 1):
            q = ex.check_sequences(refs[ex.STRICT], np.ascontiguousarray(h8[:, :k]), np.minimum(c8, k).astype(np.int32), k, (name, k))
            und = int((~ex.sequence_decided(refs[ex.FAST], k)).sum())
            print(f"{name} sequences k={k}: mirror worst t err {q['worst_t_err']:.3f}, fast undecided {und}")
            if share is not None:
                assert und <= share * len(rays), (name, k, und)
        at = fr.tmax_at_hits(rays, h8["t"], c8)
        ha, ca = fr.reference(case.view, at, 8)
        ex.check_sequences(ex.Reference(case.exact, at, ex.STRICT), ha, ca, 8, (name, "tmax at hits"))
        assert len(at) > 300


# --------------------------------------------------------------------------------- points: closest and k nearest ---
def test_point_sets_against_the_exact_distances(case):
    """The mirror's answers pass check_answers at the strict tau, at most a quarter into every band (the band leaves the
    factor four of test_sweep_host.py over the measured worst); k-nearest: the mirror's lists pass the exact checker."""
    rec, mats = case.rec, case.mats
    worst = 0.0
    for sname, pts, times, md in bm.point_sets(case):
        s = pr.check_answers(rec, mats, pts, times, md, pr.mirror_answers(rec, mats, pts, times, md), "strict", sname)
        print(f"{sname}: {pr.stats_line(s)}")
        assert s["overflow"] == (len(pts) if sname.startswith("overflow") else 0)
        assert s["open"] == 0 or sname in ("mixed_strict", "handmade")
        worst = max(worst, s["worst_dist"], s["worst_surface"], s["worst_consistency"])
    print(f"worst residual of the mirror: {worst:.3f} of its band")
    assert worst <= 0.25


def test_nearest_sets_against_the_exact_distances(case):
    rec, mats = case.rec, case.mats
    total = None
    sets = bm.nearest_sets(case)
    assert {"far@0", "overflow@0", "mixed", "mixed_strict", "mixed_kth", "handmade"} <= {s[0] for s in sets}
    batches = []
    for s in sets:
        ck = nr.FastChecker(rec, mats, *s[1:])
        hits, counts = nr.reference(rec, mats, ck.pts, ck.times, ck.md, nr.MAX_NEAREST, ck.mirror)
        for k in (8, 1):
            total = nc.add_stats(total, ck.check(*nc.cut((hits, counts), k), k, (s[0], k), "strict"))
        batches.append(ck)
    print("nearest, mirror: " + nr.stats_line(dict(total, exact_pairs=sum(len(b._exact) for b in batches), exact_decisions=0)))
    assert total["overflow"] > 0 and total["short"] > 0
    assert max(total["worst_dist"], total["worst_surface"], total["worst_consistency"]) <= 0.25


# ------------------------------------------------------------------------------------------------------- sweeps ---
def test_sweep_sets_against_the_exact_segment_distances(case):
    """The mirror on a thinned strict set (every family), the ties and one contact chain: no refusal, open sweeps at most
    2 % of the random rows, K_strict >= 4 x the worst contact residual."""
    rec, mats = case.rec, case.mats
    q = bm.strict_sweeps(case)
    fixed = len(sweep_cases.placed_sweeps()) + len(sweep_cases.skipped_sweeps())
    assert abs(np.isinf(q["tmax"][fixed:]).mean() - 1 / 7) < 0.01
    rnd = sweep_cases.thin((q[fixed:],), 400)[0]
    worst = 0.0
    for name, part in (("placed+skipped", q[:fixed]), ("random", rnd)):
        live = part[~sr.skipped(part)]
        s = sr.Checker(rec, mats, live).check(sr.answers(rec, mats, live), "strict", name)
        print(f"{name}: {sr.stats_line(s)}; worst contact residual {s['worst_contact'] * sr.K['strict']:.2f} u S")
        worst = max(worst, s["worst_contact"] * sr.K["strict"])
        if name == "random":
            assert s["open"] <= 0.02 * len(live), s["open"]
            assert 0.1 * len(live) < s["hits"]
    tq, want = bm.tie_sweeps(case)
    th = sr.answers(rec, mats, tq)
    assert np.array_equal(th["prim"], want) and np.all(th["t"] > 0), (th["prim"], want)
    cq, rest, into = bm.contact_sweeps(case, lambda x: sr.answers(rec, mats, x))
    assert len(cq) <= 300 and into.sum() >= 30
    ch = sr.answers(rec, mats, cq)
    s = sr.Checker(rec, mats, cq).check(ch, "strict", "contact")
    print(f"contact: {sr.stats_line(s)}; worst contact residual {s['worst_contact'] * sr.K['strict']:.2f} u S")
    assert np.all(ch["prim"][into] >= 0)
    worst = max(worst, s["worst_contact"] * sr.K["strict"])
    print(f"worst contact residual of the mirror: {worst:.2f} u S; K_strict = {sr.K['strict']}")
    assert sr.K["strict"] >= 4.0 * worst


# ------------------------------------------------------------------------------------------------------ ambient ---
@pytest.mark.parametrize("samples", bm.AMBIENT_SAMPLES)
def test_ambient_points_against_the_exact_hits(case, samples):
    pts, ids = bm.ambient_points(case)
    assert not ambient_ref.skipped(pts).any()
    rays = ambient_ref.rays(pts, samples, ac.SEED, ids)
    for build, unit_cut in ((ex.STRICT, False), (ex.FAST, False), (ex.FAST, True)):
        ref = ex.Reference(case.exact, rays.reshape(-1), build, unit_cut=unit_cut)
        und = ~ref.occ_decided.reshape(len(pts), samples)
        left_out = int((und.sum(axis=1) > 4).sum())
        print(f"\n{samples} samples, {build} unit_cut={unit_cut}: {int(und.sum())} undecided of {und.size} rays, {left_out} of "
              f"{len(pts)} points left out, open {1 - ref.occ.mean():.3f}")
        assert und.sum() <= SHARE * und.size and left_out <= 0.01 * len(pts)
        assert 0 < ref.occ.sum() < ref.occ.size
        if build == ex.STRICT:
            good = ambient_ref.fold(pts, rays, ref.occ.reshape(len(pts), samples))
            s = ax.check_records(ref, pts, rays, good, samples, ex.STRICT, exact=ax.Exact(pts, rays, samples, ex.STRICT, ac.SEED, ids))
            print("mirror records: " + ax.line(s))
            assert s["left_out"] == 0 and s["worst_dir"] <= 1.0 and s["worst_sky"] <= 1.0


# ---------------------------------------------------------------------------------------------------- path step ---
def test_scatter_rows_against_the_exact_scatter(case):
    rows = bm.scatter_case(case)
    kinds = {int(rows.mats[m, 5]) for m in case.view.prim_mat[np.unique(_row_prims(case, rows))]}
    assert kinds == {bm.LAMBERTIAN, bm.METAL, bm.DIELECTRIC}, kinds
    assert set(rows.bounce) == set(range(int(case.log[:, 2].max()) + 1))
    st, nx, at, hits = sc.oracle_step(rows, case.view)
    href, ref = rows.ref(ex.STRICT)
    s = sx.check(ref, st, nx, at, hits, what="big_mixed rows")
    print(f"\nrows: {s['rays']} rays, decided {s['decided']}, undecided {s['undecided']} (hit {s['hit_undecided']}), worst "
          f"direction error {s['worst_dir_err']:.3f} of bound")
    sc.assert_shares(rows, ref, "strict")
    for unit_cut in (False, True):
        sc.assert_shares(rows, rows.ref(ex.FAST, unit_cut)[1], ("fast", unit_cut))
    assert np.array_equal(hits["t"].view(np.uint64), rows.rows[:, 10].view(np.uint64))  # the oracle's own t, bit for bit


def _row_prims(case, rows):
    h = rows.ref(ex.STRICT)[0]
    return np.array([t[0] for t in h.ties if t], dtype=np.int64)


# ----------------------------------------------------------------------------------------------- frame and rows ---
def test_the_logged_frame_reaches_every_class_and_the_sky(case):
    log = case.log
    w, h, spp, depth, seed = bm.FRAME
    assert (log[:, 2] == 0).sum() == w * h * spp and 8 <= log[:, 2].max() <= depth
    hit = np.isfinite(log[:, 10])
    assert 0.2 < hit.mean() < 0.9 and np.count_nonzero(case.image) > 0.9 * case.image.size
    ref = ex.Reference(case.exact, bm.ray_sets(case)["logged"][0], ex.STRICT)
    kinds = np.bincount([case.view.kind[t[0]] for t in ref.ties if t], minlength=3)
    filler = sum(1 for t in ref.ties if t and t[0] >= bm.N_CORE)
    print(f"\nlogged set: hits per class {kinds.tolist()}, on the filler {filler}, on the core {kinds.sum() - filler}")
    assert np.all(kinds >= 15) and filler >= 100 and kinds.sum() - filler >= 100
