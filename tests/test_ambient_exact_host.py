"""The ambient query's exact reference (ambient_exact.py) on the CPU: the numpy mirror of the definition stays within the
strict build's derived bound of the exact directions; the checkers refuse eight wrong kernels, one mutation at a time;
and on the point sets of test_gpu_exact_ambient.py the hemisphere rays that exact_hits leaves undecided stay under the
caps that test enforces."""
import math

import numpy as np
import pytest

import ambient_cases as ac
import ambient_exact as ax
import ambient_ref
import exact_hits as ex
import rtow
from exact_cases import SHARE, big_mesh, logged  # noqa: F401
from support_scenes import SceneView, handmade_scene

U = 2.0 ** -53
SAMPLES = 8


# ---- directions ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs():
    """(points, ids, labels, skipped, mirror rays [n, 4], exact directions) of the direction cases."""
    pts, ids, labels = ac.direction_cases()
    rays = ambient_ref.rays(pts, ac.DIR_SAMPLES, ac.SEED, ids)
    pixel, sample = ambient_ref.identities(len(pts), ac.DIR_SAMPLES, ids)
    return pts, ids, labels, ambient_ref.skipped(pts), rays, ax.exact_directions(pts["normal"], ac.SEED, pixel, sample)


def test_direction_cases_cover_what_they_name(dirs):
    pts, ids, labels, skip, rays, exact = dirs
    assert 1500 <= len(pts) <= 2500
    assert np.array_equal(skip, labels == "skipped") and skip.sum() >= 10
    assert np.array_equal(np.isnan(exact[0][:, 0, 0]), skip)
    N = pts["normal"]
    span = np.abs(N[labels == "wide"])
    assert span.min() < 1e-140 and span.max() > 1e140
    with np.errstate(all="ignore"):
        nn = (N * N).sum(axis=1)
    live_nn = nn[~skip]
    assert live_nn.min() == 2.0 ** -1022 and live_nn.max() > 1e307
    assert np.signbit(N[labels == "axes"]).any() and (labels == "axes").sum() == 24
    # the rim: pz below 3e-3; the centre: pz within 1e-5 of 1; the clamped identity: pz = 0 exactly
    dn = (rays["direction"] * ambient_ref.unit_normal(np.where(skip[:, None], 1.0, N))[:, None, :]).sum(axis=2)
    assert np.all(dn[labels == "rim", 0] < 3e-3) and np.all(dn[labels == "centre", 0] > 1 - 1e-5)
    assert np.all(np.abs(dn[labels == "clamped", 0]) < 1e-15)


def test_mirror_stays_within_the_strict_bound_of_the_exact_directions(dirs):
    """Every component of every mirror direction, per group of cases; a skipped point's rays are dead rays."""
    pts, ids, labels, skip, rays, exact = dirs
    worst = ax.check_directions(exact, rays["direction"], ax.STRICT, "mirror")
    ratio = np.abs(rays["direction"] - exact[0]) / exact[1][ax.STRICT]
    print(f"\nmirror against exact directions: worst {worst:.3f} of the strict bound; per group: "
          + ", ".join(f"{k} {np.nanmax(ratio[labels == k]):.3f}" for k in dict.fromkeys(labels) if k != "skipped"))
    dev = np.abs(rays["direction"] - exact[0])[~skip].max()
    print(f"largest deviation {dev / U:.1f} u; median strict bound {np.nanmedian(exact[1][ax.STRICT]) / U:.0f} u, "
          f"fast {np.nanmedian(exact[1][ax.FAST]) / U:.0f} u")
    assert np.all(rays["tmax"][skip] == -1.0) and not rays["direction"][skip].any()
    assert np.all(exact[1][ax.FAST][~skip] >= exact[1][ax.STRICT][~skip])


def test_a_subnormal_squared_length_cannot_be_normalised():
    """What the skip rule keeps out: the mirror's arithmetic on normals of length 1e-158 to 1e-161 (normal . normal
    subnormal) is far outside the bound of the exact direction, and within it at 2e-154."""
    g = np.random.default_rng(3)
    lengths = np.array([1e-158, 1e-160, 1e-161, 2e-154])
    N = np.repeat(lengths, 50)[:, None] * g.normal(size=(200, 3))
    pixel, sample = ambient_ref.identities(len(N), 2)
    px, py = ambient_ref.disk_points(ac.SEED, pixel, sample)
    with np.errstate(all="ignore"):
        d = ambient_ref.hemisphere_dirs(ambient_ref.unit_normal(N), px, py)
    exact = ax.exact_directions(N, ac.SEED, pixel, sample, rule=False)
    with np.errstate(invalid="ignore"):
        ratio = (np.abs(d - exact[0]) / exact[1][ax.STRICT]).reshape(4, -1)
    ratio = np.where(np.isnan(ratio), np.inf, ratio).max(axis=1)
    print(f"\nmirror without the rule, error over bound per length {lengths}: {ratio}")
    assert np.all(ratio[:3] > 1e3) and ratio[3] <= 1.0
    assert ambient_ref.skipped(rtow.make_surface_points(np.zeros((200, 3)), N))[:150].all()


def mutant_dirs(pts, ids, kind):
    """The mirror's directions of the live direction cases with one thing wrong."""
    live = ~ambient_ref.skipped(pts)
    pixel, sample = ambient_ref.identities(len(pts), ac.DIR_SAMPLES, ids)
    px, py = ambient_ref.disk_points(ac.SEED, pixel[live], sample[live])
    nh = ambient_ref.unit_normal(pts["normal"][live])
    x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
    s = np.ones_like(z) if kind == "s = +1" else np.copysign(1.0, z)
    with np.errstate(all="ignore"):  # (s = +1 at the -z pole divides by zero; no clamp takes the root of a negative)
        a = -1.0 / (s + z)
        c = (x * y) * a
        sx = s * x
        t = np.stack([1.0 + (sx * x) * a, s * c, -sx], axis=1)
        b = np.stack([c, s + ((y * y) * a), -y], axis=1)
        if kind == "t negated":
            t = -t
        r2 = px * px + py * py
        if kind == "no clamp":
            pz = np.sqrt(1.0 - r2)
        elif kind == "uniform":  # the disk point lifted onto a uniformly sampled hemisphere
            pz = np.maximum(1.0 - r2, 0.0)
            px, py = px * np.sqrt(2.0 - r2), py * np.sqrt(2.0 - r2)
        else:
            pz = np.sqrt(np.maximum(1.0 - r2, 0.0))
        d = np.zeros((len(pts), ac.DIR_SAMPLES, 3))
        d[live] = np.stack([(t[:, None, k] * px + b[:, None, k] * py) + nh[:, None, k] * pz for k in range(3)], axis=2)
    return d


def test_direction_check_refuses_wrong_kernels(dirs):
    pts, ids, labels, skip, rays, exact = dirs
    assert np.array_equal(mutant_dirs(pts, ids, None), rays["direction"], equal_nan=True)
    for build in ax.BUILDS:
        ax.check_directions(exact, rays["direction"], build, "unmutated")
    for kind in ("s = +1", "t negated", "no clamp", "uniform"):
        wrong = mutant_dirs(pts, ids, kind)
        for build in ax.BUILDS:
            with pytest.raises(ax.CheckError):
                ax.check_directions(exact, wrong, build, kind)
    # below the equator only: s = +1 is right wherever N.z has no sign bit
    up = ~skip & ~np.signbit(pts["normal"][:, 2])
    ax.check_directions(exact, mutant_dirs(pts, ids, "s = +1"), ax.STRICT, "s = +1, upper half", live=up)
    # the clamp matters at the clamped identity only
    ax.check_directions(exact, mutant_dirs(pts, ids, "no clamp"), ax.STRICT, "no clamp", live=~skip & (labels != "clamped"))
    # one component, 200 u off: at a sample near the disk's centre, the direction's largest component
    i = int(np.nonzero(labels == "centre")[0][1])
    k = int(np.argmax(np.abs(rays["direction"][i, 0])))
    for sign in (1.0, -1.0):
        wrong = rays["direction"].copy()
        wrong[i, 0, k] += sign * 200 * U
        for build in ax.BUILDS:
            with pytest.raises(ax.CheckError):
                ax.check_directions(exact, wrong, build, "200 u")


# ---- records and the undecided share -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(logged, big_mesh):
    """name -> (exact_hits.Scene, points, ids, samples, mirror rays): the point sets of test_gpu_exact_ambient.py."""
    out = {}
    for j, name in enumerate(("cover_moving", "suzanne")):
        hs, view, sc, log = logged[name]
        pts, ids = ac.log_points(view, log, 300, 40 + j)
        out[name] = (sc, pts, ids, SAMPLES)
    hs, view, sc, log = big_mesh
    pts, ids = ac.log_points(view, log, 100, 44)
    out["mesh96k"] = (sc, pts, ids, 4)
    hm = handmade_scene()
    out["handmade"] = (ex.Scene.of(SceneView(hm)), np.concatenate([ac.handmade_points(), ac.handmade_sky_points()]), None,
                       SAMPLES)
    return {k: v + (ambient_ref.rays(v[1], v[3], ac.SEED, v[2]),) for k, v in out.items()}


SHARE_CASES = [(name, build, unit_cut) for name in ("cover_moving", "suzanne", "mesh96k", "handmade")
               for build, unit_cut in ((ex.STRICT, False), (ex.FAST, False), (ex.FAST, True))
               if not (unit_cut and name == "cover_moving")]  # (no triangles: the unit cut changes nothing)


@pytest.mark.parametrize("name,build,unit_cut", SHARE_CASES)
def test_undecided_share_of_the_hemisphere_rays(sets, name, build, unit_cut):
    """The caps of the GPU test on the reference alone: under each build's band (and the fast GRID walk's unit cut where
    there are triangles) at most SHARE of the mirror's rays are occlusion-undecided, and at most 1 % of the points have
    more than four undecided samples."""
    sc, pts, ids, samples, rays = sets[name]
    assert not ambient_ref.skipped(pts).any() and (len(sc.tri) > 0 or not unit_cut)
    ref = ex.Reference(sc, rays.reshape(-1), build, unit_cut=unit_cut)
    und = ~ref.occ_decided.reshape(len(pts), samples)
    left_out = int((und.sum(axis=1) > 4).sum())
    print(f"\n{name} {build} unit_cut={unit_cut}: {int(und.sum())} undecided of {und.size} rays, {left_out} of "
          f"{len(pts)} points left out, open {1 - ref.occ.mean():.3f}")
    assert und.sum() <= SHARE * und.size, (name, build, int(und.sum()))
    assert left_out <= 0.01 * len(pts), (name, build, left_out)
    assert 0 < ref.occ.sum() < ref.occ.size


def test_record_check_accepts_the_mirror_and_refuses_wrong_records(sets):
    sc, pts, ids, samples, rays = sets["cover_moving"]
    ref = ex.Reference(sc, rays.reshape(-1), ex.STRICT)
    occ = ref.occ.reshape(len(pts), samples)
    good = ambient_ref.fold(pts, rays, occ)
    args = dict(exact=ax.Exact(pts, rays, samples, ex.STRICT, ac.SEED, ids))
    s = ax.check_records(ref, pts, rays, good, samples, ex.STRICT, **args)
    print("\nmirror records on cover_moving: " + ax.line(s))
    assert s["points"] == len(pts) and s["left_out"] == 0 and s["worst_dir"] <= 1.0 and s["worst_sky"] <= 1.0

    def refused(records, why, ray_array=rays):
        with pytest.raises(ax.CheckError):
            ax.check_records(ref, pts, ray_array, records, samples, ex.STRICT, what=why, **args)

    # one decided sample's visibility flipped, either way
    dec = ref.occ_decided.reshape(occ.shape)
    for want in (True, False):
        i, j = (int(v) for v in np.argwhere(dec & (occ == want))[0])
        flipped = occ.copy()
        flipped[i, j] = not want
        refused(ambient_ref.fold(pts, rays, flipped), f"sample ({i}, {j}) flipped")
    # bent added in reverse sample order
    wrong = good.copy()
    acc = np.zeros((len(pts), 3))
    for j in reversed(range(samples)):
        acc = np.where(~occ[:, j, None], acc + rays["direction"][:, j], acc)
    wrong["bent"] = acc
    assert (wrong["bent"] != good["bent"]).any() and np.abs(wrong["bent"] - good["bent"]).max() < 1e-14
    refused(wrong, "bent in reverse order")
    # the sky of the wrong sample: every sample adds the colour of its neighbour's direction
    shifted = rays.copy()
    shifted["direction"] = np.roll(rays["direction"], 1, axis=1)
    wrong = good.copy()
    wrong["sky"] = ambient_ref.fold(pts, shifted, occ)["sky"]
    refused(wrong, "sky of the wrong sample")
    # the count of samples, a live ray's origin, and a skipped point that answers
    wrong = good.copy()
    wrong["samples"][3] = samples - 1
    refused(wrong, "samples")
    dead = pts.copy()
    dead["max_dist"][5] = 0.0005
    with pytest.raises(ax.CheckError):  # (other points: their own exact directions, made in the call)
        ax.check_records(ref, dead, rays, good, samples, ex.STRICT, seed=ac.SEED, ids=ids)
    with pytest.raises(AssertionError, match="other points"):
        ax.check_records(ref, dead, rays, good, samples, ex.STRICT, **args)


def test_record_check_on_enclosed_and_open_points(sets):
    """The hand-made scene: inside the hollow sphere with max_dist = inf every sample is decidedly closed and the record
    is +0.0 but for `samples`; far above the scene every sample is decidedly open."""
    sc, pts, ids, samples, rays = sets["handmade"]
    ref = ex.Reference(sc, rays.reshape(-1), ex.STRICT)
    occ, dec = ref.occ.reshape(len(pts), samples), ref.occ_decided.reshape(len(pts), samples)
    rec = ambient_ref.fold(pts, rays, occ)
    print("\nmirror records on handmade: " + ax.line(ax.check_records(ref, pts, rays, rec, samples, ex.STRICT, seed=ac.SEED)))
    inside = np.arange(len(pts)) < ac.N_ENCLOSED
    closed = inside & np.isinf(pts["max_dist"])
    assert closed.sum() >= 10 and dec[closed].all() and occ[closed].all()
    assert not rec["bent"][closed].view(np.uint64).any() and not rec["sky"][closed].view(np.uint64).any()
    above = pts["point"][:, 1] == 50.0
    assert above.sum() == 24 and dec[above].all() and not occ[above].any() and np.all(rec["open"][above] == samples)
    assert math.isclose(rec["bent"][above][:, 1].mean() / samples, 2.0 / 3.0, abs_tol=0.1)


def test_record_check_with_undecided_samples():
    """Spheres placed tangent to chosen sample rays leave those samples undecided.  With m = 1 and m = 2 undecided
    samples every one of the 2^m ways to open them is accepted and nothing else; a point with six is left out, counted,
    and held to the range of `open` alone."""
    g = np.random.default_rng(21)
    samples = SAMPLES
    picks = {0: [2], 1: [1, 5], 2: [0, 1, 2, 3, 4, 5], 3: []}  # point -> the samples a sphere is tangent to
    pts = rtow.make_surface_points(np.array([[300.0 * i, 1.0, -2.0] for i in picks]), g.normal(size=(len(picks), 3)),
                                   time=0.5)
    rays = ambient_ref.rays(pts, samples, ac.SEED)
    sph = []
    for i, js in picks.items():
        for j in js:
            d = rays["direction"][i, j]
            u = np.cross(d, g.normal(size=3))
            u /= np.linalg.norm(u)
            # the centre 0.25 from the ray, the radius 0.25: tangent up to rounding
            sph.append(np.append(pts["point"][i] + 3.0 * d + 0.25 * u, 0.25))
    sc = ex.Scene.class_major(np.array(sph), np.zeros((0, 8)), np.zeros((0, 9)), np.zeros(len(sph), np.int32))
    ref = ex.Reference(sc, rays.reshape(-1), ex.STRICT)
    occ, dec = ref.occ.reshape(len(pts), samples), ref.occ_decided.reshape(len(pts), samples)
    und = [np.nonzero(~dec[i])[0].tolist() for i in picks]
    assert und[0] == [2] and und[1] == [1, 5] and und[3] == [] and set(und[2]) <= set(picks[2]) and len(und[2]) > 4
    assert not occ[[0, 1, 3]][dec[[0, 1, 3]]].any()  # (every decided sample of these points is open)
    sure2 = int((dec[2] & ~occ[2]).sum())  # (a sphere of point 2 may stand in another of its samples' way, decidedly)
    exact = ax.Exact(pts, rays, samples, ex.STRICT, ac.SEED)

    def check(o):
        return ax.check_records(ref, pts, rays, ambient_ref.fold(pts, rays, o), samples, ex.STRICT, exact=exact)

    # every way to open the undecided samples of points 0 and 1 (and some way for point 2) is accepted
    for way in range(8):
        o = occ.copy()
        o[0, 2], o[1, 1], o[1, 5] = way & 1, way & 2, way & 4
        o[2, und[2]] = g.random(len(und[2])) < 0.5
        s = check(o)
        assert (s["undecided"], s["left_out"], s["points"]) == (3 + len(und[2]), 1, 4) and s["worst_sky"] <= 1.0
    # a decided sample closed beside an undecided one: `open` stays in its range, but no way to open gives this bent
    for i, j in ((0, 4), (1, 0)):
        o = occ.copy()
        o[i, j] = True
        with pytest.raises(ax.CheckError):
            check(o)
    # an undecided sample's direction added though the count says closed
    rec = ambient_ref.fold(pts, rays, occ)
    rec["open"][0] = float(samples - 1) if not occ[0, 2] else float(samples)
    with pytest.raises(ax.CheckError):
        ax.check_records(ref, pts, rays, rec, samples, ex.STRICT, exact=exact)
    # the point that is left out is still held to the range of open
    rec = ambient_ref.fold(pts, rays, occ)
    for value, ok in ((sure2 - 1.0, False), (float(sure2), True), (float(sure2 + len(und[2])), True),
                      (sure2 + len(und[2]) + 1.0, False)):
        rec["open"][2] = value
        if ok:
            ax.check_records(ref, pts, rays, rec, samples, ex.STRICT, exact=exact)
        else:
            with pytest.raises(ax.CheckError):
                ax.check_records(ref, pts, rays, rec, samples, ex.STRICT, exact=exact)
