"""The exact scatter reference (tests/scatter_exact.py) held to the oracle on the CPU: no GPU.

  1. The reference's own Philox, coin and ball point are the oracle's (orc_philox4x32, orc_philox_request), and its
     rational ball point and sky agree with an mpmath evaluation of the same expressions at 50 digits.
  2. orc_scatter, fed with the oracle's own hit, passes scatter_exact.check as `strict` on every family of the edge scene
     (and of its triangle-only variant) and on the logged rows of the three deep renders; the same source compiled
     with -ffp-contract=fast -mfma (liboracle_contracted.so) passes as `fast`: the bounds are not too tight for what
     rounding and contraction alone do.  (The contracted library scatters; the hit it is fed is liboracle.so's.)
  3. The undecided shares of scatter_cases.assert_shares hold for both builds' references.
  4. Every planted error is rejected on at least one ray of a named family.

Bound headroom, the worst |direction error| / bound over the decided rays, measured here (printed by test 2), the
oracle as strict / the contracted oracle as fast:
    edge scene: (a) 0.373 / 0.373, (b) 0.093 / 0.034, (c) 0.066 / 0.022, (d) 0.155 / 0.155, (e) 0.053 / 0.016, (f) 0 / 0;
    triangle-only variant: (a) 0.397 / 0.369, (d) 0.395 / 0.395, (e) 0.069 / 0.025, the others as above;
    logged rows (5,000 each): cover_d50 0.020 / 0.004, cover_moving_d50 0.012 / 0.004, suzanne_d20 0.277 / 0.267.
Undecided (scatter or hit) of the 2,032 edge rays: strict 119 (52 of them by their hit), fast 157 (64): the rays placed
on a cut by construction and the critical-angle rays at offsets below 1e-9; none of the 15,000 logged rows.  The rays
whose hit is undecided pass as one of the outcomes their hit band leaves open, and test 4 plants errors on them too.
"""
import ctypes as C

import numpy as np
import pytest

import exact_hits as ex
import orc
import scatter_cases as sc
import scatter_exact as sx
from support_scenes import SceneView

BUILDS = (ex.STRICT, ex.FAST)


class _Held:
    def __init__(self, c, keep):
        self.c, self.keep = c, keep


def _view(case):
    keep = []
    return SceneView(_Held(case.es.upload(keep), keep))


@pytest.fixture(scope="module")
def edge():
    """name -> (case, view, {build: oracle answers}) of the edge scene and its triangle-only variant."""
    out = {}
    for tri_only in (False, True):
        case = sc.edge_case(tri_only)
        out[case.name] = (case, _view(case), {})
    return out


def _library(build):
    if build == ex.STRICT:
        return None
    import sample_audit
    if not sample_audit.host_has_fma():
        pytest.skip("the contracted oracle needs a host CPU with FMA")
    return sample_audit.contracted_oracle()


def _answers(entry, build):
    case, view, cache = entry
    if build not in cache:
        cache[build] = sc.oracle_step(case, view, _library(build))
    return cache[build]


def _report(case, ref, st, nx, at, hits, what):
    lines = []
    for name, idx in case.groups().items():
        s = sx.check(ref, st, nx, at, hits, what=f"{what}/{name}", only=idx)
        lines.append(f"  {name}: rays {s['rays']}, decided {s['decided']}, undecided {s['undecided']} (hit "
                     f"{s['hit_undecided']}), worst direction error {s['worst_dir_err']:.3f} of bound, {s['tags']}")
    print(f"\n{what}\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------- the pieces ---
def test_philox_coin_and_ball_point_are_the_oracles():
    L = orc.lib()
    g = np.random.default_rng(3)
    for _ in range(200):
        seed = int(g.integers(0, 1 << 63))
        pix, smp, req = (int(x) for x in g.integers(0, 1 << 32, 3))
        w = sx.philox_words(seed, pix, smp, req)
        ctr = (C.c_uint32 * 4)(req, smp, pix, 0)
        key = (C.c_uint32 * 2)(seed & 0xffffffff, seed >> 32)
        o = (C.c_uint32 * 4)()
        L.orc_philox4x32(ctr, key, o, L.orc_philox_rounds())
        assert tuple(o) == w
        assert float(sx.coin_of(w)) == L.orc_philox_request(seed, pix, smp, req, 2, 3)
        rnd, bound = sx.ball_point(w, ex.STRICT)
        for k in range(3):
            assert abs(float(rnd[k]) - L.orc_philox_request(seed, pix, smp, req, 2, k)) <= bound[k]
    pix = np.arange(500, dtype=np.uint64)
    want = [L.orc_philox_request(sc.SEED, int(p), 3, 1 + sc.BOUNCE, 2, 3) for p in pix]
    assert np.array_equal(sc.coins(sc.SEED, pix, 3, 1 + sc.BOUNCE), np.array(want))


def test_ball_point_and_sky_against_mpmath():
    import mpmath as mp

    mp.mp.dps = 50
    g = np.random.default_rng(4)
    coef = [mp.mpf(c) for c in sx.COEF]

    def poly(x):
        x2 = x * x
        return x * (coef[0] + x2 * (coef[1] + x2 * (coef[2] + x2 * (coef[3] + x2 * coef[4]))))

    for _ in range(100):
        w = tuple(int(x) for x in g.integers(0, 1 << 32, 4))
        rnd, _ = sx.ball_point(w, ex.STRICT)
        z = mp.mpf(w[0] >> 8) / 2 ** 24
        phi = mp.mpf(w[1] >> 8) * mp.mpf(sx.HALF_PI * 2.0 ** -24)
        r = mp.mpf(max(w[2] & 0xffff, w[2] >> 16, w[3] & 0xffff)) / 2 ** 16
        rs = r * mp.sqrt(1 - z * z)
        want = [rs * poly(mp.mpf(sx.HALF_PI) - phi), rs * poly(phi), r * z]
        for k in range(3):
            f = rnd[k].fraction()
            assert abs(mp.mpf(f.numerator) / f.denominator - want[k]) <= mp.mpf(10) ** -35
        d = g.normal(size=3) * 10.0 ** g.integers(-3, 4)
        col, bound = sx.sky_exact(d, ex.STRICT)
        t = (mp.mpf(d[1]) / mp.sqrt(sum(mp.mpf(x) ** 2 for x in d)) + 1) / 2
        for c, got, b in zip(sx.SKY, col, bound):
            assert abs(mp.mpf(got) - ((1 - t) + t * mp.mpf(c))) <= mp.mpf(2.0 ** -52)
            assert 0 < b < 1e-14


# ------------------------------------------------------------------------------------- the oracle under check ---
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["edge", "edge_tri"])
def test_oracle_passes_on_the_families(edge, name, build):
    case = edge[name][0]
    st, nx, at, hits = _answers(edge[name], build)
    href, ref = case.ref(build)
    ex.check(href, hits, None, (name, build))
    _report(case, ref, st, nx, at, hits if build == ex.STRICT else None, f"{name} {build}")
    sc.assert_shares(case, ref, (name, build))
    if build == ex.FAST:  # and of the reference of the fast GRID walk, which cuts triangles at det / |d| >= 1e-6
        sc.assert_shares(case, case.ref(build, True)[1], (name, build, "unit cut"))
    assert {"lambertian", "metal", "reflect", "refract", "cut", "sky"} <= set(
        o[0].tag for o, d in zip(ref.outs, ref.decided) if o and d)
    if build == ex.STRICT:  # the strict build's sky is the oracle's, and the hits are its own
        assert np.all(st[hits["prim"] < 0] == 0)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(sc.DEEP))
def test_oracle_passes_on_the_logged_rows(name, build):
    case = sc.logged_case(name)
    st, nx, at, hits = sc.oracle_step(case, case.view, _library(build))
    href, ref = case.ref(build)
    _report(case, ref, st, nx, at, hits if build == ex.STRICT else None, f"logged {name} {build}")
    sc.assert_shares(case, ref, (name, build))
    # every segment depth and every material of the scene is among the decided rows
    dec = ref.decided & (hits["prim"] >= 0)
    assert set(case.bounce) == set(range(int(case.bounce.max()) + 1))
    kinds = set(int(case.mats[m, 5]) for m in hits["material"][dec])  # (the draw asserts the same of all its rows)
    assert kinds == set(int(k) for k in case.mats[np.unique(case.scene.prim_mat), 5]), kinds
    if build == ex.STRICT:  # the log's own t, bit for bit: the rows are what the render traced
        assert np.array_equal(hits["t"][dec], case.rows[dec, 10])


# ------------------------------------------------------------------------------------------- planted errors ---
def _m_front(inp):
    inp["front"] ^= 1


def _m_ratio(inp):
    inp["mats"][:, 4] = 1.0 / inp["mats"][:, 4]


def _m_unit_normal(inp):
    inp["normal"] /= np.linalg.norm(inp["normal"], axis=1, keepdims=True)


def _m_no_fuzz(inp):
    inp["mats"][:, 3] = 0.0


def _m_request(inp):
    inp["request"] += 1


PLANTED_INPUTS = {  # name: (mutation of orc_scatter's inputs, the family that must catch it)
    "front flag flipped": (_m_front, "a"),
    "ratio inverted": (_m_ratio, "b"),
    "normalised triangle normal": (_m_unit_normal, "e"),
    "fuzz dropped": (_m_no_fuzz, "d"),
    "coin from the wrong request": (_m_request, "c"),
}


@pytest.mark.parametrize("what", list(PLANTED_INPUTS))
def test_planted_input_errors_are_rejected(edge, what):
    case, view, _ = edge["edge"]
    mutate, fam = PLANTED_INPUTS[what]
    st, nx, at, hits = sc.oracle_step(case, view, None, mutate)
    ref = case.ref(ex.STRICT)[1]
    with pytest.raises(sx.CheckError) as e:
        sx.check(ref, st, nx, at, None, what=what, only=case.groups()[fam])
    assert all(case.family[i] == fam for i, _ in e.value.bad)
    print(what, "->", e.value.bad[0])


def test_planted_output_errors_are_rejected(edge):
    case = edge["edge"][0]
    st, nx, at, hits = _answers(edge["edge"], ex.STRICT)
    ref = case.ref(ex.STRICT)[1]
    groups = case.groups()
    sx.check(ref, st, nx, at, hits)

    def rejected(fam, st2=st, nx2=nx, at2=at):
        with pytest.raises(sx.CheckError) as e:
            sx.check(ref, st2, nx2, at2, hits, only=groups[fam])
        return e.value.bad

    # a direction component off by 1e-12 relative
    for k in range(3):
        n2 = nx.copy()
        n2["direction"][:, k] *= 1.0 + 1e-12
        for fam in "abde":
            assert rejected(fam, nx2=n2)
    # reflect and refract swapped on decided rays: the (c) rays of one fixed ray, above and below the coin
    c = groups["c"]
    tag = np.array([ref.outs[i][0].tag for i in c])
    assert ref.decided[c].all()
    a, b = c[tag == "reflect"][0], c[tag == "refract"][0]
    n2 = nx.copy()
    n2[a], n2[b] = nx[b], nx[a]
    bad = rejected("c", nx2=n2)
    assert {i for i, _ in bad} == {int(a), int(b)}
    # atten off by one ulp
    a2 = np.nextafter(at, 2.0)
    for fam in "abcdef":
        assert rejected(fam, at2=a2)
    # a live next ray after ABSORBED
    f = groups["f"]
    absorbed = f[st[f] == sx.ABSORBED]
    assert len(absorbed) >= 2
    n2 = nx.copy()
    n2[absorbed[0]] = nx[groups["a"][0]]
    assert [i for i, _ in rejected("f", nx2=n2)] == [int(absorbed[0])]
    # rays whose HIT is undecided (the tangent sphere hits of (a)): a NaN direction, a direction off by 1e-5, the
    # attenuation of another material, another ray's shutter time, and a miss where the record says hit
    und = np.array([i for i in groups["a"] if not ref.hit_decided[i] and st[i] == sx.SCATTERED])
    assert len(und) >= 40
    sx.check(ref, st, nx, at, hits, only=und)
    sx.check(ref, st, nx, at, None, only=und)
    n2 = nx.copy()
    n2["direction"][und[0], 1] = np.nan
    assert {i for i, _ in rejected("a", nx2=n2)} == {int(und[0])}
    n2 = nx.copy()
    n2["direction"][und, 0] += 1e-5
    assert len(rejected("a", nx2=n2)) == 8
    with pytest.raises(sx.CheckError):
        sx.check(ref, st, n2, at, None, only=und)
    a2 = at.copy()
    a2[und[1]] = [0.123, 0.5, 0.5]
    assert {i for i, _ in rejected("a", at2=a2)} == {int(und[1])}
    n2 = nx.copy()
    n2["time"][und[2]] += 0.125
    assert {i for i, _ in rejected("a", nx2=n2)} == {int(und[2])}
    s2, n2, a2 = st.copy(), nx.copy(), at.copy()
    s2[und[3]], n2[und[3]], a2[und[3]] = sx.MISS, nx[absorbed[0]], at[hits["prim"] < 0][0]
    assert {i for i, _ in rejected("a", st2=s2, nx2=n2, at2=a2)} == {int(und[3])}
    # and an absorbed ray reported as scattered, a scattered one as absorbed
    s2 = st.copy()
    s2[absorbed[1]] = sx.SCATTERED
    assert rejected("f", st2=s2)
    scattered = f[st[f] == sx.SCATTERED]
    s2, n2, a2 = st.copy(), nx.copy(), at.copy()
    s2[scattered[-1]], n2[scattered[-1]], a2[scattered[-1]] = sx.ABSORBED, nx[absorbed[0]], 0.0
    assert rejected("f", st2=s2, nx2=n2, at2=a2)
