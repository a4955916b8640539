"""The Philox samplers' lattices, exactly: every value of every field, enumerated — no GPU, no sampling.

The device and the oracle's Philox policy draw from LATTICES (16-, 21-, 24-, 30- and 32-bit fields of one Philox block,
a degree-9 sine), the reference from 53-bit doubles by rejection.  tests/sampler_lattice.py restates the samplers field
by field; the first test pins that restatement to orc_philox_request on random blocks, the others enumerate the
lattices and compare their moments with the continuous distributions' (DESIGN.md section 3 has the table).

Why every first-moment bias is below one lattice step (+ the polynomial's 7e-9).  A field of n bits is k = floor(2^n U)
for a uniform U, the value is g(k / 2^n): the lattice value of the sample that the continuous sampler would map to
g(U).  k / 2^n is in (U - 2^-n, U], so for a g with |g'| <= G the value is within G 2^-n of g(U), sample by sample, and
so is every mean.  G = 1 for the radius, the height, the jitter, the time and the coin; G = pi / 2 per unit of the field
for the azimuth, whose step is (pi / 2) 2^-24 of angle: 2^-24 x pi / 2 of cos or sin at most, and in the mean 2^-25 (f(0)
- f(pi / 2)) — the left Riemann sum's first error term — which is what the enumeration finds.  The polynomial is within
7e-9 of the sine, value by value.  For a second moment g = h^2 with 0 <= h <= 1 the same holds with G = 2.
"""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np

import orc
import sampler_lattice as sl

PI = Fr(math.pi)  # (binary64 pi as a rational: 1.2e-16 from pi, far below every bound here)
STEP16, STEP21, STEP24, STEP32 = Fr(1, 2**16), Fr(1, 2**21), Fr(1, 2**24), Fr(1, 2**32)
K24 = np.arange(2**24, dtype=np.uint64)


SUM_ERR = Fr(1, 10**14)  # of exact_mean, for means of values in [0, 1]


def exact_mean(a):
    """The mean of a binary64 array as a Fraction, to 2^-53 relative per chunk: math.fsum adds a chunk exactly and rounds
    once; the chunk sums are added as rationals."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return sum(Fr(math.fsum(a[i:i + 2**20].tolist())) for i in range(0, len(a), 2**20)) / len(a)


def test_the_restatement_is_the_oracles_sampler_on_random_blocks():
    L = orc.lib()
    R = L.orc_philox_rounds()
    n = 400
    words = np.zeros((n, 4), dtype=np.uint32)
    out = (C.c_uint32 * 4)()
    for p in range(n):
        L.orc_philox4x32((C.c_uint32 * 4)(1 + p % 5, p % 13, p, 0), (C.c_uint32 * 2)(7, 0), out, R)
        words[p] = list(out)
    req = lambda p, kind, k: L.orc_philox_request(7, p, p % 13, 1 + p % 5, kind, k)  # noqa: E731
    ju, jv, jt, a, b = sl.sample_fields(words)
    lens = sl.lens_point(a, b)
    kz, kphi, m, coin = sl.bounce_fields(words)
    ball = sl.ball_point(kz, kphi, m)
    for p in range(n):
        assert [req(p, 0, k) for k in range(5)] == [sl.unit21(ju)[p], sl.unit21(jv)[p], sl.unit21(jt)[p], lens[p, 0], lens[p, 1]]
        assert [req(p, 2, k) for k in range(4)] == [ball[p, 0], ball[p, 1], ball[p, 2], sl.coin_value(coin)[p]]
    # the fields of a bounce's block use every bit of it once: the coin shares no bit with the point
    for word in range(4):
        for bit in range(32):
            w = np.zeros((1, 4), dtype=np.uint32)
            w[0, word] = 1 << bit
            moved = sum(int(f[0] != 0) for f in sl.bounce_fields(w))
            assert moved == 1, (word, bit, moved)


def test_radius_lattice_moments():
    """r = m / 2^16, m the largest of three 16-bit uniforms: P(m) = ((m + 1)^3 - m^3) / 2^48.  Against the largest of
    three uniforms on [0, 1): E r = 3/4, E r^2 = 3/5."""
    n = 2**16
    w = [(m + 1) ** 3 - m**3 for m in range(n)]
    assert sum(w) == 2**48
    e1 = Fr(sum(m * wm for m, wm in enumerate(w)), 2**48 * n)
    e2 = Fr(sum(m * m * wm for m, wm in enumerate(w)), 2**48 * n * n)
    # closed forms: sum m (3 m^2 + 3 m + 1) and sum m^2 (3 m^2 + 3 m + 1) over m < n
    assert e1 == Fr(3, 4) - Fr(1, 2 * n) - Fr(1, 4 * n**2)
    print(f"radius: E r - 3/4 = {float(e1 - Fr(3, 4)):.4e}, E r^2 - 3/5 = {float(e2 - Fr(3, 5)):.4e} (step {float(STEP16):.4e})")
    assert -STEP16 < e1 - Fr(3, 4) < 0
    assert -2 * STEP16 < e2 - Fr(3, 5) < 0
    # (the restatement's radius of field m is m / 2^16, exactly)
    assert sl.radius(np.array([0, 1, 12345, n - 1])).tolist() == [0.0, 2.0**-16, 12345 / 65536, 1.0 - 2.0**-16]


def test_height_lattice_moments():
    """z = k / 2^24, k uniform: closed forms.  Against U[0, 1): E z = 1/2, E z^2 = 1/3."""
    n = 2**24
    e1, e2 = Fr(n - 1, 2 * n), Fr((n - 1) * (2 * n - 1), 6 * n * n)
    z = sl.height(K24)
    assert abs(exact_mean(z) - e1) < SUM_ERR and abs(exact_mean(z * z) - e2) < SUM_ERR  # (z^2 has 48 bits: exact)
    print(f"height: E z - 1/2 = {float(e1 - Fr(1, 2)):.4e}, E z^2 - 1/3 = {float(e2 - Fr(1, 3)):.4e} (step {float(STEP24):.4e})")
    assert e1 - Fr(1, 2) == -STEP24 / 2
    assert -STEP24 < e2 - Fr(1, 3) < 0


def test_azimuth_lattice_moments():
    """phi = k 2^-24 pi / 2 through the polynomial, all 2^24 values.  Against phi uniform on [0, pi / 2): E cos = E sin =
    2 / pi, E cos^2 = 1/2, E sin cos = 1 / pi."""
    cs, sn = sl.azimuth(K24)
    phi = K24.astype(np.float64) * (2.0**-24 * sl.HALF_PI)
    assert np.abs(sn - np.sin(phi)).max() < sl.SIN_ERR and np.abs(cs - np.cos(phi)).max() < sl.SIN_ERR
    # (the polynomial is 1 + 6.7e-9 at pi / 2: cos 0 and sin(pi / 2 - one step) are above 1, inside its error bound)
    assert cs.min() >= 0.0 and sn.min() >= 0.0 and cs.max() <= 1.0 + sl.SIN_ERR and sn.max() <= 1.0 + sl.SIN_ERR
    assert np.abs(cs * cs + sn * sn - 1.0).max() < 2e-8
    poly = Fr(sl.SIN_ERR)
    bias = {"cos": exact_mean(cs) - 2 / PI, "sin": exact_mean(sn) - 2 / PI,
            "cos^2": exact_mean(cs * cs) - Fr(1, 2), "sin cos": exact_mean(sn * cs) - 1 / PI}
    print("azimuth: " + ", ".join(f"E {k} off by {float(v):.4e}" for k, v in bias.items()) + f" (step {float(STEP24):.4e})")
    for k in ("cos", "sin"):
        assert abs(bias[k]) < STEP24 + poly, (k, float(bias[k]))
    for k in ("cos^2", "sin cos"):  # (products of two values in [0, 1] that are each within 7e-9: the rounding of the
        assert abs(bias[k]) < 2 * (STEP24 + poly), (k, float(bias[k]))  # product itself, 1.1e-16, is far below)
    # what the lattice alone does, to first order: + 2^-25 for cos (left end 1, right end 0), - 2^-25 for sin; the rest
    # is the polynomial's own mean error, below its bound
    assert abs(bias["cos"] - STEP24 / 2) < poly and abs(bias["sin"] + STEP24 / 2) < poly


def test_jitter_time_and_coin_lattices():
    """Jitter and shutter time: k / 2^21, mean 1/2 - 2^-22.  The coin: c / 2^32 over all 32-bit c, so P(coin < p) =
    ceil(2^32 p) / 2^32, in [p, p + 2^-32)."""
    n = 2**21
    u = sl.unit21(np.arange(n, dtype=np.uint64))
    assert exact_mean(u) == Fr(1, 2) - STEP21 / 2 and u[0] == 0.0 and u[-1] == 1.0 - 2.0**-21  # (42 bits: exact)
    # the coin's value is its field / 2^32 exactly, below 1, and ordered like the field: count the fields below p
    edge = np.array([0, 1, 2**31, 2**32 - 1], dtype=np.uint64)
    assert sl.coin_value(edge).tolist() == [0.0, 2.0**-32, 0.5, 1.0 - 2.0**-32]
    rng = np.random.default_rng(5)
    for p in [0.0, 2.0**-33, 2.0**-32, 0.04, 0.5, 1.0 - 2.0**-32, 1.0 - 2.0**-40, 1.0] + rng.random(50).tolist():
        count = math.ceil(Fr(p) * 2**32)  # fields c with c / 2^32 < p
        assert (count == 0 or sl.coin_value(np.uint64(count - 1)) < p) and (count == 2**32 or sl.coin_value(np.uint64(count)) >= p)
        assert 0 <= Fr(count, 2**32) - Fr(p) < STEP32


def test_lens_lattice_bounds():
    """The lens point rho (cos t, sin t): rho = sqrt(a / 2^32), t = 30 bits inside a quadrant of two more bits.
    Stated as bounds: the radius in closed form, the angle by enumerating its top 24 bits + a Lipschitz term for the low
    six.  Against the uniform disk: E rho = 2/3, E rho^2 = 1/2, E x = E y = 0, E x^2 = E y^2 = 1/4."""
    # radius: sum_{k<N} sqrt(k) lies between the integrals of sqrt over [0, N-1] and [1, N] (sqrt increases), so
    # (2/3) (1 - 1/N)^(3/2) <= E rho <= (2/3) (1 - N^(-3/2)): 0 < 2/3 - E rho < 1/N.  The inequality itself, checked by
    # enumeration where that is cheap (N = 2^16 .. 2^20), then used at N = 2^32:
    for bits in (16, 20):
        N = 2**bits
        e = exact_mean(np.sqrt(np.arange(N, dtype=np.float64) / N))
        lo, hi = Fr(2, 3) * Fr((1 - 1 / N) ** 1.5) - Fr(1, 10**15), Fr(2, 3) * (1 - Fr(N ** -1.5)) + Fr(1, 10**15)
        assert lo <= e <= hi and 0 < Fr(2, 3) - e < Fr(1, N)
    # E rho^2 = E a / 2^32 = 1/2 - 2^-33 exactly.
    # angle: the 2^24 angles with the low six bits zero ...
    cs, sn = sl.lens_angle(K24 << np.uint64(6))
    assert np.array_equal(cs, sl.azimuth(K24)[0]) and np.array_equal(sn, sl.azimuth(K24)[1])  # (the same lattice)
    # ... and the low six bits move the angle by less than 2^-24 pi / 2; the polynomial's slope is at most 1 + 1e-7
    th = np.linspace(0.0, sl.HALF_PI, 200001)
    slope = np.abs(np.diff(sl.sin_quarter(th)) / np.diff(th)).max()
    assert slope < 1.0 + 1e-7
    lip = Fr(slope) * Fr(sl.HALF_PI) * STEP24
    c2, s2 = exact_mean(cs * cs), exact_mean(sn * sn)
    # the quadrants send (cos, sin) to (c, s), (-s, c), (-c, -s), (s, -c): whatever the angle's lattice, E x = E y = 0
    # exactly (the four signs cancel term by term), and E x^2 = E y^2 = E rho^2 (E c^2 + E s^2) / 2
    pts = sl.lens_point(np.full(4, 2**31, dtype=np.uint64), (np.arange(4, dtype=np.uint64) << np.uint64(30)) | np.uint64(12345))
    assert np.array_equal(pts[0], -pts[2]) and np.array_equal(pts[1], -pts[3])
    assert np.array_equal(np.abs(pts[:, 0]), np.abs(pts[[1, 0, 3, 2], 1]))
    ex2_lo = (Fr(1, 2) - STEP32 / 2) * (c2 + s2 - 4 * lip) / 2
    ex2_hi = (Fr(1, 2) - STEP32 / 2) * (c2 + s2 + 4 * lip) / 2
    print(f"lens: E x^2 - 1/4 in [{float(ex2_lo - Fr(1, 4)):.4e}, {float(ex2_hi - Fr(1, 4)):.4e}]; "
          f"E c^2 + E s^2 - 1 = {float(c2 + s2 - 1):.4e}")
    assert abs(ex2_lo - Fr(1, 4)) < 2 * (STEP24 + Fr(sl.SIN_ERR)) and abs(ex2_hi - Fr(1, 4)) < 2 * (STEP24 + Fr(sl.SIN_ERR))


def test_scatter_offset_bias_per_component():
    """The bounce's point (r s cos, r s sin, r z), s = sqrt(1 - z^2): the three fields are independent (disjoint bits), so
    each component's mean is a product of enumerated means.  Against 3/8 per component (the octant of the unit ball).
    These are the per-bounce biases of DESIGN.md section 3's table."""
    n = 2**16
    w = [(m + 1) ** 3 - m**3 for m in range(n)]
    er = Fr(sum(m * wm for m, wm in enumerate(w)), 2**48 * n)
    z = sl.height(K24)
    es, ez = exact_mean(np.sqrt(1.0 - z * z)), exact_mean(z)
    cs, sn = sl.azimuth(K24)
    bias = [er * es * exact_mean(cs) - Fr(3, 8), er * es * exact_mean(sn) - Fr(3, 8), er * ez - Fr(3, 8)]
    print("scatter offset: E (x, y, z) - 3/8 = " + ", ".join(f"{float(b):.4e}" for b in bias))
    # E s against pi / 4: s falls from 1 to 0 and is not Lipschitz at z = 1, but it is monotone, so the left Riemann sum
    # is above the integral by at most (s(0) - s(1)) / 2^24 = one step; sqrt rounds each value by <= 1.2e-16
    assert 0 < es - PI / 4 < STEP24 + Fr(1, 10**15)
    # each factor is within its step (+ 7e-9 for the polynomial) of a value <= 1 (the polynomial's: <= 1 + 7e-9), so the
    # product of three is within the sum of the three, times 1 + 7e-9
    for b in bias:
        assert abs(b) < (STEP16 + 2 * STEP24 + Fr(sl.SIN_ERR)) * (1 + Fr(sl.SIN_ERR)), float(b)
    # the radius lattice's - 2^-17 is 100 times the other fields' steps: inwards on every axis
    assert all(b < 0 for b in bias)
