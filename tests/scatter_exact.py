"""An exact reference for the path-step query's scatter (rtow_path_step): Material::scatter over the REAL numbers, which
answers are certain, and how far a kernel's next ray may be from them.

A helper module for the tests (numpy and the standard library, no GPU), in the style of exact_hits.py, on whose exact
hit it stands.  The semantics are the oracle's (oracle/rtow_oracle.cpp scatter_lambertian / scatter_metal /
scatter_dielectric, reflect, refract, random_in_unit_sphere(PhiloxDraw &), PhiloxDraw::coin_of, ray_color's sky) read
as real-number expressions of their binary64 inputs:
  * the four Philox words of request 1 + bounce of (seed, pixel, sample + sample_first) — Philox4x32-7, restated here in
    integers and held to the oracle's in test_scatter_exact_host.py;
  * the ball point (rs cs, rs sn, r z): z = (w0 >> 8) 2^-24, phi = (w1 >> 8) (2^-24 kHalfPi), r = max of the three
    16-bit uniforms 2^-16, sn = P(phi), cs = P(kHalfPi - phi) with P the degree-9 polynomial that the oracle and
    sin_quarter evaluate (NOT the true sine), rs = r sqrt(1 - z^2); the coin is an integer 2^-32, exact;
  * a triangle's normal is the record's e1 x e2 as binary64 computes it, un-normalised, bit for bit (exact_hits.Scene
    .tri_n); a sphere's is the exact unit vector (p - c) / |p - c| at the exact hit point, faced by the hit's front flag;
  * Lambertian: absorbed iff |n_i - rnd_i| < 1e-8 (the double 1e-8) for all three i, else n + rnd;
    metal: rd - 2 (n.rd) n + fuzz rnd on the UN-normalised rd;
    glass: unit = rd / |rd|, cos = -unit.n, sin = sqrt(1 - cos^2), ratio = front ? 1 / ir : ir; reflect(unit, n) if
    ratio sin > 1, or else if R > coin with R = r0 + (1 - r0) (1 - cos)^5, r0 = ((1 - ratio) / (1 + ratio))^2; else
    refract(unit, n, ratio) = ratio unit - (ratio d + sqrt k) n, d = n.unit, k = 1 - ratio^2 (1 - d^2), and the zero
    vector if k < 0; plus fuzz rnd.  Attenuation: the albedo's bits, (1, 1, 1) for glass.
Every number is a dyadic rational m 2^e held exactly (class D: what fractions.Fraction holds for a binary64, without
the gcd); +, -, * are exact, square roots and reciprocals are taken to 130 bits as exact_hits._sqrt does.

Where the reals leave the oracle's value undefined, binary64 decides:
  * 1 - cos^2 < 0 (a triangle's |n| > 1 makes |cos| > 1): sqrt gives NaN in the strict build and the fast build's
    fast_sqrt gives 0; `ratio sin > 1` is false either way, so the coin is drawn and refract may run.  Here sin := 0.
  * k < 0 in refract: the zero vector (glm's), so the next direction is fuzz rnd.
  * cos < 0 (a hollow sphere hit from inside keeps its outward normal and front = 1): nothing is undefined, 1 - cos > 1
    and R may exceed 1 — then R > coin always.
  * a triangle is hit from its front only (det >= 1e-6), so its ratio is always 1 / ir: a glass triangle shows total
    internal reflection when ir < 1.

Decided and undecided (exact_hits.py's method).  A decision q is DECIDED when |q| exceeds its band; the decisions are
ratio sin > 1, R > coin, k >= 0, the three |n_i - rnd_i| < 1e-8 and, through the hit, the front flag (exact_hits
decides d.(p - c) < 0 with the hit; a ray whose hit is undecided or tied is undecided here).  A Lambertian ray scatters
decidedly as soon as ONE component is decidedly outside the cut.  A ray is scatter-decided when its hit is decided and
every decision on its path is.

Bounds, first order.  u = 2^-53.  Every rounding on an expression's path contributes 2 u |value| (the factor 2 of
exact_hits: gamma_k against k u, and magnitudes taken from the exact operands); input bounds enter through the
derivatives.  Per build the elementary errors are
                                   strict                         fast (RTOW_FAST_MATH, -ffp-contract=fast)
    sqrt x                         1 rounding                     fast_sqrt: seed delta = 5e-8 (rtow_trace_math.h),
                                                                  second-order step 1.5 delta^2 + 4 roundings = RSQ
    1 / ir                         1 rounding                     fast_rcp: 3 fma after the seed, 1.1e-16: 2 roundings
    a / b                          1 rounding                     fast_div = a * fast_rcp(b): 3 roundings
    normalize v = v (1 / sqrt v.v) dot 3 (1.5 after the root),    dot 1.5, fast_rsqrt RSQ, product 1
                                   sqrt 1, 1 / 1, product 1: 4.5
Contraction only removes roundings (an fma rounds once where a product and a sum round twice) and never reorders, so
every other count is the strict form's and holds for both builds:
    ball point: phi 1; P(x): x^2 1, the Horner chain 8, the last product 1 = 10 on S_P = |x| sum |c_j| x^2j, and the
      argument's error through |P'|; kHalfPi - phi 1; 1 - z^2 is exact (48 bits), sqrt, r * sqrt 1, rs * cs 1; r z exact.
    Lambertian: n_i - rnd_i 1, n_i + rnd_i 1.
    reflect(I, n) = I - (n (n.I)) 2: n.I 3 on sum |n_i I_i|, n_i * 1 (the doubling is exact), I_i - 1.
    glass: cos 3, cos^2 1, 1 - 1; 1 - cos 1, (1 - cos)^5 = (x^2 x^2) x 3, 1 - ratio 1, 1 + ratio 1, the quotient, its
      square 1, 1 - r0 1, * 1, + 1; refract: d 3, d^2 1, 1 - 1, ratio^2 1, * 1, 1 - 1, sqrt k, ratio d 1, + 1, ratio I_i
      1, (..) n_i 1, - 1.  (The oracle takes std::pow(1 - cos, 5) where the kernels multiply: one rounding instead of
      three, inside the count.)
    fuzz rnd_i 1, base_i + 1.
    sky: normalize, unit.y + 1 1, 0.5 * exact, 1 - t 1, t c_k 1, + 1.
The square root's sensitivity min(sqrt e, e / sqrt x) to an error e in x carries sin = sqrt(1 - cos^2) and sqrt(k).
Inputs from the exact hit, as exact_hits.py states them: t within E_t; the point within |d_i| E_t + 4 u (|o_i| + |t d_i|);
a sphere's normal within 2 sqrt 3 (max_i point bound + 4 u |c|) / |r| + 8 u (+ RSQ in the fast build, whose normalize
goes through fast_rsqrt); a triangle's normal is exact.  No tolerance is fixed in advance: the bounds are what this
derivation gives, and test_scatter_exact_host.py holds them to the oracle (strict) and to the oracle compiled with
-ffp-contract=fast (fast).

check(ref, status, next, atten, hits): on a decided ray the status is the exact one; next.origin lies within the point
bound of the exact point (and, strict build with hit records, equals hits.point bit for bit); every direction
component lies within its bound; next.time carries the ray's bits; tmax is +inf; atten carries the albedo's bits, or
(1, 1, 1).  ABSORBED, MISS and SKIPPED leave the dead ray; atten is 0, or for a MISS the sky within its bound.  On a
scatter-undecided ray whose hit is decided the answer must be one of the outcomes the band leaves open, within that
outcome's bound.  A ray whose HIT is undecided or tied (a tangent sphere hit, say) must give the scatter outcome of one
of the hits the band leaves open: every outcome (t, E_t, front) of every exact_hits candidate that can be the closest,
with the point and normal bounds its E_t gives, or the sky unless a candidate is a decided hit.  With hit records, on
every ray: a hit record goes with SCATTERED or ABSORBED and a miss record with MISS or SKIPPED, atten carries the bits of
the RECORD's material, the strict origin is the record's point, and the matching outcome is one of the record's
primitive; every scattered direction is finite.
"""
from __future__ import annotations

import math

import numpy as np

import exact_hits as ex

U = ex.U
U2 = 2 * U
STRICT, FAST = ex.STRICT, ex.FAST
SEED_DELTA = 5e-8  # the hardware reciprocal-square-root seed's relative error (rtow_trace_math.h)
RSQ = 1.5 * SEED_DELTA ** 2 + 4 * U
MISS, SCATTERED, ABSORBED, SKIPPED = 0, 1, 2, 3  # RTOW_STEP_*
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
K_POLY = 10
_BITS = 130
# elementary relative errors per build: sqrt, 1 / x, a / b, normalize
ELEM = {STRICT: dict(sqrt=U2, rcp=U2, div=U2, norm=2 * 4.5 * U, nrm_in=0.0),
        FAST: dict(sqrt=RSQ, rcp=2 * U2, div=3 * U2, norm=2 * 2.5 * U + RSQ, nrm_in=RSQ)}
COEF = [float.fromhex(h) for h in ("0x1.ffffffdb33084p-1", "-0x1.555549a9260fdp-3", "0x1.110eb1f04c8ffp-7",
                                   "-0x1.9f6d0201a288bp-13", "0x1.5da8d4e70fe23p-19")]
HALF_PI = 1.5707963267948966
CUT = 1e-8
SKY = (0.5, 0.7, 1.0)


class CheckError(AssertionError):
    pass


# ---- exact dyadic rationals -------------------------------------------------------------------------------------------
class D:
    """m 2^e, exactly."""
    __slots__ = ("m", "e")

    def __init__(self, m, e=0):
        self.m, self.e = m, e

    @staticmethod
    def of(x):
        if isinstance(x, D):
            return x
        if isinstance(x, int):
            return D(x, 0)
        f, e = math.frexp(float(x))
        return D(int(f * (1 << 53)), e - 53)

    def __add__(a, b):
        b = D.of(b)
        if a.e >= b.e:
            return D((a.m << (a.e - b.e)) + b.m, b.e)
        return D(a.m + (b.m << (b.e - a.e)), a.e)

    __radd__ = __add__

    def __neg__(a):
        return D(-a.m, a.e)

    def __sub__(a, b):
        return a + (-D.of(b))

    def __rsub__(a, b):
        return D.of(b) + (-a)

    def __mul__(a, b):
        b = D.of(b)
        return D(a.m * b.m, a.e + b.e)

    __rmul__ = __mul__

    def __abs__(a):
        return D(abs(a.m), a.e)

    def sign(a):
        return (a.m > 0) - (a.m < 0)

    def __float__(a):
        n = a.m.bit_length()
        if n <= 64:
            return math.ldexp(a.m, a.e)
        return math.ldexp(a.m >> (n - 64), a.e + n - 64)  # (64 leading bits, then one rounding: within 2^-52.9)

    def fraction(a):
        from fractions import Fraction
        return Fraction(a.m) * Fraction(2) ** a.e

    def trunc(a, bits=2 * _BITS):
        """The leading `bits` bits (relative error 2^-bits): caps the growth after a root or a reciprocal."""
        n = a.m.bit_length()
        return a if n <= bits else D(a.m >> (n - bits), a.e + n - bits)


def dsqrt(x):
    """sqrt(x) to 130 bits (x >= 0)."""
    if x.m <= 0:
        return D(0, 0)
    m, e = x.m, x.e
    sh = max(0, 2 * _BITS - m.bit_length())
    if (e - sh) & 1:
        sh += 1
    return D(math.isqrt(m << sh), (e - sh) // 2)


def drcp(x):
    """1 / x to 130 bits."""
    sh = _BITS + x.m.bit_length()
    return D((1 << sh) // x.m, -sh - x.e)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _f(x):
    return float(x)


def _sqrt_err(x, e):
    """The error of sqrt at x (taken as 0 below 0) from an error e in x."""
    return math.sqrt(e) if x <= 0 else min(math.sqrt(e), e / math.sqrt(x))


# ---- Philox and the bounce's block --------------------------------------------------------------------------------------
def philox_words(seed, pixel, sample, request, rounds=7):
    c0, c1, c2, c3 = request & 0xffffffff, sample & 0xffffffff, pixel & 0xffffffff, 0
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def coin_of(w):
    return D(((w[3] >> 16) << 16) | ((w[0] & 0xff) << 8) | (w[1] & 0xff), -32)


def _poly(x):
    """(P(x) exactly, S_P on |x|, |P'| on |x|) of the sine polynomial."""
    x2 = x * x
    p = D.of(COEF[4])
    for c in COEF[3::-1]:
        p = p * x2 + D.of(c)
    ax = abs(_f(x))
    s = sum(abs(c) * ax ** (2 * j) for j, c in enumerate(COEF))
    ds = sum((2 * j + 1) * abs(c) * ax ** (2 * j) for j, c in enumerate(COEF))
    return x * p, ax * s, ds


def ball_point(w, build):
    """(rnd [3] exact, bound [3]) of the bounce's point of the unit ball."""
    el = ELEM[build]
    z = D(w[0] >> 8, -24)
    phi = D(w[1] >> 8, 0) * D.of(HALF_PI * 2.0 ** -24)
    r = D(max(w[2] & 0xffff, w[2] >> 16, w[3] & 0xffff), -16)
    psi = D.of(HALF_PI) - phi
    sn, s_sn, d_sn = _poly(phi)
    cs, s_cs, d_cs = _poly(psi)
    fphi, fpsi = abs(_f(phi)), abs(_f(psi))
    e_sn = K_POLY * U2 * s_sn + d_sn * U2 * fphi
    e_cs = K_POLY * U2 * s_cs + d_cs * U2 * (fphi + fpsi)
    rs = r * dsqrt(1 - z * z)
    frs = _f(rs)
    e_rs = (el["sqrt"] + U2) * frs
    rnd = [(rs * cs).trunc(), (rs * sn).trunc(), r * z]
    bound = [frs * e_cs + abs(_f(cs)) * e_rs + U2 * abs(_f(rnd[0])), frs * e_sn + abs(_f(sn)) * e_rs + U2 * abs(_f(rnd[1])),
             0.0]
    return rnd, bound


def sky_exact(d, build):
    """(colour [3] floats, bound [3]) of the background for direction d."""
    el = ELEM[build]
    dd = [D.of(x) for x in d]
    inv = drcp(dsqrt(_dot(dd, dd)))
    uy = _f(dd[1] * inv)
    e_uy = el["norm"] * abs(uy)
    t = 0.5 * (uy + 1.0)
    e_t = 0.5 * (e_uy + U2 * abs(uy + 1.0))
    td = D.of(0.5) * (dd[1] * inv + 1)
    col = [_f((1 - td) + td * D.of(c)) for c in SKY]
    bound = [e_t * (1 + c) + U2 * (abs(1 - t) + abs(t * c)) + U2 * abs(v) for c, v in zip(SKY, col)]
    return col, bound


# ---- one ray's scatter ----------------------------------------------------------------------------------------------------
class Outcome:
    __slots__ = ("status", "dir", "bound", "tag", "prim", "origin", "obound", "albedo")

    def __init__(self, status, dr=None, bound=None, tag=""):
        self.status, self.dir, self.bound, self.tag = status, dr, bound, tag
        self.prim, self.origin, self.obound, self.albedo = -1, None, None, None  # (of a hit: Reference._hit_outcomes)


def _reflect(I, eI, n, dn):
    """(base [3] D, bound [3]) of I - 2 (n.I) n; eI, dn: the bounds of I and n."""
    fI, fn = [abs(_f(x)) for x in I], [abs(_f(x)) for x in n]
    dv = _dot(n, I)
    fd = abs(_f(dv))
    e_d = sum(dn[k] * fI[k] + fn[k] * eI[k] for k in range(3)) + 3 * U2 * sum(fn[k] * fI[k] for k in range(3))
    base, bound = [], []
    for k in range(3):
        term = 2 * (n[k] * dv)
        ft = abs(_f(term))
        e_t = 2 * (dn[k] * fd + fn[k] * e_d) + U2 * ft
        base.append(I[k] - term)
        bound.append(eI[k] + e_t + U2 * (fI[k] + ft))
    return base, bound


def _add_fuzz(base, e_base, fuzz, rnd, e_rnd):
    fz = D.of(fuzz)
    out, bound = [], []
    for k in range(3):
        f = fz * rnd[k]
        ff, fb = abs(_f(f)), abs(_f(base[k]))
        out.append(_f(base[k] + f))
        bound.append(e_base[k] + abs(fuzz) * e_rnd[k] + U2 * ff + U2 * (fb + ff))
    return out, bound


def scatter_outcomes(kind, fuzz, ir, rd, n, dn, front, w, build):
    """(outcomes, decided) of one hit: rd, n [3] floats or D (n with bound dn), the material, the block's words w."""
    el = ELEM[build]
    rd = [D.of(x) for x in rd]
    n = [D.of(x) for x in n]
    rnd, e_rnd = ball_point(w, build)
    if kind == LAMBERTIAN:
        inside, sure = [], []
        for k in range(3):
            q = abs(n[k] - rnd[k]) - D.of(CUT)
            band = dn[k] + e_rnd[k] + U2 * abs(_f(n[k] - rnd[k]))
            inside.append(q.sign() < 0)
            sure.append(abs(_f(q)) > band)
        scat_sure = any(s and not i for i, s in zip(inside, sure))
        abs_sure = all(s and i for i, s in zip(inside, sure))
        dr = [_f(n[k] + rnd[k]) for k in range(3)]
        bound = [dn[k] + e_rnd[k] + U2 * abs(dr[k]) for k in range(3)]
        outs = []
        if not abs_sure:
            outs.append(Outcome(SCATTERED, dr, bound, "lambertian"))
        if not scat_sure:
            outs.append(Outcome(ABSORBED, tag="cut"))
        if all(inside):
            outs.reverse()
        return outs, scat_sure or abs_sure
    if kind == METAL:
        base, e_base = _reflect(rd, [0.0] * 3, n, dn)
        dr, bound = _add_fuzz(base, e_base, fuzz, rnd, e_rnd)
        return [Outcome(SCATTERED, dr, bound, "metal")], True
    # glass
    inv = drcp(dsqrt(_dot(rd, rd)))
    unit = [(x * inv).trunc() for x in rd]
    fu, fn = [abs(_f(x)) for x in unit], [abs(_f(x)) for x in n]
    e_u = [el["norm"] * x for x in fu]
    cos = -_dot(unit, n)
    fcos = _f(cos)
    e_cos = sum(e_u[k] * fn[k] + fu[k] * dn[k] for k in range(3)) + 3 * U2 * sum(fu[k] * fn[k] for k in range(3))
    s2 = (1 - cos * cos).trunc()
    fs2 = _f(s2)
    e_s2 = 2 * abs(fcos) * e_cos + 2 * U2 * (1 + fcos * fcos)
    sin = dsqrt(s2)
    fsin = _f(sin)
    e_sin = _sqrt_err(fs2, e_s2) + el["sqrt"] * fsin
    if front:
        ratio, e_r = drcp(D.of(ir)), el["rcp"] * abs(1.0 / ir)
    else:
        ratio, e_r = D.of(ir), 0.0
    fr = _f(ratio)
    q = ratio * sin - 1
    band = abs(fr) * e_sin + fsin * e_r + U2 * abs(fr) * fsin
    tir, tir_sure = q.sign() > 0, abs(_f(q)) > band
    decided = tir_sure
    want_reflect = tir or not tir_sure
    want_refract = False
    if not (tir and tir_sure):
        a, b = 1 - ratio, 1 + ratio
        fa, fb = abs(_f(a)), abs(_f(b))
        q0 = (a * drcp(b)).trunc()
        fq0 = abs(_f(q0))
        e_q0 = (e_r + U2 * fa) / fb + fa * (e_r + U2 * fb) / (fb * fb) + el["div"] * fq0
        r0 = q0 * q0
        fr0 = _f(r0)
        e_r0 = 2 * fq0 * e_q0 + U2 * fr0
        x = 1 - cos
        fx = abs(_f(x))
        e_x = e_cos + U2 * fx
        x5 = (x * x) * (x * x) * x
        fx5 = abs(_f(x5))
        e_x5 = 5 * fx ** 4 * e_x + 3 * U2 * fx5
        R = r0 + (1 - r0) * x5
        # dR/dr0 = 1 - x^5; the roundings of 1 - r0, of the product and of the sum
        e_R = e_r0 * (1 + fx5) + abs(1 - fr0) * e_x5 + U2 * (abs(1 - fr0) * fx5 + abs(1 - fr0) * fx5 + abs(_f(R)))
        qc = R - coin_of(w)
        rc, rc_sure = qc.sign() > 0, abs(_f(qc)) > e_R
        if not tir:
            decided = decided and rc_sure
        want_reflect = want_reflect or rc or not rc_sure
        want_refract = (not rc) or not rc_sure
        prefer_reflect = tir or rc
    else:
        prefer_reflect = True
    outs = []
    if want_reflect:
        base, e_base = _reflect(unit, e_u, n, dn)
        dr, bound = _add_fuzz(base, e_base, fuzz, rnd, e_rnd)
        outs.append(Outcome(SCATTERED, dr, bound, "reflect"))
    if want_refract:
        dv = _dot(n, unit)
        fd = abs(_f(dv))
        e_d = e_cos
        g = 1 - dv * dv
        e_g = 2 * fd * e_d + 2 * U2 * (1 + fd * fd)
        e2 = ratio * ratio
        fe2, fg = _f(e2), abs(_f(g))
        e_e2 = 2 * abs(fr) * e_r + U2 * fe2
        k = (1 - e2 * g).trunc()
        fk = _f(k)
        e_k = e_e2 * fg + fe2 * e_g + U2 * (2 * fe2 * fg + 1)
        k_pos, k_sure = k.sign() >= 0, abs(fk) > e_k
        if not prefer_reflect:
            decided = decided and k_sure
        ro = []
        if k_pos or not k_sure:
            sk = dsqrt(k)
            fsk = _f(sk)
            e_sk = _sqrt_err(fk, e_k) + el["sqrt"] * fsk
            c = ratio * dv + sk
            fc = abs(_f(c))
            e_c = e_r * fd + abs(fr) * e_d + e_sk + U2 * (2 * abs(fr) * fd + fsk)
            base = [ratio * unit[j] - c * n[j] for j in range(3)]
            e_base = [e_r * fu[j] + abs(fr) * e_u[j] + e_c * fn[j] + fc * dn[j] + 2 * U2 * (abs(fr) * fu[j] + fc * fn[j])
                      for j in range(3)]
            dr, bound = _add_fuzz(base, e_base, fuzz, rnd, e_rnd)
            ro.append(Outcome(SCATTERED, dr, bound, "refract"))
        if not k_pos or not k_sure:
            dr, bound = _add_fuzz([D(0, 0)] * 3, [0.0] * 3, fuzz, rnd, e_rnd)
            ro.append(Outcome(SCATTERED, dr, bound, "refract-zero"))
            if not k_pos:
                ro.reverse()
        outs = ro + outs if not prefer_reflect else outs + ro
    return outs, decided


# ---- the reference over a ray set -------------------------------------------------------------------------------------
class Reference:
    """Per ray of hits_ref.rays (an exact_hits.Reference of the same build): the exact status and the outcomes a kernel
    may produce.  mats [n_materials, 6]: albedo xyz, fuzz, ir, kind (orc.scene_arrays); ids [n, 2] or None: (i, 0);
    bounce: one for all rays, or [n].

    outs[i]: every outcome the band leaves open, the reals' own first (None where the hit is undecided or tied);
    decided[i], hit_decided[i]; origin[i], origin_bound[i] and albedo[i] (what atten must carry) for a hit."""

    def __init__(self, hits_ref, mats, seed, ids, bounce, sample_first=0):
        self.hits, self.build = hits_ref, hits_ref.build
        self.scene, self.rays = hits_ref.scene, hits_ref.rays
        self.mats = np.asarray(mats, np.float64).reshape(-1, 6)
        n = len(self.rays)
        ids = np.stack([np.arange(n), np.zeros(n)], axis=1) if ids is None else np.asarray(ids)
        self.seed, self.ids = int(seed), ids.astype(np.uint64)
        self.request = np.broadcast_to(1 + np.asarray(bounce, np.int64), (n,))
        self.sample_first = int(sample_first)
        self.outs = [None] * n
        self.decided = np.zeros(n, bool)
        self.hit_decided = np.zeros(n, bool)
        for i in range(n):
            self._ray(i)

    def words(self, i, request=None):
        return philox_words(self.seed, int(self.ids[i, 0]), (int(self.ids[i, 1]) + self.sample_first) & 0xffffffff,
                            int(self.request[i]) if request is None else request)

    def surface(self, i):
        """(prim, pe [3] D, point bound [3], normal [3] D or floats, normal bound [3], front) of a decided hit."""
        h = self.hits
        return self.surface_at(i, h.ties[i][0], float(h.t[i]), float(h.E[i]), int(h.front[i]))

    def surface_at(self, i, gp, te, E, front):
        """The same for ray i hitting primitive gp at te +- E with the front flag `front`."""
        sc, r = self.scene, self.rays[i]
        o, d = r["origin"].astype(np.float64), r["direction"].astype(np.float64)
        pe = [D.of(o[k]) + D.of(te) * D.of(d[k]) for k in range(3)]
        pb = np.abs(d) * E + 4 * U * (np.abs(o) + np.abs(te * d)) + 1e-300
        if sc.kind[gp] == ex.TRIANGLE:
            return gp, pe, pb, list(sc.tri_n[sc.index[gp]]), [0.0] * 3, front
        k, ci = int(sc.kind[gp]), int(sc.index[gp])
        if k == ex.SPHERE:
            g = sc.sph[ci]
            c, rad, cm = [D.of(x) for x in g[:3]], g[3], float(np.max(np.abs(g[:3])))
        else:
            g = sc.mov[ci]
            tm = D.of(float(r["time"]))
            c = [D.of(g[j]) + tm * (D.of(g[3 + j]) - D.of(g[j])) for j in range(3)]
            rad = g[6]
            cm = float(np.max(np.abs(g[:3]) + np.abs(float(r["time"]) * (g[3:6] - g[:3]))))
        v = [pe[j] - c[j] for j in range(3)]
        inv = drcp(dsqrt(_dot(v, v)))
        nrm = [(x * inv).trunc() for x in v]
        if not front:
            nrm = [-x for x in nrm]
        nb = 2 * math.sqrt(3) * (float(np.max(pb)) + 4 * U * cm) / abs(rad) + 8 * U + ELEM[self.build]["nrm_in"]
        return gp, pe, pb, nrm, [nb] * 3, front

    def _hit_outcomes(self, i, gp, te, E, front):
        """(outcomes, decided) of ray i hitting gp at te +- E: every outcome carries its primitive, its origin with the
        point bound and the bits atten must carry."""
        gp, pe, pb, nrm, dn, front = self.surface_at(i, gp, te, E, front)
        m = self.mats[self.scene.prim_mat[gp]]
        kind = int(m[5])
        outs, decided = scatter_outcomes(kind, float(m[3]), float(m[4]), self.rays[i]["direction"], nrm, dn, front,
                                         self.words(i), self.build)
        for o in outs:
            o.prim, o.origin, o.obound = gp, np.array([_f(x) for x in pe]), pb
            o.albedo = np.array(m[0:3]) if kind != DIELECTRIC else np.ones(3)
        return outs, decided

    def _sky(self, i):
        col, bound = sky_exact(self.rays[i]["direction"], self.build)
        return Outcome(MISS, col, bound, "sky")

    def _ray(self, i):
        h, r = self.hits, self.rays[i]
        tmax = float(r["tmax"])
        if math.isnan(tmax) or tmax < 0.001:
            self.outs[i], self.decided[i], self.hit_decided[i] = [Outcome(SKIPPED)], True, True
            return
        if not h.decided[i] or len(h.ties[i]) > 1:
            self.outs[i] = self._open_hits(i)
            return
        self.hit_decided[i] = True
        if not h.ties[i]:
            self.outs[i], self.decided[i] = [self._sky(i)], True
            return
        self.outs[i], self.decided[i] = self._hit_outcomes(i, h.ties[i][0], float(h.t[i]), float(h.E[i]), int(h.front[i]))

    def _open_hits(self, i):
        """A ray whose hit is undecided or tied: the scatter outcomes of every hit the band leaves open — each outcome
        (t, E, front) of each candidate of exact_hits that can be the closest, with the point and normal bounds that E
        gives — and the sky unless some candidate is a decided hit.  None when a candidate allows any t (a triangle whose
        cut is undecided at det <= 0): then only what needs no arithmetic is checked."""
        cs = self.hits.cands[i]
        sure = [c for c in cs if c.status == ex.HIT]
        nearest = min((c.t + c.E for c in sure), default=math.inf)
        outs = [] if sure else [self._sky(i)]
        for c in cs:
            for (t, E, front) in c.outs:
                if math.isnan(t) or not math.isfinite(E):
                    return None
                if t - E <= nearest:
                    outs += self._hit_outcomes(i, c.prim, t, E, front)[0]
        return outs


# ---- the checker ------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dead(nx):
    return bool(np.all(nx["origin"] == 0) and np.all(nx["direction"] == 0) and nx["time"] == 0 and nx["tmax"] == -1.0)


def _fits(out, st, nx, at, h):
    """(ok, worst direction error over bound, message) of one answer (h: its hit record or None) against one outcome."""
    if st != out.status:
        return False, 0.0, f"status {st}, exact {out.status} ({out.tag})"
    if out.status == MISS:
        if not np.all(np.abs(at - np.asarray(out.dir)) <= np.asarray(out.bound)):
            return False, 0.0, f"sky {at}, exact {out.dir} +- {out.bound}"
        return True, 0.0, ""
    if h is not None and out.prim >= 0 and int(h["prim"]) != out.prim:
        return False, 0.0, f"hit record of prim {h['prim']}, outcome of prim {out.prim} ({out.tag})"
    if out.status != SCATTERED:
        return True, 0.0, ""
    if not np.array_equal(_bits(at), _bits(out.albedo)):
        return False, 0.0, f"atten {at}, material {out.albedo} ({out.tag})"
    if not np.all(np.abs(nx["origin"] - out.origin) <= out.obound):
        return False, 0.0, f"origin {nx['origin']}, exact {out.origin} +- {out.obound} ({out.tag})"
    err = np.abs(np.asarray(nx["direction"], np.float64) - np.asarray(out.dir))
    b = np.asarray(out.bound)
    if not np.all(err <= b):
        return False, 0.0, f"direction {nx['direction']}, exact {out.dir} +- {b} ({out.tag})"
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)
    return True, float(rel.max()), ""


def check(ref, status, nxt, atten, hits=None, build=None, what="", only=None):
    """The step's status, next rays, attenuations (and hit records, or None) against the reference: see the header.
    `only`: the ray indices to look at (default all).  Returns the counts over those rays, worst_dir_err in units of the
    bound (decided rays) and the tags of the decided outcomes; raises CheckError (`.bad`: the first failures)."""
    assert build is None or build == ref.build
    rays, sc = ref.rays, ref.scene
    bad, worst, tags = [], 0.0, {}

    def fail(i, msg):
        if len(bad) < 8:
            bad.append((int(i), msg))

    sel = np.arange(len(rays)) if only is None else np.asarray(only, np.int64)
    for i in sel:
        st, nx, at = int(status[i]), nxt[i], np.asarray(atten[i], np.float64)
        h = None if hits is None else hits[i]
        outs = ref.outs[i]
        # what needs no arithmetic, on every ray
        if st != SCATTERED:  # the dead ray; atten 0 but for the sky
            if not _dead(nx):
                fail(i, f"status {st} with a live next ray {nx}")
            if st != MISS and not np.all(at == 0.0):
                fail(i, f"status {st} with atten {at}")
        else:
            if _bits(nx["time"]) != _bits(rays[i]["time"]) or nx["tmax"] != math.inf:
                fail(i, f"time {nx['time']} tmax {nx['tmax']}")
            if not np.all(np.isfinite(nx["direction"])):
                fail(i, f"direction {nx['direction']}")
        if h is not None:
            if (int(h["prim"]) >= 0) != (st in (SCATTERED, ABSORBED)):
                fail(i, f"status {st} with the hit record of prim {h['prim']}")
            elif st == SCATTERED:
                m = ref.mats[sc.prim_mat[int(h["prim"])]]
                want = m[0:3] if int(m[5]) != DIELECTRIC else np.ones(3)
                if not np.array_equal(_bits(at), _bits(want)):
                    fail(i, f"atten {at}, the hit record's material {want}")
                if ref.build == STRICT and not np.array_equal(_bits(nx["origin"]), _bits(h["point"])):
                    fail(i, f"origin {nx['origin']} is not the hit record's point {h['point']}")
        if outs is None:  # (a candidate of the hit allows any t)
            if st not in (MISS, SCATTERED, ABSORBED):
                fail(i, f"status {st} on a live ray")
            continue
        msgs = []
        for o in outs if not ref.decided[i] else outs[:1]:
            ok, w, msg = _fits(o, st, nx, at, h)
            if ok:
                if ref.decided[i]:
                    worst = max(worst, w)
                    tags[o.tag] = tags.get(o.tag, 0) + 1
                break
            msgs.append(msg)
        else:
            fail(i, ("decided: " if ref.decided[i] else "undecided: ") + "; ".join(msgs[:6]))
    n = len(sel)
    stats = {"rays": n, "decided": int(ref.decided[sel].sum()), "undecided": int(n - ref.decided[sel].sum()),
             "hit_undecided": int(n - ref.hit_decided[sel].sum()), "worst_dir_err": worst, "tags": tags}
    if bad:
        e = CheckError(f"{what}: {len(bad)}+ failures: {bad}")
        e.bad = bad
        raise e
    return stats
