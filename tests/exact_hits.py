"""An exact reference for the ray queries (rtow_intersect / rtow_occluded): which answers are certain, and how far a
kernel's answer may be from them.

A helper module for the tests (numpy and the standard library, no GPU).  The semantics are the reference's hit tests
(oracle/rtow_oracle.cpp sphere_hit_helper / triangle_hit, src/common-model.cpp) over the REAL numbers: every binary64
input is the dyadic rational it denotes, including tmin (the double nearest 0.001), tmax and the double 1e-6 of the
triangle cut.
  * triangle A, B, C: n = (B - A) x (C - A), det = -d.n, ao = o - A, ud = e2.(ao x d), vd = -e1.(ao x d), td = ao.n;
    a hit iff det >= 1e-6, ud >= 0, vd >= 0, ud + vd <= det, tmin det <= td <= tmax det; t = td / det; front_face 1.
  * sphere (c, r), the moving sphere's c = c0 + time (c1 - c0): oc = o - c, a = d.d, h = oc.d, c' = oc.oc - r^2,
    disc = h^2 - a c'; the near root (-h - sqrt disc) / a if it lies in [tmin, tmax], else the far root; front_face =
    (d.(p - c) < 0) xor (r < 0), i.e. (near root and disc > 0) xor (r < 0).  The kernels evaluate d.(p - c) at their
    computed p: -+sqrt(disc) + a (t_computed - t), so front_face is decided when sqrt(disc) > a E_t + tau S_ff.  The roots are compared with tmin and tmax
    exactly, by sign and squaring; where a value is needed it is computed to 130 bits with math.isqrt.

Decided and undecided.  Every decision q of a test is DECIDED when |q| > tau * S_q, where S_q is q's expression
evaluated on the absolute values of its operands, in the form the kernels evaluate.  A floating-point evaluation of an
expression of depth k (k roundings on its longest path, inputs included) is within gamma_k * S_q of q, gamma_k ~ k u,
u = 2^-53; so on a decided decision every kernel takes the exact branch.  A ray is decided when every decision that can
change its answer is, and the gap between its nearest and its second-nearest hit exceeds both their t bounds.

  * strict (-ffp-contract=off, the reference's expressions): the records round e1 = B - A, e2 = C - A (1), n = e1 x e2
    (+2: 3); det = -d.n (+3: 6); ao (1), ao x d (3), ud, vd = dot (6); u + v <= 1 on ud * (1/det) (+3: 9); t = td * (1/det)
    (8).  Sphere: the moving centre c0 + time * dc (2), oc (3), h (6), c' (+1 for the record's r^2: 7), disc (9).
    k = 9; tau_strict = 2 * 9 u = 18 u (a factor 2 for gamma_k = k u / (1 - k u) and for S taken from the exact operands).
  * fast (-ffp-contract=fast, rtow_trace_hit.h under RTOW_FAST_MATH): the same forms with fewer roundings, plus the
    GRID walk on the unit direction (rtow_trace_grid.h): |d|^2 (3), rsqrt and one Newton step (2), d * inv_len (1) perturb
    every operand that carries d by 6 u, which the quadratic terms of disc see twice (+12 on 9: k = 21, rounded down
    to 17 for the contractions: every fma saves one rounding in each of the eight two-term sums above).  The fat 48-byte
    cell-list entries test h = o.d - C.d and c' = |o|^2 - 2 C.o + (|C|^2 - r^2) in WORLD coordinates, so fast S_q takes
    |o_i| + |c_i| where strict takes |o_i - c_i|.  tau_fast = 2 * 17 u = 34 u.
  * f32 (RTOW_F32: rtow_trace_f32.hip; sphere_test<float> / triangle_test<float> of rtow_trace_hit.h on the binary32
    records of leaf_test, rtow_trace_bvh.h; u32 = 2^-24).  Every record word is the binary64 record's rounded (1).
    Sphere, the strict form oc = o - c on rounded o and c, so S takes |o_i| + |c_i| like the fast world form: the
    moving centre c0 + time * delta (delta 1, product 2, sum 3), oc (4), h (7), c' (+1 for the record's r^2: 8), disc
    (10).  Triangle, the det-multiplied form: det = -d.n (n 1, +3: 4), ao = o - A (2), ao x d (4), ud, vd (7),
    ud + vd <= det (8), td = ao.n (5), tmin * det (5): 8.  K32_ARITH = 10 is this arithmetic alone.  The ray: a primary
    is llc + u h + v w - from in binary32 (rtow_trace_body.h): cam32 (1), u = (j + ju) * inv_wm1 (sum 1, product 2),
    u * h (3), + llc (4), + v * w (5), - from (6) — K_CAM = 6 roundings on the magnitudes |llc_i| + |u h_i| + |v w_i| +
    |from_i|, which stand for |d_i| (and |origin_i| + the lens offset for |o_i|) in S_q; the quadratic terms of disc
    see them twice (+12 on 10): K32 = 22, no discount for contractions (they are the compiler's choice), tau_f32 =
    2 * 22 u32 = 44 u32.  fast_rcp / fast_rsqrt / fast_sqrt for float (rtow_trace_math.h: the hardware's 1 ulp
    seed, one Newton step on rcp and rsq) are within these counts like the fast build's.  The binary32 Closest::t
    adds u32 |t| to every t bound (also to those of spheres tested in binary64).  Spheres that a kernel tests in
    binary64 on the widened ray (the GRID walk's large list, every sphere of the BVH and STREAM kernels) see the
    ray's error alone: `large`.  Because S_q on |o_i| + |c_i| overstates the strict form's error by (|o| + |c|) /
    |o - c| squared, a second bound stands beside it where the ray's error is known in absolute terms (operr, derr):
    TAU_ARITH S_q' + 2 D_q with S_q' on |o_i - c_i|, and for a sphere D_disc = 2 a max(|r|, b) |do + s dd| + |disc| da / a
    (disc = a (r^2 - b^2): the line moves by |do + s dd| at its point nearest the centre) and the t bound through
    dt = (p - c).(do + t dd) / sqrt(disc); tests/test_f32_audit_host.py holds both bounds to binary32 restatements of
    the tests.
  * every other test in the fast build (1/a by rcp + Newton, t = td * rcp(det), the t * det forms of the triangle test)
    is within those counts.
  * tmin / tmax against a root t: decided when |t - tmin| (|t - tmax|) exceeds t's bound E_t (below).

The t bound (condition-aware, for the form that computes t):
  * triangle t = td / det:   E_t = tau (S_td + |t| S_det) / |det|;
  * sphere t = (-h -+ sqrt disc) / a:   E_t = (tau S_h + min(sqrt(tau S_disc), tau S_disc / sqrt disc) + tau sqrt disc
    + tau |t| a) / a — the square root's sensitivity min(sqrt e, e / sqrt x) to an error e in x is what makes a nearly
    tangent ray's root uncertain;
  * plus u |t| for the rounding of the exact t to binary64 (and the filter's own bound, below, where the filter decided).
The hit point: |p_i - (o_i + t d_i)| <= |d_i| E_t + 4 u (|o_i| + |t d_i|).  A sphere's normal (p - c) * rsqrt(|p - c|^2):
within 2 sqrt(3) (max_i |p_i err| + 4 u |c|) / |r| + 8 u of the exact unit normal (dot 3, rsqrt with one Newton step 2,
product 1: 6 u, rounded up).  A triangle's normal is the record's e1 x e2, bit for bit.

The fast build's GRID walk applies the triangle cut to the UNIT direction: det / |d| >= 1e-6 (rtow_trace_grid.h walks
d / |d|; the triangle test is the render's).  For |d| = 1 the two agree; the reference is told which one a walk uses
(`unit_cut`).

First-k-hits sequences (rtow_first_hits; sequence_decided, check_sequences).  The exact answer is every primitive whose
test accepts a t in [tmin, tmax], ascending by (t, insertion index), cut at k.  Per ray, with H its HIT candidates
(decided hits) sorted by exact t and the UND candidates beside them:
  * decided at k: every gap between consecutive members of H up to and including the one between entry k - 1 and the
    first one left out is clear, t[j+1] - E[j+1] > t[j] + E[j] (so no kernel can order or cut them otherwise), and no UND
    candidate has an outcome with t - E at or before t[k-1] + E[k-1]; with fewer than k decided hits any UND candidate
    makes the ray undecided.  tmax is one of every candidate's decisions already (|t - tmax| > E_t), and the bound of a
    full list is the computed t of entry k - 1: within E[k-1] of t[k-1], so what the clear gap separates from it stays
    out and what lies in front of it stays in.  On a decided ray the primitive sequence is H cut at k and the count is
    min(|H|, k) (members of an exact tie, equal exact t, in either order: a tie is never clear, so this can only matter
    to a caller that passes its own notion of decided).
  * every ray, decided or not (what the band allows): 0 <= count <= k, slots >= count the miss record, slots < count
    distinct primitives; every reported primitive is a candidate of the ray (it may hit within tmax) and its record
    has t within E of one of that candidate's outcomes with that outcome's front_face — for a decided hit also the
    point, the triangle normal and the sphere normal of the closest-hit rules; reported t is non-decreasing, and
    bit-equal consecutive t come in ascending insertion index (not required of the fast GRID walk, which sorts
    distances t |d| and converts them at output: two distances that differ may round to one t); a decided hit that
    is not reported requires count == k and t + E >= t_reported[k-1] - E(the candidate reported there): it may be
    missing only from behind the cut.
  * the band is TAU as for the other queries: the fast GRID walk's second fast_rsqrt at output repeats the walk's own
    (the same operands, the same instruction sequence: the same bits), so distance * inv_len at output inverts the
    direction's scaling with the one rounding the closest-hit walk spends there (d * inv_len: 1, in the count above).

Speed.  A vectorised binary64 filter runs over every (ray, primitive) pair first, with the forward error bound
GF * S_q, GF = 32 u (the filter's own expressions are at most 10 roundings deep): a pair all of whose decisions are
beyond (tau + GF) S_q is decided there.  The few others go to the exact path (fractions.Fraction).  Large meshes take a
box prefilter (exact vertex bounds, padded by 1e-6 of the scene's scale: far more than any band) before the filter.
"""
from __future__ import annotations

import math
from fractions import Fraction as Fr

import numpy as np

U = 2.0 ** -53
TMIN = 0.001
CUT = 1e-6
U32 = 2.0 ** -24
STRICT, FAST, F32 = "strict", "fast", "f32"
K32 = 22  # (the header's count for the binary32 build)
K32_ARITH = 10  # (... of the binary32 tests alone, on the values they are given)
TAU = {STRICT: 18 * U, FAST: 34 * U, F32: 2 * K32 * U32}
TAU_ARITH = 2 * K32_ARITH * U32
GF = 32 * U
SPHERE, MOVING, TRIANGLE = 0, 1, 2
MISS, HIT, UND = 0, 1, 2
_SQRT_BITS = 130
_FTMIN, _FCUT = Fr(TMIN), Fr(CUT)


def _second(x, y):
    return y


class CheckError(AssertionError):
    pass


class Cand:
    """One (ray, primitive) pair that may hit.  status HIT: decided (t, E, front are the exact answer's); UND: the
    outcomes a kernel may produce, outs = [(t, E, front)] (t NaN: any t).  hit: the exact answer."""
    __slots__ = ("prim", "status", "hit", "t", "E", "front", "outs", "tex", "key")

    def __init__(self, prim, status, hit, t, E, front, outs, tex=None, key=None):
        self.prim, self.status, self.hit, self.t, self.E, self.front, self.outs = prim, status, hit, t, E, front, outs
        self.tex, self.key = tex, key

    def __repr__(self):
        return f"Cand(prim={self.prim}, status={self.status}, hit={self.hit}, t={self.t}, E={self.E}, outs={self.outs})"


# ---- the scene ----------------------------------------------------------------------------------------------------
class Scene:
    """Geometry per class and the insertion order: sph [n,4], mov [n,8], tri [n,9], kind / index / material per
    inserted primitive (support_scenes.SceneView has these fields)."""

    def __init__(self, sph, mov, tri, kind, index, prim_mat):
        self.sph = np.asarray(sph, np.float64).reshape(-1, 4)
        self.mov = np.asarray(mov, np.float64).reshape(-1, 8)
        self.tri = np.asarray(tri, np.float64).reshape(-1, 9)
        self.kind = np.asarray(kind, np.int32)
        self.index = np.asarray(index, np.int32)
        self.prim_mat = np.asarray(prim_mat, np.int32)
        self.ins = {}
        for p, (k, i) in enumerate(zip(self.kind, self.index)):
            self.ins[(int(k), int(i))] = p
        g = self.tri
        e1, e2 = g[:, 3:6] - g[:, :3], g[:, 6:9] - g[:, :3]
        self.tri_n = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0],
                               e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], axis=1)  # the record's n (rtow_scene_records.h)

    @classmethod
    def of(cls, v):
        return cls(v.sph, v.mov, v.tri, v.kind, v.index, v.prim_mat)

    @classmethod
    def class_major(cls, sph, mov, tri, pmat):
        """Insertion order = class-major order (rtow.Scene built by support_scenes.scene_of); pmat class-major."""
        ns, nm, nt = len(np.reshape(sph, (-1, 4))), len(np.reshape(mov, (-1, 8))), len(np.reshape(tri, (-1, 9)))
        kind = np.array([SPHERE] * ns + [MOVING] * nm + [TRIANGLE] * nt, np.int32)
        index = np.concatenate([np.arange(ns), np.arange(nm), np.arange(nt)]).astype(np.int32)
        return cls(sph, mov, tri, kind, index, pmat)

    def scale(self):
        pts = [self.sph[:, :3], self.mov[:, :3], self.mov[:, 3:6]] + [self.tri[:, 3 * k:3 * k + 3] for k in range(3)]
        pts = np.concatenate([p for p in pts if len(p)] or [np.zeros((1, 3))])
        return max(1.0, float(np.max(np.abs(pts))))


# ---- exact helpers ------------------------------------------------------------------------------------------------
def _f3(v):
    return [Fr(float(x)) for x in v]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(x, y):
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def _sqrt(x: Fr) -> Fr:
    """sqrt(x) to _SQRT_BITS bits (x >= 0)."""
    if x == 0:
        return Fr(0)
    p, q = x.numerator, x.denominator
    sh = max(0, 2 * _SQRT_BITS - (p.bit_length() - q.bit_length()))
    sh += sh & 1
    return Fr(math.isqrt((p << sh) // q), 1 << (sh // 2))


def _gt(x: Fr, band: float) -> bool:
    """|x| > band, exactly (band a float)."""
    return abs(x) > Fr(band) if math.isfinite(band) else False


# ---- the exact path, one pair ---------------------------------------------------------------------------------------
def _cross_abs(x, y):
    return [x[1] * y[2] + y[1] * x[2], x[2] * y[0] + y[2] * x[0], x[0] * y[1] + y[0] * x[1]]


def exact_triangle(o, d, tmax, A, B, C, tau, unit_cut=False, u=U, aomag=None, dmag=None, pert=None):
    """(hit, decided-or-not outcome, t Fraction, E, outs): see Cand.  aomag, dmag: the magnitudes that stand for
    |o - A| and |d| in S (the binary32 build: rounded inputs, camera rays), default the operands' own."""
    o, d, A, B, C = _f3(o), _f3(d), _f3(A), _f3(B), _f3(C)
    e1 = [B[k] - A[k] for k in range(3)]
    e2 = [C[k] - A[k] for k in range(3)]
    n = _cross(e1, e2)
    det = -_dot(d, n)
    ao = [o[k] - A[k] for k in range(3)]
    dao = _cross(ao, d)
    ud, vd, td = _dot(e2, dao), -_dot(e1, dao), _dot(ao, n)
    fa = lambda v: [abs(float(x)) for x in v]  # noqa: E731
    E1a, E2a, AOa, Da = fa(e1), fa(e2), fa(ao), fa(d)
    if aomag is not None:
        AOa = [float(x) for x in aomag]
    if dmag is not None:
        Da = [float(x) for x in dmag]
    Na = [E1a[1] * E2a[2] + E2a[1] * E1a[2], E1a[2] * E2a[0] + E2a[2] * E1a[0], E1a[0] * E2a[1] + E2a[0] * E1a[1]]
    DAOa = [AOa[1] * Da[2] + Da[1] * AOa[2], AOa[2] * Da[0] + Da[2] * AOa[0], AOa[0] * Da[1] + Da[0] * AOa[1]]
    S_det, S_ud, S_vd, S_td = (sum(x * y for x, y in zip(p, q)) for p, q in ((Da, Na), (E2a, DAOa), (E1a, DAOa), (AOa, Na)))
    if pert is None:
        b_det, b_ud, b_vd, b_td = tau * S_det, tau * S_ud, tau * S_vd, tau * S_td
        b_sum = tau * (S_det + S_ud + S_vd)
    else:  # absolute input errors eo, ed: first-order terms D_q beside the arithmetic band taub on the plain magnitudes
        eo, ed, aonat, taub, comb = pert
        Dn = fa(d)
        DAOn = _cross_abs(aonat, Dn)
        DAOe = [x + y for x, y in zip(_cross_abs(eo, Dn), _cross_abs(fa(ao), ed))]
        sm = lambda p, q: sum(x * y for x, y in zip(p, q))  # noqa: E731
        n_det, n_ud, n_vd, n_td = sm(Dn, Na), sm(E2a, DAOn), sm(E1a, DAOn), sm(aonat, Na)
        D_det, D_ud, D_vd, D_td = sm(ed, Na), sm(E2a, DAOe), sm(E1a, DAOe), sm(eo, Na)
        b_det = comb(tau * S_det, taub * n_det + 2 * D_det)
        b_ud = comb(tau * S_ud, taub * n_ud + 2 * D_ud)
        b_vd = comb(tau * S_vd, taub * n_vd + 2 * D_vd)
        b_td = comb(tau * S_td, taub * n_td + 2 * D_td)
        b_sum = b_det + b_ud + b_vd
    dd = _dot(d, d)
    if unit_cut:  # det >= 1e-6 |d|
        ok_cut = det >= 0 and det * det >= _FCUT * _FCUT * dd
        hi, lo = det - Fr(b_det), det + Fr(b_det)  # decided: det -+ band both on one side of 1e-6 |d|
        above = hi > 0 and hi * hi > _FCUT * _FCUT * dd
        below = lo < 0 or lo * lo < _FCUT * _FCUT * dd
        dec_cut = above or below
    else:
        ok_cut = det >= _FCUT
        dec_cut = _gt(det - _FCUT, b_det)
    if not ok_cut and dec_cut:
        return None
    if det <= 0:  # (the cut is undecided and the forms below mean nothing: any outcome)
        return Cand(-1, UND, False, None, math.inf, 1, [(math.nan, math.inf, 1)])
    t = td / det
    at = abs(float(t))
    if pert is None:
        S_t = S_td + at * S_det
        E = tau * S_t / float(det) + u * at
    else:
        E = (b_td + at * b_det) / float(det) + u * at
    decs = [(ud >= 0, _gt(ud, b_ud)), (vd >= 0, _gt(vd, b_vd)),
            (det - ud - vd >= 0, _gt(det - ud - vd, b_sum)),
            (t >= _FTMIN, _gt(t - _FTMIN, E))]
    if math.isfinite(tmax):
        decs.append((t <= Fr(tmax), _gt(Fr(tmax) - t, E)))
    decs.append((ok_cut, dec_cut))
    hit = all(ok for ok, _ in decs)
    if any(not ok and dec for ok, dec in decs):
        return None
    if all(dec for _, dec in decs):
        return Cand(-1, HIT, True, float(t), E, 1, [(float(t), E, 1)], tex=t)
    return Cand(-1, UND, hit, float(t) if hit else None, E, 1, [(float(t), E, 1)], tex=t)


def exact_sphere(o, d, tmax, c, r, omag, tau, u=U, dmag=None, pert=None):
    """c: the exact centre (Fractions); omag[i]: the |o_i - c_i| (strict) or |o_i| + |c_i| (fast) of S, per axis; dmag:
    the magnitudes that stand for |d_i| in S (default |d_i|)."""
    o, d = _f3(o), _f3(d)
    r = Fr(float(r))
    oc = [o[k] - c[k] for k in range(3)]
    a = _dot(d, d)
    h = _dot(oc, d)
    cc = _dot(oc, oc) - r * r
    disc = h * h - a * cc
    Da = [abs(float(x)) for x in d]
    fa = float(a)
    faS = fa
    if dmag is not None:
        Da = [float(x) for x in dmag]
        faS = sum(x * x for x in Da)
    S_h = sum(m * x for m, x in zip(omag, Da))
    S_c = sum(m * m for m in omag) + float(r) ** 2
    S_d = S_h * S_h + faS * S_c
    if pert is None:
        b_h, b_d = tau * S_h, tau * S_d
    else:  # (eo, ed, plain omag, arithmetic band, large: tested in binary64) — see Reference
        eo, ed, onat, taub, lg, comb = pert
        Dn = [abs(float(x)) for x in d]
        ocn = [abs(float(x)) for x in oc]
        sm = lambda p, q: sum(x * y for x, y in zip(p, q))  # noqa: E731
        n_h = sm(onat, Dn)
        n_d = n_h * n_h + fa * (sm(onat, onat) + float(r) ** 2)
        D_h = sm(eo, Dn) + sm(ocn, ed)
        D_a = 2 * sm(Dn, ed)
        # disc = a (r^2 - b^2), b the distance of the centre from the line: the line moves by |eo + |s| ed| at its
        # closest point o + s d, s = -h / a (termwise bounds of h^2 and a c' would not see that the two cancel)
        fs = abs(float(h)) / fa
        fb = math.sqrt(max(float(_dot(oc, oc)) - float(h) ** 2 / fa, 0.0))
        mv = math.sqrt(sum((eo[k] + fs * ed[k]) ** 2 for k in range(3)))
        D_d = 2 * fa * max(abs(float(r)), fb) * mv + D_a * abs(float(disc)) / fa
        a_h, a_d, a_a = taub * n_h + 2 * D_h, taub * n_d + 2 * D_d, taub * fa + 2 * D_a
        b_h, b_d, b_a = (a_h, a_d, a_a) if lg else (comb(tau * S_h, a_h), comb(tau * S_d, a_d), comb(tau * faS, a_a))
    dec_disc = _gt(disc, b_d)
    inward = r < 0
    if disc < 0:
        if dec_disc:
            return None
        t0 = float(-h / a)
        if pert is None:
            E0 = (tau * S_h + math.sqrt(tau * S_d) + tau * abs(t0) * faS) / fa + u * abs(t0)
        else:
            E0 = (b_h + math.sqrt(b_d) + abs(t0) * b_a) / fa + u * abs(t0)
        return Cand(-1, UND, False, None, E0, int(inward), [(t0, E0, 0), (t0, E0, 1)])
    sq = _sqrt(disc)
    fsq = float(sq)
    t1, t2 = (-h - sq) / a, (-h + sq) / a

    def E(t):
        at = abs(float(t))
        if pert is not None:
            # the arithmetic alone on the strict form, and the input errors through dt = -(p - c).(do + t dd) /
            # ((p - c).d), (p - c).d = -+sqrt(disc): the termwise forms above do not see that h^2 and a c' cancel
            an_d = taub * n_d
            s = math.sqrt(an_d) if fsq == 0 else min(math.sqrt(an_d), an_d / fsq)
            pc = [abs(float(oc[k] + t * d[k])) for k in range(3)]
            ein = math.inf if fsq == 0 else 2 * sum(pc[k] * (eo[k] + at * ed[k]) for k in range(3)) / fsq
            new = (taub * n_h + s + taub * fsq + taub * at * fa) / fa + ein + u * at
            if lg:
                return new
            s = math.sqrt(tau * S_d) if fsq == 0 else min(math.sqrt(tau * S_d), tau * S_d / fsq)
            return comb((tau * S_h + s + tau * fsq + tau * at * faS) / fa + u * at, new)
        s = math.sqrt(tau * S_d) if fsq == 0 else min(math.sqrt(tau * S_d), tau * S_d / fsq)
        return (tau * S_h + s + tau * fsq + tau * at * faS) / fa + u * at

    E1, E2 = E(t1), E(t2)
    tmx = Fr(tmax) if math.isfinite(tmax) else None
    X = -h - _FTMIN * a  # t1 >= tmin  <=>  X >= sqrt(disc)
    n1 = X >= 0 and X * X >= disc
    if tmx is None:
        x1 = x2 = True
    else:
        Y = -h - tmx * a  # t1 <= tmax  <=>  Y <= sqrt(disc)
        x1 = Y <= 0 or Y * Y <= disc
        W = tmx * a + h  # t2 <= tmax  <=>  sqrt(disc) <= W
        x2 = W >= 0 and disc <= W * W
    Z = _FTMIN * a + h  # t2 >= tmin  <=>  sqrt(disc) >= Z
    n2 = Z <= 0 or disc >= Z * Z
    dn1, dn2 = _gt(t1 - _FTMIN, E1), _gt(t2 - _FTMIN, E2)
    dx1 = tmx is None or _gt(tmx - t1, E1)
    dx2 = tmx is None or _gt(tmx - t2, E2)
    S_ff = lambda t: sum(Da[k] * (omag[k] + abs(float(t)) * Da[k]) for k in range(3))  # noqa: E731
    f_near = int((disc > 0) != inward)
    f_far = int(inward)
    if n1:
        hit, t, Et, front = x1, t1, E1, f_near
        dec = dn1 and dx1
    else:
        hit, t, Et, front = n2 and x2, t2, E2, f_far
        dec = dn1 and dn2 and dx2
    if pert is None:
        b_ff = tau * S_ff(t)
    else:
        aft = abs(float(t))
        n_ff = sum(Dn[k] * (onat[k] + aft * Dn[k]) for k in range(3))
        D_ff = sum(ed[k] * (ocn[k] + aft * Dn[k]) + Dn[k] * (eo[k] + aft * ed[k]) for k in range(3))
        a_ff = taub * n_ff + 2 * D_ff
        b_ff = a_ff if lg else comb(tau * S_ff(t), a_ff)
    dec_front = fsq > fa * max(E1, E2) + b_ff  # (d.(p - c) = -+sqrt(disc) + a (t_computed - t))
    outs = []
    if (n1 or not dn1) and (x1 or not dx1):
        outs.append((float(t1), E1, f_near))
        if not dec_front:
            outs.append((float(t1), E1, 1 - f_near))
    if (not n1 or not dn1) and (n2 or not dn2) and (x2 or not dx2):
        outs.append((float(t2), E2, f_far))
        if not dec_front:
            outs.append((float(t2), E2, 1 - f_far))
    if not dec_disc:  # and the miss
        dec = False
    if dec and hit and dec_front:
        return Cand(-1, HIT, True, float(t), Et, front, [(float(t), Et, front)], tex=t)
    if dec and not hit:
        return None
    if not outs:
        return None
    return Cand(-1, UND, hit, float(t) if hit else None, Et, front, outs, tex=t if hit else None)


# ---- the binary64 filter over pairs ----------------------------------------------------------------------------------
def _cross_abs_v(x, y):
    return np.stack([x[:, 1] * y[:, 2] + y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] + y[:, 2] * x[:, 0],
                     x[:, 0] * y[:, 1] + y[:, 0] * x[:, 1]], axis=1)


def _tri_filter(o, d, tmax, A, e1, e2, tau, unit_cut, u=U, aomag=None, dmag=None, pert=None):
    """Pairs [m]: status (0 miss, 1 hit, 2 exact path), t, E."""
    n = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0],
                  e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], axis=1)
    Na = np.stack([np.abs(e1[:, 1] * e2[:, 2]) + np.abs(e2[:, 1] * e1[:, 2]),
                   np.abs(e1[:, 2] * e2[:, 0]) + np.abs(e2[:, 2] * e1[:, 0]),
                   np.abs(e1[:, 0] * e2[:, 1]) + np.abs(e2[:, 0] * e1[:, 1])], axis=1)
    det = -np.einsum("ij,ij->i", d, n)
    ao = o - A
    dao = np.stack([ao[:, 1] * d[:, 2] - d[:, 1] * ao[:, 2], ao[:, 2] * d[:, 0] - d[:, 2] * ao[:, 0],
                    ao[:, 0] * d[:, 1] - d[:, 0] * ao[:, 1]], axis=1)
    AOa, Da = np.abs(ao) if aomag is None else aomag, np.abs(d) if dmag is None else dmag
    DAOa = np.stack([AOa[:, 1] * Da[:, 2] + Da[:, 1] * AOa[:, 2], AOa[:, 2] * Da[:, 0] + Da[:, 2] * AOa[:, 0],
                     AOa[:, 0] * Da[:, 1] + Da[:, 0] * AOa[:, 1]], axis=1)
    ud = np.einsum("ij,ij->i", e2, dao)
    vd = -np.einsum("ij,ij->i", e1, dao)
    td = np.einsum("ij,ij->i", ao, n)
    S_det = np.einsum("ij,ij->i", Da, Na)
    S_ud = np.einsum("ij,ij->i", np.abs(e2), DAOa)
    S_vd = np.einsum("ij,ij->i", np.abs(e1), DAOa)
    S_td = np.einsum("ij,ij->i", AOa, Na)
    k = tau + GF
    cut = CUT * np.sqrt(np.einsum("ij,ij->i", d, d)) if unit_cut else CUT
    S_cut = S_det + (CUT * np.sqrt(np.einsum("ij,ij->i", Da, Da)) * 4 * U if unit_cut else 0.0)
    q_cut = det - cut
    if pert is not None:
        eo, ed, aonat, taub, comb = pert
        comb = np.minimum if comb is min else _second
        kb = taub + GF
        Dn, E1a, E2a = np.abs(d), np.abs(e1), np.abs(e2)
        DAOn = _cross_abs_v(aonat, Dn)
        DAOe = _cross_abs_v(eo, Dn) + _cross_abs_v(np.abs(ao), ed)
        sm = lambda p, q: np.einsum("ij,ij->i", p, q)  # noqa: E731
        b_det = comb(k * S_cut, kb * sm(Dn, Na) + 2 * sm(ed, Na))
        b_ud = comb(k * S_ud, kb * sm(E2a, DAOn) + 2 * sm(E2a, DAOe))
        b_vd = comb(k * S_vd, kb * sm(E1a, DAOn) + 2 * sm(E1a, DAOe))
        b_td = comb(k * S_td, kb * sm(aonat, Na) + 2 * sm(eo, Na))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = td / det
        at = np.abs(t)
        if pert is None:
            E = k * (S_td + at * S_det) / det + 2 * u * at
            decs = [(q_cut, k * S_cut), (ud, k * S_ud), (vd, k * S_vd), (det - ud - vd, k * (S_det + S_ud + S_vd)),
                    (t - TMIN, E), (tmax - t, np.where(np.isfinite(tmax), E, 0.0))]
        else:
            E = (b_td + at * b_det) / det + 2 * u * at
            decs = [(q_cut, b_det), (ud, b_ud), (vd, b_vd), (det - ud - vd, b_det + b_ud + b_vd),
                    (t - TMIN, E), (tmax - t, np.where(np.isfinite(tmax), E, 0.0))]
        fail = np.zeros(len(o), bool)
        sure = np.ones(len(o), bool)
        for q, b in decs:
            fail |= q < -b
            sure &= q > b
    st = np.where(fail, MISS, np.where(sure & (det > 0), HIT, UND)).astype(np.int8)
    return st, t, E


def _sph_filter(o, d, tmax, c, r, omag, tau, u=U, dmag=None, pert=None):
    oc = o - c
    a = np.einsum("ij,ij->i", d, d)
    h = np.einsum("ij,ij->i", oc, d)
    cc = np.einsum("ij,ij->i", oc, oc) - r * r
    disc = h * h - a * cc
    Da = np.abs(d) if dmag is None else dmag
    aS = a if dmag is None else np.einsum("ij,ij->i", Da, Da)
    S_h = np.einsum("ij,ij->i", omag, Da)
    S_d = S_h * S_h + aS * (np.einsum("ij,ij->i", omag, omag) + r * r)
    k = tau + GF
    st = np.full(len(o), UND, np.int8)
    if pert is None:
        b_d = k * S_d
    else:
        eo, ed, onat, taub, lg, comb = pert
        comb = np.minimum if comb is min else _second
        kb = taub + GF
        Dn, ocn = np.abs(d), np.abs(oc)
        sm = lambda p, q: np.einsum("ij,ij->i", p, q)  # noqa: E731
        n_h = sm(onat, Dn)
        n_d = n_h * n_h + a * (sm(onat, onat) + r * r)
        D_h = sm(eo, Dn) + sm(ocn, ed)
        D_a = 2 * sm(Dn, ed)
        # disc = a (r^2 - b^2), b the distance of the centre from the line: the line moves by |eo + |s| ed| at its
        # closest point o + s d, s = -h / a (termwise bounds of h^2 and a c' would not see that the two cancel)
        bb = np.sqrt(np.maximum(sm(oc, oc) - h * h / a, 0.0))
        mv = np.linalg.norm(eo + (np.abs(h) / a)[:, None] * ed, axis=1)
        D_d = 2 * a * np.maximum(np.abs(r), bb) * mv + D_a * np.abs(disc) / a
        a_h, a_d, a_a = kb * n_h + 2 * D_h, kb * n_d + 2 * D_d, kb * a + 2 * D_a
        b_h = np.where(lg, a_h, comb(k * S_h, a_h))
        b_d = np.where(lg, a_d, comb(k * S_d, a_d))
        b_a = np.where(lg, a_a, comb(k * aS, a_a))
    st[disc < -b_d] = MISS
    pos = disc > b_d
    t = np.full(len(o), np.nan)
    E = np.full(len(o), np.inf)
    front = np.zeros(len(o), np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sq = np.sqrt(np.where(pos, disc, 0.0))
        t1, t2 = (-h - sq) / a, (-h + sq) / a

        def Eof(tt):
            if pert is not None:  # (see exact_sphere)
                an_d = kb * n_d
                s = np.minimum(np.sqrt(an_d), an_d / sq)
                att = np.abs(tt)[:, None]
                ein = 2 * sm(np.abs(oc + tt[:, None] * d), eo + att * ed) / sq
                new = (kb * n_h + s + kb * sq + kb * np.abs(tt) * a) / a + ein + 2 * u * np.abs(tt)
                s = np.minimum(np.sqrt(k * S_d), k * S_d / sq)
                old = (k * S_h + s + k * sq + k * np.abs(tt) * aS) / a + 2 * u * np.abs(tt)
                return np.where(lg, new, comb(old, new))
            s = np.minimum(np.sqrt(k * S_d), k * S_d / sq)
            return (k * S_h + s + k * sq + k * np.abs(tt) * aS) / a + 2 * u * np.abs(tt)

        E1, E2 = Eof(t1), Eof(t2)
        fin = np.isfinite(tmax)
        near = pos & (t1 - TMIN > E1)
        far = pos & (TMIN - t1 > E1)
        near_in = near & ((tmax - t1 > E1) | ~fin)
        near_out = near & fin & (t1 - tmax > E1)
        far_in = far & (t2 - TMIN > E2) & ((tmax - t2 > E2) | ~fin)
        far_out = far & ((TMIN - t2 > E2) | (fin & (t2 - tmax > E2)))
        tt = np.where(near_in, t1, t2)
        S_ff = np.einsum("ij,ij->i", Da, omag + np.abs(tt)[:, None] * Da)
        if pert is None:
            b_ff = k * S_ff
        else:
            att = np.abs(tt)[:, None]
            a_ff = kb * sm(Dn, onat + att * Dn) + 2 * (sm(ed, ocn + att * Dn) + sm(Dn, eo + att * ed))
            b_ff = np.where(lg, a_ff, comb(k * S_ff, a_ff))
        ff_ok = sq > b_ff + a * np.where(near_in, E1, E2)  # (d.(p - c) at the computed t)
    inward = r < 0
    st[near_out | far_out] = MISS
    hit = (near_in | far_in) & ff_ok
    st[hit] = HIT
    t[hit] = tt[hit]
    E[hit] = np.where(near_in, E1, E2)[hit]
    front[hit] = np.where(near_in, ~inward, inward)[hit]
    return st, t, E, front


# ---- the reference over a ray set -------------------------------------------------------------------------------------
class Reference:
    """Per ray of `rays` (RAY_DTYPE) against `scene` (Scene) under `build` (STRICT / FAST / F32): the exact closest
    hit and any-hit, decided or not, and the candidates (Cand) that explain an undecided ray's answers.

    tau: the band, default TAU[build].  omag, dmag [n, 3]: the magnitudes that stand for |o_i| and |d_i| in every S_q
    (the world-coordinate forms only: FAST and F32) — for a ray that the build computes itself, the sum of the
    magnitudes of the terms of its expression.  exclude [n, 2]: per ray a (class, class index) that is no candidate
    (the primitive a scattered ray leaves), class -1 for none.

    operr, derr [n, 3] (F32 only): ABSOLUTE bounds on the error of the origin and direction the build traces against
    the ray given.  Beside tau S_q every decision then has the first-order band TAU_ARITH S_q' + 2 D_q: S_q' on the
    magnitudes of the strict form (|o_i - c_i|, |o_i - A_i|), D_q the effect of the input errors on q (|dq/do| (operr
    + the record's rounding) + |dq/dd| derr, term by term; the header's factor 2).  Both are bounds where tau S_q
    counts the same input errors (omag, dmag): the band is the smaller one; `first_order`: tau S_q does not cover
    operr / derr (the scattered rays of f32_audit), the band is the first-order one.  large: the (class, class index) pairs of the spheres that the kernel tests in
    binary64 on the widened ray — their band is the input error alone, TAU[FAST] S_q' + 2 D_q."""

    def __init__(self, scene, rays, build, unit_cut=False, chunk=1 << 20, tau=None, omag=None, dmag=None,
                 exclude=None, operr=None, derr=None, large=None, first_order=False):
        self.scene, self.rays, self.build, self.unit_cut = scene, rays, build, unit_cut
        self.tau = TAU[build] if tau is None else tau
        self.u = U32 if build == F32 else U
        self._world = build in (FAST, F32)
        assert (omag is None and dmag is None) or self._world
        self._oa = None if omag is None else np.ascontiguousarray(omag, np.float64)
        self._da = None if dmag is None else np.ascontiguousarray(dmag, np.float64)
        self._ex = None if exclude is None else np.asarray(exclude, np.int64).reshape(-1, 2)
        assert (operr is None) == (derr is None) and (operr is None or build == F32)
        self._eo = None if operr is None else np.ascontiguousarray(operr, np.float64)
        self._ed = None if derr is None else np.ascontiguousarray(derr, np.float64)
        self._large = {SPHERE: np.zeros(len(scene.sph), bool), MOVING: np.zeros(len(scene.mov), bool)}
        for cls, ci in (large or ()):
            self._large[int(cls)][int(ci)] = True
        assert not (large and operr is None)
        self._comb = _second if first_order else min
        n = len(rays)
        self.cands = [[] for _ in range(n)]
        self._o = np.ascontiguousarray(rays["origin"], np.float64)
        self._d = np.ascontiguousarray(rays["direction"], np.float64)
        self._time = np.ascontiguousarray(rays["time"], np.float64)
        self._tmax = np.ascontiguousarray(rays["tmax"], np.float64)
        self.n_exact = 0
        self._spheres(chunk)
        self._triangles(chunk)
        self._resolve()

    # -- spheres (static and moving) --
    def _centres(self, ri, cls, ci):
        if cls == SPHERE:
            return self.scene.sph[ci, :3], np.zeros((len(ci), 3))
        g = self.scene.mov[ci]
        tm = self._time[ri][:, None]
        dc = g[:, 3:6] - g[:, :3]
        return g[:, :3] + tm * dc, np.abs(g[:, :3]) + np.abs(tm * dc)

    def _omag(self, o, c, extra, oa=None):
        return ((np.abs(o) if oa is None else oa) + np.abs(c) if self._world else np.abs(o - c)) + extra

    def _mags(self, ri):
        """(omag, dmag) of the rays ri: the caller's, or None."""
        return (None if self._oa is None else self._oa[ri]), (None if self._da is None else self._da[ri])

    def _excluded(self, ri, cls, ci):
        if self._ex is None:
            return np.zeros(len(ri), bool)
        return (self._ex[ri, 0] == cls) & (self._ex[ri, 1] == ci)

    def _spheres(self, chunk):
        for cls, g in ((SPHERE, self.scene.sph), (MOVING, self.scene.mov)):
            if len(g) == 0:
                continue
            r = g[:, 3] if cls == SPHERE else g[:, 6]
            per = max(1, chunk // len(g))
            for r0 in range(0, len(self.rays), per):
                ri = np.repeat(np.arange(r0, min(r0 + per, len(self.rays))), len(g))
                ci = np.tile(np.arange(len(g)), len(ri) // len(g))
                c, extra = self._centres(ri, cls, ci)
                o = self._o[ri]
                oa, da = self._mags(ri)
                pert = None
                if self._eo is not None:
                    lg = self._large[cls][ci]
                    ec = np.where(lg[:, None], 0.0, 3 * U32 * (np.abs(c) + extra))
                    pert = (self._eo[ri] + ec, self._ed[ri], np.abs(o - c), np.where(lg, TAU[FAST], TAU_ARITH), lg,
                            self._comb)
                st, t, E, fr = _sph_filter(o, self._d[ri], self._tmax[ri], c, r[ci], self._omag(o, c, extra, oa),
                                           self.tau, self.u, da, pert)
                st[self._excluded(ri, cls, ci)] = MISS
                for j in np.nonzero(st == HIT)[0]:
                    self._add(ri[j], cls, ci[j], Cand(-1, HIT, True, float(t[j]), float(E[j]), int(fr[j]),
                                                      [(float(t[j]), float(E[j]), int(fr[j]))]))
                for j in np.nonzero(st == UND)[0]:
                    self._exact(ri[j], cls, ci[j])

    def _exact_sphere_pair(self, i, cls, ci):
        o, d = self._o[i], self._d[i]
        if cls == SPHERE:
            g = self.scene.sph[ci]
            c, r, extra = _f3(g[:3]), g[3], np.zeros(3)
        else:
            g = self.scene.mov[ci]
            c0, c1 = _f3(g[:3]), _f3(g[3:6])
            tm = Fr(float(self._time[i]))
            c, r = [c0[k] + tm * (c1[k] - c0[k]) for k in range(3)], g[6]
            extra = np.abs(g[:3]) + np.abs(self._time[i] * (g[3:6] - g[:3]))
        cf = np.array([float(x) for x in c])
        oa, da = self._mags(np.array([i]))
        om = self._omag(o[None], cf[None], extra[None], oa)[0]
        pert = None
        if self._eo is not None:
            lg = bool(self._large[cls][ci])
            ec = np.zeros(3) if lg else 3 * U32 * (np.abs(cf) + extra)
            pert = ([float(x) for x in self._eo[i] + ec], [float(x) for x in self._ed[i]],
                    [float(x) for x in np.abs(o - cf)], TAU[FAST] if lg else TAU_ARITH, lg, self._comb)
        return exact_sphere(o, d, float(self._tmax[i]), c, r, [float(x) for x in om], self.tau, self.u,
                            None if da is None else da[0], pert)

    def _exact_pair(self, i, cls, ci):
        self.n_exact += 1
        if cls == TRIANGLE:
            g = self.scene.tri[ci]
            am, da = self._tri_mags(np.array([i]), g[None, 0:3])
            pert = None
            if self._eo is not None:
                pert = ([float(x) for x in self._eo[i] + U32 * np.abs(g[0:3])], [float(x) for x in self._ed[i]],
                        [float(x) for x in np.abs(self._o[i] - g[0:3])], TAU_ARITH, self._comb)
            return exact_triangle(self._o[i], self._d[i], float(self._tmax[i]), g[0:3], g[3:6], g[6:9], self.tau,
                                  self.unit_cut, self.u, None if am is None else am[0], None if da is None else da[0],
                                  pert)
        return self._exact_sphere_pair(i, cls, ci)

    def _exact(self, i, cls, ci):
        c = self._exact_pair(i, cls, ci)
        if c is not None:
            self._add(i, cls, ci, c)

    def _add(self, i, cls, ci, cand):
        cand.prim = self.scene.ins[(cls, int(ci))]
        cand.key = (cls, int(ci))
        self.cands[int(i)].append(cand)

    # -- triangles --
    def _tri_pairs(self, chunk):
        tri = self.scene.tri
        nt, n = len(tri), len(self.rays)
        if nt * n <= 4 * chunk:
            per = max(1, chunk // nt)
            for r0 in range(0, n, per):
                ri = np.repeat(np.arange(r0, min(r0 + per, n)), nt)
                yield ri, np.tile(np.arange(nt), len(ri) // nt)
            return
        # box prefilter: exact vertex bounds padded by 1e-6 of the scene's scale, slab test over [0, tmax]
        v = tri.reshape(-1, 3, 3)
        pad = 1e-6 * self.scene.scale()
        lo, hi = v.min(1) - pad, v.max(1) + pad
        per = max(1, chunk // nt)
        for r0 in range(0, n, per):
            ids = np.arange(r0, min(r0 + per, n))
            o, d, tm = self._o[ids][:, None, :], self._d[ids][:, None, :], self._tmax[ids][:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / d
                a, b = (lo[None] - o) * inv, (hi[None] - o) * inv
                tn = np.fmax(np.fmax.reduce(np.fmin(a, b), axis=2), 0.0)
                tf = np.fmin(np.fmin.reduce(np.fmax(a, b), axis=2), tm * (1 + 1e-9))
            rr, cc = np.nonzero(~(tn > tf * (1 + 1e-9) + 1e-300))
            yield ids[rr], cc

    def _tri_mags(self, ri, A):
        """(|o - A| magnitudes, dmag) of the pairs: F32 tests ao = o - A on a rounded o and a rounded A."""
        oa, da = self._mags(ri)
        if self.build != F32:
            return None, da
        return (np.abs(self._o[ri]) if oa is None else oa) + np.abs(A), da

    def _triangles(self, chunk):
        if len(self.scene.tri) == 0:
            return
        g = self.scene.tri
        for ri, ci in self._tri_pairs(chunk):
            if len(ri) == 0:
                continue
            A = g[ci, 0:3]
            am, da = self._tri_mags(ri, A)
            pert = None
            if self._eo is not None:
                pert = (self._eo[ri] + U32 * np.abs(A), self._ed[ri], np.abs(self._o[ri] - A), TAU_ARITH, self._comb)
            st, t, E = _tri_filter(self._o[ri], self._d[ri], self._tmax[ri], A, g[ci, 3:6] - A, g[ci, 6:9] - A,
                                   self.tau, self.unit_cut, self.u, am, da, pert)
            st[self._excluded(ri, TRIANGLE, ci)] = MISS
            for j in np.nonzero(st == HIT)[0]:
                self._add(ri[j], TRIANGLE, ci[j], Cand(-1, HIT, True, float(t[j]), float(E[j]), 1,
                                                       [(float(t[j]), float(E[j]), 1)]))
            for j in np.nonzero(st == UND)[0]:
                self._exact(ri[j], TRIANGLE, ci[j])

    # -- per ray --
    def _tex(self, i, c):
        if c.tex is None:
            e = self._exact_pair(i, *c.key)
            c.tex = e.tex
        return c.tex

    def _resolve(self):
        n = len(self.rays)
        self.decided = np.zeros(n, bool)
        self.occ = np.zeros(n, bool)
        self.occ_decided = np.zeros(n, bool)
        self.ties = [()] * n
        self.t = np.full(n, np.inf)
        self.E = np.zeros(n)
        self.front = np.zeros(n, np.int32)
        for i, cs in enumerate(self.cands):
            H = [c for c in cs if c.status == HIT]
            Uc = [c for c in cs if c.status == UND]
            self.occ[i] = any(c.hit for c in cs)
            self.occ_decided[i] = bool(H) or not Uc
            hits = sorted((c for c in cs if c.hit), key=lambda c: c.t)
            if hits:  # the exact closest hit and its ties
                b = hits[0]
                close = [c for c in hits if c.t - c.E <= b.t + b.E]
                if len(close) > 1:
                    m = min(self._tex(i, c) for c in close)
                    tied = [c for c in close if abs(self._tex(i, c) - m) <= abs(m) * Fr(1, 1 << 120)]
                else:
                    tied = [b]
                self.ties[i] = tuple(sorted(c.prim for c in tied))
                self.t[i], self.E[i], self.front[i] = tied[0].t, max(c.E for c in tied), tied[0].front
            if not H:
                self.decided[i] = not Uc
                continue
            best = min(H, key=lambda c: c.t)
            ok = all(c.status == HIT for c in tied) and len({c.front for c in tied}) == 1
            for c in cs:
                if c.prim in self.ties[i]:
                    continue
                for (t, E, _) in c.outs:
                    if not (t - E > best.t + best.E):  # (NaN: any t)
                        ok = False
            self.decided[i] = ok


# ---- the checker ----------------------------------------------------------------------------------------------------
def _sphere_of(scene, prim, time):
    k, i = int(scene.kind[prim]), int(scene.index[prim])
    if k == SPHERE:
        g = scene.sph[i]
        return _f3(g[:3]), g[3], float(np.max(np.abs(g[:3])))
    g = scene.mov[i]
    c0, c1, tm = _f3(g[:3]), _f3(g[3:6]), Fr(float(time))
    return [c0[k] + tm * (c1[k] - c0[k]) for k in range(3)], g[6], float(np.max(np.abs(g[:3]) + np.abs(time * (g[3:6] - g[:3]))))


# -- the per-record checks, shared by check (closest hit) and check_sequences (first k hits) --
def _is_miss_record(h):
    """The miss-record layout: t = inf, kind = material = -1, front_face = 0."""
    return bool(math.isinf(h["t"]) and h["kind"] == -1 and h["material"] == -1 and h["front_face"] == 0)


def _scene_fields_ok(sc, h):
    """prim within the scene, kind and material the scene's."""
    gp = int(h["prim"])
    return bool(0 <= gp < len(sc.kind) and h["kind"] == sc.kind[gp] and h["material"] == sc.prim_mat[gp])


def _explained(h, mine):
    """t within E of an outcome of one of the candidates `mine`, with that outcome's front_face (t NaN: any)."""
    t = float(h["t"])
    for c in mine:
        for (te, E, fr) in c.outs:
            if math.isnan(te) or (abs(t - te) <= E and int(h["front_face"]) == fr):
                return True
    return False


def _check_exact_record(sc, rays, i, h, te, E, front, fail):
    """A record that must be the exact hit (te, front) of ray i on primitive h.prim: t within E, front_face, the point
    bound, a triangle's normal bit for bit, the sphere-normal bound.  Returns |t - te| / E."""
    gp = int(h["prim"])
    t = float(h["t"])
    o, d = rays["origin"][i].astype(np.float64), rays["direction"][i].astype(np.float64)
    err = abs(t - te) / E if E > 0 else (0.0 if t == te else math.inf)
    if not err <= 1.0:
        fail(i, f"t {t!r}, exact {te!r} +- {E:.3g}")
    if int(h["front_face"]) != int(front):
        fail(i, f"front_face {h['front_face']}, exact {front}")
    pe = o + te * d
    pb = np.abs(d) * E + 4 * U * (np.abs(o) + np.abs(te * d)) + 1e-300
    if not np.all(np.abs(h["point"] - pe) <= pb):
        fail(i, f"point {h['point']}, exact {pe} +- {pb}")
    if sc.kind[gp] == TRIANGLE:
        if not np.array_equal(np.asarray(h["normal"]).view(np.uint64), sc.tri_n[sc.index[gp]].view(np.uint64)):
            fail(i, f"triangle normal {h['normal']}, record {sc.tri_n[sc.index[gp]]}")
    else:
        cf, r, cm = _sphere_of_f(sc, gp, float(rays["time"][i]))
        nb = 2 * math.sqrt(3) * (float(np.max(pb)) + 4 * U * cm) / abs(r) + 8 * U
        # in binary64 first: (o + te d - c) / |r| there is within (4 u (|o_i| + |te d_i|) + 5 u cm) / |r| of the exact
        # quotient (pe 2 roundings, the moving centre 3, the difference and the quotient 1 each), less than nb / 2 — so a
        # normal within nb / 2 of it is within nb of the exact one and needs no exact arithmetic
        nf = (pe - cf) / abs(r)
        if np.all(np.abs(h["normal"] - (nf if h["front_face"] else -nf)) <= 0.5 * nb):
            return err
        c, r, cm = _sphere_of(sc, gp, float(rays["time"][i]))
        ng = [(Fr(float(o[k])) + Fr(te) * Fr(float(d[k])) - c[k]) / abs(Fr(float(r))) for k in range(3)]
        ng = np.array([float(x) for x in ng])
        ne = ng if h["front_face"] else -ng
        nb = 2 * math.sqrt(3) * (float(np.max(pb)) + 4 * U * cm) / abs(r) + 8 * U
        if not np.all(np.abs(h["normal"] - ne) <= nb):
            fail(i, f"sphere normal {h['normal']}, exact {ne} +- {nb:.3g}")
    return err


def _sphere_of_f(scene, prim, time):
    """_sphere_of in binary64: (centre, r, the magnitude of the centre's terms)."""
    k, i = int(scene.kind[prim]), int(scene.index[prim])
    if k == SPHERE:
        g = scene.sph[i]
        return g[:3], g[3], float(np.max(np.abs(g[:3])))
    g = scene.mov[i]
    dc = time * (g[3:6] - g[:3])
    return g[:3] + dc, g[6], float(np.max(np.abs(g[:3]) + np.abs(dc)))


def check(ref, hits, occ=None, what=""):
    """Every field of `hits` (HIT_DTYPE) and `occ` (bool, optional) against the reference.  Returns the counts; raises
    CheckError with the first failures."""
    sc, rays = ref.scene, ref.rays
    bad = []
    worst = 0.0
    diff = 0

    def fail(i, msg):
        if len(bad) < 8:
            bad.append((int(i), msg))

    for i in range(len(rays)):
        h = hits[i]
        gp = int(h["prim"])
        if occ is not None and ref.occ_decided[i] and bool(occ[i]) != bool(ref.occ[i]):
            fail(i, f"occluded {bool(occ[i])}, exact {bool(ref.occ[i])}")
        if occ is not None and not ref.occ_decided[i]:
            if occ[i] and not ref.cands[i]:
                fail(i, "occluded with no candidate")
            if not occ[i] and any(c.status == HIT for c in ref.cands[i]):
                fail(i, "not occluded with a decided hit")
        if gp < 0:
            if not _is_miss_record(h):
                fail(i, f"miss record {h}")
            if ref.decided[i] and ref.ties[i]:
                fail(i, f"miss, exact hit {ref.ties[i]} at {ref.t[i]!r}")
            elif not ref.decided[i] and any(c.status == HIT for c in ref.cands[i]):
                fail(i, "miss with a decided hit")
            continue
        if not _scene_fields_ok(sc, h):
            fail(i, f"prim {gp}: kind {h['kind']} material {h['material']}")
            continue
        t = float(h["t"])
        if ref.decided[i]:
            if gp not in ref.ties[i]:
                fail(i, f"prim {gp} t {t!r}, exact {ref.ties[i]} at {ref.t[i]!r}")
                continue
            if t != ref.t[i]:
                diff += 1
            worst = max(worst, _check_exact_record(sc, rays, i, h, ref.t[i], ref.E[i], ref.front[i], fail))
        else:
            mine = [c for c in ref.cands[i] if c.prim == gp]
            if not mine:
                fail(i, f"undecided: prim {gp} cannot hit")
                continue
            if not _explained(h, mine):
                fail(i, f"undecided: prim {gp} t {t!r} front {h['front_face']}, outcomes {mine[0].outs}")
            for c in ref.cands[i]:
                if c.status == HIT and c.prim != gp and c.t + c.E < t - max(c.E for c in mine):
                    fail(i, f"undecided: prim {gp} t {t!r} behind decided prim {c.prim} at {c.t!r}")
                    break
    n = len(rays)
    stats = {"rays": n, "decided": int(ref.decided.sum()), "undecided": int(n - ref.decided.sum()),
             "occ_undecided": int(n - ref.occ_decided.sum()), "t_differs": diff, "worst_t_err": worst,
             "exact_pairs": ref.n_exact}
    if bad:
        raise CheckError(f"{what}: {len(bad)}+ failures: {bad}")
    return stats


# ---- first-k-hits sequences ---------------------------------------------------------------------------------------------
def _decided_hits(cs):
    """The HIT candidates of one ray, ascending by exact t (a stable sort: equal t in insertion order)."""
    return sorted((c for c in cs if c.status == HIT), key=lambda c: (c.t, c.prim))


def _sequence_decided(cs, k):
    H = _decided_hits(cs)
    und = [c for c in cs if c.status == UND]
    for j in range(min(len(H) - 1, k)):  # gaps j | j + 1, up to the one between entry k - 1 and the first one left out
        if not (H[j + 1].t - H[j + 1].E > H[j].t + H[j].E):
            return False
    if len(H) < k:
        return not und
    last = H[k - 1]
    for c in und:
        for (t, E, _) in c.outs:
            if not (t - E > last.t + last.E):  # (NaN: any t)
                return False
    return True


def sequence_decided(ref, k):
    """Per ray: the first-k-hits sequence is certain (the header's sequence rules)."""
    return np.array([_sequence_decided(cs, k) for cs in ref.cands], dtype=bool).reshape(len(ref.cands))


def check_sequences(ref, hits, counts, k, what="", sorted_by_index=True):
    """`hits` [n, k] (HIT_DTYPE) and `counts` [n] of a first-k-hits query against the reference (built with the rays'
    own tmax): shape, soundness, order, completeness, and the exact sequence on decided rays (the header's sequence
    rules).  sorted_by_index=False drops only the index order of bit-equal t (the fast GRID walk).  Returns the counts;
    raises CheckError with the first failures."""
    sc, rays = ref.scene, ref.rays
    n = len(rays)
    assert hits.shape == (n, k) and len(counts) == n, (hits.shape, len(counts), n, k)
    bad = []
    worst = 0.0
    unordered = 0
    n_decided = 0
    cols = {f: np.ascontiguousarray(hits[f]) for f in ("t", "point", "normal", "prim", "kind", "material", "front_face")}

    def rec(i, s):  # (slot s of ray i as a mapping: plain arrays index faster than structured ones)
        return {f: a[i, s] for f, a in cols.items()}

    def fail(i, msg):
        if len(bad) < 8:
            bad.append((int(i), msg))

    for i in range(n):
        cs = ref.cands[i]
        decided = _sequence_decided(cs, k)
        n_decided += decided
        cnt = int(counts[i])
        # shape
        if not 0 <= cnt <= k:
            fail(i, f"count {cnt} outside [0, {k}]")
            continue
        for s in range(cnt, k):
            if cols["prim"][i, s] >= 0 or not _is_miss_record(rec(i, s)):
                fail(i, f"slot {s} >= count {cnt} is no miss record: {hits[i, s]}")
        prims = [int(cols["prim"][i, s]) for s in range(cnt)]
        if any(p < 0 for p in prims):
            fail(i, f"a miss record below count {cnt}: prims {prims}")
            continue
        if len(set(prims)) != cnt:
            fail(i, f"a primitive reported twice: {prims}")
        # soundness
        by_prim = {}
        for c in cs:
            by_prim.setdefault(c.prim, []).append(c)
        ok = True
        for s, gp in enumerate(prims):
            h = rec(i, s)
            if not _scene_fields_ok(sc, h):
                fail(i, f"slot {s} prim {gp}: kind {h['kind']} material {h['material']}")
                ok = False
                continue
            mine = by_prim.get(gp)
            if not mine:
                fail(i, f"slot {s}: prim {gp} t {float(h['t'])!r} cannot hit within tmax {float(rays['tmax'][i])!r}")
                ok = False
                continue
            if not _explained(h, mine):
                fail(i, f"slot {s}: prim {gp} t {float(h['t'])!r} front {h['front_face']}, outcomes {mine[0].outs}")
            for c in mine:
                if c.status == HIT:
                    worst = max(worst, _check_exact_record(sc, rays, i, h, c.t, c.E, c.front, fail))
        if not ok:
            continue
        # order
        ts = [float(cols["t"][i, s]) for s in range(cnt)]
        for s in range(cnt - 1):
            if not ts[s] <= ts[s + 1]:
                fail(i, f"t descends at slot {s}: {ts[s]!r} > {ts[s + 1]!r}")
            elif ts[s] == ts[s + 1] and prims[s] > prims[s + 1]:
                unordered += 1
                if sorted_by_index:
                    fail(i, f"equal t {ts[s]!r} at slots {s}, {s + 1} out of index order: {prims[s]}, {prims[s + 1]}")
        # completeness: a decided hit may be missing only from behind the cut
        H = _decided_hits(cs)
        got = set(prims)
        for c in H:
            if c.prim in got:
                continue
            if cnt < k:
                fail(i, f"decided hit prim {c.prim} at {c.t!r} missing, count {cnt} < {k}")
                break
            e_last = max(x.E for x in by_prim[prims[k - 1]])
            if not c.t + c.E >= ts[k - 1] - e_last:
                fail(i, f"decided hit prim {c.prim} at {c.t!r} missing in front of the last entry at {ts[k - 1]!r}")
                break
        # decided rays: the exact sequence (members of an exact tie in either order)
        if decided:
            want = H[:k]
            if cnt != len(want):
                fail(i, f"decided: count {cnt}, exact {len(want)}")
            elif prims != [c.prim for c in want]:
                tex = {c.prim: ref._tex(i, c) for c in want}
                same = sorted(prims) == sorted(tex) and all(tex[p] == tex[c.prim] for p, c in zip(prims, want))
                if not same:
                    fail(i, f"decided: prims {prims}, exact {[c.prim for c in want]}")
    stats = {"rays": n, "decided": int(n_decided), "undecided": int(n - n_decided), "worst_t_err": worst,
             "unordered_equal_t": unordered, "exact_pairs": ref.n_exact}
    if bad:
        raise CheckError(f"{what}: {len(bad)}+ failures: {bad}")
    return stats
