"""An exact reference for the ambient query (rtow_ambient / rtow_ambient_device): the sample directions over the REAL
numbers, which samples are certainly open, and how far a kernel's directions and records may be from them.

A helper module for the tests (numpy and the standard library, no GPU), in the style of scatter_exact.py, on whose
dyadic rationals (D, dsqrt, drcp: 130 bits), sine polynomial (_poly), Philox (philox_words), sky (sky_exact) and per-build
elementary errors (ELEM) it stands, and of exact_hits.py, which decides the visibility.  The semantics are the
definition of include/rtow.h read as real-number expressions of the binary64 inputs; for (normal N, seed, pixel, sample):
  * the four Philox words w of request 0 of (pixel, sample);
  * the disk point of lens_from_block: b = the 11 + 11 + 10 low bits of w0, w1, w2; rho = sqrt(w3 2^-32); th = (b mod
    2^30) C with C the double 2^-30 kHalfPi; sn = P(th), cs = P(kHalfPi - th) with P the degree-9 polynomial that the
    kernels evaluate (NOT the true sine); the quadrant b >> 30 swaps and negates; (px, py) = rho (+-cx, +-sy);
  * pz = sqrt(max(1 - (px^2 + py^2), 0));
  * n = N / sqrt(N.N);
  * Duff et al.'s frame with s = -1 if N.z has its sign bit set (-0.0 included) and +1 otherwise: a = -1 / (s + n.z),
    c = n.x n.y a, t = (1 + s n.x^2 a, s c, -s n.x), b = (c, s + n.y^2 a, -n.y);
  * d = t px + b py + n pz.
Nothing here is copied from tests/ambient_ref.py, which restates the kernel's binary64 operations in their order: this
module evaluates the definition exactly and says how far ANY evaluation of the kernel's expressions may be from it.

Bounds, first order, by counting roundings on the kernel's expressions (csrc/rtow_ambient.h, rtow_trace_rng.h), as
scatter_exact.py's header does: u = 2^-53, every rounding on a path contributes 2 u |value| (the factor 2: gamma_k against
k u, and magnitudes taken from the exact operands), input bounds enter through the derivatives, and the per-build
elementary errors are ELEM's (strict: sqrt, 1 / x and a / b one rounding each; fast: fast_sqrt / fast_sqrt_pos RSQ =
1.5 delta^2 + 4 u, fast_div = a * fast_rcp(b) three roundings).  Contraction only removes roundings and never reorders, so
every other count is the strict form's and holds for both builds.
    rho    w3 2^-32 is exact (32 bits); sqrt: ELEM.sqrt.
    th     one rounding (the product is made opaque to contraction in both builds); kHalfPi - th one more.
    P(x)   K_POLY = 10 roundings on S_P = |x| sum |c_j| x^2j, and the argument's error through |P'|.
    px, py the product rho * cx: 1.
    pz     px^2, py^2 and their sum: 2 on r2 = px^2 + py^2 (positive terms), and 2 |px| e_px + 2 |py| e_py; 1 - r2: 1;
           max(., 0) is exact and 1-Lipschitz; the square root's sensitivity min(sqrt e, e / sqrt x) to the error e of
           x = 1 - r2 — at the rim x is a few 1e-8 and e a few 1e-15, so pz is known to 1e-10 only, and where x <= 0 to
           sqrt e — plus ELEM.sqrt on pz.
    n      N.N: 3 roundings on positive terms, and products that underflow individually: a live point has N.N >=
           2^-1022, every underflow costs at most 2^-1075, three of them 3 u relative — counted as 3 more roundings.
           sqrt halves the relative error and adds ELEM.sqrt; the quotient adds ELEM.div.
    frame  s + n.z lies in [1, 2] in magnitude (s has n.z's sign): 1 rounding, so a = -1 / (s + n.z) is well conditioned:
           e_a = e_(s + n.z) / (s + n.z)^2 + ELEM.div |a|.  c = (n.x n.y) a: 2.  s n.x is exact.  (s n.x) n.x a: 2, 1 + .: 1.
           s c, -s n.x, -n.y: exact.  (n.y n.y) a: 2, s + .: 1.
    d.k    (t.k px + b.k py) + n.k pz: two products, a sum, a product and a sum.
    floor  a result below 2^-1022 is rounded to a multiple of 2^-1074 whatever its size: 64 x 2^-1074 is added to every
           bound (fewer than 32 operations lie on any path).
No tolerance is fixed in advance: the bounds are what this count gives.

Records (check_records).  `ref` is an exact_hits.Reference over the build's own exported rays, so every sample's
visibility is decided by exact arithmetic on the direction the kernel walked, or left undecided inside exact_hits' band.
Per live point, with m undecided samples:
  * every exported ray carries the point's origin, time and max_dist bit for bit, and its direction lies within the
    bound of the exact one;
  * `samples` is the sample count; `open` is the number of open samples; `bent` is the in-order binary64 sum, from +0.0,
    of the exported directions of the open samples, bit for bit in both builds (an accumulation has no product: nothing
    to contract); `sky` lies within the sum of sky_exact's per-sample bounds, plus 2 u per addition on the running sum,
    of the exact sum of sky_exact over the open samples;
  * m = 0: the open samples are the exactly open ones.  0 < m <= 4: the record matches one of the 2^m ways to open the
    undecided samples.  m > 4: only decided-open <= open <= decided-open + m is checked; the point is counted as left out.
A skipped point (ambient_ref.skipped: the rule, not the arithmetic) has an all +0.0 record and dead rays.

Importing this module loads no library.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

import ambient_ref
import rtow
import scatter_exact as sx
from scatter_exact import D, ELEM, FAST, HALF_PI, K_POLY, STRICT, U2, _f, _poly, _sqrt_err, drcp, dsqrt, philox_words, sky_exact

TH_SCALE = 2.0 ** -30 * HALF_PI  # the double the kernels multiply the 30 angle bits by
FLOOR = 64 * 2.0 ** -1074
NN_ROUNDINGS = 3 + 3  # the dot's three, and 3 u for products that underflow (twice, as every rounding)
BUILDS = (STRICT, FAST)


class CheckError(AssertionError):
    pass


# ---- the direction -----------------------------------------------------------------------------------------------------
def disk_exact(w):
    """(px, py, pz exact; |.| floats; {build: (e_px, e_py, e_pz)}) of the Philox block w of request 0."""
    b = (w[0] & 0x7ff) | ((w[1] & 0x7ff) << 11) | ((w[2] & 0x3ff) << 22)
    rho = dsqrt(D(w[3], -32))
    frho = _f(rho)
    th = D(b & 0x3fffffff, 0) * D.of(TH_SCALE)
    psi = D.of(HALF_PI) - th
    sn, s_sn, d_sn = _poly(th)
    cs, s_cs, d_cs = _poly(psi)
    fth, fpsi = abs(_f(th)), abs(_f(psi))
    e_sn = K_POLY * U2 * s_sn + d_sn * U2 * fth
    e_cs = K_POLY * U2 * s_cs + d_cs * U2 * (fth + fpsi)
    q = b >> 30
    (cx, e_cx), (sy, e_sy) = ((sn, e_sn), (cs, e_cs)) if q & 1 else ((cs, e_cs), (sn, e_sn))
    if q in (1, 2):
        cx = -cx
    if q >= 2:
        sy = -sy
    px, py = (rho * cx).trunc(), (rho * sy).trunc()
    fpx, fpy, fcx, fsy = abs(_f(px)), abs(_f(py)), abs(_f(cx)), abs(_f(sy))
    r2 = px * px + py * py
    x = (1 - r2).trunc()
    fr2, fx = _f(r2), _f(x)
    pz = dsqrt(x) if x.sign() > 0 else D(0, 0)
    fpz = _f(pz)
    err = {}
    for build in BUILDS:
        el = ELEM[build]
        e_rho = el["sqrt"] * frho
        e_px = frho * e_cx + fcx * e_rho + U2 * fpx
        e_py = frho * e_sy + fsy * e_rho + U2 * fpy
        e_x = 2 * fpx * e_px + 2 * fpy * e_py + 2 * U2 * fr2 + U2 * abs(fx)
        err[build] = (e_px, e_py, _sqrt_err(max(fx, 0.0), e_x) + el["sqrt"] * fpz)
    return (px, py, pz), (fpx, fpy, fpz), err


def frame_exact(N):
    """(t, b, n exact [3] each; {build: (e_t, e_b, e_n)}) of the normal N [3] (binary64, N.N a normal number)."""
    Nd = [D.of(float(v)) for v in N]
    inv = drcp(dsqrt(Nd[0] * Nd[0] + Nd[1] * Nd[1] + Nd[2] * Nd[2]))
    n = [(v * inv).trunc() for v in Nd]
    fn = [abs(_f(v)) for v in n]
    s = -1 if math.copysign(1.0, float(N[2])) < 0 else 1
    sp = s + n[2]
    a = -drcp(sp)
    fsp, fa = abs(_f(sp)), abs(_f(a))
    c = (n[0] * n[1] * a).trunc()
    qx, qy = (n[0] * n[0] * a).trunc(), (n[1] * n[1] * a).trunc()
    t = [1 + s * qx, s * c, -s * n[0]]
    b = [c, s + qy, -n[1]]
    fc, fqx, fqy = abs(_f(c)), abs(_f(qx)), abs(_f(qy))
    err = {}
    for build in BUILDS:
        el = ELEM[build]
        rel = 0.5 * NN_ROUNDINGS * U2 + el["sqrt"] + el["div"]
        e_n = [rel * v for v in fn]
        e_sp = e_n[2] + U2 * fsp
        e_a = e_sp / (fsp * fsp) + el["div"] * fa
        e_c = (e_n[0] * fn[1] + fn[0] * e_n[1]) * fa + fn[0] * fn[1] * e_a + 2 * U2 * fc
        e_qx = 2 * fn[0] * e_n[0] * fa + fn[0] * fn[0] * e_a + 2 * U2 * fqx
        e_qy = 2 * fn[1] * e_n[1] * fa + fn[1] * fn[1] * e_a + 2 * U2 * fqy
        e_t = [e_qx + U2 * abs(_f(t[0])), e_c, e_n[0]]
        e_b = [e_c, e_qy + U2 * abs(_f(b[1])), e_n[1]]
        err[build] = (e_t, e_b, e_n)
    return t, b, n, err


def direction_exact(frame, disk):
    """(d [3] floats, {build: bound [3]}) of frame_exact's and disk_exact's results."""
    t, b, n, ferr = frame
    (px, py, pz), (fpx, fpy, fpz), derr = disk
    d, mags = [], []
    for k in range(3):
        A, B, Cn = t[k] * px, b[k] * py, n[k] * pz
        d.append(_f(A + B + Cn))
        mags.append((abs(_f(t[k])), abs(_f(b[k])), abs(_f(n[k])), abs(_f(A)), abs(_f(B)), abs(_f(Cn))))
    bound = {}
    for build in BUILDS:
        e_t, e_b, e_n = ferr[build]
        e_px, e_py, e_pz = derr[build]
        out = []
        for k, (ft, fb, fn, fA, fB, fC) in enumerate(mags):
            inputs = e_t[k] * fpx + ft * e_px + e_b[k] * fpy + fb * e_py + e_n[k] * fpz + fn * e_pz
            out.append(inputs + U2 * (fA + fB) + U2 * (fA + fB) + U2 * fC + U2 * (fA + fB + fC) + FLOOR)
        bound[build] = out
    return d, bound


def exact_directions(normals, seed, pixel, sample, rule=True):
    """(d [n, s, 3], {build: bound [n, s, 3]}) for normals [n, 3] and the identities pixel, sample [n, s]; NaN in both for
    a normal that ambient_ref.skipped would skip.  rule=False: every finite normal but the zero vector gets its exact
    direction and the bound of a normal whose N.N is a normal number (what the skip rule protects, made visible)."""
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    pixel, sample = np.asarray(pixel, np.uint64), np.asarray(sample, np.uint64)
    n, s = pixel.shape
    words = np.stack([np.asarray(w, np.uint64) for w in philox_words(int(seed), pixel, sample, 0)], axis=2)
    d = np.full((n, s, 3), np.nan)
    bound = {build: np.full((n, s, 3), np.nan) for build in BUILDS}
    with np.errstate(all="ignore"):
        nn = (normals[:, 0] * normals[:, 0] + normals[:, 1] * normals[:, 1]) + normals[:, 2] * normals[:, 2]
    for i in range(n):
        if rule and not (nn[i] >= 2.0 ** -1022 and nn[i] < math.inf):
            continue
        if not (np.all(np.isfinite(normals[i])) and np.any(normals[i] != 0.0)):
            continue
        fr = frame_exact(normals[i])
        for j in range(s):
            d[i, j], bd = direction_exact(fr, disk_exact([int(v) for v in words[i, j]]))
            for build in BUILDS:
                bound[build][i, j] = bd[build]
    return d, bound


def check_directions(exact, dirs, build, what="", live=None):
    """The directions dirs [n, s, 3] against exact_directions' result under `build`'s bound, on the points `live` (default:
    those with an exact direction).  Returns the worst error as a fraction of its bound; raises CheckError."""
    d, bound = exact[0], exact[1][build]
    dirs = np.asarray(dirs, np.float64).reshape(d.shape)
    live = ~np.isnan(d[:, 0, 0]) if live is None else np.asarray(live, bool)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(dirs - d) / bound
    ok = ratio <= 1.0  # (a NaN direction fails)
    bad = np.argwhere(~ok & live[:, None, None])
    if len(bad):
        i, j, k = (int(v) for v in bad[0])
        raise CheckError(f"{what}: {len(bad)} direction components outside the {build} bound; first: point {i} sample {j} "
                         f"component {k}: {dirs[i, j, k]!r}, exact {d[i, j, k]!r} +- {bound[i, j, k]:.3g} "
                         f"(error {ratio[i, j, k]:.3g} of the bound)")
    return float(ratio[live].max()) if live.any() else 0.0


# ---- the records -------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _sum_in_order(d, opened):
    acc = np.zeros(3)
    for j in opened:
        acc = acc + d[j]
    return acc


def _sky_fits(sky, cols, bounds, opened):
    """(ok, worst error over bound) of a record's sky against the exact sum over `opened`."""
    worst = 0.0
    for k in range(3):
        exact = math.fsum(cols[j][k] for j in opened)
        bound, run = 0.0, 0.0
        for j in opened:
            run += cols[j][k]
            bound += bounds[j][k] + U2 * run
        err = abs(float(sky[k]) - exact)
        if not err <= bound:
            return False, math.inf
        if bound > 0:
            worst = max(worst, err / bound)
    return True, worst


class Exact:
    """The exact directions (exact_directions' result) and skies (sky_exact per ray, None for a skipped point's) of the
    rays [n, samples] that an ambient call on `points` exported under `build`: what check_records compares with, made
    once per set of exported rays and passed to every check of that set."""

    def __init__(self, points, rays, samples, build, seed=1, ids=None, sample_first=0):
        points = np.ascontiguousarray(points, dtype=rtow.SURFACE_POINT_DTYPE).reshape(-1)
        n = len(points)
        rays = np.asarray(rays).reshape(n, samples)
        skip = ambient_ref.skipped(points)
        pixel, sample = ambient_ref.identities(n, samples, ids, sample_first)
        normals = np.where(skip[:, None], 0.0, points["normal"])  # (a point skipped for its max_dist needs no direction)
        self.build, self.points, self.rays = build, points.tobytes(), rays.tobytes()
        self.dirs = exact_directions(normals, seed, pixel, sample)
        self.sky = [[None if skip[i] else sky_exact(rays["direction"][i, j], build) for j in range(samples)]
                    for i in range(n)]


def check_records(ref, points, rays, records, samples, build, seed=1, ids=None, sample_first=0, what="", exact=None):
    """The exported rays [n, samples] and the records [n] of an ambient call against the exact reference: see the header.
    ref: an exact_hits.Reference of `build` over rays.reshape(-1); exact: the Exact of these points and rays (default: made
    here from seed, ids and sample_first).  Returns the counts — points, rays, undecided (rays), left_out (points),
    worst_dir and worst_sky (errors as fractions of their bounds; worst_sky over the points without an undecided sample);
    raises CheckError with the first failures."""
    points = np.ascontiguousarray(points, dtype=rtow.SURFACE_POINT_DTYPE).reshape(-1)
    n = len(points)
    rays = np.asarray(rays).reshape(n, samples)
    assert ref.build == build and len(ref.rays) == n * samples and records.shape == (n,)
    assert ref.rays.tobytes() == rays.tobytes(), "the reference is not over these rays"
    if exact is None:
        exact = Exact(points, rays, samples, build, seed, ids, sample_first)
    assert exact.build == build and exact.points == points.tobytes() and exact.rays == rays.tobytes(), \
        "`exact` was made for other points or rays"
    occ, decided = ref.occ.reshape(n, samples), ref.occ_decided.reshape(n, samples)
    skip = ambient_ref.skipped(points)
    bad = []

    def fail(i, msg):
        if len(bad) < 8:
            bad.append((int(i), msg))

    live = ~skip
    try:
        worst_dir = check_directions(exact.dirs, rays["direction"], build, what, live)
    except CheckError as e:
        fail(-1, str(e))
        worst_dir = math.inf
    worst_sky, left_out = 0.0, 0
    for i in range(n):
        rec, r = records[i], rays[i]
        if skip[i]:
            if np.ascontiguousarray(records[i:i + 1]).view(np.uint8).any():
                fail(i, f"skipped point with the record {rec}")
            if not (np.all(r["tmax"] == -1.0) and not r["origin"].any() and not r["direction"].any() and not r["time"].any()):
                fail(i, "skipped point with live rays")
            continue
        p = points[i]
        if not (np.all(_bits(r["origin"]) == _bits(p["point"])) and np.all(_bits(r["time"]) == _bits(p["time"]))
                and np.all(_bits(r["tmax"]) == _bits(p["max_dist"]))):
            fail(i, "an exported ray does not carry the point's origin, time and max_dist")
        if rec["samples"] != float(samples):
            fail(i, f"samples {rec['samples']}")
        und = [j for j in range(samples) if not decided[i, j]]
        sure = [j for j in range(samples) if decided[i, j] and not occ[i, j]]
        if not len(sure) <= rec["open"] <= len(sure) + len(und):
            fail(i, f"open {rec['open']}, decided open {len(sure)}, undecided {len(und)}")
            continue
        if len(und) > 4:
            left_out += 1
            continue
        cols = [c for c, _ in exact.sky[i]]
        bounds = [b for _, b in exact.sky[i]]
        d = r["direction"]
        # the ways to open the undecided samples, the exact answer's own first
        first = tuple(j for j in und if not occ[i, j])
        ways = [first] + [w for k in range(len(und) + 1) for w in itertools.combinations(und, k) if w != first]
        msgs = []
        for w in ways:
            opened = sorted(sure + list(w))
            if rec["open"] != float(len(opened)):
                msgs.append(f"open {rec['open']}, exact {len(opened)}")
                continue
            want = _sum_in_order(d, opened)
            if not np.array_equal(_bits(rec["bent"]), _bits(want)):
                msgs.append(f"bent {rec['bent']}, in-order sum of the open directions {want}")
                continue
            ok, ws = _sky_fits(rec["sky"], cols, bounds, opened)
            if not ok:
                msgs.append(f"sky {rec['sky']} outside its bound of the exact sum over samples {opened}")
                continue
            if not und:
                worst_sky = max(worst_sky, ws)
            break
        else:
            fail(i, ("decided: " if not und else f"{len(und)} undecided: ") + "; ".join(msgs[:3]))
    stats = {"points": n, "rays": n * samples, "undecided": int((~decided[live]).sum()), "left_out": left_out,
             "worst_dir": worst_dir, "worst_sky": worst_sky}
    if bad:
        e = CheckError(f"{what}: {len(bad)}+ failures: {bad}")
        e.bad = bad
        raise e
    return stats


def line(stats):
    """The counts of check_records as one printed line."""
    return (f"points {stats['points']}, rays {stats['rays']}, undecided {stats['undecided']}, left out {stats['left_out']}, "
            f"worst direction {stats['worst_dir']:.3g} of its bound, worst sky {stats['worst_sky']:.3g} of its bound")


assert sx.COEF == ambient_ref.SIN_C  # (one polynomial: the kernels' sin_quarter)
