"""The first-hit guide buffers (rtow_guides*, csrc/rtow_guides.h) against exact first hits, pixel by pixel.

A helper module for the tests (numpy, the standard library and tests/exact_hits.py; no GPU).  Given the primaries of a
guides call (`rays`, `ids`: what camera_rays(cfg) returns for the same cfg), the scene, the material attenuations and the
samples per pixel, it states what every sample must contribute — from the EXACT closest hit of the primary
(exact_hits.Reference) — and how far a kernel's value may be from that, and holds a guide buffer to the sums.

The rays and the band.  The guides kernel does not read the exported rays: it evaluates camera_ray inline, and the
contraction pass may fuse its multiplies and adds differently than in the camera-ray kernel.  STRICT: no contraction,
IEEE operations, the same written expressions: the two rays carry the same bits, the band is exact_hits.TAU[STRICT] and
no perturbation is added.  FAST: both rays are evaluations of
    u = (j + ju) * inv_wm1,  v = (H - 1 - i + jv) * inv_hm1          (j + ju is exact: 11 + 21 bits)
    from = origin + (cam_u * (lens * px) + cam_v * (lens * py))
    d    = llc + u * horizontal + v * vertical - from
with the same operands.  Uncontracted, the direction's terms pass u (1), u * horizontal (2), llc + (3), + v * vertical
(4), - from (5) roundings and the origin's terms lens * px (1), cam_u * (2), + cam_v * (3), origin + (4); a contracted
evaluation has fewer.  Each ray is therefore within 5 u S (direction) and 4 u S (origin) of the real value, S the sum of
the magnitudes of the component's terms (guides_ref.camera_ray_scales), and the two rays within
    K_CAM_D = 10 on the direction,  K_CAM_O = 8 on the origin
of each other: twice the depth of one evaluation, because the exported ray is itself a rounded evaluation and not the
real value (a count of 7 and 4 holds for one evaluation against the real value, with inv_wm1's own rounding counted;
both kernels read the same inv_wm1, so it does not separate them, but the second evaluation does).  The lens point
(px, py) is behind a second-order square root and a degree-9 polynomial (rtow_trace_rng.h lens_from_block: th 1, x^2 3,
four Horner levels of 5, the last product 2, rho * 3: about 30 roundings uncontracted on top of the 4 above), so the
lens offset's magnitude enters S with weight LENS_W = 8 (8 x 8 = 64 >= 2 x 34), as f32_audit.py weighs it (ray_magnitudes).
The band is widened the way the binary32 build's is (exact_hits.py: the quadratic terms of disc see the ray twice):
    tau_fast = 2 (17 + 2 K_CAM_D) u = 74 u
on S_q with omag / dmag in the place of |o_i| / |d_i|.  Below, eo = K_CAM_O u omag and ed = K_CAM_D u dmag are the
componentwise bounds on (kernel's ray - exported ray), |ed| their Euclidean norm; both are 0 in the strict build.  The
shutter time jt * (t1 - t0) + t0 is one product and one sum: et = 2 u tmag, which moves a moving sphere's centre by
|c1 - c0| et.

A sample is DECIDED when the reference's closest hit is (exact_hits: every decision outside the band, the nearest hit
clear of the second-nearest) and not an exact tie of two primitives.  With (t, E, front, primitive) the exact answer and
its t bound, the kernel's t_k is within E of t, and the sample's values are (u = 2^-53 per rounding, R = 0 in the strict
build and R_SQRT in the fast build):
  * R_SQRT = 1.5 * 2^-46: fast_sqrt_pos / fast_rsqrt (rtow_trace_math.h) are the hardware seed y = rsq(x) (1 + e) and ONE
    second-order step, y (1 + (1 - x y^2) / 2) = (1 - 3/2 e^2 - ...) / sqrt(x); the instruction set's documented accuracy
    of the binary64 rsq / rcp seeds is 2^29 ulp, |e| <= 2^-23.  fast_rcp's step is third order: 1 ulp.
  * hit, albedo: the attenuation of the primitive's material, a table value: no error.
  * hit, depth t * sqrt(d.d): |t_k |d'| - t |d|| <= E (|d| + |ed|) + t |ed|, and the roundings — the kernel's dot (3, halved
    by the root), root (1) and product (1), the same three in this module's binary64 evaluation, t's own rounding (1):
    8, K_DEPTH = 10 — so E (|d| + |ed|) + t |ed| + (K_DEPTH u + R) t |d|.
  * hit, sphere normal: exact_hits' record bound with the ray's perturbation in the point,
    pb_i = |d_i| E + 4 u (|o_i| + |t d_i|) + eo_i + (t + E) ed_i + |c1_i - c0_i| et,
    nb = 2 sqrt(3) (max_i pb_i + 4 u |c|) / |r| + 8 u + R, plus this module's own binary64 evaluation of
    (o + t d - c) / |r|: (4 u max_i (|o_i| + |t d_i|) + 5 u |c|) / |r| (exact_hits._check_exact_record).  The sign is the
    exact front_face's (decided with the hit): N if front else -N, N = (p - c) / |r|.
  * hit, triangle normal n / sqrt(n.n), n the record's e1 x e2 (bit-equal to exact_hits.Scene.tri_n): dot (3, halved), root
    (1), quotient (1; the fast build's rcp and product 2) in the kernel and in this module: K_TRI = 10, bound K_TRI u + R
    per component.  The ray does not enter.
  * miss, the sky c = (1 - w) + w (0.5, 0.7, 1), w = 0.5 (y + 1), y = d.y * rsqrt(d.d): y is within 2 |ed| / |d| (the
    ray) + 4.5 u + R (dot 1.5, 1 / sqrt 2, product 1) of d.y / |d|; w adds 1 u; |dc / dw| <= 0.5 and c's three operations
    add 3 u: 0.5 |ed| / |d| + 4.6 u + 0.25 R in the kernel and 4.6 u here: bound 0.5 |ed| / |d| + K_SKY u + 0.25 R, K_SKY = 10.

A pixel is decided when all its samples are.  Its sums are added in sample order from +0.0 on rounded operands, so
  * hits is the exact count, bit for bit;
  * albedo is the in-order binary64 sum of the table values bit for bit when every sample hits; otherwise, and for normal
    and depth, |got - in-order sum of the expected values| <= (sum of the samples' bounds) + spp u (sum of |expected| +
    bounds): the kernel's adds round partial sums that differ from this module's.
Every pixel, decided or not: eight finite values; hits an integer in [decided hits, decided hits + undecided samples];
|normal|_2 <= hits (1 + K_TRI u + R + spp u) (a sum of hits vectors of at most unit length, each within the normal's
rounding of it); depth >= 0; every albedo component in [0, spp] (attenuations and sky components are at most 1: the
sky's (1 - w) + w rounds to at most 1).

No constant here was fitted to a GPU result.
"""
from __future__ import annotations

import math

import numpy as np

import exact_hits as ex

U = ex.U
STRICT, FAST = ex.STRICT, ex.FAST
K_CAM_D, K_CAM_O, LENS_W = 10, 8, 8.0
TAU_FAST = 2 * (17 + 2 * K_CAM_D) * U
R_SQRT = 1.5 * 2.0 ** -46
K_DEPTH, K_TRI, K_SKY = 10, 10, 10
SKY = np.array([0.5, 0.7, 1.0])
FIELDS = ("albedo", "normal", "depth", "hits")
_COLS = {"albedo": slice(0, 3), "normal": slice(3, 6), "depth": slice(6, 7), "hits": slice(7, 8)}


class CheckError(AssertionError):
    """failures: [{pixel, samples, field, got, expected, bound}] (the first few)."""

    def __init__(self, msg, failures):
        super().__init__(msg)
        self.failures = failures


def ray_magnitudes(s_org, s_dir, cam_origin):
    """(omag, dmag) from guides_ref.camera_ray_scales' (S_origin, S_direction): the lens offset's magnitude
    S_origin - |camera origin| weighted LENS_W in both (the module docstring)."""
    extra = (LENS_W - 1.0) * (s_org - np.abs(np.asarray(cam_origin, np.float64))[None, :])
    assert np.all(extra >= 0)
    return s_org + extra, s_dir + extra


def _in_order(v, spp):
    """[n * spp, ...] -> [n, ...]: ((0 + v_0) + v_1) + ..."""
    c = v.reshape((-1, spp) + v.shape[1:])
    s = np.zeros((c.shape[0],) + v.shape[1:])
    for j in range(spp):
        s = s + c[:, j]
    return s


class GuideReference:
    """What a guides call must return for the primaries `rays` (RAY_DTYPE, pixel-major, `spp` samples per pixel
    ascending) with identities `ids` [n, 2] (pixel, sample).  scene: exact_hits.Scene; att [materials, 3]:
    guides_ref.attenuations; build: STRICT or FAST; unit_cut: the fast GRID walk (exact_hits); omag, dmag [n, 3]:
    ray_magnitudes (FAST only, required there); tmag [n]: camera_ray_scales' S_time (default |time|)."""

    def __init__(self, rays, ids, scene, att, spp, build, unit_cut=False, omag=None, dmag=None, tmag=None):
        n = len(rays)
        assert spp >= 1 and n % spp == 0 and ids.shape == (n, 2)
        idp = ids.reshape(-1, spp, 2).astype(np.int64)
        assert np.all(idp[:, :, 0] == idp[:, :1, 0]), "a pixel's samples are not consecutive"
        assert np.all(idp[:, :, 1] == idp[:, :1, 1] + np.arange(spp)[None, :]), "a pixel's samples do not ascend"
        self.rays, self.ids, self.scene, self.spp, self.build = rays, idp, scene, spp, build
        self.att = np.asarray(att, np.float64)
        self.R = R_SQRT if build == FAST else 0.0
        if build == FAST:
            assert omag is not None and dmag is not None
            self.eo, self.ed = K_CAM_O * U * np.asarray(omag), K_CAM_D * U * np.asarray(dmag)
            tm = np.abs(rays["time"]) if tmag is None else np.asarray(tmag, np.float64)
            self.et = 2 * U * tm
            self.ref = ex.Reference(scene, rays, FAST, unit_cut=unit_cut, tau=TAU_FAST, omag=omag, dmag=dmag)
        else:
            assert build == STRICT and omag is None and dmag is None
            self.eo = self.ed = np.zeros((n, 3))
            self.et = np.zeros(n)
            self.ref = ex.Reference(scene, rays, STRICT, unit_cut=False)
        self._expect()

    # -- per sample --
    def _expect(self):
        ref, sc, R = self.ref, self.scene, self.R
        n = len(self.rays)
        o = np.ascontiguousarray(self.rays["origin"], np.float64)
        d = np.ascontiguousarray(self.rays["direction"], np.float64)
        time = np.ascontiguousarray(self.rays["time"], np.float64)
        eo, ed, et = self.eo, self.ed, self.et
        single = np.array([len(t) <= 1 for t in ref.ties], bool).reshape(n)
        self.decided = ref.decided & single
        self.hit = np.array([len(t) >= 1 for t in ref.ties], bool).reshape(n)  # (the exact answer)
        prim = np.array([t[0] if len(t) else -1 for t in ref.ties], np.int64).reshape(n)
        self.prim = prim
        dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        ed2 = np.linalg.norm(ed, axis=1)
        # the miss
        y = d[:, 1] * (1.0 / dn)
        w = 0.5 * (y + 1.0)
        sky = (1.0 - w)[:, None] + w[:, None] * SKY[None, :]
        sky_b = 0.5 * ed2 / dn + K_SKY * U + 0.25 * R
        # the hit
        h = self.hit
        hp = np.where(h, prim, 0)
        t = np.where(h, ref.t, 0.0)
        E = np.where(h, ref.E, 0.0)
        kind, index = sc.kind[hp], sc.index[hp]
        alb = np.where(h[:, None], self.att[sc.prim_mat[hp]], sky)
        alb_b = np.where(h, 0.0, sky_b)
        dep = np.where(h, t * dn, 0.0)
        dep_b = np.where(h, E * (dn + ed2) + t * ed2 + (K_DEPTH * U + R) * t * dn, 0.0)
        nrm = np.zeros((n, 3))
        nrm_b = np.zeros(n)
        tri = h & (kind == ex.TRIANGLE)
        if tri.any():
            tn = sc.tri_n[index[tri]]
            s = np.sqrt(tn[:, 0] * tn[:, 0] + tn[:, 1] * tn[:, 1] + tn[:, 2] * tn[:, 2])
            nrm[tri] = tn / s[:, None]
            nrm_b[tri] = K_TRI * U + R
        sph = h & (kind != ex.TRIANGLE)
        if sph.any():
            c = np.zeros((n, 3))
            r = np.ones(n)
            cm = np.zeros(n)
            dc = np.zeros((n, 3))
            st = sph & (kind == ex.SPHERE)
            g = sc.sph[index[st]]
            c[st], r[st], cm[st] = g[:, :3], g[:, 3], np.max(np.abs(g[:, :3]), axis=1).reshape(-1)
            mv = sph & (kind == ex.MOVING)
            if mv.any():
                g = sc.mov[index[mv]]
                dcm = g[:, 3:6] - g[:, :3]
                step = time[mv][:, None] * dcm
                c[mv], r[mv], dc[mv] = g[:, :3] + step, g[:, 6], np.abs(dcm)
                cm[mv] = np.max(np.abs(g[:, :3]) + np.abs(step), axis=1)
            td = t[:, None] * d
            pe = o + td
            own = np.abs(o) + np.abs(td)
            pb = np.abs(d) * E[:, None] + 4 * U * own + eo + (t + E)[:, None] * ed + dc * et[:, None]
            ar = np.abs(r)
            nf = (pe - c) / ar[:, None]
            nb = (2 * math.sqrt(3) * (pb.max(axis=1) + 4 * U * cm) / ar + 8 * U + R
                  + (4 * U * own.max(axis=1) + 5 * U * cm) / ar)
            front = np.asarray(ref.front, bool)
            nrm[sph] = np.where(front[:, None], nf, -nf)[sph]
            nrm_b[sph] = nb[sph]
        self.value = np.concatenate([alb, nrm, dep[:, None], h.astype(np.float64)[:, None]], axis=1)  # [n, 8]
        self.bound = np.concatenate([np.repeat(alb_b[:, None], 3, 1), np.repeat(nrm_b[:, None], 3, 1), dep_b[:, None],
                                     np.zeros((n, 1))], axis=1)

    def counts(self):
        """(pixels, pixels with an undecided sample, undecided samples, the exact hit share of the samples)."""
        dec = self.decided.reshape(-1, self.spp)
        return len(dec), int((~dec.all(axis=1)).sum()), int((~dec).sum()), float(self.hit.mean())

    # -- per pixel --
    def check(self, guides, what=""):
        """`guides` [pixels, 8] float64 (albedo, normal, depth, hits per pixel, the pixels of `ids` in order) against the
        expectation.  Returns {"pixels", "undecided_pixels", "undecided_samples", "hit_share", "worst": {field: the
        largest error / bound over the decided pixels}}; raises CheckError naming pixel, samples, field, got, expected
        and bound of the first failures."""
        spp = self.spp
        got = np.ascontiguousarray(guides, np.float64)
        npix = len(self.rays) // spp
        assert got.shape == (npix, 8), (got.shape, npix)
        pixel = self.ids[:, 0, 0]
        first = self.ids[:, 0, 1]
        bad = []

        def fail(p, field, g, e, b):
            if len(bad) < 8:
                s = list(range(int(first[p]), int(first[p]) + spp))
                bad.append({"pixel": int(pixel[p]), "samples": s, "field": field, "got": np.array(g).tolist(),
                            "expected": np.array(e).tolist(), "bound": np.array(b).tolist()})

        dec = self.decided.reshape(npix, spp)
        hit = self.hit.reshape(npix, spp)
        full = dec.all(axis=1)
        want = _in_order(self.value, spp)
        slack = _in_order(self.bound, spp)
        slack = slack + spp * U * (_in_order(np.abs(self.value), spp) + slack)
        all_hit = full & hit.all(axis=1)
        slack[all_hit, 0:3] = 0.0  # table values added in order: the bits
        err = np.abs(got - want)
        finite = np.isfinite(got).all(axis=1)
        worst = {}
        for f in ("albedo", "normal", "depth"):
            e, b = err[full & finite][:, _COLS[f]], slack[full & finite][:, _COLS[f]]
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0))
            worst[f] = float(q.max()) if q.size else 0.0
        # every pixel
        d_hits = (dec & hit).sum(axis=1)
        und = (~dec).sum(axis=1)
        small = K_TRI * U + self.R + spp * U
        for p in np.nonzero(~finite)[0]:
            f = next(f for f in FIELDS if not np.isfinite(got[p, _COLS[f]]).all())
            fail(p, f, got[p, _COLS[f]], want[p, _COLS[f]], slack[p, _COLS[f]])
        hv = got[:, 7]
        with np.errstate(invalid="ignore"):
            wrong = finite & ~((hv == np.floor(hv)) & (hv >= d_hits) & (hv <= d_hits + und))
            for p in np.nonzero(wrong)[0]:
                fail(p, "hits", hv[p], [int(d_hits[p]), int(d_hits[p] + und[p])], 0.0)
            ok = finite & ~wrong
            long = ok & ~(np.linalg.norm(got[:, 3:6], axis=1) <= hv * (1 + small))
            for p in np.nonzero(long)[0]:
                fail(p, "normal", got[p, 3:6], f"|normal| <= hits = {hv[p]}", hv[p] * small)
            for p in np.nonzero(ok & ~(got[:, 6] >= 0))[0]:
                fail(p, "depth", got[p, 6], ">= 0", 0.0)
            for p in np.nonzero(ok & ~((got[:, 0:3] >= 0) & (got[:, 0:3] <= spp)).all(axis=1))[0]:
                fail(p, "albedo", got[p, 0:3], f"in [0, {spp}]", 0.0)
            # decided pixels: the sums
            for f in ("albedo", "normal", "depth"):
                c = _COLS[f]
                for p in np.nonzero(full & ok & ~(err[:, c] <= slack[:, c]).all(axis=1))[0]:
                    fail(p, f, got[p, c], want[p, c], slack[p, c])
        n_pix, n_und, n_unds, share = self.counts()
        stats = {"pixels": n_pix, "undecided_pixels": n_und, "undecided_samples": n_unds, "hit_share": share,
                 "worst": worst}
        if bad:
            lines = [f"pixel {b['pixel']} samples {b['samples']} {b['field']}: got {b['got']}, expected {b['expected']}, "
                     f"bound {b['bound']}" for b in bad]
            raise CheckError(f"{what}: {len(bad)}+ failures:\n  " + "\n  ".join(lines), bad)
        return stats


def report(what, stats):
    w = stats["worst"]
    return (f"{what}: {stats['undecided_pixels']} of {stats['pixels']} pixels undecided ({stats['undecided_samples']} "
            f"samples), hit share {stats['hit_share']:.3f}, worst error / bound: albedo {w['albedo']:.3g}, normal "
            f"{w['normal']:.3g}, depth {w['depth']:.3g}")
