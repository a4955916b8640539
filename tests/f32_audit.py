"""Sample audit of the binary32 build (RTOW_F32): every shallow sample of a frame against the exact reference
(tests/exact_hits.py) — test infrastructure (numpy + ctypes, importable without a GPU).

The queries refuse RTOW_F32, so the render is the only window into that build; a shallow one-sample frame
(sample_audit.sample_cfg) is a read-out of decisions (oracle/rtow_oracle.cpp ray_color):

  * max_child_rays = 0 (layer P): black iff the primary ray hits anything, else the sky of the primary direction;
  * max_child_rays = 1 (layer S): a hit sample is albedo * sky(scattered direction) if the scattered ray misses, black
    if it hits (or the scatter was absorbed).

The oracle's ray log gives the primary and the scattered ray of every sample identity in binary64.  A sample is KEPT when
every decision that makes its colour is certain under the binary32 band (exact_hits.F32: tau_f32 = 2 * K32 * 2^-24 on
S_q, or the first-order bound beside it where that is smaller; the count and both bounds are in that module's header); on a kept sample the build must show the exact decision, with no exception.

Layer P.  The build's primary is llc + u h + v w - from evaluated in binary32 from cam32, not the oracle's ray: the
magnitudes of that expression's terms stand for |d_i| and |o_i| in S_q (omag, dmag of exact_hits.Reference; u, v are
recovered from the logged ray), and the K_CAM roundings of the camera are part of K32.  The lens offset passes through
the binary32 sine polynomial and a square root (about 20 roundings, against K_CAM = 6 on the other terms): its magnitude
is weighted by LENS_W.  Kept = Reference.occ_decided.  A kept miss must be within
    tol_sky = 2 (0.25 K_CAM 2^-24 |dmag|_2 / |d|_2 + K_SKY 2^-24)
of the oracle's colour per channel: d(unit.y) <= |delta d|_2 / |d|_2, the sky 0.5 (unit.y + 1) blended with a slope of at
most 0.5 per channel, and K_SKY = 13 roundings on values <= 1 in normalize (dot 3, rsqrt with its Newton step 4,
product 1) and the blend (5).

Layer S.  Kept when
  * the primary is fully decided (Reference.decided: which primitive, which face);
  * the material is Lambertian or metal (dielectric primaries are counted and left out);
  * the hit is on the outside of a sphere of positive radius, or on a triangle;
  * conditioning: with E_p the bound on the build's hit point (|d_i| E_t + the camera's error at t + 4 roundings of the
    point) and E_d the bound on its scattered direction (through the normal bound of exact_hits' header, n + rnd or
    reflect, and the binary32 sampler: sine polynomial, sqrt(1 - z^2), whose error grows like 1 / sqrt(1 - z^2)),
    E_p <= A 2^-24 |r| (a triangle: the square root of |e1 x e2|), the normal bound <= A 2^-24 |n| and |E_d|_2 <=
    A 2^-24 |d2|_2, with A = 2^18: every bound below 2^-6 of its scale, so that what the first-order bounds neglect
    is 2^-6 of what they state, well inside their factor 2.  (A few 2^-24 would keep nothing: ten units from the
    camera the binary32 sphere test leaves E_p near 1e-3, see exact_hits' header.);
  * the scattered ray leaves its primitive: (p - c).d2 stays positive under the bounds, and the root of the primitive's
    own quadratic that the build may compute near 0, (off-surface distance of the build's point) / (cos theta |d2|)
    plus the binary32 test's own error, is below tmin / 2.  A triangle's own plane cannot be hit again once
    det = -d2.n is certainly below the cut;
  * the scattered ray's any-hit against every OTHER primitive is decided under the first-order band TAU_ARITH S_q' +
    2 D_q, D_q the effect of E_p and E_d on q (exact_hits.Reference operr / derr, first_order).  A relative band
    2 (K32 + A) 2^-24 S_q cannot stand in for it: E_p on a small sphere ten units away is a few 1e-3 (thousands of
    2^-24 x scale), and an error along the ground (y ~ 0) is not dominated by S_q's per-axis magnitudes.
On a kept sample the build is black iff the scattered ray hits; otherwise within
    tol_S = albedo 2 (0.25 |E_d|_2 / |d2|_2 + K_SKY 2^-24) + 6 2^-24 colour
of the oracle's colour (the albedo's rounding and the product: 3 roundings, doubled).

Spheres tested in binary64 (`assumed_large`): every kernel of the build tests the ground sphere in binary64 on the
widened ray (GRID: the large list; BVH and STREAM: every sphere), so its band is the input error alone
(Reference large=).  The audit assumes this only for spheres with |r| >= 10 x the median |r|; the GPU tests check the
assumption against the resident grid image.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import exact_hits as ex
import orc
import rtow
import sample_audit as sa
from support_oracle import log_rays, rays_of
from support_scenes import SceneView, handmade_scene, suzanne

U32 = ex.U32
K_CAM = 6        # roundings on the camera's direction: llc (1), u = (j + ju) * inv (2), two products and sums, - from
LENS_W = 4.0     # weight of the lens offset's magnitude (about 4 x K_CAM roundings behind it)
K_SKY = 13
K_ARITH = ex.K32_ARITH  # the binary32 sphere test alone, without the ray's own error (exact_hits' header)
A = 2 ** 18      # conditioning threshold of layer S, in units of 2^-24 x scale: bounds below 2^-6 of their scale
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2


class AuditError(AssertionError):
    pass


# ---- scenes: arrays <-> rtow.Scene ---------------------------------------------------------------------------------
class Held:
    """An rtow.Scene (`.c`) and the arrays it points into."""

    def __init__(self, c, keep):
        self.c, self.keep = c, keep


def arrays_of(scene):
    return orc.scene_arrays(scene.c if hasattr(scene, "c") else scene)


def camera_of(scene):
    return rtow.Camera.from_buffer_copy((scene.c if hasattr(scene, "c") else scene).camera)


def scene_from(a, camera):
    """The rtow.Scene of the arrays `a` (orc.scene_arrays' layout) with `camera`."""
    g = {k: np.ascontiguousarray(a[k], np.float64) for k in ("sphere_geom", "moving_geom", "triangle_geom")}
    m = {k: np.ascontiguousarray(a[k], np.int32) for k in ("sphere_mat", "moving_mat", "triangle_mat", "prim_kind",
                                                          "prim_index")}
    mats = (rtow.Material * len(a["materials"]))()
    for i, r in enumerate(np.asarray(a["materials"], np.float64)):
        mats[i].albedo[:] = [float(x) for x in r[:3]]
        mats[i].fuzz, mats[i].ir, mats[i].kind = float(r[3]), float(r[4]), int(r[5])
    s = rtow.Scene()
    s.camera = camera
    pd = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    pi = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    s.n_spheres, s.sphere_geom, s.sphere_mat = len(m["sphere_mat"]), pd(g["sphere_geom"]), pi(m["sphere_mat"])
    s.n_moving, s.moving_geom, s.moving_mat = len(m["moving_mat"]), pd(g["moving_geom"]), pi(m["moving_mat"])
    s.n_triangles, s.triangle_geom, s.triangle_mat = len(m["triangle_mat"]), pd(g["triangle_geom"]), pi(m["triangle_mat"])
    s.n_materials, s.materials = len(mats), mats
    s.n_prims, s.prim_kind, s.prim_index = len(m["prim_kind"]), pi(m["prim_kind"]), pi(m["prim_index"])
    return Held(s, [g, m, mats, camera])


def translated(scene, off):
    """`scene` and its camera moved by `off`."""
    a, cam = arrays_of(scene), camera_of(scene)
    off = np.asarray(off, np.float64)
    for k, w, cols in (("sphere_geom", 4, (0,)), ("moving_geom", 8, (0, 3)), ("triangle_geom", 9, (0, 3, 6))):
        v = a[k].reshape(-1, w)
        for c0 in cols:
            v[:, c0:c0 + 3] += off
    for f in ("origin", "lower_left_corner"):
        v = getattr(cam, f)
        for k in range(3):
            v[k] += float(off[k])
    return scene_from(a, cam)


def with_camera(scene, lookfrom, lookat, vfov, aspect):
    """`scene` seen from `lookfrom` towards `lookat` (the reference's camera construction, up = +y, focused on lookat;
    the scene's own lens radius and shutter): a nearer camera, for frames whose binary32 hit points are too uncertain
    from where the scene's own camera stands."""
    a, cam = arrays_of(scene), camera_of(scene)
    lf, la = np.asarray(lookfrom, np.float64), np.asarray(lookat, np.float64)
    unit = lambda x: x / np.sqrt(np.dot(x, x))  # noqa: E731
    w = unit(lf - la)
    u = unit(np.cross(np.array([0.0, 1.0, 0.0]), w))
    v = unit(np.cross(w, u))
    vh = 2.0 * math.tan(math.radians(vfov) / 2)
    fd = math.sqrt(np.dot(lf - la, lf - la))
    hor, ver = fd * aspect * vh * u, fd * vh * v
    llc = lf - hor / 2.0 - ver / 2.0 - fd * w
    for f, val in (("origin", lf), ("u", u), ("v", v), ("w", w), ("horizontal", hor), ("vertical", ver),
                   ("lower_left_corner", llc)):
        getattr(cam, f)[:] = [float(x) for x in val]
    return scene_from(a, cam)


# ---- planted faults: the arrays of a scene that is wrong in one way ---------------------------------------------------
def without_triangle(a, k):
    a = {n: v.copy() for n, v in a.items()}
    a["triangle_geom"] = np.delete(a["triangle_geom"].reshape(-1, 9), k, axis=0).reshape(-1)
    a["triangle_mat"] = np.delete(a["triangle_mat"], k)
    tri = a["prim_kind"] == ex.TRIANGLE
    drop = np.flatnonzero(tri & (a["prim_index"] == k))
    a["prim_index"] = np.where(tri & (a["prim_index"] > k), a["prim_index"] - 1, a["prim_index"])
    a["prim_kind"], a["prim_index"] = np.delete(a["prim_kind"], drop), np.delete(a["prim_index"], drop)
    return a


def with_radius(a, cls, k, delta):
    a = {n: v.copy() for n, v in a.items()}
    if cls == ex.SPHERE:
        a["sphere_geom"][4 * k + 3] += delta
    else:
        a["moving_geom"][8 * k + 6] += delta
    return a


def frozen(a, k):
    a = {n: v.copy() for n, v in a.items()}
    a["moving_geom"][8 * k + 3:8 * k + 6] = a["moving_geom"][8 * k:8 * k + 3]
    return a


def _mat_slot(a, cls, k):
    return a[("sphere_mat", "moving_mat", "triangle_mat")[cls]], k


def with_materials_swapped(a, p, q):
    """p, q: (class, class index)."""
    a = {n: v.copy() for n, v in a.items()}
    (ma, i), (mb, j) = _mat_slot(a, *p), _mat_slot(a, *q)
    ma[i], mb[j] = int(mb[j]), int(ma[i])
    return a


def with_albedo_rotated(a):
    a = {n: v.copy() for n, v in a.items()}
    a["materials"][:, :3] = np.roll(a["materials"][:, :3], 1, axis=1)
    return a


# ---- the oracle's shallow one-sample frames ----------------------------------------------------------------------------
def shallow_cfg(cfg, depth, precision=rtow.F64_STRICT, kernel=rtow.KERNEL_AUTO):
    return sa.copy_cfg(cfg, max_child_rays=depth, precision=precision, kernel=kernel)


def oracle_frames(scene, cfg):
    """(c0, c1) [spp, H, W, 3]: the oracle's one-sample frames of `cfg` at max_child_rays 0 and 1."""
    return tuple(sa.oracle_samples(scene, shallow_cfg(cfg, k))[0] for k in (0, 1))


def assumed_large(view):
    """The (class, index) of the spheres the audit takes as tested in binary64 by every kernel of the build."""
    r = np.concatenate([np.abs(view.sph[:, 3]), np.abs(view.mov[:, 6])])
    if len(r) == 0:
        return []
    med = float(np.median(r))
    return [(ex.SPHERE, int(i)) for i in np.flatnonzero(np.abs(view.sph[:, 3]) >= 10 * med)]


def _sky(d):
    y = d[:, 1] / np.linalg.norm(d, axis=1)
    t = 0.5 * (y + 1.0)
    return (1.0 - t)[:, None] * np.ones(3) + t[:, None] * np.array([0.5, 0.7, 1.0])


# ---- the nearest decision of a ray, for the messages and the write-up -----------------------------------------------------
def margins(sc, o, d, time, exclude=None, chunk=1 << 19):
    """Per ray: (|q| / S_q in units of 2^-24 of the decision that its any-hit answer hangs on, the primitive (class,
    index) it belongs to).  A ray that hits: the most certain of its hits; a ray that misses: the least certain of its
    misses.  Per primitive q is the decision nearest to flipping (a sphere's discriminant; of a triangle that passes
    every test the smallest, of one that fails some the largest of the failing ones), S_q on the plain magnitudes of the
    binary32 forms (|o_i| + |c_i|, |o_i| + |A_i|).  The t-window decisions are left out: this is a diagnostic."""
    n = len(o)
    lo, hi = np.full(n, np.inf), np.full(n, -np.inf)  # the least certain miss, the most certain hit
    wlo, whi = np.full((n, 2), -1, np.int64), np.full((n, 2), -1, np.int64)

    def fold(ri, cls, ci, m, hits):
        m = np.where(np.isfinite(m), m, np.inf)
        if exclude is not None:
            ex_ = (exclude[ri, 0] == cls) & (exclude[ri, 1] == ci)
            m, hits = np.where(ex_, np.inf, m), hits & ~ex_
        for sel, acc, who_, sign in ((~hits, lo, wlo, 1.0), (hits, hi, whi, -1.0)):
            r_, c_, m_ = ri[sel], ci[sel], sign * m[sel]
            order = np.argsort(m_, kind="stable")
            r_, c_, m_ = r_[order], c_[order], m_[order]
            first = np.unique(r_, return_index=True)[1]
            r_, c_, m_ = r_[first], c_[first], m_[first]
            upd = m_ < sign * acc[r_]
            acc[r_[upd]] = sign * m_[upd]
            who_[r_[upd], 0], who_[r_[upd], 1] = cls, c_[upd]

    for cls, g in ((ex.SPHERE, sc.sph), (ex.MOVING, sc.mov)):
        if len(g) == 0:
            continue
        per = max(1, chunk // len(g))
        for r0 in range(0, n, per):
            ri = np.repeat(np.arange(r0, min(r0 + per, n)), len(g))
            ci = np.tile(np.arange(len(g)), len(ri) // len(g))
            if cls == ex.SPHERE:
                c, r = g[ci, :3], g[ci, 3]
                cm = np.abs(c)
            else:
                dc = g[ci, 3:6] - g[ci, :3]
                c, r = g[ci, :3] + time[ri][:, None] * dc, g[ci, 6]
                cm = np.abs(g[ci, :3]) + np.abs(time[ri][:, None] * dc)
            oc, dd = o[ri] - c, d[ri]
            a = np.einsum("ij,ij->i", dd, dd)
            h = np.einsum("ij,ij->i", oc, dd)
            disc = h * h - a * (np.einsum("ij,ij->i", oc, oc) - r * r)
            om = np.abs(o[ri]) + cm
            S_h = np.einsum("ij,ij->i", om, np.abs(dd))
            S_d = S_h * S_h + a * (np.einsum("ij,ij->i", om, om) + r * r)
            behind = (disc > 0) & (-h + np.sqrt(np.maximum(disc, 0)) < ex.TMIN * a)  # both roots behind the origin
            fold(ri, cls, ci, np.where(behind, np.inf, np.abs(disc) / S_d / U32), (disc > 0) & ~behind)
    g = sc.tri
    if len(g):
        per = max(1, chunk // len(g))
        for r0 in range(0, n, per):
            ri = np.repeat(np.arange(r0, min(r0 + per, n)), len(g))
            ci = np.tile(np.arange(len(g)), len(ri) // len(g))
            Av, e1, e2, nn = g[ci, :3], g[ci, 3:6] - g[ci, :3], g[ci, 6:9] - g[ci, :3], sc.tri_n[ci]
            Na = ex._cross_abs_v(np.abs(e1), np.abs(e2))
            dd, ao = d[ri], o[ri] - Av
            aom, dm = np.abs(o[ri]) + np.abs(Av), np.abs(dd)
            dao = np.cross(ao, dd)
            DAOa = ex._cross_abs_v(aom, dm)
            sm = lambda p, q: np.einsum("ij,ij->i", p, q)  # noqa: E731
            det, ud, vd, td = -sm(dd, nn), sm(e2, dao), -sm(e1, dao), sm(ao, nn)
            S_det, S_ud, S_vd = sm(dm, Na), sm(np.abs(e2), DAOa), sm(np.abs(e1), DAOa)
            q = np.stack([(det - ex.CUT) / S_det, ud / S_ud, vd / S_vd, (det - ud - vd) / (S_det + S_ud + S_vd)], axis=1)
            q = np.where(np.isfinite(q), q, np.inf)
            fails = q < 0
            m = np.where(fails.any(1), np.max(np.where(fails, -q, 0.0), axis=1), np.min(np.abs(q), axis=1)) / U32
            back = (det > 0) & (td < ex.TMIN * det)  # behind the origin
            fold(ri, ex.TRIANGLE, ci, np.where(back, np.inf, m), ~fails.any(1) & ~back)
    anyhit = np.isfinite(hi)
    return np.where(anyhit, hi, lo), np.where(anyhit[:, None], whi, wlo)


# ---- the audit of one frame ------------------------------------------------------------------------------------------
class Audit:
    """The reference side of one frame (scene, cfg): which samples layers P and S keep, and what they must show.
    Everything here comes from the oracle's ray log and the exact reference; `check_P` / `check_S` take the one-sample
    frames of the build under test, [spp, H, W, 3]."""

    def __init__(self, scene, cfg, name="", all_spheres_f64=False):
        """all_spheres_f64: the frame is only rendered by kernels that test EVERY sphere in binary64 (STREAM, BVH)."""
        self.scene, self.cfg, self.name, self.all_f64 = scene, cfg, name, all_spheres_f64
        self.view = SceneView(scene)
        self.sc = ex.Scene.of(self.view)
        self.W, self.H, self.spp = cfg.image_width, cfg.image_height, rtow.spp_effective(cfg)
        self.large = assumed_large(self.view)
        if all_spheres_f64:
            self.large = [(ex.SPHERE, i) for i in range(len(self.view.sph))] + \
                         [(ex.MOVING, i) for i in range(len(self.view.mov))]
        a = arrays_of(scene)
        self.mats = a["materials"]
        log = log_rays(scene, shallow_cfg(cfg, 1), accel=len(self.view.kind) > 2000)
        self.prim = log[log[:, 2] == 0]
        sec = log[log[:, 2] == 1]
        n = len(self.prim)
        assert n == self.W * self.H * self.spp, (n, self.W, self.H, self.spp)
        pix, self.pj = self.prim[:, 0].astype(np.int64), self.prim[:, 1].astype(np.int64)
        self.prow, self.pcol = pix // self.W, pix % self.W
        key = pix * self.spp + self.pj
        order = np.argsort(key)
        skey = sec[:, 0].astype(np.int64) * self.spp + sec[:, 1].astype(np.int64)
        at = np.searchsorted(key[order], skey)
        self.sec_of = np.full(n, -1, np.int64)  # primary -> row of `sec`
        self.sec_of[order[at]] = np.arange(len(sec))
        self.sec = sec
        self._primaries()
        self._secondaries()
        self._oracle = None

    # -- layer P --
    def _primaries(self):
        cam = self.scene.c.camera if hasattr(self.scene, "c") else self.scene.camera
        O, Hh, Vv, LLC = (np.array(getattr(cam, f)[:]) for f in ("origin", "horizontal", "vertical", "lower_left_corner"))
        o, d = self.prim[:, 3:6], self.prim[:, 6:9]
        uv = (d + o - LLC) @ np.linalg.pinv(np.stack([Hh, Vv], axis=1)).T
        self.omagP = np.abs(O) + LENS_W * np.abs(o - O)
        self.dmagP = np.abs(LLC) + np.abs(uv[:, :1] * Hh) + np.abs(uv[:, 1:] * Vv) + self.omagP
        self.raysP = rays_of(self.prim)
        self.refP = ex.Reference(self.sc, self.raysP, ex.F32, omag=self.omagP, dmag=self.dmagP,
                                 operr=K_CAM * U32 * self.omagP, derr=K_CAM * U32 * self.dmagP, large=self.large)
        self.keptP = self.refP.occ_decided.copy()
        self.tol_sky = 2 * (0.25 * K_CAM * U32 * np.linalg.norm(self.dmagP, axis=1) / np.linalg.norm(d, axis=1)
                            + K_SKY * U32)

    # -- layer S --
    def _secondaries(self):
        ref, sc, view = self.refP, self.sc, self.view
        n = len(self.prim)
        o, d, tm = self.prim[:, 3:6], self.prim[:, 6:9], self.prim[:, 9]
        why = np.full(n, "", dtype=object)  # why a sample is not kept ("" = kept so far)
        hit = np.array([len(t) == 1 for t in ref.ties]) & ref.decided
        why[~ref.decided] = "undecided"
        why[ref.decided & ~hit] = "sky"  # (a decided miss: layer P's business)
        prim = np.array([t[0] if len(t) == 1 else -1 for t in ref.ties])
        idx = np.flatnonzero(hit)
        cls, ci = view.kind[prim[idx]].astype(np.int64), view.index[prim[idx]].astype(np.int64)
        self.cls, self.ci = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        self.cls[idx], self.ci[idx] = cls, ci
        m = self.mats[view.prim_mat[prim[idx]]]
        kind, albedo, fuzz = m[:, 5].astype(np.int64), m[:, :3], np.clip(m[:, 3], 0.0, 1.0)
        self.albedo = np.zeros((n, 3))
        self.albedo[idx] = albedo
        why[idx[kind == DIELECTRIC]] = "dielectric"
        s_row = self.sec_of[idx]
        why[idx[(kind != DIELECTRIC) & (s_row < 0)]] = "absorbed"
        ok = (kind != DIELECTRIC) & (s_row >= 0)
        idx, cls, ci, kind, albedo, fuzz, s_row = (v[ok] for v in (idx, cls, ci, kind, albedo, fuzz, s_row))
        o, d, tm = o[idx], d[idx], tm[idx]
        o2, d2 = self.sec[s_row, 3:6], self.sec[s_row, 6:9]
        t, Et = ref.t[idx], ref.E[idx]
        omP, dmP = self.omagP[idx], self.dmagP[idx]
        Ep = np.abs(d) * Et[:, None] + K_CAM * U32 * (omP + t[:, None] * dmP) + 4 * U32 * (np.abs(o) + np.abs(t[:, None] * d))
        k = len(idx)
        # the primitive: centre, radius, normal and its bound
        c, r, cmag, nrm, nerr = np.zeros((k, 3)), np.ones(k), np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3))
        s0, s1, s2 = cls == ex.SPHERE, cls == ex.MOVING, cls == ex.TRIANGLE
        c[s0], r[s0], cmag[s0] = sc.sph[ci[s0], :3], sc.sph[ci[s0], 3], np.abs(sc.sph[ci[s0], :3])
        g = sc.mov[ci[s1]]
        c[s1], r[s1] = g[:, :3] + tm[s1][:, None] * (g[:, 3:6] - g[:, :3]), g[:, 6]
        cmag[s1] = np.abs(g[:, :3]) + np.abs(tm[s1][:, None] * (g[:, 3:6] - g[:, :3]))
        sph = s0 | s1
        inside = sph & ((ref.front[idx] != 1) | (r < 0))
        nrm[sph] = (o2[sph] - c[sph]) / r[sph][:, None]
        nerr[sph] = (2 * math.sqrt(3) * (Ep[sph].max(1) + 4 * U32 * cmag[sph].max(1)) / np.abs(r[sph]) + 8 * U32)[:, None]
        nrm[s2] = sc.tri_n[ci[s2]]
        nerr[s2] = U32 * np.abs(nrm[s2])
        # the sampler's point rnd and its bound (binary32 sine polynomial, sqrt(1 - z^2))
        refl = d - 2.0 * np.einsum("ij,ij->i", nrm, d)[:, None] * nrm
        lam = kind == LAMBERTIAN
        with np.errstate(divide="ignore", invalid="ignore"):
            rnd = np.where(lam[:, None], d2 - nrm, np.where(fuzz[:, None] > 0, (d2 - refl) / fuzz[:, None], 0.0))
            rb = np.linalg.norm(rnd, axis=1)
            z2 = np.clip(1.0 - (rnd[:, 2] / np.where(rb > 0, rb, 1.0)) ** 2, 2.0 ** -24, 1.0)
        Ernd = (U32 * rb * (12 + 2 / np.sqrt(z2)))[:, None] * np.ones(3)
        rderr = K_CAM * U32 * dmP
        ndot = np.einsum("ij,ij->i", np.abs(nrm), np.abs(d))
        ddot = np.einsum("ij,ij->i", nerr, np.abs(d)) + np.einsum("ij,ij->i", np.abs(nrm), rderr) + 3 * U32 * ndot
        Ed_l = nerr + Ernd + U32 * (np.abs(nrm) + np.abs(rnd))
        Ed_m = (rderr + 2 * (nerr * np.abs(np.einsum("ij,ij->i", nrm, d))[:, None] + np.abs(nrm) * ddot[:, None])
                + 3 * U32 * (np.abs(d) + 2 * np.abs(nrm) * ndot[:, None])
                + fuzz[:, None] * (Ernd + 2 * U32 * np.abs(rnd)) + U32 * np.abs(d2))
        Ed = np.where(lam[:, None], Ed_l, Ed_m)
        nEd, nd2 = np.linalg.norm(Ed, axis=1), np.linalg.norm(d2, axis=1)
        scale_o = np.where(sph, np.abs(r), np.sqrt(np.linalg.norm(nrm, axis=1)))  # the radius; a triangle's size
        nscale = np.linalg.norm(nrm, axis=1)  # (1 on a sphere; |e1 x e2| on a triangle)
        ill = ~((Ep.max(1) <= A * U32 * scale_o) & (nerr.max(1) <= A * U32 * nscale) & (nEd <= A * U32 * nd2))
        # the scattered ray leaves its primitive
        a2 = np.einsum("ij,ij->i", d2, d2)
        h2 = np.einsum("ij,ij->i", o2 - c, d2)
        h2lo = h2 - np.abs(r) * nEd - nd2 * math.sqrt(3) * Ep.max(1)
        is_large = np.zeros(k, bool)
        for (lc, li) in self.large:
            is_large |= (cls == lc) & (ci == li)
        om = np.abs(o - c)  # (the strict form's magnitudes: the arithmetic alone, on the values the test is given)
        S_h = np.einsum("ij,ij->i", om, np.abs(d))
        a1 = np.einsum("ij,ij->i", d, d)
        S_d = S_h * S_h + a1 * (np.einsum("ij,ij->i", om, om) + r * r)
        oc1 = o - c
        disc1 = np.maximum(np.einsum("ij,ij->i", oc1, d) ** 2 - a1 * (np.einsum("ij,ij->i", oc1, oc1) - r * r), 0.0)
        ta = 2 * K_ARITH * U32
        with np.errstate(divide="ignore", invalid="ignore"):
            Et_arith = (ta * S_h + np.minimum(np.sqrt(ta * S_d), ta * S_d / np.sqrt(disc1)) + ta * np.sqrt(disc1)
                        + ta * t * a1) / a1 + U32 * t
            Et_own = np.where(is_large, U32 * t, Et_arith)
            e_off = np.sqrt(a1) * Et_own + math.sqrt(3) * 3 * U32 * (np.abs(o) + np.abs(t[:, None] * d)).max(1)
            own32 = ((2 * np.abs(r) * math.sqrt(3) * 2 * U32 * (np.abs(o2) + cmag).max(1) + 8 * U32 * r * r) / (2 * h2lo)
                     + 16 * U32 * np.abs(h2) / a2)
            # (no further factor 2: Et_own carries the band's, the rounding counts above are 1.5 x what the code has)
            rehit = np.abs(r) * e_off / h2lo + np.where(is_large, 0.0, own32)
        inward_s = sph & ~(h2lo > 0)
        rehit_s = sph & ~inward_s & ~(rehit < ex.TMIN / 2)
        Na = np.zeros((k, 3))
        gt = sc.tri[ci[s2]]
        Na[s2] = ex._cross_abs_v(np.abs(gt[:, 3:6] - gt[:, :3]), np.abs(gt[:, 6:9] - gt[:, :3]))
        b_det = ex.TAU[ex.F32] * np.einsum("ij,ij->i", np.abs(d2), Na) + 2 * np.einsum("ij,ij->i", Ed, Na)
        # a triangle: outward, det = -d2.n is certainly below the cut; inward (the reference adds the sampler's point to
        # the UN-normalised normal, so half of a small triangle's scattered rays go through it), the plane's own root
        # (off-plane distance of the build's point) / (cos theta |d2|) must be certainly below tmin
        d2n = np.einsum("ij,ij->i", d2, nrm)
        ao1 = np.zeros((k, 3))
        ao1[s2] = np.abs(o[s2] - gt[:, :3])
        oA = np.zeros((k, 3))
        oA[s2] = np.abs(o[s2]) + np.abs(gt[:, :3])
        with np.errstate(divide="ignore", invalid="ignore"):
            det1 = np.abs(np.einsum("ij,ij->i", d, nrm))
            Et_tri = ((ex.TAU_ARITH * (np.einsum("ij,ij->i", ao1, Na) + t * np.einsum("ij,ij->i", np.abs(d), Na))
                       + 2 * U32 * np.einsum("ij,ij->i", oA, Na)) / det1 + U32 * t)
            e_off_t = np.sqrt(a1) * Et_tri + math.sqrt(3) * 3 * U32 * (np.abs(o) + np.abs(t[:, None] * d)).max(1)
            own_t = 2 * e_off_t * np.linalg.norm(nrm, axis=1) / (np.abs(d2n) - b_det)
        out_t = d2n + ex.CUT > b_det
        in_t = (d2n < -b_det - ex.CUT) & (own_t < ex.TMIN / 2)
        inward_t = s2 & ~(out_t | in_t)
        for mask, label in ((inside, "inside"), (ill & ~inside, "ill-conditioned"),
                            ((inward_s | inward_t) & ~inside & ~ill, "inward"),
                            (rehit_s & ~inside & ~ill, "own-root")):
            why[idx[mask]] = label
        cand = why[idx] == ""
        # the scattered ray's any-hit against every other primitive
        ii = idx[cand]
        rays2 = rtow.make_rays(o2[cand], d2[cand], time=tm[cand])
        self.exclude = np.stack([cls[cand], ci[cand]], axis=1)
        self.refS = ex.Reference(sc, rays2, ex.F32, exclude=self.exclude, operr=Ep[cand], derr=Ed[cand],
                                 large=self.large, first_order=True)
        und = ~self.refS.occ_decided
        why[ii[und]] = "secondary undecided"
        self.why = why
        self.keptS = why == ""
        self.idxS = ii[~und]                       # primaries kept by layer S
        self.hitS = self.refS.occ[~und]            # ... whose scattered ray hits: black
        self.raysS, self.excludeS = rays2[~und], self.exclude[~und]
        nE, nD = nEd[cand][~und], nd2[cand][~und]
        self.tol_dir = 2 * (0.25 * nE / nD + K_SKY * U32)  # x albedo, + 6 u32 colour: tol_S
        self.n_hits = int(hit.sum())
        self.n_lm = int(len(idx) - inside.sum())  # decided Lambertian and metal hits from outside, with a scattered ray

    # -- shares (the host test's conditions) --
    def shares(self):
        n = len(self.prim)
        cnt = {k: int((self.why == k).sum()) for k in ("undecided", "sky", "dielectric", "absorbed", "inside",
                                                      "ill-conditioned", "inward", "own-root", "secondary undecided")}
        lm = self.n_lm
        left = cnt["ill-conditioned"] + cnt["inward"] + cnt["own-root"] + cnt["secondary undecided"]
        return dict(samples=n, P_left_out=int((~self.keptP).sum()), P_share=float((~self.keptP).mean()),
                    S_undecided_share=cnt["undecided"] / n, S_lm_hits=lm, S_left_for_secondary=left,
                    S_left_share=left / max(lm, 1), S_kept=int(self.keptS.sum()), S_kept_black=int(self.hitS.sum()), **cnt)

    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_frames(self.scene, self.cfg)
        return self._oracle

    def worst_margins(self):
        """(layer P, layer S): the smallest |q| / band among the kept samples' nearest decisions (plain binary32 forms)."""
        kp = self.keptP
        mP, _ = margins(self.sc, self.prim[kp, 3:6], self.prim[kp, 6:9], self.prim[kp, 9])
        mS, _ = margins(self.sc, self.raysS["origin"], self.raysS["direction"], self.raysS["time"], self.excludeS)
        return (float(mP.min()) / (2 * ex.K32) if len(mP) else math.inf,
                float(mS.min()) / (2 * ex.K32) if len(mS) else math.inf)

    # -- the checks --
    def _where(self, i):
        return f"sample {int(self.pj[i])} row {int(self.prow[i])} column {int(self.pcol[i])}"

    def _margin_text(self, o, d, tm, exclude=None):
        m, who = margins(self.sc, o[None], d[None], np.array([tm]), None if exclude is None else exclude[None])
        return (f"nearest decision |q| / S_q = {m[0]:.3g} x 2^-24 (class {int(who[0, 0])} index {int(who[0, 1])}; "
                f"band {2 * ex.K32} x 2^-24)")

    def check_P(self, c0, what=""):
        """c0 [spp, H, W, 3]: the one-sample frames at max_child_rays = 0.  Returns the statistics; raises AuditError."""
        col = np.asarray(c0)[self.pj, self.prow, self.pcol]
        want = self.oracle()[0][self.pj, self.prow, self.pcol]
        hit = self.refP.occ
        with np.errstate(invalid="ignore"):
            err = np.abs(col - want).max(1)
        bad_hit = self.keptP & hit & (col != 0).any(1)
        bad_sky = self.keptP & ~hit & ~(err <= self.tol_sky)
        msgs = []
        for i in np.flatnonzero(bad_hit | bad_sky)[:8]:
            prims = [c.prim for c in self.refP.cands[i] if c.hit]
            msgs.append(f"  {self._where(i)}: the primary {'hits primitive ' + str(prims) if hit[i] else 'misses'}; colour "
                        f"{col[i].tolist()}, exact {want[i].tolist()} (tolerance {self.tol_sky[i]:.3g}); "
                        + self._margin_text(self.prim[i, 3:6], self.prim[i, 6:9], self.prim[i, 9]))
        nbad = int((bad_hit | bad_sky).sum())
        sky = self.keptP & ~hit
        stats = dict(kept=int(self.keptP.sum()), left_out=int((~self.keptP).sum()), kept_hits=int((self.keptP & hit).sum()),
                     worst_err_over_tol=float((err[sky] / self.tol_sky[sky]).max()) if sky.any() else 0.0)
        if nbad:
            raise AuditError(f"{what} layer P: {nbad} of {stats['kept']} kept samples are wrong\n" + "\n".join(msgs))
        return stats

    def check_S(self, c1, what=""):
        """c1 [spp, H, W, 3]: the one-sample frames at max_child_rays = 1."""
        ii = self.idxS
        col = np.asarray(c1)[self.pj[ii], self.prow[ii], self.pcol[ii]]
        want = self.oracle()[1][self.pj[ii], self.prow[ii], self.pcol[ii]]
        tol = self.albedo[ii] * self.tol_dir[:, None] + 6 * U32 * np.abs(want)
        with np.errstate(invalid="ignore"):
            err = np.abs(col - want)
        black = (col == 0).all(1)
        bad = np.where(self.hitS, ~black, black | ~(err <= tol).all(1))
        msgs = []
        for k in np.flatnonzero(bad)[:8]:
            i = ii[k]
            r = self.raysS[k]
            msgs.append(f"  {self._where(i)}: primary hits primitive {self.refP.ties[i][0]} (class {int(self.cls[i])} index "
                        f"{int(self.ci[i])}); the scattered ray {'hits' if self.hitS[k] else 'misses'}; colour "
                        f"{col[k].tolist()}, exact {want[k].tolist()} (tolerance {tol[k].tolist()}); "
                        + self._margin_text(r["origin"], r["direction"], float(r["time"]), self.excludeS[k]))
        lit = ~self.hitS
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, 0.0)
        stats = dict(kept=len(ii), kept_black=int(self.hitS.sum()),
                     worst_err_over_tol=float(ratio[lit].max()) if lit.any() else 0.0)
        if bad.any():
            raise AuditError(f"{what} layer S: {int(bad.sum())} of {len(ii)} kept samples are wrong\n" + "\n".join(msgs))
        return stats

    def check(self, c0, c1, what=""):
        return self.check_P(c0, what), self.check_S(c1, what)


def check_conditions(au):
    """The caps on what an audit may leave out, from the reference alone: layer P leaves out <= 1e-3 of the samples,
    <= 10 % of the primaries are not fully decided, <= 10 % of the decided Lambertian and metal hits are left out for
    the secondary's sake; and both outcomes of layer S occur.  A frame that exceeds a cap is the wrong frame (nearer
    camera, fewer grazing primaries): the caps stay."""
    s = au.shares()
    assert s["P_share"] <= 1e-3, (au.name, s)
    assert s["S_undecided_share"] <= 0.10, (au.name, s)
    assert s["S_left_share"] <= 0.10, (au.name, s)
    assert s["S_kept"] >= 1000 and s["S_kept_black"] >= 100 and s["S_kept"] - s["S_kept_black"] >= 100, (au.name, s)
    return s


# ---- the frames ---------------------------------------------------------------------------------------------------------
# 120 x 80 (suzanne 96 x 54), 4 samples, the seeds of support_oracle.LOGGED.  The cover scenes are seen from (2.6, 2.2, 2)
# towards (0.6, 0.2, 0.4), 40 degrees: from the scene's own camera at (13, 2, 3) the binary32 sphere test (h^2 and a c'
# cancel to a 2500th of their size on an r = 0.2 sphere ten units away) leaves the hit point and the normal of the small
# spheres too uncertain for layer S — 41 % and 37 % of the decided hits were left out there, against a cap of 10 %.
NEAR = ((2.6, 2.2, 2.0), (0.6, 0.2, 0.4), 40.0, 1.5)
FAR_OFFSET = (40.0, 0.0, 40.0)


def _cover(moving):
    return with_camera(rtow.HostScene.cover(11, 1.5, moving), *NEAR)


def _handmade():
    return with_camera(handmade_scene(), (6.0, 3.0, 5.0), (0.5, 0.8, -0.5), 40.0, 1.5)


def rotated(scene, angle=0.6):
    """`scene` with every point turned about the vertical axis through the origin (a motion of
    support_scenes.motions, for the case after a refit)."""
    a, cam = arrays_of(scene), camera_of(scene)
    rot = np.array([[math.cos(angle), 0, math.sin(angle)], [0, 1, 0], [-math.sin(angle), 0, math.cos(angle)]])
    for k, w, cols in (("sphere_geom", 4, (0,)), ("moving_geom", 8, (0, 3)), ("triangle_geom", 9, (0, 3, 6))):
        v = a[k].reshape(-1, w)
        for c0 in cols:
            v[:, c0:c0 + 3] = v[:, c0:c0 + 3] @ rot.T
    return scene_from(a, cam)


# name -> (scene, width, height, spp, seed, every sphere is tested in binary64 by the kernels that render the frame)
FRAMES = {
    "cover_static": (lambda: _cover(False), 120, 80, 4, 21, False),
    "cover_moving": (lambda: _cover(True), 120, 80, 4, 22, False),
    "suzanne": (suzanne, 96, 54, 4, 23, False),
    "cover0": (lambda: rtow.HostScene.cover(0, 1.5, True), 120, 80, 4, 21, True),
    "handmade": (_handmade, 120, 80, 4, 22, True),
    "cover_far": (lambda: translated(_cover(False), FAR_OFFSET), 120, 80, 4, 21, False),
    "cover_refit": (lambda: rotated(_cover(True)), 120, 80, 4, 22, False),
}
_audits = {}


def frame_cfg(name):
    mk, w, h, spp, seed, f64 = FRAMES[name]
    return rtow.make_config(w, h, spp, 1, 1, seed=seed, precision=rtow.F64_STRICT)


def audit(name):
    """The Audit of FRAMES[name]: computed once per process and shared; read-only."""
    if name not in _audits:
        mk, w, h, spp, seed, f64 = FRAMES[name]
        _audits[name] = Audit(mk(), frame_cfg(name), name, all_spheres_f64=f64)
    return _audits[name]
