"""The sample audit of the binary32 build (tests/f32_audit.py) on the CPU: the binary32 band of tests/exact_hits.py is
sound against binary32 restatements of the build's hit tests, the frames keep enough samples, and the checker rejects
planted faults.  tests/test_gpu_f32_audit.py runs the audit on the RTOW_F32 renders.

Shares measured on the frames of f32_audit.FRAMES (K32 = 22; samples / layer P left out / primaries not fully decided /
decided Lambertian and metal hits / of those left out for the secondary's sake: ill-conditioned, own root not certainly
below tmin (a triangle: scattered ray in its plane), scattered ray undecided against ANOTHER primitive):
  cover_static   38,400 / 0 / 20 (0.05 %) / 29,483 / 1,731 (5.9 %: 1,080, 424, 227)
  cover_moving   38,400 / 0 / 14 (0.04 %) / 29,553 / 1,357 (4.6 %:   776, 314, 267)
  suzanne        20,736 / 2 /  5 (0.02 %) / 19,280 /   381 (2.0 %:     0, 367,  14)
  cover0         38,400 / 0 /  0          / 30,119 /    23 (0.08 %)
  handmade       38,400 / 0 /  0          / 27,269 /     8 (0.03 %)
  cover_far      38,400 / 0 / 50 (0.13 %) / 29,455 / 2,704 (9.2 %: 2,311,  98, 295)
  cover_refit    38,400 / 0 / 22 (0.06 %) / 29,373 / 1,501 (5.1 %: 1,003, 277, 221)
So with the scattering primitive excluded properly, 0.8 - 1.0 % of the decided hits of the cover frames and 0.07 % of
suzanne's have a scattered ray undecided through another primitive.  From the scene's own camera at (13, 2, 3) the
cover frames left 4 and 2 primaries out of layer P and 0.5 % not fully decided, but 41 % and 37 % of the decided hits
out of layer S (the small spheres' binary32 hit points): hence the nearer camera (f32_audit.NEAR); translated by
(100, 0, 100) the frame left 13.4 % out, hence (40, 0, 40).
"""
import numpy as np
import pytest

import accel_images as ai
import exact_hits as ex
import f32_audit as fa
import rtow

F = np.float32
MAIN = ["cover_static", "cover_moving", "suzanne"]


# ---- binary32 restatements of the build's tests (rtow_trace_hit.h under RTOW_FAST_MATH, T = float) ------------------
def _fma(x, y, z):
    """x * y + z with one rounding (the product of two binary32 values is exact in binary64)."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(F)


def _dot(x, y, fused):
    if fused:
        return _fma(x[2], y[2], _fma(x[1], y[1], x[0] * y[0]))
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _cross(x, y, fused):
    if fused:
        return [_fma(x[1], y[2], -(y[1] * x[2])), _fma(x[2], y[0], -(y[2] * x[0])), _fma(x[0], y[1], -(y[0] * x[1]))]
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def sphere32(o, d, c, r2, fused):
    """sphere_test<float> over [tmin, inf): does it accept a root?  o, d, c: lists of three float32 arrays."""
    tmin = F(ex.TMIN)
    oc = [o[k] - c[k] for k in range(3)]
    a = _dot(d, d, fused)
    h = _dot(oc, d, fused)
    cc = _dot(oc, oc, fused) - np.abs(r2)
    disc = _fma(h, h, -(a * cc)) if fused else h * h - a * cc
    y = (F(1) / a).astype(F)
    inv_a = y * (F(2) - a * y)
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
        root1, root2 = (-h - sq) * inv_a, (-h + sq) * inv_a
        root = np.where(root1 >= tmin, root1, root2)
        return (disc >= 0) & (root >= tmin)


def triangle32(o, d, A, e1, e2, n, fused):
    """triangle_test<float>, the det-multiplied form, over [tmin, inf)."""
    tmin = F(ex.TMIN)
    det = -_dot(d, n, fused)
    ao = [o[k] - A[k] for k in range(3)]
    dao = _cross(ao, d, fused)
    ud, vd, td = _dot(e2, dao, fused), -_dot(e1, dao, fused), _dot(ao, n, fused)
    return (det >= F(1e-6)) & (td >= tmin * det) & (ud >= 0) & (vd >= 0) & (ud + vd <= det)


def _status(ref, n_prims):
    """[rays, class-major primitive]: MISS (decided), HIT (decided) or UND, from the reference's candidates."""
    sc = ref.scene
    base = {ex.SPHERE: 0, ex.MOVING: len(sc.sph), ex.TRIANGLE: len(sc.sph) + len(sc.mov)}
    st = np.full((len(ref.rays), n_prims), ex.MISS, np.int8)
    for i, cs in enumerate(ref.cands):
        for c in cs:
            st[i, base[c.key[0]] + c.key[1]] = c.status
    return st


@pytest.mark.parametrize("name", MAIN)
def test_the_binary32_band_is_sound(name):
    """The primaries of the frame rounded to binary32, against the binary32 records (the binary64 records rounded,
    accel_images.check_image32): on every (ray, primitive) pair that the reference calls decided — under tau_f32 S_q
    alone, and under the smaller of that and the first-order band — the restated tests take the exact branch, evaluated
    plainly and with every two-term sum fused."""
    au = fa.audit(name)
    sc = au.sc
    g = np.random.default_rng(7)
    pick = np.sort(g.choice(len(au.prim), size=min(6000, len(au.prim)), replace=False))
    o32, d32, t32 = (au.prim[pick][:, s].astype(F) for s in (slice(3, 6), slice(6, 9), 9))
    rays = rtow.make_rays(o32.astype(np.float64), d32.astype(np.float64), time=t32.astype(np.float64))
    G = ai.Geometry.of_scene(au.scene.c)
    srec, mrec, trec = G.sph_records().astype(F), G.mov_records().astype(F), G.tri_records().astype(F)
    ns, nm, nt = len(srec), len(mrec), len(trec)
    zero = np.zeros((len(rays), 3))
    refs = {"tau S_q": ex.Reference(sc, rays, ex.F32),
            "first order": ex.Reference(sc, rays, ex.F32, operr=zero, derr=zero)}
    o = [o32[:, k:k + 1] for k in range(3)]
    d = [d32[:, k:k + 1] for k in range(3)]
    tm = t32[:, None]
    decided = {}
    for fused in (False, True):
        got = np.zeros((len(rays), ns + nm + nt), bool)
        if ns:
            got[:, :ns] = sphere32(o, d, [srec[None, :, k] for k in range(3)], srec[None, :, 3], fused)
        if nm:
            c = [(_fma(tm, mrec[None, :, 3 + k], mrec[None, :, k]) if fused else mrec[None, :, k] + tm * mrec[None, :, 3 + k])
                 for k in range(3)]
            got[:, ns:ns + nm] = sphere32(o, d, c, mrec[None, :, 6], fused)
        for t0 in range(0, nt, 128):
            q = trec[None, t0:t0 + 128]
            got[:, ns + nm + t0:ns + nm + t0 + q.shape[1]] = triangle32(
                o, d, *([q[:, :, 3 * v + k] for k in range(3)] for v in range(4)), fused)
        for label, ref in refs.items():
            st = _status(ref, ns + nm + nt)
            wrong = ((st == ex.HIT) & ~got) | ((st == ex.MISS) & got)
            assert not wrong.any(), (name, label, fused, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
            decided[label] = (int((st == ex.UND).sum()), int((st == ex.HIT).sum()))
    assert decided["first order"][0] <= decided["tau S_q"][0]
    assert decided["tau S_q"][1] > len(rays) // 2  # (the frames' primaries mostly hit something: the test has hits)
    print(f"\n{name}: {len(rays)} rays x {ns + nm + nt} primitives; undecided pairs / decided hits: {decided}")


@pytest.mark.parametrize("name", MAIN + ["cover_far"])
def test_the_frames_keep_enough_samples(name):
    """The caps of the audit's conditions (f32_audit.check_conditions), from the reference alone.  The frames that only
    the GPU tests use (cover0, handmade, cover_refit) are held to the same caps there, where their audits exist."""
    s = fa.check_conditions(fa.audit(name))
    print(f"\n{name}: {s}")


# ---- planted faults ---------------------------------------------------------------------------------------------------
def _planted(au, arrays):
    return fa.oracle_frames(fa.scene_from(arrays, fa.camera_of(au.scene)), au.cfg)


def _most_kept(au, cls, lit=True, but=()):
    """The class index of the primitive of class `cls` with the most samples kept by layer S (whose scattered ray
    misses, if `lit`)."""
    sel = (au.cls[au.idxS] == cls) & (~au.hitS if lit else True)
    ids, cnt = np.unique(au.ci[au.idxS][sel], return_counts=True)
    order = [int(i) for i in ids[np.argsort(-cnt)] if (cls, int(i)) not in but]
    return order[0]


@pytest.mark.parametrize("name", MAIN)
def test_the_oracles_own_frames_pass(name):
    au = fa.audit(name)
    p, s = au.check(*au.oracle(), name)
    assert p["worst_err_over_tol"] == 0.0 and s["worst_err_over_tol"] == 0.0
    print(f"\n{name}: layer P {p}, layer S {s}, smallest |q| / band among the kept: {au.worst_margins()}")


def test_a_removed_triangle_is_caught():
    au = fa.audit("suzanne")
    k = _most_kept(au, ex.TRIANGLE, lit=False)
    with pytest.raises(fa.AuditError):
        au.check(*_planted(au, fa.without_triangle(fa.arrays_of(au.scene), k)))


def test_a_shrunk_sphere_is_caught():
    au = fa.audit("cover_static")
    ground = {(c, i) for c, i in au.large}
    k = _most_kept(au, ex.SPHERE, but=ground)
    with pytest.raises(fa.AuditError):
        au.check(*_planted(au, fa.with_radius(fa.arrays_of(au.scene), ex.SPHERE, k, -1e-3)))


def test_a_frozen_moving_sphere_is_caught():
    au = fa.audit("cover_moving")
    k = _most_kept(au, ex.MOVING)
    with pytest.raises(fa.AuditError):
        au.check(*_planted(au, fa.frozen(fa.arrays_of(au.scene), k)))


def test_swapped_materials_are_caught():
    au = fa.audit("cover_moving")
    a = fa.arrays_of(au.scene)
    p = (ex.MOVING, _most_kept(au, ex.MOVING))
    ground = {(c, i) for c, i in au.large}
    q = (ex.SPHERE, _most_kept(au, ex.SPHERE, but=ground))
    assert a["moving_mat"][p[1]] != a["sphere_mat"][q[1]]
    with pytest.raises(fa.AuditError):
        au.check_S(_planted(au, fa.with_materials_swapped(a, p, q))[1])


def test_acne_on_one_row_of_the_ground_is_caught():
    au = fa.audit("cover_static")
    c0, c1 = (c.copy() for c in au.oracle())
    (gc, gi), = au.large
    ground = (au.cls[au.idxS] == gc) & (au.ci[au.idxS] == gi) & ~au.hitS
    rows, cnt = np.unique(au.prow[au.idxS][ground], return_counts=True)
    row = int(rows[np.argmax(cnt)])
    sel = au.idxS[ground & (au.prow[au.idxS] == row)]
    c1[au.pj[sel], au.prow[sel], au.pcol[sel]] = 0.0
    au.check_P(c0)
    with pytest.raises(fa.AuditError, match=f"row {row}"):
        au.check_S(c1)


def test_rotated_albedo_channels_are_caught():
    au = fa.audit("cover_moving")
    with pytest.raises(fa.AuditError):
        au.check_S(_planted(au, fa.with_albedo_rotated(fa.arrays_of(au.scene)))[1])
