"""The cases of the exact scatter checks (test_scatter_exact_host.py, test_gpu_exact_scatter.py): the "material edge"
scene, the ray families aimed at the branches of Material::scatter, and the logged rows of the three deep renders of
test_gpu_path_step.py.  Importing this module loads no library.

The scene: one primitive per place, far enough apart that a ray aimed at one meets it first.  Static spheres in every
material, lone negative-radius spheres (Lambertian, metal, glass of ir 1.5, 1 / 1.5 and 2.4), a glass shell (r = 1 around
r = -0.8), moving spheres, and triangles whose |e1 x e2| runs from 1e-3 to 1e3 in all three materials; glass of ir 1.5,
1 / 1.5, 1.0 and 2.4, fuzz 0, 0.3 and 1.0 and a fuzzed glass; and the CUT triangles, whose e1 x e2 is the ball point of
one chosen Philox identity plus a chosen offset per component.  `tri_only` keeps the triangles alone (the BVH4 kernel).

What the geometry does not allow is left out, and said here: a triangle is hit from its front only (det >= 1e-6), so
there are no back-face triangle rays, and a glass triangle's total internal reflection comes from ir < 1; a ray from
inside a sphere of radius r starts at the middle of its chord and leaves at t = |r| c for cos_theta = c, which must reach
tmin = 0.001: with |r| from 0.7 to 1 the back-face sweep of the spheres stops at c = 2e-3 (t >= 1.4 tmin).  For a triangle cos_theta is the kernel's dot(-unit, n) = |n| cos(angle):
the grazing end of its sweep is reached with |d| up to 1e3, which keeps det = |d| cos_theta above the cut.  A sphere hit
at cos_theta <= 1e-5 is a tangent ray whose HIT exact_hits cannot decide in every build (the fast build's world-coordinate
forms first), and a glass of ir = 1 has ratio sin_theta = 1 at grazing incidence: those rays are the ones "on a cut by
construction" (`on_cut`), with the Lambertian triangle whose normal lies on the 1e-8 cut.
"""
import math

import numpy as np

import accel_images as ai
import exact_hits as ex
import rtow
import scatter_exact as sx

SEED, BOUNCE = 77, 2
CUT_ID = (1234, 2)  # the (pixel, sample) whose ball point the CUT triangles carry
L, M, G = rtow.MAT_LAMBERTIAN, rtow.MAT_METAL, rtow.MAT_DIELECTRIC
MATS = [(L, (0.5, 0.5, 0.5), 0.0, 1.5), (L, (0.8, 0.3, 0.2), 0.0, 1.5), (M, (0.7, 0.6, 0.5), 0.0, 1.5),
        (M, (0.9, 0.8, 0.3), 0.3, 1.5), (M, (0.4, 0.9, 0.6), 1.0, 1.5), (G, (1.0, 1.0, 1.0), 0.0, 1.5),
        (G, (1.0, 1.0, 1.0), 0.0, 1 / 1.5), (G, (1.0, 1.0, 1.0), 0.0, 1.0), (G, (1.0, 1.0, 1.0), 0.0, 2.4),
        (G, (0.9, 0.9, 0.9), 0.3, 1.5)]
GLASS = (5, 6, 7, 8, 9)
COS_SWEEP = (1.0, 0.9, 0.5, 0.1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)
COS_BACK = (1.0, 0.9, 0.5, 0.1, 0.02, 5e-3, 2e-3)
CRIT_OFFSETS = tuple(s * v for v in (1e-3, 1e-6, 1e-9, 1e-12, 1e-15) for s in (1.0, -1.0))
# offsets per component from the ball point (in units of the 1e-8 cut): absorbed, absorbed, on the cut, and outside it
CUT_OFFSETS = ((0, 0, 0), (0.5, 0.5, 0.5), (-0.5, 0.5, 0), (1.0, 0, 0), (2, 0, 0), (0, -2, 0), (0.5, 0.5, 2), (2, 2, 2))
CUT_ON = 3  # (the index in CUT_OFFSETS of the triangle on the cut)
_ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # orthonormal rows


def cut_ball_point():
    w = sx.philox_words(SEED, CUT_ID[0], CUT_ID[1], 1 + BOUNCE)
    return np.array([float(x) for x in sx.ball_point(w, sx.STRICT)[0]])


def _triangle_with_normal(nrm, at):
    """A triangle A, A + e1, A + e2 with e1 x e2 = nrm up to rounding, its centroid near `at`."""
    e1 = np.cross(nrm, [0.0, 0.0, 1.0] if abs(nrm[2]) < 0.9 * np.linalg.norm(nrm) else [1.0, 0.0, 0.0])
    e2 = np.cross(nrm, e1) / np.dot(e1, e1)
    a = np.asarray(at, float) - (e1 + e2) / 3
    return np.concatenate([a, a + e1, a + e2])


class EdgeScene:
    """The geometry (G: accel_images.Geometry, class-major = insertion order), its exact_hits.Scene, the materials as
    [n, 6] rows (albedo, fuzz, ir, kind), the |e1 x e2| each sized triangle was made with (tri_size) and the index of the
    first CUT triangle (cut_first)."""

    def __init__(self, tri_only=False):
        sph, smat, mov, mmat, tri, tmat = [], [], [], [], [], []
        # the spheres sit on a 3.5-spaced lattice around the origin: the fast build tests spheres in world coordinates,
        # and exact_hits' bound on its t grows with (|o| + |c|)^2
        slots = iter([np.array([x, y, z]) for x in (0.0, 3.5, -3.5) for y in (0.0, 3.5, -3.5) for z in (0.0, 3.5, -3.5)])
        if not tri_only:
            for i in range(len(MATS)):  # static spheres, every material
                sph.append(list(next(slots)) + [1.0]), smat.append(i)
            for m in (0, 3, 5, 6, 8):  # lone negative-radius spheres
                sph.append(list(next(slots) + [0.0, 0.125, 0.0]) + [-1.0]), smat.append(m)
            c = next(slots)
            sph.append(list(c) + [1.0]), smat.append(5)
            sph.append(list(c) + [-0.8]), smat.append(5)
            for m in (0, 3, 5, 6, 9):
                c0 = next(slots) + [-0.125, -0.25, 0.125]
                mov.append(list(c0) + list(c0 + [0.25, 0.5, -0.25]) + [0.7, 0.0]), mmat.append(m)
        self.tri_size = []
        k = 0
        for m in range(len(MATS)):
            sizes = (1e-3, 0.03, 1.0, 3.0, 1e3) if m in GLASS else (1e-3, 1.0, 1e3)
            for a in sizes:
                ln = math.sqrt(a)
                at = np.array([100.0 * (k % 8), 3.0 * (k % 3), 200.0 + 100.0 * (k // 8)])
                A = at - ln * (_ROT[0] + _ROT[1]) / 3
                tri.append(np.concatenate([A, A + ln * _ROT[0], A + ln * _ROT[1]])), tmat.append(m)
                self.tri_size.append(a)
                k += 1
        self.cut_first = len(tri)
        rnd = cut_ball_point()
        for j, off in enumerate(CUT_OFFSETS):
            tri.append(_triangle_with_normal(rnd + 1e-8 * np.array(off, float), [20.0 * j, 0.0, -200.0])), tmat.append(0)
        self.G = ai.Geometry(np.array(sph).reshape(-1, 4), np.array(mov).reshape(-1, 8), np.array(tri).reshape(-1, 9),
                             np.array(smat + mmat + tmat, np.int32), MATS, (0.0, 0.0, 0.0))
        self.scene = ex.Scene.class_major(self.G.sph, self.G.mov, self.G.tri, self.G.pmat)
        self.mats = np.array([list(a) + [f, ir, kd] for kd, a, f, ir in MATS], np.float64)

    def mat_of(self, cls, ci):
        g = self.G
        return int(g.pmat[{0: 0, 1: g.ns, 2: g.ns + g.nm}[cls] + ci])

    def upload(self, keep):
        from support_scenes import scene_of
        return scene_of(self.G, keep)


# ---- aiming -----------------------------------------------------------------------------------------------------------
def _frame(g):
    w = g.normal(size=3)
    w /= np.linalg.norm(w)
    t = np.cross(w, g.normal(size=3))
    return w, t / np.linalg.norm(t)


class Rays:
    def __init__(self):
        self.o, self.d, self.tm, self.fam, self.note = [], [], [], [], []

    def add(self, o, d, tm, fam, note=""):
        self.o.append(o), self.d.append(d), self.tm.append(tm), self.fam.append(fam), self.note.append(note)


def _sphere_ray(out, g, c, r, tm, cos, fam, back=False, mag=1.0, note=""):
    w, t = _frame(g)
    sin = math.sqrt(max(0.0, 1.0 - cos * cos))
    p = c + abs(r) * w
    if back:  # from inside, outward
        dh = cos * w + sin * t
        o = p - abs(r) * cos * dh
    else:
        dh = -cos * w + sin * t
        o = p - 1.5 * dh  # (short of the lattice's neighbours)
    out.add(o, mag * dh, tm, fam, note)


def _triangle_ray(out, tri, cosk, fam, mag=None, note=""):
    """cosk: the kernel's cos_theta = dot(-unit, e1 x e2)."""
    A, e1, e2 = tri[0:3], tri[3:6] - tri[0:3], tri[6:9] - tri[0:3]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n)
    cosg = cosk / ln
    assert cosg <= 1.0 + 1e-12, (cosk, ln)
    cosg = min(cosg, 1.0)
    sing = math.sqrt(1.0 - cosg * cosg)
    dh = -cosg * n / ln + sing * e1 / np.linalg.norm(e1)
    p = A + (e1 + e2) / 3
    if mag is None:
        mag = max(1.0, 1e-5 / cosk)  # det = |d| cos_theta stays above the 1e-6 cut
    out.add(p - 2.0 * dh, mag * dh, 0.5, fam, note)


def _centre(es, cls, ci, tm):
    if cls == 0:
        return es.G.sph[ci, :3], es.G.sph[ci, 3]
    m = es.G.mov[ci]
    return m[:3] + tm * (m[3:6] - m[:3]), m[6]


def families(es, tri_only=False):
    """(rays RAY_DTYPE, ids [n, 2] uint32, family [n] of 'a'..'f', on_cut: the indices placed on a cut by construction,
    notes [n]: a (b) ray's offset).  The (c) identities are searched among 2^20 pixels with `coins`, the oracle's coin on
    numpy integers (test_scatter_exact_host.py holds it to orc_philox_request)."""
    g = np.random.default_rng(31)
    out = Rays()
    G_ = es.G
    spheres = [] if tri_only else [(0, i) for i in range(G_.ns)] + [(1, i) for i in range(G_.nm)]
    ntri = es.cut_first
    # (a) incidence sweep
    for cls, ci in spheres:
        for tm in ((0.5,) if cls == 0 else (0.0, 0.7)):
            c, r = _centre(es, cls, ci, tm)
            for cos in COS_SWEEP:
                _sphere_ray(out, g, c, r, tm, cos, "a", note="tangent" if cos <= 1e-5 else "")
            for cos in COS_BACK:
                _sphere_ray(out, g, c, r, tm, cos, "a", back=True)
    for i in range(ntri):
        ln = float(np.linalg.norm(es.scene.tri_n[i]))
        for cos in COS_SWEEP:
            if cos == 1e-6:
                cos = 3e-6  # (the fast GRID walk cuts at det / |d| = cos_theta >= 1e-6; below it the ray misses there)
            # (noted: ir = 1, where ratio sin_theta reaches 1 at grazing incidence)
            _triangle_ray(out, G_.tri[i], cos * ln if cos >= 0.1 else min(cos, 0.05 * ln), "a",
                          note="grazing" if cos <= 1e-7 and MATS[es.mat_of(2, i)][3] == 1.0 else "")
    for mag in (1e-3, 1.0, 7.0, 1e3):  # and rays that leave the scene: the sky, for every direction magnitude
        out.add(np.array([1.0, 900.0, 2.0]), mag * np.array([0.3, 1.0, -0.2]), 0.5, "a")
    # (b) critical angle: ratio sin_theta = 1 + offset where ratio > 1
    crit = []
    for cls, ci in spheres:
        m = es.mat_of(cls, ci)
        if MATS[m][0] != G:
            continue
        r = _centre(es, cls, ci, 0.0)[1]
        ratio = 1 / MATS[m][3] if r < 0 else MATS[m][3]  # inside: front = 0 xor inward
        if ratio > 1:
            crit.append((cls, ci, ratio))
    for cls, ci, ratio in crit:
        for tm in ((0.5,) if cls == 0 else (0.3,)):
            c, r = _centre(es, cls, ci, tm)
            for off in CRIT_OFFSETS:
                for _ in range(3):
                    sin = (1.0 + off) / ratio
                    _sphere_ray(out, g, c, r, tm, math.sqrt(1.0 - sin * sin), "b", back=True, note=f"{off:g}")
    for i in range(ntri):
        m = es.mat_of(2, i)
        if MATS[m][0] == G and MATS[m][3] < 1 and es.tri_size[i] >= 1.0:  # (cos_theta <= |n|)
            for off in CRIT_OFFSETS:
                sin = (1.0 + off) * MATS[m][3]
                _triangle_ray(out, G_.tri[i], math.sqrt(1.0 - sin * sin), "b", note=f"{off:g}")
    n_b_end = len(out.o)
    # (c) Schlick coin: fixed rays, the identities are chosen below
    coin_targets = []
    if not tri_only:
        c, r = _centre(es, 0, 5, 0.5)
        for cos in (0.5, 0.2):
            coin_targets.append(len(out.o))
            _sphere_ray(out, g, c, r, 0.5, cos, "c")
    for i in range(ntri):
        if es.mat_of(2, i) in (5, 8) and es.tri_size[i] == 1.0:
            coin_targets.append(len(out.o))
            _triangle_ray(out, G_.tri[i], 0.4, "c")
    # (d) direction magnitudes on metal and glass
    for mag in (1e-3, 1e-1, 10.0, 1e3):
        for cls, ci in spheres:
            if MATS[es.mat_of(cls, ci)][0] == L:
                continue
            c, r = _centre(es, cls, ci, 0.25)
            for cos in (0.95, 0.3):
                _sphere_ray(out, g, c, r, 0.25, cos, "d", mag=mag)
        for i in range(ntri):
            ln = float(np.linalg.norm(es.scene.tri_n[i]))
            if MATS[es.mat_of(2, i)][0] != L and mag * 0.6 * ln >= 1e-5:  # (det = |d| cos_theta above the 1e-6 cut)
                _triangle_ray(out, G_.tri[i], 0.6 * ln, "d", mag=mag)
    # (e) steep triangle normals: |cos_theta| across 1 and far beyond
    for i in range(ntri):
        ln = float(np.linalg.norm(es.scene.tri_n[i]))
        if MATS[es.mat_of(2, i)][0] == G and ln > 1.5:
            for ck in (0.5, 0.9, 0.999, 1 - 1e-9, 1 + 1e-9, 1.001, 1.5, 0.5 * ln, ln):
                if ck <= ln:
                    _triangle_ray(out, G_.tri[i], ck, "e")
    # (f) the Lambertian cut
    f_first = len(out.o)
    for j in range(len(CUT_OFFSETS)):
        _triangle_ray(out, G_.tri[es.cut_first + j], 0.7 * float(np.linalg.norm(es.scene.tri_n[es.cut_first + j])), "f")
        _triangle_ray(out, G_.tri[es.cut_first + j], 0.2 * float(np.linalg.norm(es.scene.tri_n[es.cut_first + j])), "f")
    n0 = len(out.o)
    fam = list(out.fam)
    o, d, tm = [np.array(x) for x in (out.o, out.d, out.tm)]
    ids = np.stack([np.arange(n0) + 100000, np.arange(n0) % 7], axis=1).astype(np.uint32)
    ids[f_first:n0] = CUT_ID
    # (c): for every fixed ray the identities whose coin lies nearest its R on either side
    extra_o, extra_d, extra_tm, extra_ids = [], [], [], []
    for k in coin_targets:
        R = _reflectance_of(es, o[k], d[k], tm[k])
        pix = np.arange(1 << 20, dtype=np.uint64)
        coin = coins(SEED, pix, 3, 1 + BOUNCE)
        order = np.argsort(np.abs(coin - R))
        above = order[np.nonzero(coin[order] > R)[0][:60]]
        below = order[np.nonzero(coin[order] < R)[0][:60]]
        for p in (int(x) for x in np.concatenate([above, below])):
            extra_o.append(o[k]), extra_d.append(d[k]), extra_tm.append(tm[k]), extra_ids.append((p, 3))
            fam.append("c")
    o, d, tm = np.concatenate([o, extra_o]), np.concatenate([d, extra_d]), np.concatenate([tm, extra_tm])
    ids = np.concatenate([ids, np.array(extra_ids, np.uint32).reshape(-1, 2)])
    rays = rtow.make_rays(o, d, time=tm)
    fam = np.array(fam)
    notes = out.note + [""] * (len(fam) - n0)  # (the c-family copies carry no note)
    on_cut = [i for i in range(n0) if notes[i] in ("tangent", "grazing")] + [f_first + 2 * CUT_ON, f_first + 2 * CUT_ON + 1]
    return rays, ids, fam, np.array(on_cut, np.int64), np.array(notes)


def _reflectance_of(es, o, d, tm):
    """Schlick's R of the ray's first hit in binary64 (what the search aims at; the reference decides afterwards)."""
    rays = rtow.make_rays([o], [d], time=tm)
    h = ex.Reference(es.scene, rays, ex.STRICT)
    r = sx.Reference(h, es.mats, SEED, np.array([[0, 0]]), BOUNCE)
    gp, pe, pb, nrm, dn, front = r.surface(0)
    u = np.asarray(d) / np.linalg.norm(d)
    cos = -float(np.dot(u, [float(x) for x in nrm]))
    ir = es.mats[es.scene.prim_mat[gp], 4]
    ratio = 1 / ir if front else ir
    r0 = ((1 - ratio) / (1 + ratio)) ** 2
    return r0 + (1 - r0) * (1 - cos) ** 5


def coins(seed, pixel, sample, request):
    """The dielectric coin of request `request` of (seed, pixel [n], sample): Philox4x32-7 on numpy integers."""
    m32 = np.uint64(0xffffffff)
    pixel = np.asarray(pixel, np.uint64)
    c0 = np.full(len(pixel), request, np.uint64)
    c1 = np.full(len(pixel), sample, np.uint64)
    c2, c3 = pixel.copy(), np.zeros(len(pixel), np.uint64)
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    w = (((c3 >> np.uint64(16)) << np.uint64(16)) | ((c0 & np.uint64(0xff)) << np.uint64(8)) | (c1 & np.uint64(0xff)))
    return w.astype(np.float64) * 2.0 ** -32


# ---- logged rows ------------------------------------------------------------------------------------------------------
DEEP = {
    # name: (scene, width, height, spp, max_child_rays, seed) — the three deep renders of test_gpu_path_step.py
    "cover_d50": ("cover", 48, 32, 4, 50, 21),
    "cover_moving_d50": ("cover_moving", 48, 32, 4, 50, 22),
    "suzanne_d20": ("suzanne", 48, 27, 4, 20, 23),
}


def logged_rows(name, n=5000):
    """(host scene, view, exact_hits.Scene, mats, rows): at most n rows of every segment of the render, every segment
    depth up to the deepest and every material of the scene among them (asserted).  A row is support_oracle's (pixel, sample, segment, o, d, time, t, class index)."""
    import orc
    import support_scenes
    from exact_cases import subsample
    from support_oracle import logged_render

    mk, w, h, spp, depth, seed = DEEP[name]
    hs = getattr(support_scenes, mk)()
    cfg = rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=rtow.F64_STRICT)
    log = logged_render(hs, cfg)[1]
    seg = log[:, 2].astype(np.int64)
    first = np.array([np.nonzero(seg == b)[0][0] for b in range(int(seg.max()) + 1)])
    rest = np.setdiff1d(np.arange(len(log)), first)
    rows = np.concatenate([log[first], subsample(log[rest], n - len(first), 12)])
    assert set(rows[:, 2].astype(int)) == set(range(int(seg.max()) + 1)) and len(rows) <= n
    view = support_scenes.SceneView(hs)
    mats = orc.scene_arrays(hs.c)["materials"]
    # every material of the scene is among the rows: a row's primitive is the one of its class index (one per class at
    # most) whose oracle hit test gives the row's t
    kinds = set()
    for row in rows[np.isfinite(rows[:, 10])]:
        for p in np.nonzero(view.index == int(row[11]))[0]:
            got = view.oracle_hit(int(p), row[3:6], row[6:9], row[9])
            if got is not None and got[0] == row[10]:
                kinds.add(int(mats[view.prim_mat[p], 5]))
                break
        else:
            raise AssertionError(("no primitive gives the row's t", row))
    assert kinds == set(int(k) for k in mats[np.unique(view.prim_mat), 5]), kinds
    return hs, view, ex.Scene.of(view), mats, rows, seed


# ---- a case: rays with their identities, the references per build, and the shares that must hold ------------------------
class Case:
    """Rays against one scene: `scene` (exact_hits.Scene), `mats`, rays, ids, bounce (one, or per ray), seed; for the
    families also family [n], on_cut and notes.  ref(build, unit_cut): (exact_hits.Reference, scatter_exact.Reference),
    built once per pair."""

    def __init__(self, name, scene, mats, rays, ids, bounce, seed, family=None, on_cut=(), notes=None):
        self.name, self.scene, self.mats, self.rays, self.ids = name, scene, mats, rays, np.ascontiguousarray(ids, np.uint32)
        self.bounce, self.seed = np.broadcast_to(np.asarray(bounce, np.int64), (len(rays),)), seed
        self.family, self.on_cut, self.notes = family, np.asarray(on_cut, np.int64), notes
        self._refs = {}
        self.reftree_blind, self._outward = frozenset(), None  # (see without_reftree_blind_hits)

    def ref(self, build, unit_cut=False):
        key = (build, bool(unit_cut) and len(self.scene.tri) > 0)
        if key not in self._refs:
            h = ex.Reference(self.scene, self.rays, build, unit_cut=key[1])
            self._refs[key] = (h, sx.Reference(h, self.mats, self.seed, self.ids, self.bounce))
        return self._refs[key]

    def without_reftree_blind_hits(self):
        """The case without the rays whose exact hit is one of `reftree_blind`, for the REFTREE strategy: that walk is the
        reference's tree over the reference's boxes, and the reference's box of a sphere, centre -+ (r, r, r), is inside
        out for r < 0 — such a sphere is found only where the box of its node's other child covers it.  The hollow glass
        of the reference's scenes is found (the logged cases name nothing and are checked whole).  The edge scene names
        its negative-radius spheres: the lone ones, and the shell's inner sphere, which the reference's median split does
        not put beside its shell (REFTREE reports the shell behind it).  The same case when it names none."""
        if self._outward is None:
            h = self.ref(ex.STRICT)[0]
            k = np.array([not any(p in self.reftree_blind for p in t) for t in h.ties], bool)
            if k.all():
                self._outward = self
            else:
                self._outward = Case(self.name + "/outward", self.scene, self.mats, self.rays[k], self.ids[k],
                                     self.bounce[k], self.seed, None if self.family is None else self.family[k],
                                     np.nonzero(np.isin(np.nonzero(k)[0], self.on_cut))[0],
                                     None if self.notes is None else self.notes[k])
        return self._outward

    def groups(self):
        """name -> indices: the families, or the whole case."""
        if self.family is None:
            return {"rows": np.arange(len(self.rays))}
        return {f: np.nonzero(self.family == f)[0] for f in "abcdef" if np.any(self.family == f)}


def edge_case(tri_only=False):
    es = EdgeScene(tri_only)
    rays, ids, fam, on_cut, notes = families(es, tri_only)
    c = Case("edge_tri" if tri_only else "edge", es.scene, es.mats, rays, ids, BOUNCE, SEED, fam, on_cut, notes)
    c.es = es
    c.reftree_blind = frozenset(i for i in range(es.G.ns) if es.G.sph[i, 3] < 0)  # (class-major: spheres first)
    return c


def logged_case(name, n=5000):
    hs, view, scene, mats, rows, seed = logged_rows(name, n)
    from support_oracle import rays_of
    c = Case(name, scene, mats, rays_of(rows), rows[:, 0:2].astype(np.uint32), rows[:, 2].astype(np.int64), seed)
    c.hs, c.view, c.rows = hs, view, rows
    return c


def oracle_step(case, view, L=None, mutate=None):
    """What the oracle answers for the case's rays: its own hit test on the primitive the exact reference names (the
    strict one's: a decided hit is the same primitive in every build), then orc_scatter — from library L (default
    liboracle.so; the hit test is always liboracle.so's) — and the sky for a miss.  Rays whose hit is undecided get
    the primitive nearest in exact t.  mutate(inputs dict) may change what orc_scatter is given.
    Returns (status, next, atten, hits)."""
    import orc
    from support_oracle import sky_of_strict

    h = case.ref(ex.STRICT)[0]
    n = len(case.rays)
    hits = np.zeros(n, dtype=rtow.HIT_DTYPE)
    hits["t"], hits["prim"], hits["kind"], hits["material"] = math.inf, -1, -1, -1
    for i, r in enumerate(case.rays):
        if h.ties[i]:
            p = h.ties[i][0]
            got = view.oracle_hit(p, r["origin"], r["direction"], r["time"])
            if got is not None:
                t, pt, nr, front = got
                hits[i] = (t, pt, nr, p, case.scene.kind[p], case.scene.prim_mat[p], front)
    status = np.zeros(n, np.int32)
    nxt = np.zeros(n, rtow.RAY_DTYPE)
    nxt["tmax"] = -1.0
    atten = np.zeros((n, 3))
    hit = hits["prim"] >= 0
    atten[~hit] = sky_of_strict(case.rays["direction"][~hit])
    for b in np.unique(case.bounce[hit]):
        s = np.nonzero(hit & (case.bounce == b))[0]
        inp = dict(point=hits["point"][s].copy(), normal=hits["normal"][s].copy(), front=hits["front_face"][s].copy(),
                   rd=case.rays["direction"][s].copy(), time=case.rays["time"][s].copy(),
                   mats=case.mats[hits["material"][s]].copy(), ids=case.ids[s].copy(), request=1 + int(b), index=s)
        if mutate is not None:
            mutate(inp)
        status[s], nxt[s], atten[s] = orc.scatter(inp["point"], inp["normal"], inp["front"], inp["rd"], inp["time"],
                                                  inp["mats"], case.seed, inp["ids"], inp["request"], L)
    return status, nxt, atten, hits


def assert_shares(case, ref, what=""):
    """The undecided shares the cases must meet (ref: the scatter_exact.Reference that was checked): logged rows and
    families (a), (d), (e), (f) at most exact_cases.SHARE but for the rays on a cut by construction; (b) every offset of
    1e-9 or more decided and both branches present; (c) both outcomes present and decided."""
    from exact_cases import SHARE
    und = ~ref.decided
    if case.family is None:
        assert und.sum() <= SHARE * len(und), (what, int(und.sum()), len(und))
        return
    listed = np.zeros(len(und), bool)
    listed[case.on_cut] = True
    tag = np.array([o[0].tag if o else "" for o in ref.outs])
    for f in "adef":
        s = case.family == f
        if s.any():
            assert (und & s & ~listed).sum() <= SHARE * s.sum(), (what, f, np.nonzero(und & s & ~listed)[0][:10])
    b = case.family == "b"
    if b.any():
        big = np.zeros(len(und), bool)
        for i in np.nonzero(b)[0]:  # (a (b) ray's note is its offset)
            big[i] = abs(float(case.notes[i])) >= 1e-9
        assert big.sum() >= 0.5 * b.sum() and not (und & big).any(), (what, "b", np.nonzero(und & big)[0][:10])
        assert {"reflect", "refract"} <= set(tag[big]), (what, "b", set(tag[big]))
    c = case.family == "c"
    if c.any():
        assert not (und & c).any(), (what, "c", np.nonzero(und & c)[0][:10])
        assert {"reflect", "refract"} <= set(tag[c]), (what, "c", set(tag[c]))
