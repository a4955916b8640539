"""`big_mixed`: one scene whose BVH image and grid image both exceed the 160 KiB the query kernels can stage in LDS, and
which carries every primitive class, every material kind and every hard primitive of the hand scene — so that each
query kind runs its global-memory instantiations (Image<false>) on spheres, moving spheres and triangles at once.

Core: the primitives of sweep_cases.hand_geometry(), coordinates unchanged, first in insertion order in the hand scene's
own (permuted) order: insertion indices 0 .. N_CORE - 1 and the class indices of the core are those of the hand scene, so
handmade_rays, handmade_points, placed_sweeps, aimed_sweeps, resting_sweeps and the pinned rests aim at what they always did.
Filler, beside the core (x from about 5.5 to 11) and inside the core's R = 40 sphere: a prefix of suzanne_tris(2) scaled
by 1.7 and moved by (8.3137, 1.9071, 0.7043), small static spheres of two radii and moving spheres scattered about the mesh's own
triangles (leaves and cells mix classes), all three material kinds on spheres, Lambertian and metal on triangles,
inserted after the core in a fixed random order.  No coordinate of the filler is a round binary number.

Two materials of the core differ from the hand scene's.  The R = 40 sphere is glass, not metal: paths leave through it and
the oracle image is not black.  The two EQUAL spheres share one material (the hand scene gives them a Lambertian and a
glass one).  A path that meets them meets both at exactly the same t, and no trace or closest-hit kernel has a rule for
an exact tie ("results do not depend on the tree, exact ties aside", csrc/rtow_bvh4.h): the oracle's tree reports the
one its traversal reaches first.  With the hand scene's two materials, measured on one MI355X with both builders, strict
REFTREE — the oracle's own tree — equals the oracle image and its 7,262 segments bit for bit, while strict BRUTE, BVH,
GRID and AUTO agree with one another (7,273 segments) and differ from the oracle in nine pixels, exactly those whose
oracle paths touch the equal spheres: they report the other sphere.  That is the reference's hittable list (a later
primitive with an equal t replaces the earlier), not a fault, but it makes the frame useless as a bit-for-bit reference
for those walks.  geometry(two_twin_materials=True) is that variant; test_gpu_big_mixed.py renders it and asserts what
is said here, so the render still shows which of two tied primitives each walk chose.

Importing this module loads no library; everything that needs librtow.so or liboracle.so is a function.
"""
import functools

import numpy as np

import accel_images as ai
import sweep_cases

LDS_LIMIT = 160 * 1024  # kLdsLimit of csrc/rtow_ctx.h
N_TRI, N_SPH, N_MOV = 1300, 300, 100  # the filler: the fewest triangles, in steps of 100, that put the grid image over the limit
SCALE, OFFSET = 1.7, np.array([8.3137, 1.9071, 0.7043])
RADII = (0.0437, 0.0811)
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2  # RTOW_MAT_* of include/rtow.h
MATS = (
    (LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 1.5), (DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 1.5), (METAL, (0.7, 0.6, 0.5), 0.1, 1.5),
    # ... the hand scene's three, at its indices; the filler's:
    (LAMBERTIAN, (0.8, 0.3, 0.2), 0.0, 1.5), (METAL, (0.7, 0.8, 0.9), 0.0, 1.5), (LAMBERTIAN, (0.2, 0.6, 0.3), 0.0, 1.5),
    (DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 1.33), (METAL, (0.9, 0.5, 0.3), 0.35, 1.5),
)
TRI_MATS = (0, 2, 3, 4, 5, 7)  # Lambertian and metal
FRAME = (48, 32, 2, 20, 31)  # width, height, spp, max_child_rays, seed of the oracle render the logged rows come from
LOOK = ((7.2, 2.4, 7.5), (7.4, 1.8, 0.5), (0.0, 1.0, 0.0))  # from, at, up: the filler and the core's side next to it


class Geometry(ai.Geometry):
    """accel_images.Geometry (class-major) plus `perm`: the class-major slot of each insertion index."""

    def __init__(self, sph, mov, tri, pmat, mats, cam, perm):
        super().__init__(sph, mov, tri, pmat, mats, cam)
        self.perm = np.asarray(perm, dtype=np.int64)
        self.n_core = N_CORE


def _core(two_twin_materials=False):
    sph, mov, tri, kind, index, cmat = sweep_cases.hand_geometry()
    cmat = [m.copy() for m in cmat]
    assert sph[ENCLOSING, 3] == 40.0
    cmat[0][ENCLOSING] = 1  # glass, not the hand scene's metal: paths leave through it, so the oracle image is not black
    assert np.array_equal(sph[TWINS[0]], sph[TWINS[1]])
    if not two_twin_materials:
        cmat[0][TWINS[1]] = cmat[0][TWINS[0]]  # the equal spheres: one material (see the module docstring)
    return sph, mov, tri, kind, index, cmat


N_CORE = 40  # primitives of the hand geometry (asserted in geometry())
N_CORE_SPH, N_CORE_MOV, N_CORE_TRI = 8, 2, 30  # ... per class: the core leads each class
ENCLOSING = 5  # the sphere class index of the R = 40 sphere around everything
TWINS = (3, 4)  # the sphere class indices of the two equal spheres


def geometry(n_tri=N_TRI, n_sph=N_SPH, n_mov=N_MOV, two_twin_materials=False):
    """The scene as a Geometry: classes hold the core first, then the filler; `perm` puts the core first in the hand
    scene's order and the filler behind it in a fixed random order."""
    from support_scenes import suzanne_tris

    csph, cmov, ctri, kind, index, cmat = _core(two_twin_materials)
    assert len(kind) == N_CORE and (len(csph), len(cmov), len(ctri)) == (N_CORE_SPH, N_CORE_MOV, N_CORE_TRI)
    g = np.random.default_rng(97)
    mesh = suzanne_tris(2)[:n_tri].reshape(-1, 3, 3) * SCALE + OFFSET
    assert len(mesh) == n_tri
    ctr = mesh.mean(axis=1)

    def about(n):  # points scattered about the mesh's own triangles
        return ctr[g.integers(len(ctr), size=n)] + g.normal(scale=0.12, size=(n, 3))

    fsph = np.c_[about(n_sph), np.asarray(RADII)[np.arange(n_sph) % 2]]
    c0 = about(n_mov)
    fmov = np.c_[c0, c0 + g.uniform(-0.11, 0.11, size=(n_mov, 3)), g.uniform(0.031, 0.067, size=n_mov), np.zeros(n_mov)]
    sph, mov, tri = np.concatenate([csph, fsph]), np.concatenate([cmov, fmov]), np.concatenate([ctri, mesh.reshape(-1, 9)])
    pmat = np.concatenate([cmat[0], g.integers(len(MATS), size=n_sph), cmat[1], g.integers(len(MATS), size=n_mov),
                           cmat[2], np.asarray(TRI_MATS)[g.integers(len(TRI_MATS), size=n_tri)]]).astype(np.int32)
    ns, nm = len(sph), len(mov)
    base = np.array([0, ns, ns + nm])
    core_slots = base[kind] + index  # the hand scene's insertion order, in this scene's class-major slots
    n_cls = np.array([len(csph), len(cmov), len(ctri)])
    filler = np.concatenate([base[k] + np.arange(n_cls[k], (ns, nm, len(tri))[k]) for k in range(3)])
    perm = np.concatenate([core_slots, filler[np.random.default_rng(98).permutation(len(filler))]])
    assert np.array_equal(np.sort(perm), np.arange(ns + nm + len(tri)))
    return Geometry(sph, mov, tri, pmat, MATS, LOOK[0], perm)


def scene_of(G, keep, cam_shift=None):
    """The rtow.Scene of G in its insertion order, under the LOOK camera (translated by cam_shift); G.cam follows."""
    from support_scenes import look_at, set_order, to_scene

    sc = to_scene(G, keep)
    sc.camera = look_at(*LOOK, vfov=40.0, aspect=FRAME[0] / FRAME[1])
    if cam_shift is not None:
        for f in ("origin", "lower_left_corner"):
            v = getattr(sc.camera, f)
            for k in range(3):
                v[k] += float(cam_shift[k])
    G.cam = np.array(sc.camera.origin[:])
    return set_order(sc, G, keep, G.perm)


def moved(G, H):
    """H (a deformation of G by support_scenes.deform / motions) with G's insertion order."""
    return Geometry(H.sph, H.mov, H.tri, H.pmat, H.mats, H.cam, G.perm)


class Held:
    """What SceneView, orc.render and Context.upload take: `.c` is the rtow.Scene, the arrays live in `.keep`."""

    def __init__(self, G, cam_shift=None):
        self.G, self.keep = G, []
        self.c = scene_of(G, self.keep, cam_shift)


class Case:
    """The scene in every form the checkers take, each built on first use and once: hs (upload, .c), view (SceneView),
    exact (exact_hits.Scene), rec and mats (point_ref records, material per insertion index), image and log (the
    single-threaded oracle render of FRAME with its ray log)."""

    def __init__(self, G=None, cam_shift=None):
        self.G = geometry() if G is None else G
        self.hs = Held(self.G, cam_shift)

    @functools.cached_property
    def view(self):
        from support_scenes import SceneView

        return SceneView(self.hs)

    @functools.cached_property
    def exact(self):
        import exact_hits as ex

        return ex.Scene.of(self.view)

    @functools.cached_property
    def rec(self):
        import point_ref as pr

        return pr.records(self.view)

    @property
    def mats(self):
        return self.view.prim_mat

    def config(self, precision=None, **kw):
        import rtow

        w, h, spp, depth, seed = FRAME
        return rtow.make_config(w, h, spp, kw.pop("nstreams", 1), kw.pop("max_child_rays", depth), seed=seed,
                                precision=rtow.F64_STRICT if precision is None else precision, **kw)

    @functools.cached_property
    def _render(self):
        from support_oracle import logged_render

        return logged_render(self.hs, self.config())

    @property
    def image(self):
        return self._render[0]

    @property
    def log(self):
        return self._render[1]


@functools.lru_cache(maxsize=None)
def case():
    """The one Case every test of a process shares (nothing of it is ever changed)."""
    return Case()


# ------------------------------------------------------------------------------------------------ the grid's rules ---
def grid_rules(G, large_ratio=4.0, cells_per_prim=1.0, flat_ratio=1.5):
    """build_grid_image's two refusals (csrc/rtow_grid.h) on G: (number of large primitives — box diagonal above 4 x the
    median; the grid is dropped above 64 —, longest cell list — dropped above 255 —, cells per axis).  The boxes are
    accel_images.record_bounds of the records an upload computes (the builder's boxes moved outwards by an ulp, the
    moving spheres' over the builder's widened shutter interval); the median, grid_header and the registration follow the
    builder in numpy.  Nothing on the host ties this to rtow_grid.h: if it drifted from the builder, only the GPU tests'
    assertion that the grid image is resident and above the limit (big_mixed.resident) would show it."""
    lo, hi = ai.record_bounds(G.sph_records(), G.mov_records(), G.tri_records(), widen=2e-6)
    diag = np.sqrt(((hi - lo) ** 2).sum(axis=1))
    med = max(np.sort(diag)[len(diag) // 2], 1e-12)
    large = diag > large_ratio * med
    small = ~large
    gmn, gmx = lo[small].min(axis=0), hi[small].max(axis=0)
    scale = max(1.0, np.abs(gmn).max(), np.abs(gmx).max(), np.abs(lo[large]).max(initial=0.0), np.abs(hi[large]).max(initial=0.0),
                np.abs(G.cam).max())
    pad = 4e-6 * scale
    gmn, gmx = gmn - 2 * pad, gmx + 2 * pad
    ext = np.maximum(gmx - gmn, 1e-9)
    target = min(max(cells_per_prim * small.sum(), 8.0), 32768.0)
    step = np.cbrt(ext.prod() / target)
    flat = ext < flat_ratio * step
    if 0 < (~flat).sum() < 3:
        step = (ext[~flat].prod() / target) ** (1.0 / (~flat).sum())
    n = np.where(flat, 1, np.clip(np.ceil(ext / step), 1, 128)).astype(np.int64)
    gminf = np.nextafter(gmn.astype(np.float32), np.float32(-np.inf))
    cellf = np.nextafter(((gmx - gminf.astype(np.float64)) / n).astype(np.float32), np.float32(np.inf))
    c_lo = np.clip(np.floor((lo[small] - pad - gminf) / cellf.astype(np.float64)), 0, n - 1).astype(np.int64)
    c_hi = np.clip(np.floor((hi[small] + pad - gminf) / cellf.astype(np.float64)), 0, n - 1).astype(np.int64)
    count = np.zeros(n[::-1], dtype=np.int64)  # [z, y, x]
    for a, b in zip(c_lo, c_hi):
        count[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1] += 1
    return int(large.sum()), int(count.max()), n.tolist()


# --------------------------------------------------------------------------------------------------- query sets ---
def _finite_tmax(rays, share, seed):
    g = np.random.default_rng(seed)
    rays = rays.copy()
    rays["tmax"] = np.where(g.random(len(rays)) < share, g.uniform(0.1, 5.0, len(rays)), np.inf)
    return rays


def rtow_rays(o, d, time):
    import rtow

    return rtow.make_rays(o, d, time=time)


@functools.lru_cache(maxsize=None)
def ray_sets(c):
    """name -> (rays, share of undecided rays allowed or None): the families of test_gpu_exact_hits.py on this scene."""
    import types

    import exact_cases as ec
    from support_oracle import rays_of
    from support_scenes import handmade_rays

    view, log = c.view, c.log
    g = np.random.default_rng(5)
    nc = N_CORE_TRI  # the core's triangles lead the class
    tri = np.concatenate([view.tri[:nc], view.tri[nc:][np.sort(g.choice(len(view.tri) - nc, 80, replace=False))]])
    tri = tri[::2]  # (every other one of the core's 30 and of 80 of the filler's: 55 triangles, 26 rays each)
    # the core's spheres and six of the filler's of each class
    some = types.SimpleNamespace(sph=view.sph[:N_CORE_SPH + 6], mov=view.mov[:N_CORE_MOV + 6])
    mags = []
    for k, s in enumerate((1e-4, 1e-2, 1e2, 1e4)):
        r = rays_of(ec.subsample(log, 250, 20 + k))
        r["direction"] *= s
        mags.append(r)
    lo, hi = view.tri[nc:].reshape(-1, 3).min(0), view.tri[nc:].reshape(-1, 3).max(0)  # the filler's box
    ext = float(np.max(hi - lo))
    rnd = rtow_rays(g.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(1000, 3)), g.normal(size=(1000, 3)), g.random(1000))
    return {
        "logged": (_finite_tmax(rays_of(ec.subsample(log, 1500, 1)), 0.3, 2), ec.SHARE),
        "random": (_finite_tmax(rnd, 0.3, 7), ec.SHARE),
        "handmade": (handmade_rays(), None),
        "tangent": (ec.handmade_tangent_rays(some), None),
        "edges": (ec.edge_rays(tri, len(tri), 3), None),
        "surfaces": (ec.surface_rays(ec.subsample(log, 3000, 6)), None),
        "magnitudes": (np.concatenate(mags), None),
    }


def sequence_sets(c, sets=None):
    """The ray sets of the first-k-hits checks: the logged and the hand-made rays.  The logged set leaves out the rays
    whose line passes the core's two EQUAL spheres (within 1e-6 of their radius of the centre, by the ray and the sphere
    alone): both are met at exactly the same t, and an exact tie is never a decided sequence — 5 of the 1,500 logged rays,
    over the cap of 1e-3 on the reference side alone."""
    sets = ray_sets(c) if sets is None else sets
    rays, share = sets["logged"]
    twin = c.view.sph[3]
    oc = twin[:3] - rays["origin"]
    d = rays["direction"] / np.linalg.norm(rays["direction"], axis=1, keepdims=True)
    along = (oc * d).sum(axis=1)
    off = np.linalg.norm(oc - along[:, None] * d, axis=1)
    keep = ~((off < abs(twin[3]) * (1 + 1e-6)) & (along > -abs(twin[3])))
    return {"logged": (rays[keep], share), "handmade": sets["handmade"]}


RAY_SETS = ("logged", "random", "handmade", "tangent", "edges", "surfaces", "magnitudes")
SEQUENCE_SETS = ("logged", "handmade")
POINT_SIZES = dict(tri=6, sph=5, mov=5, far_dirs=2, near=60, random=60, mixed=125)


def point_inputs(c):
    """(near, random, handmade set): pr.all_sets' `near` and `rnd` from the log, and handmade_points' points as one
    more set at their own times and max_dist."""
    import ambient_cases as ac
    import point_cases as pc

    ps = pc.point_sets(c.rec, c.log, POINT_SIZES["mixed"], 9)
    hp = ac.handmade_points()
    return ps["near"], ps["random"][0], ("handmade", hp["point"].copy(), hp["time"].copy(), hp["max_dist"].copy())


def point_sets(c):
    import point_cases as pc
    import point_ref as pr

    near, rnd, hand = point_inputs(c)
    return pr.all_sets(c.rec, pc.SEED, near, rnd, sizes=POINT_SIZES) + [hand]


def nearest_sets(c):
    import nearest_cases as nc
    import point_cases as pc

    near, rnd, hand = point_inputs(c)
    return nc.nearest_sets(c.rec, pc.SEED, near, rnd, sizes=POINT_SIZES) + [hand]


AMBIENT_SAMPLES = (4, 8)
SWEEP_RADII = (0.0, 0.002, 0.01, 0.05)  # x the extent (about 15): the hand scene's 0.2 is a ball of hundreds of filler primitives


def strict_sweeps(c, n=4097):
    """sweep_cases.strict_sets with the scene's radii: placed, skipped, random with finite, infinite (1 in 7) and zero tmax."""
    a, b = sweep_cases.placed_sweeps(), sweep_cases.skipped_sweeps()
    return np.concatenate([a, b, sweep_cases.random_sweeps(c.rec, n - len(a) - len(b), 5, finite=False, radii=SWEEP_RADII)])


def tie_sweeps(c):
    """(sweeps, expected insertion index): onto the quad's shared edge and onto the two equal spheres of the core."""
    import sweep_ref as sr

    rec = c.rec
    q = sr.make_sweeps([[0.0, 1.0, -5.0], [0.0, 1.0, -5.0], [2.5, 0.4, 6.0]], [[0, 0, 1], [0, 0, 1], [0, 0, -1]], [0.25, 0.0, 0.2], 0.0, 10.0)
    ins = rec.cls2ins
    ns, nm = rec.ns, rec.nm
    return q, np.array([min(ins[ns + nm], ins[ns + nm + 1])] * 2 + [min(ins[3], ins[4])])


def contact_sweeps(c, answer, limit=300):
    """One three-stage chain (sweep_cases.contact_set) of the aimed first stage and 100 random sweeps, thinned to `limit`."""
    first = np.concatenate([sweep_cases.aimed_sweeps(1), sweep_cases.random_sweeps(c.rec, 100, 3, radii=SWEEP_RADII)])
    return sweep_cases.thin(sweep_cases.contact_set(c.rec, first, answer, 4), limit)


def ambient_points(c, n=80):
    """(points, ids): log_points of the scene's own log and every other one of the hand-placed points (ids drawn with a
    fixed seed)."""
    import ambient_cases as ac
    import ambient_ref

    pts, ids = ac.log_points(c.view, c.log, n, 45)
    hp = ac.handmade_points()[::2]
    g = np.random.default_rng(46)
    hid = np.stack([g.integers(0, 1 << 32, len(hp)), g.integers(0, 1 << 32, len(hp))], axis=1).astype(np.uint32)
    pts, ids = np.concatenate([pts, hp]), np.concatenate([ids, hid])
    live = ~ambient_ref.skipped(pts)  # (log_points names a hit's primitive by its class index alone, and the core's zero-area triangles share theirs
    # with two filler spheres: a point on one of those gets the triangle's zero normal)
    return pts[live], ids[live]


def scatter_case(c, n=1500):
    """scatter_cases.logged_case on this scene's own log: at most n rows, every segment depth and all three material
    kinds among them (the host test asserts it).  Rows that end on the core's two EQUAL spheres are left out, by the
    logged hit point alone (within 1e-6 of that surface): the spheres tie exactly, and the scatter reference decides no
    ray whose hit is a tie — 2 of 1,500 rows, over the cap of 1e-3 on the reference side alone.  Closest hit, first k and
    the sweeps' tie rule keep such rays."""
    import exact_cases as ec
    import orc
    import scatter_cases as sc
    from support_oracle import rays_of

    log = c.log
    twin = c.view.sph[TWINS[0]]
    p = log[:, 3:6] + np.where(np.isfinite(log[:, 10:11]), log[:, 10:11], 0.0) * log[:, 6:9]
    on_twin = np.isfinite(log[:, 10]) & (np.abs(np.linalg.norm(p - twin[:3], axis=1) - twin[3]) < 1e-6)
    log = log[~on_twin]
    seg = log[:, 2].astype(np.int64)
    first = np.array([np.nonzero(seg == b)[0][0] for b in range(int(seg.max()) + 1)])
    rest = np.setdiff1d(np.arange(len(log)), first)
    rows = np.concatenate([log[first], ec.subsample(log[rest], n - len(first), 12)])
    mats = orc.scene_arrays(c.hs.c)["materials"]
    case = sc.Case("big_mixed", c.exact, mats, rays_of(rows), rows[:, 0:2].astype(np.uint32), rows[:, 2].astype(np.int64), FRAME[4])
    case.hs, case.view, case.rows = c.hs, c.view, rows
    return case


# ------------------------------------------------------------------------- what every GPU test of the scene asserts ---
def used():
    """walk name -> the kernel_used a ray query must report on this scene (support_oracle.expected_kernel: BVH4 walks
    triangle meshes only; there is a grid)."""
    import rtow

    return {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID, "bvh4": rtow.KERNEL_BVH}


def resident(ctx, bname):
    """Both images of the resident scene are beyond LDS and there is no 4-wide image: asserted after every upload and
    refit of the scene, by every test that runs on it.  This is what identifies the instantiation such a test runs: the
    launcher stages an image in LDS only if it fits (csrc/rtow_capi.cpp:630, `lds_bytes = (image_kernel && image_bytes <=
    kLdsLimit) ? image_bytes : 0u`, kLdsLimit = 160 KiB in csrc/rtow_ctx.h:57), and lds_bytes == 0 selects the
    <kernel, false> form of a query kernel (csrc/rtow_query.h:151-157 and its siblings).  So a BVH image above 160 KiB with
    kernel_used BVH is rtow_*<BVH, false>, a grid image above 160 KiB with kernel_used GRID is rtow_*<GRID, false>, and
    bvh4_nodes == 0 says no 4-wide image takes a launch over.  The sizes are those of the resident images themselves
    (rtow_debug_image returns the byte counts the launcher reads); after an upload they are also build_info()'s, which
    keeps the upload's figures through a refit ("facts about the last rtow_scene_upload", include/rtow.h).
    Returns (BVH image bytes, grid image bytes)."""
    bi = ctx.build_info()
    bvh, grid = len(ctx.debug_image(0)), len(ctx.debug_image(1))
    assert bvh > LDS_LIMIT and grid > LDS_LIMIT and bi.bvh4_nodes == 0 and not ctx.debug_image(4), (bname, bvh, grid, bi.bvh4_nodes)
    if ctx.refit_info().refits == 0:
        assert (bi.bvh_image_bytes, bi.grid_image_bytes) == (bvh, grid), (bname, bi.bvh_image_bytes, bi.grid_image_bytes)
    return bvh, grid


REFITS = ("jitter", "translate")


@functools.lru_cache(maxsize=None)
def refitted(motion):
    """The Case of the deformed geometry (support_scenes.motions; same insertion order; `translate` also moves the camera)."""
    from support_scenes import motions

    G = case().G
    todo = motions(G)
    return Case(moved(G, todo[motion][0]), cam_shift=todo["camera"][1] if motion == "translate" else None)
