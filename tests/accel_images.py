"""Ray-independent checks of the resident acceleration images against the exact bounds of their geometry.

A helper module for the tests (pure numpy, no GPU): it parses the images rtow_debug_image returns — the binary BVH
(0) and its binary32 twin (2), the uniform grid (1) and its binary32 twin (3), the 4-wide BVH (4) with the frame its
walk decodes binary16 planes in (5) — and checks the claim every walk rests on: the culling is conservative, so the
closest hit cannot depend on the tree, for ANY ray.

Reference: the exact bounds of what the hit tests see, from the image's own binary64 records.
  * triangle (a, e1, e2): vertices a, a+e1, a+e2 — the sums rounded outwards (np.nextafter), because the real vertex,
    not fl(a+e1), is what the test intersects;
  * sphere (c, r2 = copysign(r*r, r)): c +- sqrt(|r2|), rounded outwards;
  * moving sphere (c0, dc, r2, r): the union over both ends c0 and c0+dc, time in [0, 1] (include/rtow.h, ray queries).
  S = max(1, max |coordinate| of those bounds): a lower bound of the builders' `scale`, which also takes the camera.

Margins and bounds (each derived from the builders):
  * containment, binary32 planes: every plane encloses the exact bounds below it by at least MARGIN * S on each side.
    Both builders pad by 2e-6 * scale + 2e-6 * max(|lo|, |hi|) (rtow_bvh.h make_scene_image, rtow_bvh4.h,
    rtow_build.hip k_morton) and round outwards; the f32 rounding of a ray's origin is about 6e-8 * S, so 1e-6 * S is
    a margin the pad keeps with room to spare and a walk needs.
  * containment, binary16 planes: decoded exactly in the frame the walk uses, c + h * is (rtow_trace_bvh4.h
    bvh4_ray), then the same rule.  +-inf and +-65504 are what they are: the decoded value is compared as it is.
  * tightness (secondary: a child given its parent's box): no plane lies further outside the union below it than
        4e-6 * (scale + |plane|) + 1e-9 * (1 + scale) + 2 binary32 ulps at the plane,
    scale = max(1, S, |camera origin|) (plus a relative 1e-6 for the device builder's binary32 scale, rounded up).
    The pad is at most 2e-6 * scale + 2e-6 * scale (max(|lo|, |hi|) <= scale), the pad_box slack on every primitive
    box is 1e-9 * (1 + ext) with ext <= scale (rtow_bvh.h pad_box, rtow_build.hip k_bounds: a plane near 0 of the
    r = 1000 ground sphere's box sits that far out), and the conversion to binary32 moves a plane by at most one ulp
    before nextafterf moves it by one more (host: round to nearest, half an ulp; device: __double2float_rd, one).  Moving
    spheres are taken over the builders' widened shutter [-w, 1 + w], w = 1e-6 * (1 + |t0| + |t1|) = 3e-6
    (rtow_bvh.h build_bvh, rtow_build.hip k_bounds).  binary16 planes add one binary16 spacing at the plane (the
    directed rounding), one binary32 spacing in the frame (the device's intermediate __double2float_rd) and the
    rounding of `is` to binary32 (2^-24 of |h * is|), all in world units; saturated planes (|h| >= 65504) are skipped.
  * records: bit for bit the scene's primitives with the precomputed terms of rtow_scene_records.h (sphere
    copysign(r*r, r); moving c1-c0, copysign(r*r, r), r; triangle e1 = b-a, e2 = c-a, n = e1 x e2 in its operation
    order; numpy rounds each operation like the host code built with -ffp-contract=off).  Leaf-ordered images (the
    host builder's triangle meshes, every 4-wide image) are matched as a multiset of (record bytes, material index).
  * binary32 images: the same prefix (nodes + ids, or header + cells + ids + fat lists) as their binary64 image, and
    binary32 records = the binary64 records of the same slot rounded to nearest (rtow_scene.cpp make_image32).
  * grid: every small primitive is listed in every cell its exact box, widened by MARGIN * S, touches (the host pads
    by 4e-6 * scale, rtow_grid.h grid_header); the others are in the large list; counts <= 255; fat entries match
    rtow_grid.h write_fat_entry bit for bit (k = (cx^2 + cy^2 + cz^2) - |r2|).
"""
from __future__ import annotations

import numpy as np

MARGIN = 1e-6          # containment margin, in units of S
TIGHT = 4e-6           # tightness: the pad's upper bound, in units of (scale + |plane|)
PAD_BOX = 1e-9         # the builders' binary64 slack on every primitive box, in units of (1 + its extent)
TIME_WIDEN = 3e-6      # the builders' widening of the shutter interval [0, 1]: 1e-6 * (1 + |t0| + |t1|)
KREF_NONE, KREF_LEAF = 0x1FFFFF, 1 << 20
MAT_LAMBERTIAN, MAT_DIELECTRIC = 0, 2

NODE2 = np.dtype([("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("skip", "<u4"), ("leaf", "<u4")])
MAT_DT = np.dtype([("att", "<f8", (3,)), ("fuzz", "<f8"), ("ir", "<f8"), ("kind", "<i4"), ("pad", "<i4")])
FRAME_DT = np.dtype([("c", "<f8", (3,)), ("is", "<f4", (3,)), ("half", "<u4"), ("lds_limit", "<u4"), ("pad", "<u4")])


class ImageError(AssertionError):
    pass


def _up16(v):
    return (int(v) + 15) // 16 * 16


def _dn(x):
    return np.nextafter(x, -np.inf)


def _upw(x):
    return np.nextafter(x, np.inf)


class Geometry:
    """The scene as uploaded: sphere [n][4] (c, r), moving [n][8] (c0, c1, r, pad), triangle [n][9] (a, b, c),
    material index per primitive (class-major), materials as (kind, albedo[3], fuzz, ir), the camera origin."""

    def __init__(self, sph, mov, tri, pmat, mats, cam_origin):
        self.sph = np.asarray(sph, np.float64).reshape(-1, 4)
        self.mov = np.asarray(mov, np.float64).reshape(-1, 8)
        self.tri = np.asarray(tri, np.float64).reshape(-1, 9)
        self.ns, self.nm, self.nt = len(self.sph), len(self.mov), len(self.tri)
        self.np = self.ns + self.nm + self.nt
        self.pmat = np.asarray(pmat, np.int32).reshape(-1)
        assert len(self.pmat) == self.np
        self.mats = list(mats)
        self.cam = np.asarray(cam_origin, np.float64).reshape(3)

    @classmethod
    def of_scene(cls, sc):
        """From an rtow.Scene (the ctypes struct of include/rtow.h)."""
        def arr(ptr, n, w, dt=np.float64):
            return np.ctypeslib.as_array(ptr, shape=(n * w,)).astype(dt).reshape(n, w) if n else np.zeros((0, w), dt)
        sph, mov, tri = arr(sc.sphere_geom, sc.n_spheres, 4), arr(sc.moving_geom, sc.n_moving, 8), arr(sc.triangle_geom, sc.n_triangles, 9)
        pm = [arr(sc.sphere_mat, sc.n_spheres, 1, np.int32), arr(sc.moving_mat, sc.n_moving, 1, np.int32),
              arr(sc.triangle_mat, sc.n_triangles, 1, np.int32)]
        mats = [(m.kind, tuple(m.albedo), m.fuzz, m.ir) for m in (sc.materials[i] for i in range(sc.n_materials))]
        return cls(sph, mov, tri, np.concatenate([p.reshape(-1) for p in pm]), mats, tuple(sc.camera.origin))

    # ---- the records an upload computes (rtow_scene_records.h), in its operation order ---------------------------
    def sph_records(self):
        g = self.sph
        r = np.empty((self.ns, 4))
        r[:, :3] = g[:, :3]
        r[:, 3] = np.copysign(g[:, 3] * g[:, 3], g[:, 3])
        return r

    def mov_records(self):
        g = self.mov
        r = np.empty((self.nm, 8))
        r[:, :3] = g[:, :3]
        r[:, 3:6] = g[:, 3:6] - g[:, :3]
        r[:, 6] = np.copysign(g[:, 6] * g[:, 6], g[:, 6])
        r[:, 7] = g[:, 6]
        return r

    def tri_records(self):
        g = self.tri
        e1, e2 = g[:, 3:6] - g[:, :3], g[:, 6:9] - g[:, :3]
        r = np.empty((self.nt, 12))
        r[:, :3], r[:, 3:6], r[:, 6:9] = g[:, :3], e1, e2
        r[:, 9] = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]
        r[:, 10] = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]
        r[:, 11] = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
        return r

    def mat_records(self):
        out = np.zeros(len(self.mats), MAT_DT)
        for i, (kind, albedo, fuzz, ir) in enumerate(self.mats):
            out[i]["att"] = (1.0, 1.0, 1.0) if kind == MAT_DIELECTRIC else albedo
            out[i]["fuzz"] = 0.0 if kind == MAT_LAMBERTIAN else fuzz
            out[i]["ir"] = ir
            out[i]["kind"] = kind
        return out.tobytes()


# ---- exact bounds of the geometry the hit tests see ----------------------------------------------------------------
def sph_bounds(rec):
    R = _upw(np.sqrt(np.abs(rec[:, 3])))[:, None]
    return _dn(rec[:, :3] - R), _upw(rec[:, :3] + R)


def mov_bounds(rec, widen=0.0):
    c0, dc = rec[:, :3], rec[:, 3:6]
    R = _upw(np.sqrt(np.abs(rec[:, 6])))[:, None]
    lo = np.minimum(c0, _dn(c0 + dc)) - widen * np.abs(dc)
    hi = np.maximum(c0, _upw(c0 + dc)) + widen * np.abs(dc)
    return _dn(lo - R), _upw(hi + R)


def tri_bounds(rec):
    a, e1, e2 = rec[:, :3], rec[:, 3:6], rec[:, 6:9]
    lo = np.minimum(a, np.minimum(_dn(a + e1), _dn(a + e2)))
    hi = np.maximum(a, np.maximum(_upw(a + e1), _upw(a + e2)))
    return lo, hi


def record_bounds(sph, mov, tri, widen=0.0):
    """[n][3] lo, hi over the class-major slots of an image's binary64 records."""
    parts = [sph_bounds(sph), mov_bounds(mov, widen), tri_bounds(tri)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def scale_of(lo, hi):
    if len(lo) == 0:
        return 1.0
    return float(max(1.0, np.abs(lo).max(), np.abs(hi).max()))


class Checker:
    """Collects failures; `done()` raises one ImageError that lists them (the first few in full)."""

    def __init__(self, what):
        self.what = what
        self.errors = []

    def fail(self, msg):
        self.errors.append(msg)

    def expect(self, ok, msg):
        if not ok:
            self.fail(msg)
        return ok

    def done(self):
        if self.errors:
            head = "\n  ".join(self.errors[:12])
            more = f"\n  ... and {len(self.errors) - 12} more" if len(self.errors) > 12 else ""
            raise ImageError(f"{self.what}: {len(self.errors)} failure(s)\n  {head}{more}")


def _first_bad(mask, n=4):
    return [int(i) for i in np.flatnonzero(mask)[:n]]


def _containment(ck, where, plo, phi, elo, ehi, S):
    """plo/phi [m][3] planes (f64), elo/ehi [m][3] exact bounds below them: plo <= elo - MARGIN*S, phi >= ehi + MARGIN*S."""
    m = MARGIN * S
    with np.errstate(invalid="ignore"):
        bad_lo = ~(elo - plo >= m)
        bad_hi = ~(phi - ehi >= m)
    for name, bad, p, e in (("lo", bad_lo, plo, elo), ("hi", bad_hi, phi, ehi)):
        rows = bad.any(axis=1)
        for i in _first_bad(rows):
            k = int(np.flatnonzero(bad[i])[0])
            ck.fail(f"{where(i)}: {name} plane of axis {k} = {p[i, k]!r} does not enclose the exact bound {e[i, k]!r} "
                    f"with the margin {m:.3g} (1e-6 S, S = {S:.6g})")
        if rows.sum() > 4:
            ck.fail(f"... {int(rows.sum())} entries with a {name} plane inside the margin")


def _tightness(ck, where, plo, phi, elo, ehi, lo_tol, hi_tol, scale_hi):
    """No plane further outside the union below it than its tolerance (an infinite tolerance skips the plane)."""
    with np.errstate(invalid="ignore"):
        loose_lo = np.isfinite(plo) & (elo - plo > lo_tol)
        loose_hi = np.isfinite(phi) & (phi - ehi > hi_tol)
    for name, bad, p, e, tol in (("lo", loose_lo, plo, elo, lo_tol), ("hi", loose_hi, phi, ehi, hi_tol)):
        rows = bad.any(axis=1)
        for i in _first_bad(rows):
            k = int(np.flatnonzero(bad[i])[0])
            ck.fail(f"{where(i)}: {name} plane of axis {k} = {p[i, k]!r} lies {abs(p[i, k] - e[i, k]):.6g} outside the "
                    f"union below it ({e[i, k]!r}), more than the pad's bound {tol[i, k]:.6g} (scale {scale_hi:.6g})")
        if rows.sum() > 4:
            ck.fail(f"... {int(rows.sum())} entries with a {name} plane beyond the pad's bound")


def _f32_tol(planes, scale_hi):
    a = np.abs(planes)
    ulp = np.spacing(np.float32(np.where(np.isfinite(a), a, 0.0)).astype(np.float32)).astype(np.float64)
    return TIGHT * (scale_hi + a) + PAD_BOX * (1.0 + scale_hi) + 2.0 * ulp


def _check_records(ck, name, got_rec, got_mat, want_rec, want_mat, leaf_order):
    """got_*/want_*: [n][w] float64 records and [n] material indices of one class."""
    if len(want_rec) == 0:
        return
    g = np.ascontiguousarray(got_rec).view(np.uint64)
    w = np.ascontiguousarray(want_rec).view(np.uint64)
    if not leaf_order:
        bad = ~((g == w).all(axis=1) & (got_mat == want_mat))
        for i in _first_bad(bad):
            ck.fail(f"{name} record slot {i}: {got_rec[i].tolist()} (material {int(got_mat[i])}) != the scene's "
                    f"{want_rec[i].tolist()} (material {int(want_mat[i])})")
        if bad.sum() > 4:
            ck.fail(f"... {int(bad.sum())} {name} records differ from the scene")
        return
    # multiset of (record bytes, material index): sort both by the same key
    gk = np.concatenate([g, got_mat.astype(np.uint64)[:, None]], axis=1)
    wk = np.concatenate([w, want_mat.astype(np.uint64)[:, None]], axis=1)
    gs = gk[np.lexsort(gk.T[::-1])]
    ws = wk[np.lexsort(wk.T[::-1])]
    bad = ~(gs == ws).all(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        ck.fail(f"{name} records in leaf order are not a permutation of the scene's (record, material) pairs: "
                f"{int(bad.sum())} of {len(bad)} sorted entries differ, first {gs[i].view(np.float64)[:-1].tolist()} "
                f"against {ws[i].view(np.float64)[:-1].tolist()}")


# ---- binary BVH (images 0 and 2) -----------------------------------------------------------------------------------
def _layout_tail(G, tri_bytes, with32):
    ids = _up16(4 * G.np)
    rest = G.ns * 32 + G.nm * 64 + G.nt * tri_bytes
    if with32:
        rest = _up16(rest) + G.ns * 16 + G.nm * 32
    return ids, rest


def parse_bvh2(blob, G):
    """Sections of image 0: nodes (threaded, n_nodes + END), ids, records, material indices, materials."""
    ids_b, rest = _layout_tail(G, 96, False)
    tail = ids_b + rest
    tail = _up16(tail) + _up16(4 * G.np) + 48 * len(G.mats)
    nodes_bytes = len(blob) - tail
    if nodes_bytes < 32 or nodes_bytes % 32:
        raise ImageError(f"BVH image of {len(blob)} bytes does not fit the layout of {G.np} primitives")
    n = nodes_bytes // 32 - 1
    b = np.frombuffer(blob, np.uint8)
    nodes = np.frombuffer(blob, NODE2, count=n + 1)
    off_ids = nodes_bytes
    off_sph = off_ids + ids_b
    off_mov, off_tri = off_sph + 32 * G.ns, off_sph + 32 * G.ns + 64 * G.nm
    off_pmat = _up16(off_tri + 96 * G.nt)
    off_mats = _up16(off_pmat + 4 * G.np)
    f8 = lambda off, n_, w: np.frombuffer(blob, np.float64, count=n_ * w, offset=off).reshape(n_, w)
    return dict(n=n, nodes=nodes, ids=np.frombuffer(blob, np.int32, count=G.np, offset=off_ids),
                sph=f8(off_sph, G.ns, 4), mov=f8(off_mov, G.nm, 8), tri=f8(off_tri, G.nt, 12),
                pmat=np.frombuffer(blob, np.int32, count=G.np, offset=off_pmat),
                mats=bytes(b[off_mats:off_mats + 48 * len(G.mats)]), off_sph=off_sph)


def check_bvh2(blob, G, what="BVH image"):
    ck = Checker(what)
    P = parse_bvh2(blob, G)
    n, nodes, ids = P["n"], P["nodes"], P["ids"]
    skip = nodes["skip"].astype(np.int64)
    leaf = nodes["leaf"].astype(np.int64)
    # ---- structure: threaded depth-first layout
    ck.expect(skip[n] == n and leaf[n] == 0, f"END record {n}: skip {skip[n]}, leaf {leaf[n]:#x} (want skip {n}, leaf 0)")
    ck.expect(skip[0] == n, f"root: skip {skip[0]} != {n} nodes (the root's subtree is not the whole image)")
    idx = np.arange(n)
    sk = skip[:n]
    bad = ~((sk > idx) & (sk <= n))
    for i in _first_bad(bad):
        ck.fail(f"node {i}: skip link {sk[i]} does not point forward inside [{i + 1}, {n}]")
    is_leaf = leaf[:n] != 0
    inner = ~is_leaf
    bad = is_leaf & (sk != idx + 1)
    for i in _first_bad(bad):
        ck.fail(f"leaf node {i}: skip link {sk[i]} != {i + 1} (its subtree is [i, skip))")
    skc = np.clip(skip, 0, n)
    c2 = skc[np.minimum(idx + 1, n)]
    bad = inner & ~((idx + 1 < n) & (c2 < sk) & (skc[c2] == sk))
    for i in _first_bad(bad):
        ck.fail(f"inner node {i}: children {i + 1} and skip({i + 1}) = {c2[i]} do not tile its subtree [{i}, {sk[i]})")
    # ---- leaves: counts 1..7, every primitive id exactly once
    first, cnt = leaf[:n] >> 3, leaf[:n] & 7
    bad = is_leaf & ((cnt == 0) | (first + cnt > G.np))
    for i in _first_bad(bad):
        ck.fail(f"leaf node {i}: (first {first[i]}, count {cnt[i]}) outside the id section of {G.np}")
    lf = np.flatnonzero(is_leaf & ~bad)
    pos = np.concatenate([np.arange(first[i], first[i] + cnt[i]) for i in lf]) if len(lf) else np.zeros(0, np.int64)
    ref_ids = ids[pos].astype(np.int64)
    bad_ids = (ref_ids < 0) | (ref_ids >= G.np)
    if bad_ids.any():
        ck.fail(f"leaf ids out of range [0, {G.np}): {ref_ids[bad_ids][:4].tolist()}")
    seen = np.bincount(ref_ids[~bad_ids], minlength=G.np)
    for p in _first_bad(seen != 1):
        ck.fail(f"primitive {p} appears in {seen[p]} leaves (want exactly one)")
    if (seen != 1).sum() > 4:
        ck.fail(f"... {int((seen != 1).sum())} primitives not in exactly one leaf")
    if ck.errors:  # geometry needs a sound tree
        ck.done()
    # ---- containment and tightness of the binary32 planes
    lo, hi = record_bounds(P["sph"], P["mov"], P["tri"])
    llo, lhi = record_bounds(P["sph"], P["mov"], P["tri"], widen=TIME_WIDEN)
    S = scale_of(lo, hi)
    scale_hi = max(1.0, S * (1 + 1e-6) + 1e-6, float(np.abs(G.cam).max()))
    elo, ehi, eloo, ehil = (np.full((n + 1, 3), v) for v in (np.inf, -np.inf, np.inf, -np.inf))
    leaf_slots = np.repeat(lf, cnt[lf])  # node of each referenced id, in `pos` order
    np.minimum.at(elo, leaf_slots, lo[ref_ids])
    np.maximum.at(ehi, leaf_slots, hi[ref_ids])
    np.minimum.at(eloo, leaf_slots, llo[ref_ids])
    np.maximum.at(ehil, leaf_slots, lhi[ref_ids])
    # subtree of node i = nodes [i, skip(i)): one segmented reduction (reduceat over the interleaved bounds)
    seg = np.empty(2 * n, np.int64)
    seg[0::2], seg[1::2] = idx, sk
    sub = [np.minimum.reduceat(elo, seg)[0::2], np.maximum.reduceat(ehi, seg)[0::2],
           np.minimum.reduceat(eloo, seg)[0::2], np.maximum.reduceat(ehil, seg)[0::2]]
    plo, phi = nodes["lo"][:n].astype(np.float64), nodes["hi"][:n].astype(np.float64)
    where = lambda i: f"node {i} ({'leaf' if is_leaf[i] else 'inner'}, subtree [{i}, {sk[i]}))"
    _containment(ck, where, plo, phi, sub[0], sub[1], S)
    _tightness(ck, where, plo, phi, sub[2], sub[3], _f32_tol(plo, scale_hi), _f32_tol(phi, scale_hi), scale_hi)
    # ---- records and shading data
    leaf_order = G.ns == 0 and G.nm == 0 and np.array_equal(ids, np.arange(G.np))
    _check_records(ck, "sphere", P["sph"], P["pmat"][:G.ns], G.sph_records(), G.pmat[:G.ns], False)
    _check_records(ck, "moving sphere", P["mov"], P["pmat"][G.ns:G.ns + G.nm], G.mov_records(),
                   G.pmat[G.ns:G.ns + G.nm], False)
    _check_records(ck, "triangle", P["tri"], P["pmat"][G.ns + G.nm:], G.tri_records(), G.pmat[G.ns + G.nm:], leaf_order)
    ck.expect(P["mats"] == G.mat_records(), "material records differ from the scene's materials")
    ck.done()
    return dict(n_nodes=n, S=S, leaf_order=leaf_order)


# ---- binary32 twins (images 2 and 3) -------------------------------------------------------------------------------
def check_image32(blob32, blob64, off_sph64, G, what):
    """`off_sph64`: size of the prefix both images share (BVH: nodes + ids; grid: header, cells, ids, fat lists)."""
    ck = Checker(what)
    pre = off_sph64
    off_mov = pre + 32 * G.ns
    off_tri = off_mov + 64 * G.nm
    off_sph32 = _up16(off_tri + 48 * G.nt)
    off_mov32 = off_sph32 + 16 * G.ns
    off_pmat = _up16(off_mov32 + 32 * G.nm)
    off_mats = _up16(off_pmat + 4 * G.np)
    want_len = _up16(off_mats + 48 * len(G.mats))
    if len(blob32) != want_len:
        raise ImageError(f"{what}: {len(blob32)} bytes, the layout of the binary64 image's prefix gives {want_len}")
    ck.expect(blob32[:pre] == blob64[:pre], f"the prefix (first {pre} bytes: nodes / cells and ids) differs from the "
              f"binary64 image's at byte {next((i for i in range(pre) if blob32[i] != blob64[i]), -1)}")
    f8 = lambda b, off, n_, w: np.frombuffer(b, np.float64, count=n_ * w, offset=off).reshape(n_, w)
    f4 = lambda b, off, n_, w: np.frombuffer(b, np.float32, count=n_ * w, offset=off).reshape(n_, w)
    o64_mov = pre + 32 * G.ns
    o64_tri = o64_mov + 64 * G.nm
    o64_pmat = _up16(o64_tri + 96 * G.nt)
    sph64, mov64, tri64 = f8(blob64, pre, G.ns, 4), f8(blob64, o64_mov, G.nm, 8), f8(blob64, o64_tri, G.nt, 12)
    ck.expect(blob32[pre:off_tri] == blob64[pre:o64_tri], "binary64 sphere / moving records differ from the binary64 image's")
    for name, got, want in (("triangle", f4(blob32, off_tri, G.nt, 12), tri64.astype(np.float32)),
                            ("sphere", f4(blob32, off_sph32, G.ns, 4), sph64.astype(np.float32)),
                            ("moving sphere", f4(blob32, off_mov32, G.nm, 8)[:, :7], mov64[:, :7].astype(np.float32))):
        bad = ~(got.view(np.uint32) == want.view(np.uint32)).all(axis=1) if len(want) else np.zeros(0, bool)
        for i in _first_bad(bad):
            ck.fail(f"binary32 {name} record slot {i}: {got[i].tolist()} != the binary64 record of slot {i} rounded "
                    f"to nearest {want[i].tolist()}")
    if G.nm:
        ck.expect((f4(blob32, off_mov32, G.nm, 8)[:, 7] == 0).all(), "binary32 moving records: the 8th word is not 0")
    ck.expect(blob32[off_pmat:off_pmat + 4 * G.np] == blob64[o64_pmat:o64_pmat + 4 * G.np],
              "material indices differ from the binary64 image's")
    ck.expect(blob32[off_mats:off_mats + 48 * len(G.mats)] == G.mat_records(), "material records differ from the scene's")
    ck.done()


def check_bvh2_f32(blob32, blob64, G):
    check_image32(blob32, blob64, parse_bvh2(blob64, G)["off_sph"], G, "binary32 BVH image")


# ---- uniform grid (images 1 and 3) ---------------------------------------------------------------------------------
def parse_grid(blob, G):
    h = np.frombuffer(blob, np.uint8, count=64)
    gmin = np.frombuffer(blob, np.float32, 3, 0).astype(np.float64)
    cell = np.frombuffer(blob, np.float32, 3, 12).astype(np.float64)
    n = np.frombuffer(blob, np.int32, 3, 36).astype(np.int64)
    n_large, off_large, off_fat, stride = (int(x) for x in np.frombuffer(blob, np.uint32, 4, 48))
    ncell = int(np.prod(n))
    off_cells = 64
    off_ids = 64 + _up16(4 * ncell)
    n_cell_ids = (off_large - off_ids) // 4
    total_ids = n_cell_ids + n_large
    off_sph = off_ids + _up16(4 * total_ids) + (n_cell_ids * stride if off_fat else 0)
    return dict(h=h, gmin=gmin, cell=cell, n=n, n_large=n_large, off_large=off_large, off_fat=off_fat, stride=stride,
                ncell=ncell, off_cells=off_cells, off_ids=off_ids, n_cell_ids=n_cell_ids, off_sph=off_sph)


def check_grid(blob, G, what="grid image"):
    ck = Checker(what)
    P = parse_grid(blob, G)
    n, ncell = P["n"], P["ncell"]
    if not ((n >= 1).all() and (n <= 128).all()) or P["off_large"] < P["off_ids"] or (P["off_large"] - P["off_ids"]) % 4:
        raise ImageError(f"{what}: header n {n.tolist()}, off_large {P['off_large']} / off_ids {P['off_ids']} inconsistent")
    off_mov = P["off_sph"] + 32 * G.ns
    off_tri = off_mov + 64 * G.nm
    off_pmat = _up16(off_tri + 96 * G.nt)
    off_mats = _up16(off_pmat + 4 * G.np)
    want_len = _up16(off_mats + 48 * len(G.mats))
    if len(blob) != want_len:
        raise ImageError(f"{what}: {len(blob)} bytes, the header's layout gives {want_len}")
    if P["off_fat"]:
        ck.expect(P["off_fat"] == P["off_ids"] + _up16(4 * (P["n_cell_ids"] + P["n_large"])) and P["stride"] in (48, 80),
                  f"fat lists at {P['off_fat']} with stride {P['stride']}: not behind the id section")
    cells = np.frombuffer(blob, np.uint32, ncell, P["off_cells"]).astype(np.int64)
    ids = np.frombuffer(blob, np.int32, P["n_cell_ids"] + P["n_large"], P["off_ids"]).astype(np.int64)
    cell_ids, large = ids[:P["n_cell_ids"]], ids[P["n_cell_ids"]:]
    first, cnt = cells >> 8, cells & 255
    bad = (cnt > 0) & (first + cnt > P["n_cell_ids"])
    for c in _first_bad(bad):
        ck.fail(f"cell {c}: (first {first[c]}, count {cnt[c]}) outside the {P['n_cell_ids']} cell ids")
    ck.expect(bad.any() or cnt.sum() == P["n_cell_ids"],
              f"cells list {int(cnt.sum())} ids, the id section holds {P['n_cell_ids']} before the large list")
    oob = (ids < 0) | (ids >= G.np)
    ck.expect(not oob.any(), f"ids out of range [0, {G.np}): {ids[oob][:4].tolist()}")
    ck.expect(len(np.unique(large)) == len(large), f"the large list names a primitive twice: {large.tolist()}")
    in_large = np.zeros(G.np, bool)
    in_large[large[(large >= 0) & (large < G.np)]] = True
    if bad.any() or oob.any():
        ck.done()
    rec = dict(sph=np.frombuffer(blob, np.float64, 4 * G.ns, P["off_sph"]).reshape(G.ns, 4),
               mov=np.frombuffer(blob, np.float64, 8 * G.nm, off_mov).reshape(G.nm, 8),
               tri=np.frombuffer(blob, np.float64, 12 * G.nt, off_tri).reshape(G.nt, 12))
    lo, hi = record_bounds(rec["sph"], rec["mov"], rec["tri"])
    S = scale_of(lo, hi)
    m = MARGIN * S
    # the cells each small primitive's box, widened by the margin, touches (closed cells: a box on a boundary touches both)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (lo - m - P["gmin"]) / P["cell"]
        b = (hi + m - P["gmin"]) / P["cell"]
    c_lo = np.clip(np.floor(a - 1e-9 * (1 + np.abs(a))), 0, n - 1).astype(np.int64)
    c_hi = np.clip(np.floor(b + 1e-9 * (1 + np.abs(b))), 0, n - 1).astype(np.int64)
    # membership set of (cell, id) pairs from the cell lists
    owner = np.repeat(np.arange(ncell), cnt)
    listed_pos = np.concatenate([np.arange(first[c], first[c] + cnt[c]) for c in np.flatnonzero(cnt)]) if cnt.any() \
        else np.zeros(0, np.int64)
    listed = np.unique(owner * G.np + cell_ids[listed_pos])
    ck.expect(len(listed) == len(listed_pos), "a cell lists a primitive twice")
    small = np.flatnonzero(~in_large)
    wants, prims = [], []
    for p in small:
        xs, ys, zs = (np.arange(c_lo[p, k], c_hi[p, k] + 1) for k in range(3))
        wants.append(((zs[:, None, None] * n[1] + ys[None, :, None]) * n[0] + xs[None, None, :]).reshape(-1))
        prims.append(np.full(len(wants[-1]), p))
    if wants:
        cs, ps = np.concatenate(wants), np.concatenate(prims)
        hit = np.isin(cs * G.np + ps, listed)
        miss_p = np.unique(ps[~hit])
        for p in miss_p[:4]:
            c = int(cs[~hit & (ps == p)][0])
            ck.fail(f"primitive {p} (box {lo[p].tolist()} .. {hi[p].tolist()}) is not listed in cell {c} "
                    f"({c % n[0]}, {c // n[0] % n[1]}, {c // (n[0] * n[1])}) that its box touches")
        if len(miss_p) > 4:
            ck.fail(f"... {len(miss_p)} small primitives missing from cells they touch")
    # records: the grid keeps the class-major order
    _check_records(ck, "sphere", rec["sph"], np.frombuffer(blob, np.int32, G.ns, off_pmat), G.sph_records(), G.pmat[:G.ns], False)
    _check_records(ck, "moving sphere", rec["mov"], np.frombuffer(blob, np.int32, G.nm, off_pmat + 4 * G.ns),
                   G.mov_records(), G.pmat[G.ns:G.ns + G.nm], False)
    _check_records(ck, "triangle", rec["tri"], np.frombuffer(blob, np.int32, G.nt, off_pmat + 4 * (G.ns + G.nm)),
                   G.tri_records(), G.pmat[G.ns + G.nm:], False)
    ck.expect(bytes(blob[off_mats:off_mats + 48 * len(G.mats)]) == G.mat_records(), "material records differ from the scene's")
    # fat lists: the entry of id-list position e, as write_fat_entry writes it
    if P["off_fat"] and P["n_cell_ids"]:
        st = P["stride"]
        ent = np.frombuffer(blob, np.uint8, P["n_cell_ids"] * st, P["off_fat"]).reshape(-1, st)
        want = np.zeros_like(ent)
        want[:, :4] = cell_ids.astype("<i4").view(np.uint8).reshape(-1, 4)
        srec, mrec = G.sph_records(), G.mov_records()
        if st == 48:
            q = srec[np.clip(cell_ids, 0, max(G.ns - 1, 0))]
            k = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) - np.abs(q[:, 3])
            want[:, 8:16] = k.view(np.uint8).reshape(-1, 8)
            want[:, 16:48] = np.ascontiguousarray(q).view(np.uint8).reshape(-1, 32)
        else:
            r8 = np.zeros((len(cell_ids), 8))
            s = cell_ids < G.ns
            q = srec[np.clip(cell_ids[s], 0, max(G.ns - 1, 0))]
            r8[s, 0:3], r8[s, 6] = q[:, :3], q[:, 3]
            mq = mrec[np.clip(cell_ids[~s] - G.ns, 0, max(G.nm - 1, 0))]
            r8[~s, 0:7] = mq[:, :7]
            want[:, 16:80] = r8.view(np.uint8).reshape(-1, 64)
        bad = ~(ent == want).all(axis=1)
        for e in _first_bad(bad):
            ck.fail(f"fat entry {e} (primitive {cell_ids[e]}): bytes differ from write_fat_entry's")
    ck.done()
    return dict(S=S, ncell=ncell, n_large=P["n_large"], fat=P["stride"] if P["off_fat"] else 0)


def check_grid_f32(blob32, blob64, G):
    check_image32(blob32, blob64, parse_grid(blob64, G)["off_sph"], G, "binary32 grid image")


# ---- 4-wide BVH (images 4 and 5) -----------------------------------------------------------------------------------
def parse_frame(rec):
    if len(rec) != 48:
        raise ImageError(f"4-wide frame record of {len(rec)} bytes (want 48)")
    return np.frombuffer(rec, FRAME_DT, 1)[0]


def check_bvh4(blob, frame_rec, G, what="4-wide BVH image"):
    ck = Checker(what)
    fr = parse_frame(frame_rec)
    half = bool(fr["half"])
    nb = 64 if half else 128
    if G.ns or G.nm:
        raise ImageError(f"{what}: a 4-wide image for a scene with spheres")
    nt = G.nt
    tail = 96 * nt + _up16(4 * nt) + 48 * len(G.mats)
    nodes_bytes = len(blob) - tail
    if nodes_bytes < nb or nodes_bytes % nb:
        raise ImageError(f"{what}: {len(blob)} bytes do not fit the layout of {nt} triangles with {nb}-byte nodes")
    n4 = nodes_bytes // nb
    raw = np.frombuffer(blob, np.uint8, nodes_bytes).reshape(n4, nb)
    if half:
        planes = raw[:, :48].copy().view("<f2").reshape(n4, 3, 2, 4).astype(np.float64)
        cw = raw[:, 48:64].copy().view("<u4").astype(np.int64)
    else:
        planes = raw[:, :96].copy().view("<f4").reshape(n4, 3, 2, 4).astype(np.float64)
        cw = raw[:, 96:112].copy().view("<u4").astype(np.int64)
        ck.expect(not raw[:, 112:].any(), "the 16 unused bytes of a 128-byte node are not zero")
    off_tri = nodes_bytes
    off_pmat = off_tri + 96 * nt
    off_mats = off_pmat + _up16(4 * nt)
    recs = np.frombuffer(blob, np.float64, 12 * nt, off_tri).reshape(nt, 12)
    pmat = np.frombuffer(blob, np.int32, nt, off_pmat)
    # ---- structure
    empty = cw == KREF_NONE
    ck.expect(not (cw & ~0x1FFFFF).any(), f"child words with bits above 21: {cw[(cw & ~0x1FFFFF) != 0][:4].tolist()}")
    is_leaf = ~empty & ((cw & KREF_LEAF) != 0)
    is_inner = ~empty & ~is_leaf
    ck.expect((~empty[0]).any(), "the root has no child")
    node_of = np.repeat(np.arange(n4), 4).reshape(n4, 4)
    back = is_inner & ((cw <= node_of) | (cw >= n4))
    for i, c in zip(*np.nonzero(back)):
        if len(ck.errors) < 4:
            ck.fail(f"node {i} slot {c}: child link {cw[i, c]} does not point to a later node (< {n4})")
    order = cw[is_inner]  # node-major, slot order
    if not back.any():
        parents = np.bincount(order, minlength=n4)
        for j in _first_bad(parents[1:] != 1):
            ck.fail(f"node {j + 1} has {parents[j + 1]} parents (want exactly one)")
        ck.expect(parents[0] == 0, "the root is somebody's child")
        ck.expect(np.array_equal(order, np.arange(1, n4)) or (parents[1:] != 1).any(),
                  f"inner children are not numbered breadth-first: {order[:8].tolist()} ...")
    lfirst, lcnt = (cw & (KREF_LEAF - 1)) >> 2, (cw & 3) + 1
    oob = is_leaf & (lfirst + lcnt > nt)
    for i, c in zip(*np.nonzero(oob)):
        if len(ck.errors) < 8:
            ck.fail(f"node {i} slot {c}: leaf records [{lfirst[i, c]}, {lfirst[i, c] + lcnt[i, c]}) beyond {nt}")
    lmask = is_leaf & ~oob
    seen = np.zeros(nt, np.int64)
    for k in range(4):
        sel = lmask & (lcnt > k)
        np.add.at(seen, lfirst[sel] + k, 1)
    for r in _first_bad(seen != 1):
        ck.fail(f"triangle record {r} lies in {seen[r]} leaves (want exactly one)")
    inv = empty[:, None, :].repeat(3, axis=1)
    ck.expect((planes[:, :, 0, :][inv] == np.inf).all() and (planes[:, :, 1, :][inv] == -np.inf).all(),
              "an empty slot's box is not inverted (+inf / -inf)")
    if ck.errors:
        ck.done()
    # ---- exact bounds per slot, bottom-up by level (children have larger indices than their parents)
    lo, hi = tri_bounds(recs)
    S = scale_of(lo, hi)
    scale_hi = max(1.0, S * (1 + 1e-6) + 1e-6, float(np.abs(G.cam).max()))
    slo, shi = np.full((n4, 4, 3), np.inf), np.full((n4, 4, 3), -np.inf)
    for k in range(4):
        sel = lmask & (lcnt > k)
        r = np.where(sel, lfirst + k, 0)
        slo = np.where(sel[..., None], np.minimum(slo, lo[r]), slo)
        shi = np.where(sel[..., None], np.maximum(shi, hi[r]), shi)
    parent = np.full(n4, -1, np.int64)
    pi, pc = np.nonzero(is_inner)
    parent[cw[pi, pc]] = pi
    level = np.zeros(n4, np.int64)
    for _ in range(n4):
        nl = np.where(parent >= 0, level[np.maximum(parent, 0)] + 1, 0)
        if np.array_equal(nl, level):
            break
        level = nl
    nlo, nhi = np.full((n4, 3), np.inf), np.full((n4, 3), -np.inf)
    for lv in range(int(level.max()), -1, -1):
        at = np.flatnonzero(level == lv)
        sub = is_inner[at]
        ch = np.where(sub, cw[at], 0)
        slo[at] = np.where(sub[..., None], nlo[ch], slo[at])
        shi[at] = np.where(sub[..., None], nhi[ch], shi[at])
        nlo[at], nhi[at] = slo[at].min(axis=1), shi[at].max(axis=1)
    # ---- planes in world units
    P_lo = planes[:, :, 0, :].transpose(0, 2, 1).reshape(-1, 3)  # [node * 4 + slot][axis]
    P_hi = planes[:, :, 1, :].transpose(0, 2, 1).reshape(-1, 3)
    occ = ~empty.reshape(-1)
    E_lo, E_hi = slo.reshape(-1, 3), shi.reshape(-1, 3)
    where = lambda j: (f"node {j // 4} slot {j % 4} ({'leaf' if is_leaf.reshape(-1)[j] else 'inner'} "
                       f"{cw.reshape(-1)[j]:#x})")
    if half:
        c = fr["c"].astype(np.float64)
        isc = fr["is"].astype(np.float32).astype(np.float64)
        W_lo, W_hi = _upw(c + P_lo * isc), _dn(c + P_hi * isc)  # rounded inwards: containment is checked strictly
        sat = lambda v: np.abs(v) >= 65504.0
        h16 = lambda v: np.spacing(np.float16(np.minimum(np.abs(v), 65000.0))).astype(np.float64)  # (saturated: skipped)
        f32f = lambda v: np.spacing(np.float32(np.minimum(np.abs(v), 3e38))).astype(np.float64)
        slack = lambda v, w: (_f32_tol(w, scale_hi) + (h16(v) * 1.0 + f32f(v)) * isc + np.abs(v) * isc * 2.0 ** -24)
        tol_lo = np.where(sat(P_lo), np.inf, slack(P_lo, W_lo))
        tol_hi = np.where(sat(P_hi), np.inf, slack(P_hi, W_hi))
    else:
        W_lo, W_hi = P_lo, P_hi
        tol_lo, tol_hi = _f32_tol(W_lo, scale_hi), _f32_tol(W_hi, scale_hi)
    ix = np.flatnonzero(occ)
    _containment(ck, lambda i: where(ix[i]), W_lo[ix], W_hi[ix], E_lo[ix], E_hi[ix], S)
    _tightness(ck, lambda i: where(ix[i]), W_lo[ix], W_hi[ix], E_lo[ix], E_hi[ix], tol_lo[ix], tol_hi[ix], scale_hi)
    # ---- records (leaf order) and shading data
    _check_records(ck, "triangle", recs, pmat, G.tri_records(), G.pmat, True)
    ck.expect(bytes(blob[off_mats:off_mats + 48 * len(G.mats)]) == G.mat_records(), "material records differ from the scene's")
    ck.done()
    return dict(n4=n4, half=half, S=S, depth=int(level.max()) + 1)


def check_resident(images, G):
    """`images`: {which: bytes} as rtow_debug_image returns them (empty = not resident).  Checks every resident one;
    returns {which: info}."""
    out = {}
    if images.get(0):
        out[0] = check_bvh2(images[0], G)
        if images.get(2):
            check_bvh2_f32(images[2], images[0], G)
            out[2] = True
    if images.get(1):
        out[1] = check_grid(images[1], G)
        if images.get(3):
            check_grid_f32(images[3], images[1], G)
            out[3] = True
    if images.get(4):
        out[4] = check_bvh4(images[4], images.get(5, b""), G)
    return out


# ---- scenes for the tests: triangle meshes with exact binary64 coordinates -----------------------------------------
LAMBERTIAN_GREY = (MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 1.5)


def mesh_geometry(tris, cam=(1.0, 0.0, -1.0), mats=(LAMBERTIAN_GREY,)):
    """[n][3][3] vertices -> a triangle-only Geometry (material i % len(mats) for triangle i)."""
    t = np.ascontiguousarray(np.asarray(tris, np.float64).reshape(-1, 9))
    return Geometry(np.zeros((0, 4)), np.zeros((0, 8)), t, np.arange(len(t)) % len(mats), mats, cam)


def unit_mesh(n, seed):
    """n small triangles in the unit cube (0..1 on every axis)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 0.95, size=(n, 1, 3))
    return c + rng.uniform(-0.05, 0.05, size=(n, 3, 3))


def sheet_stack(layers, m, seed):
    """[layers * 2 m^2][3][3]: wavy sheets z = 0.1 k + 0.03 sin(5 x + phi_k) cos(4 y + psi_k), k = 0 .. layers - 1, over
    the unit square, each an m x m grid of two triangles per cell wound so n_z < 0: a ray along +z meets the front of
    every sheet, one hit per sheet (deep first-k-hits sequences)."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, m + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    out = []
    for k in range(layers):
        phi, psi = rng.uniform(0, 2 * np.pi, 2)
        v = np.stack([x, y, 0.1 * k + 0.03 * np.sin(5 * x + phi) * np.cos(4 * y + psi)], axis=-1)
        p00, p10, p01, p11 = v[:-1, :-1], v[1:, :-1], v[:-1, 1:], v[1:, 1:]
        # (B - A) x (C - A) along -z: A, then the +y neighbour, then the +x neighbour
        out.append(np.stack([p00, p01, p10], axis=-2).reshape(-1, 3, 3))
        out.append(np.stack([p11, p10, p01], axis=-2).reshape(-1, 3, 3))
    return np.concatenate(out)


def edge_meshes():
    """name -> [n][3][3]: the shapes where builders and emitters go wrong."""
    rng = np.random.default_rng(7)
    out = {f"n{n}": unit_mesh(n, n) for n in (1, 2, 3, 4, 5, 8, 9, 17, 65)}
    one = unit_mesh(1, 3)
    out["coincident"] = np.repeat(one, 40, axis=0)
    p = rng.uniform(0, 1, size=(60, 1, 3))
    d = rng.uniform(-0.2, 0.2, size=(60, 1, 3))
    collinear = np.concatenate([p, p + d, p + 2.5 * d], axis=1)
    point = np.repeat(rng.uniform(0, 1, size=(30, 1, 3)), 3, axis=1)
    out["zero_area"] = np.concatenate([collinear, point, unit_mesh(20, 11)])
    flat = unit_mesh(2100, 5) * [40.0, 30.0, 1.0]
    flat[:, :, 2] = 0.375
    out["flat_z"] = flat
    out["off_1e4"] = unit_mesh(2100, 6) + [1e4, -1e4, 1e4]
    out["off_1e5"] = unit_mesh(2100, 8) + [1e5, 1e5, -1e5]
    big = np.array([[[-5e3, 0.0, -5e3], [5e3, 0.5, -5e3], [0.0, 1.0, 5e3]]])
    out["big_and_small"] = np.concatenate([big, unit_mesh(2000, 9)])
    return out


def sphere_geometry(sph=(), mov=(), cam=(13.0, 2.0, 3.0)):
    """Spheres [n][4] (c, r) and moving spheres [n][8] (c0, c1, r, 0), one Lambertian material."""
    s, m = np.asarray(sph, np.float64).reshape(-1, 4), np.asarray(mov, np.float64).reshape(-1, 8)
    return Geometry(s, m, np.zeros((0, 9)), np.zeros(len(s) + len(m), np.int32), (LAMBERTIAN_GREY,), cam)


def sphere_edge_scenes():
    rng = np.random.default_rng(12)
    c = rng.uniform(-3, 3, size=(40, 3)) * [1, 0.3, 1]
    neg = np.concatenate([c, rng.uniform(0.1, 0.5, size=(40, 1)) * rng.choice([-1, 1], size=(40, 1))], axis=1)
    neg = np.concatenate([[[0, -1000, 0, -1000.0]], neg])  # a hollow ground sphere among small spheres
    same = np.tile([[0.25, 1.0, -0.5, 0.0]], (24, 1))
    same[:, 3] = np.linspace(0.1, 1.2, 24)
    mov = np.zeros((30, 8))
    mov[:, :3] = rng.uniform(-1, 1, size=(30, 3))
    mov[:, 3:6] = mov[:, :3] + rng.uniform(-40, 40, size=(30, 3))  # displacements far larger than the scene
    mov[:, 6] = rng.uniform(0.05, 0.3, size=30)
    return {"negative_radius": sphere_geometry(neg), "same_centre": sphere_geometry(same),
            "far_moving": sphere_geometry(np.c_[c[:10], np.full(10, 0.2)], mov)}


# ---- corrupted copies (the tests prove the checker rejects each) ---------------------------------------------------
def _f32_inward(x, lo_side):
    """The binary32 value nearest to x on the inner side (>= x for a lo plane, <= x for a hi plane)."""
    v = np.float32(x)
    if lo_side and float(v) < x:
        v = np.nextafter(v, np.float32(np.inf))
    if not lo_side and float(v) > x:
        v = np.nextafter(v, np.float32(-np.inf))
    return v


def bvh2_plane_inward(blob, G):
    """The lo x plane of the first one-primitive leaf moved onto the primitive's exact bound."""
    P = parse_bvh2(blob, G)
    nodes = P["nodes"][:P["n"]]
    lo, _ = record_bounds(P["sph"], P["mov"], P["tri"])
    i = int(np.flatnonzero((nodes["leaf"] & 7) == 1)[0])
    prim = int(P["ids"][nodes["leaf"][i] >> 3])
    out = bytearray(blob)
    out[i * 32:i * 32 + 4] = _f32_inward(lo[prim, 0], True).tobytes()
    return bytes(out), i


def bvh2_leaf_count(blob, G, delta):
    """delta = +1: the first leaf that can grow takes the next id too (a duplicated id); -1: the first leaf of two or
    more ids loses its last (a dropped id)."""
    P = parse_bvh2(blob, G)
    leaf = P["nodes"]["leaf"][:P["n"]].astype(np.int64)
    first, cnt = leaf >> 3, leaf & 7
    ok = (cnt >= 1) & ((cnt < 7) & (first + cnt < G.np) if delta > 0 else (cnt >= 2))
    i = int(np.flatnonzero(ok)[0])
    out = bytearray(blob)
    out[i * 32 + 28:i * 32 + 32] = np.uint32(leaf[i] + delta).tobytes()
    return bytes(out), i


def _bvh4_parts(blob, frame_rec, G):
    half = bool(parse_frame(frame_rec)["half"])
    nb = 64 if half else 128
    n4 = (len(blob) - 96 * G.nt - _up16(4 * G.nt) - 48 * len(G.mats)) // nb
    return half, nb, n4


def bvh4_child_backwards(blob, frame_rec, G):
    """The first inner child link of the first node after the root that has one, pointed at the root."""
    half, nb, n4 = _bvh4_parts(blob, frame_rec, G)
    co = 48 if half else 96
    cw = np.frombuffer(blob, np.uint8, n4 * nb).reshape(n4, nb)[:, co:co + 16].copy().view("<u4")
    inner = (cw != KREF_NONE) & ((cw & KREF_LEAF) == 0)
    i, c = (int(x[0]) for x in np.nonzero(inner[1:]))
    i += 1
    out = bytearray(blob)
    out[i * nb + co + 4 * c:i * nb + co + 4 * c + 4] = np.uint32(0).tobytes()
    return bytes(out), i


def bvh4_plane_inward(blob, frame_rec, G):
    """A leaf slot's lo x plane moved inwards past the margin: binary32 nodes onto the exact bound of its records;
    binary16 nodes by ONE binary16 step, at the first leaf slot where that step crosses the margin."""
    half, nb, n4 = _bvh4_parts(blob, frame_rec, G)
    co = 48 if half else 96
    raw = np.frombuffer(blob, np.uint8, n4 * nb).reshape(n4, nb)
    cw = raw[:, co:co + 16].copy().view("<u4").astype(np.int64)
    recs = np.frombuffer(blob, np.float64, 12 * G.nt, n4 * nb).reshape(G.nt, 12)
    lo, _ = tri_bounds(recs)
    S = scale_of(*tri_bounds(recs))
    fr = parse_frame(frame_rec)
    out = bytearray(blob)
    for i, c in zip(*np.nonzero((cw != KREF_NONE) & ((cw & KREF_LEAF) != 0))):
        f, k = (cw[i, c] & (KREF_LEAF - 1)) >> 2, (cw[i, c] & 3) + 1
        e = lo[f:f + k, 0].min()
        if not half:
            off = i * nb + 4 * c  # lo.x[c]
            out[off:off + 4] = _f32_inward(e, True).tobytes()
            return bytes(out), (int(i), int(c))
        off = i * nb + 2 * c
        h = np.frombuffer(blob, "<f2", 1, off)[0]
        if not np.isfinite(h):
            continue
        h2 = np.nextafter(h, np.float16(np.inf))
        if float(fr["c"][0]) + float(h2) * float(fr["is"][0]) > e - MARGIN * S:
            out[off:off + 2] = np.float16(h2).tobytes()
            return bytes(out), (int(i), int(c))
    raise AssertionError("no binary16 plane that one step moves past the margin")


def grid_drop_one(blob, G):
    """The last id of the first non-empty cell removed (its count decremented)."""
    P = parse_grid(blob, G)
    cells = np.frombuffer(blob, np.uint32, P["ncell"], P["off_cells"])
    c = int(np.flatnonzero(cells & 255)[0])
    out = bytearray(blob)
    off = P["off_cells"] + 4 * c
    out[off:off + 4] = np.uint32(cells[c] - 1).tobytes()
    return bytes(out), c


def image32_swap_records(blob32, blob64, G):
    """Two binary32 triangle (or sphere) records of different content swapped in a BVH image of the f32 build."""
    pre = parse_bvh2(blob64, G)["off_sph"]
    if G.nt >= 2:
        off, w, n = pre + 32 * G.ns + 64 * G.nm, 48, G.nt
    else:
        off, w, n = _up16(pre + 32 * G.ns + 64 * G.nm + 48 * G.nt), 16, G.ns
    recs = [blob32[off + w * i:off + w * (i + 1)] for i in range(n)]
    j = next(j for j in range(1, n) if recs[j] != recs[0])
    out = bytearray(blob32)
    out[off:off + w], out[off + w * j:off + w * (j + 1)] = recs[j], recs[0]
    return bytes(out), j
