"""The cases of the closest-point checkers (test_gpu_point_query.py, test_gpu_exact_points.py and the host self-tests in
test_point_query_host.py): the point sets of a scene, the small scenes by name with their records, and the bit-for-bit
comparison of strict answers with the mirror (point_ref.py).  Importing this module loads no library."""
import math

import numpy as np

import accel_images as ai
import point_ref as pr
import rtow
from support_oracle import LOGGED, same_bits
from support_scenes import SceneView, handmade_scene, scene_of
from support_tables import WALKS

KERNELS = dict(WALKS, auto=rtow.KERNEL_AUTO)
EDGE_MESHES = ["n4", "coincident", "zero_area", "flat_z", "off_1e4", "off_1e5", "big_and_small"]
SPHERE_SCENES = ["negative_radius", "same_centre", "far_moving"]
REFITS = [(n, m) for n in ("cover_moving", "suzanne") for m in ("translate", "scale1000", "flatten")]
SEED = 41


def extent_box(rec):
    pts = [rec.tri[:, 0:3], rec.tri[:, 0:3] + rec.tri[:, 3:6], rec.tri[:, 0:3] + rec.tri[:, 6:9]]
    small = rec.sph[np.sqrt(np.abs(rec.sph[:, 3])) < 100.0]
    if len(small):
        r = np.sqrt(np.abs(small[:, 3:4]))
        pts += [small[:, 0:3] - r, small[:, 0:3] + r]
    if rec.nm:
        r = np.abs(rec.mov[:, 7:8])
        pts += [rec.mov[:, 0:3] - r, rec.mov[:, 0:3] + rec.mov[:, 3:6] + r]
    pts = np.concatenate([p for p in pts if len(p)])
    return pts.min(0), pts.max(0)


def point_sets(rec, log, n, seed):
    """name -> (points, max_dist): near (logged hit points offset by up to 2 % of the extent, max_dist 5 %), volume (a
    lattice over the box, unbounded) and random (uniform in the box, shuffled, unbounded)."""
    g = np.random.default_rng(seed)
    lo, hi = extent_box(rec)
    ext = float(np.max(hi - lo))
    out = {}
    if log is not None:
        hit = log[np.isfinite(log[:, 10])]
        rows = hit[g.choice(len(hit), size=min(n, len(hit)), replace=False)]
        p = rows[:, 3:6] + rows[:, 10:11] * rows[:, 6:9] + g.uniform(-0.02, 0.02, size=(len(rows), 3)) * ext
        out["near"] = (p, 0.05 * ext)
    k = max(2, round(n ** (1 / 3)))
    ax = [np.linspace(lo[j] - 0.05 * ext, hi[j] + 0.05 * ext, k) for j in range(3)]
    out["volume"] = (np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3), math.inf)
    out["random"] = (g.uniform(lo - 0.05 * ext, hi + 0.05 * ext, size=(n, 3)), math.inf)
    return out


def check_strict(exp, view_mat, hits, what):
    """Strict answers against the mirror's (`exp`: rec, pts, time, md, dmin, ties): dist and point bit for bit, prim one of
    the exactly tied minima, kind and material of that primitive, the miss record."""
    rec = exp.rec
    assert same_bits(hits["dist"], exp.dmin), (what, int((hits["dist"].view(np.uint64) != exp.dmin.view(np.uint64)).sum()))
    miss = ~(exp.md >= exp.dmin)
    assert np.all(hits["prim"][miss] == -1) and np.all(hits["kind"][miss] == -1) and np.all(hits["material"][miss] == -1)
    assert np.all(hits["point"][miss] == 0.0)
    hit = np.nonzero(~miss)[0]
    prim = hits["prim"][hit]
    assert np.all(prim >= 0), what
    cid = rec.ins2cls[prim]
    for j, c in zip(hit, cid):
        assert c in exp.ties[j], (what, j, c, exp.ties[j][:8])
    time = np.broadcast_to(np.asarray(exp.time, dtype=np.float64), (len(exp.pts),))
    d, q = pr.prim_point(rec, cid, exp.pts[hit], time[hit])
    assert same_bits(d, hits["dist"][hit]) and same_bits(q, hits["point"][hit]), what
    assert np.array_equal(rec.kind_of(cid), hits["kind"][hit]), what
    assert np.array_equal(view_mat[prim], hits["material"][hit]), what


def geometry_case(G, keep):
    """(scene to upload, records, material per insertion index) of an accel_images.Geometry (class-major insertion)."""
    return scene_of(G, keep), pr.make_records(G.sph, G.mov, G.tri), G.pmat


def small_case(name, logged, keep):
    """(scene to upload, records, materials, near set or None, random set or None) of a small scene by name."""
    if name == "handmade":
        hs = handmade_scene()
        keep.append(hs)
        view = SceneView(hs)
        return hs.c, pr.records(view), view.prim_mat, None, None
    if name in LOGGED:
        hs, view, log = logged[name]
        rec = pr.records(view)
        sets = point_sets(rec, log, pr.SIZES["mixed"], 7)
        return hs.c, rec, view.prim_mat, sets["near"], sets["random"][0]
    G = ai.mesh_geometry(ai.edge_meshes()[name]) if name in EDGE_MESHES else ai.sphere_edge_scenes()[name]
    return geometry_case(G, keep) + (None, None)
