"""Queue order of the 64-pixel tiles (no GPU): rtow_debug_tile_order, the host arithmetic behind the trace kernels' tile
table.  The classification "empty" must be conservative — no ray the camera can generate through an empty tile reaches a
primitive — the table a permutation of the rank's tiles with the empty ones at its low end (they run last), and every
(level, pixel) item must be issued exactly once by the decode the kernels apply to it.

The brute force is this file's own binary64 closest-hit test in numpy (spheres by the discriminant, triangles by
Moeller-Trumbore), independent of the cones the classification uses."""
import numpy as np
import pytest

import rtow
from conftest import GOLDEN
from support_oracle import tile_order


def _prims(s, times):
    """Spheres (centre, radius) at every shutter time asked for, and the triangles."""
    cen, rad = [], []
    sg = np.array(s.sphere_geom[:4 * s.n_spheres]).reshape(-1, 4)
    cen.append(sg[:, :3]); rad.append(sg[:, 3])
    mg = np.array(s.moving_geom[:8 * s.n_moving]).reshape(-1, 8)
    for t in times:
        cen.append(mg[:, 0:3] + t * (mg[:, 3:6] - mg[:, 0:3])); rad.append(mg[:, 6])
    tri = np.array(s.triangle_geom[:9 * s.n_triangles]).reshape(-1, 3, 3)
    return np.concatenate(cen), np.abs(np.concatenate(rad)), tri


def _any_hit(origins, d0, cen, rad, tri):
    """Does any ray from one of `origins` to a viewport point (origins[0] + d0[i]) touch a primitive at t > 0
    (binary64; touching counts)."""
    if len(tri):
        A, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = np.cross(e1, e2)
    for o in origins:
        d = d0 - (o - origins[0])[None, :]                         # [R, 3]
        if len(cen):
            oc = o[None, :] - cen                                  # [S, 3]
            a = (d * d).sum(1)[:, None]
            hb = d @ oc.T                                          # [R, S]
            cq = ((oc * oc).sum(1) - rad * rad)[None, :]
            if bool(((hb * hb - a * cq >= 0) & ~((hb > 0) & (cq > 0))).any()):
                return True
        if len(tri):
            # Moeller-Trumbore with its triple products turned so that the direction is the outer factor
            tv = o[None, :] - A                                    # [T, 3]
            q = np.cross(tv, e1)
            det = -(d @ n.T)                                       # [R, T]
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                u = -(d @ np.cross(tv, e2).T) * inv
                v = (d @ q.T) * inv
                t = ((q * e2).sum(1))[None, :] * inv
                if bool(((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)).any()):
                    return True
    return False


def _tile_rays(cam, W, H, x0, y0, tw, th):
    """Camera rays through the pixel corners and centres of the tile at column x0, global row y0 — the corners are the
    corners of every pixel's jitter square — from the centre and eight rim points of the lens disk."""
    xs = np.concatenate([x0 + np.arange(tw + 1.0), x0 + np.arange(tw) + 0.5])
    ys = np.concatenate([y0 + np.arange(th + 1.0), y0 + np.arange(th) + 0.5])
    # the kernel's u = (j + ju) / (W - 1), v = (H - 1 - i + jv) / (H - 1) with ju, jv in [0, 1]: x = j + ju, y = i + 1 - jv
    su = (xs / (W - 1))[None, :].repeat(len(ys), 0).ravel()
    sv = ((H - ys) / (H - 1))[:, None].repeat(len(xs), 1).ravel()
    o = np.array(cam.origin[:])
    llc, hor, ver = np.array(cam.lower_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    cu, cv = np.array(cam.u[:]), np.array(cam.v[:])
    P = llc[None] + su[:, None] * hor[None] + sv[:, None] * ver[None]
    ang = np.arange(8) * (np.pi / 4)
    lens = [(0.0, 0.0)] + [(np.cos(a), np.sin(a)) for a in ang]
    origins = [o + cam.lens_radius * (px * cu + py * cv) for px, py in lens]
    return origins, P - o[None]   # (origins[0] is the eye; _any_hit turns the pinhole directions into each lens point's)


def _check_empty_tiles(scene, cfg, tiles, tw, th):
    s = scene.c
    cam = s.camera
    times = (cam.t0, 0.5 * (cam.t0 + cam.t1), cam.t1) if s.n_moving else ()
    cen, rad, tri = _prims(s, times)
    rows = rtow.local_rows(cfg)
    tpr = cfg.image_width >> tw
    for t in tiles:
        tr, tc = divmod(int(t), tpr)
        o, d = _tile_rays(cam, cfg.image_width, cfg.image_height, tc << tw, rows[tr << th], 1 << tw, 1 << th)
        assert not _any_hit(o, d, cen, rad, tri), (int(t), tr, tc)


@pytest.mark.parametrize("moving", [False, True])
def test_empty_tiles_of_the_cover_scene_see_nothing(moving):
    """Cover scene at the benchmark's size: every tile classed empty is checked by brute force — rays through the
    corners and centres of all its pixels, from the centre and the rim of the lens, against every sphere (a moving one
    at the shutter's ends and middle).  Round 4's classification found 13 % of the tiles; below 10 % the widening for
    lens and jitter would be too generous to be worth a queue segment.  The static scene's count is pinned: it is
    what this file's reference computation accepts, tile for tile, and the queue's second segment starts there."""
    scene = rtow.HostScene.cover(11, 1.5, moving)
    W, H = 1200, 800
    cfg = rtow.make_config(W, H, 100, 10, 50)
    table, empty, ne, tw, th = tile_order(scene, cfg)
    assert (tw, th) == (3, 3) and len(table) == (W // 8) * (H // 8)
    assert ne == int(empty.sum())
    print("empty tiles:", ne, "of", len(table))
    assert ne >= 0.10 * len(table)
    if not moving:
        assert ne == 2027
    _check_empty_tiles(scene, cfg, np.flatnonzero(empty), tw, th)
    # and the classification is not vacuous the other way: the ground alone fills the lower half
    assert (~empty).sum() >= 0.5 * len(table)


@pytest.mark.parametrize("scale", [1.0, 0.35])
def test_empty_tiles_of_a_triangle_mesh_see_nothing(scale):
    """suzanne (triangles, by their bounding spheres), as the scene script frames it — the head fills the frame — and
    shrunk about the origin so that sky shows around it: the empty tiles next to a tile that sees the mesh, where a
    wrong bound would show, and every fifth of the others, by brute force against every triangle."""
    scene = rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)
    s = scene.c
    for i in range(9 * s.n_triangles):
        s.triangle_geom[i] *= scale
    W, H = 384, 216
    cfg = rtow.make_config(W, H, 16, 1, 20)
    table, empty, ne, tw, th = tile_order(scene, cfg)
    assert (tw, th) == (3, 3) and len(table) == 48 * 27 and ne < len(table)
    print("empty tiles:", ne, "of", len(table))
    if scale < 1.0:
        assert ne > 0.3 * len(table)
    grid = empty.reshape(27, 48)
    pad = np.pad(~grid, 1)
    near = np.zeros_like(grid)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= pad[dy:dy + 27, dx:dx + 48]
    border = np.flatnonzero((grid & near).ravel())
    rest = np.flatnonzero((grid & ~near).ravel())[::5]
    _check_empty_tiles(scene, cfg, np.concatenate([border, rest]), tw, th)


def test_a_camera_inside_the_geometry_has_no_empty_tile():
    scene = rtow.HostScene.cover(11, 1.5, False)
    s = scene.c
    for k in range(3):  # the ground sphere becomes a ball around the eye
        s.sphere_geom[k] = s.camera.origin[k]
    s.sphere_geom[3] = 5.0
    table, empty, ne, tw, th = tile_order(scene, rtow.make_config(480, 320, 20, 2, 50))
    assert len(table) == 60 * 40 and ne == 0 and not empty.any()
    assert sorted(table) == list(range(len(table)))


def test_small_and_untiled_images():
    """64x48 is 8 x 6 whole tiles; an image whose width no tile shape divides is not tiled and has no table."""
    scene = rtow.HostScene.cover(11, 1.5, False)
    table, empty, ne, tw, th = tile_order(scene, rtow.make_config(64, 48, 8, 2, 50))
    assert len(table) == 48 and sorted(table) == list(range(48)) and ne == int(empty.sum())
    _check_empty_tiles(scene, rtow.make_config(64, 48, 8, 2, 50), np.flatnonzero(empty), tw, th)
    table, empty, ne, tw, th = tile_order(scene, rtow.make_config(100, 50, 8, 2, 50))
    assert len(table) == 0 and (tw, th) == (0, 0)


def _decode(cfg, table, tw, th, nlevels, rows):
    """The kernels' decode of every queue position (rtow_trace_body.h, decode_item): slot and pixel."""
    W = cfg.image_width
    npix = len(rows) * W
    n_items = npix * nlevels
    mine = np.arange(n_items, dtype=np.int64)
    qi = n_items - 1 - mine
    g64, w = qi >> 6, qi & 63
    t, k = g64 // nlevels, g64 % nlevels
    tile = table[t]
    tpr = W >> tw
    tr, tc = tile // tpr, tile % tpr
    j = (tc << tw) + (w & ((1 << tw) - 1))
    lr = (tr << th) + (w >> tw)
    gi = np.array(rows, dtype=np.int64)[lr]
    slot = k * npix + (tile << 6) + w
    return k, slot, gi, j


@pytest.mark.parametrize("nranks,rank", [(1, 0), (2, 1), (3, 2), (8, 3)])
@pytest.mark.parametrize("tile_rows", [4, 8])
@pytest.mark.parametrize("order", ["1", "0"])
def test_table_is_a_permutation_and_every_item_is_issued_once(monkeypatch, nranks, rank, tile_rows, order):
    """For N = 1, 2, 3, 8 and both strip heights: the table is a permutation of the rank's tiles, the empty tiles hold
    its low positions (traced last) and both segments keep the row order — rows below the top band top-down first, the
    top band last — so with the switch off, or no empty tile, the order is the one the queue always had.  Decoding every
    queue position as the kernels do issues each (level, pixel) exactly once, each to its own partial-sum slot."""
    monkeypatch.setenv("RTOW_TILE_ORDER", order)
    scene = rtow.HostScene.cover(11, 1.5, False)
    W, H, nlevels = 480, 320, 3
    cfg = rtow.make_config(W, H, 30, 3, 50, rank=rank, nranks=nranks, tile_rows=tile_rows)
    rows = rtow.local_rows(cfg)
    table, empty, ne, tw, th = tile_order(scene, cfg)
    tpr, ntr = W >> tw, len(rows) >> th
    assert (1 << th) == tile_rows and len(table) == tpr * ntr
    assert sorted(table) == list(range(tpr * ntr))
    sky = ntr // 8
    legacy = np.array([(trq if trq < sky else sky + (ntr - 1 - trq)) * tpr + tc for trq in range(ntr) for tc in range(tpr)])
    if order == "0":
        assert ne == 0 and not empty.any() and np.array_equal(table, legacy)
    else:
        assert ne == int(empty.sum()) and empty[table[:ne]].all() and not empty[table[ne:]].any()
        assert np.array_equal(table[:ne], legacy[empty[legacy]]) and np.array_equal(table[ne:], legacy[~empty[legacy]])
        if nranks == 1:
            assert ne > 0
    k, slot, gi, j = _decode(cfg, table, tw, th, nlevels, rows)
    assert len(np.unique(slot)) == len(slot) == len(rows) * W * nlevels
    issued = (k * H + gi) * W + j
    assert len(np.unique(issued)) == len(issued)
    assert set(np.unique(gi)) == set(rows) and j.min() == 0 and j.max() == W - 1
