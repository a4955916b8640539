"""Digests of the resident scene images, for pinning the host code that makes them resident (rtow_scene.cpp).

A helper for tests/test_gpu_scene_image_digests.py, also runnable as a module (`python tests/scene_digests.py
[OUT.json]` prints / writes what `record()` returns).  `record()` builds a fixed list of small scenes, makes each
resident by every route and with both builders, and returns per (scene, builder, route) the SHA-256 of every image
rtow_debug_image returns and the integer fields of rtow_build_info.  No timing is recorded: the values are a pure
function of the library, so a change that is meant to leave every image byte-identical compares equal, with no
tolerance, to tests/golden/scene_image_digests.json recorded before it.

Scenes (the smallest that reach each branch of the upload; all under 2,000 primitives):
  mixed           spheres (one hollow: negative radius), moving spheres and triangles; takes a grid (plain id lists)
  spheres_fat     spheres only, few: the grid has fat cell lists
  spheres_plain   spheres only, many: the image with fat lists would not fit LDS, plain id lists
  spheres_nogrid  seventy large spheres among a hundred and two tiny ones: the grid is refused (more than 64 large primitives)
  suzanne         968 triangles: the 4-wide image is staged whole, binary32 planes (128-byte nodes)
  mesh1400        unit_mesh just past the LDS limit: binary16 planes (64-byte nodes, b4_half = 1)
  tri1, tri2      meshes of one and of two triangles
Every other scene has a multiple of four primitives (see _resident).
Routes:
  upload          rtow_scene_upload: everything
  refit           that upload, then rtow_scene_refit with every centre / vertex displaced by a seeded 2 % of the extent
  render_grid, render_bvh, render_bvh4, render_f32
                  the lean upload of a 2x2-pixel, 1-spp rtow_render with that kernel (fast build) / with RTOW_F32: each
                  `need` mask of upload_for and both of its retries (no grid: spheres_nogrid; no 4-wide image: suzanne
                  under RTOW_BVH_LEAF=5, below)
  and, for suzanne only, all of the above again under RTOW_NO_LEAF_ORDER, under RTOW_NO_BVH4 and under RTOW_BVH_LEAF=5
  (leaves too large for the 4-wide format), each in a fresh child process (the knobs are read when a context is created).
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

import conftest  # noqa: F401  (the import paths of the package and the tests)
import accel_images as ai
import rtow
from support_scenes import random_scene, suzanne_tris, to_scene
from support_tables import BUILDERS

KNOBS = {"RTOW_NO_LEAF_ORDER": "1", "RTOW_NO_BVH4": "1", "RTOW_BVH_LEAF": "5"}
BUILD_INFO_INTS = ("builder", "bvh_nodes", "bvh_image_bytes", "grid_image_bytes", "bvh4_nodes", "bvh4_image_bytes",
                   "bvh4_node_bytes")
RENDERS = {"render_grid": dict(kernel=rtow.KERNEL_GRID), "render_bvh": dict(kernel=rtow.KERNEL_BVH),
           "render_bvh4": dict(kernel=rtow.KERNEL_BVH4), "render_f32": dict(precision=rtow.F32)}


def _mixed():
    keep = []
    G = ai.Geometry.of_scene(random_scene(57, 23, 6, 10, keep))
    G.sph[3, 3] = -G.sph[3, 3]  # a hollow sphere
    return G


def _spheres_fat():
    keep = []
    return ai.Geometry.of_scene(random_scene(47, 31, 0, 0, keep))


def _spheres_plain():
    rng = np.random.default_rng(21)
    c = rng.uniform(-6, 6, size=(1500, 3)) * [1, 0.05, 1] + [0, 0.2, 0]
    return ai.sphere_geometry(np.c_[c, np.full(1500, 0.08)])


def _spheres_nogrid():
    # (the shape of test_gpu_device_build's test_device_grid_build_falls_back_like_the_host, with enough tiny spheres
    # that the median is one of them)
    rng = np.random.default_rng(1)
    geom = np.zeros((172, 4))
    geom[:, :3] = rng.uniform(-3, 3, size=(172, 3))
    geom[:102, 3] = 0.01
    geom[102:, 3] = 1.5
    return ai.sphere_geometry(geom)


SCENES = {
    "mixed": _mixed, "spheres_fat": _spheres_fat, "spheres_plain": _spheres_plain, "spheres_nogrid": _spheres_nogrid,
    "suzanne": lambda: ai.mesh_geometry(suzanne_tris(1)), "mesh1400": lambda: ai.mesh_geometry(ai.unit_mesh(1400, 5)),
    "tri1": lambda: ai.mesh_geometry(ai.unit_mesh(1, 1)), "tri2": lambda: ai.mesh_geometry(ai.unit_mesh(2, 2)),
}


def displaced(G, seed=9, amount=0.02):
    """A copy of G with every sphere centre, both ends of every moving sphere and every vertex moved by up to `amount`
    of the scene's extent along each axis."""
    H = ai.Geometry(G.sph.copy(), G.mov.copy(), G.tri.copy(), G.pmat.copy(), list(G.mats), G.cam.copy())
    parts = [H.sph[:, 0:3], H.mov[:, 0:3], H.mov[:, 3:6]] + [H.tri[:, 3 * v:3 * v + 3] for v in range(3)]
    pts = np.concatenate([p for p in parts if len(p)])
    ext = float(max(np.max(pts.max(0) - pts.min(0)), 1e-3))
    rng = np.random.default_rng(seed)
    for p in parts:
        p += rng.uniform(-amount, amount, size=p.shape) * ext
    return H


def _resident(ctx, which, G):
    bi = ctx.build_info()
    # The device builder writes every section of its binary BVH image but not the alignment gap behind the material
    # indices (4 bytes per primitive, sections 16-byte aligned): those bytes are whatever the allocation held, so image 0
    # of a device build is compared only where there is no gap.  The scenes above have a multiple of four primitives,
    # except tri1 and tri2, which cannot.  (The host builder's image is zeroed whole; so are all other images.)
    if bi.builder == rtow.BUILDER_DEVICE_LBVH and G.np % 4:
        which = [w for w in which if w != 0]
    return {"images": {str(w): hashlib.sha256(ctx.debug_image(w)).hexdigest() for w in which},
            "build_info": {f: int(getattr(bi, f)) for f in BUILD_INFO_INTS}}


def _check_branch(name, ctx, G):
    """The branch the scene is in the list for (on the full upload)."""
    bi = ctx.build_info()
    grid = ctx.debug_image(1)
    if name in ("mixed", "spheres_fat", "spheres_plain"):
        assert grid, f"{name}: no grid image"
        fat = ai.parse_grid(grid, G)["off_fat"] != 0
        assert fat == (name == "spheres_fat"), f"{name}: fat lists {fat}"
    if name == "spheres_nogrid":
        assert not grid and bi.grid_image_bytes == 0, f"{name}: the grid was not refused"
    if name in ("suzanne", "mesh1400") and not (os.environ.get("RTOW_NO_BVH4") or os.environ.get("RTOW_BVH_LEAF")):
        assert bi.bvh4_node_bytes == (128 if name == "suzanne" else 64), f"{name}: {bi.bvh4_node_bytes}-byte nodes"


def record_scene(name):
    """{"<name>/<builder>/<route>": {"images": {which: sha256}, "build_info": {field: int}}} for one scene."""
    out = {}
    keep = []
    G = SCENES[name]()
    sc, moved = to_scene(G, keep), to_scene(displaced(G), keep)
    for bname, builder in BUILDERS.items():
        ctx = rtow.Context(0)
        try:
            ctx.set_builder(builder)
            ctx.upload(sc)
            _check_branch(name, ctx, G)
            out[f"{name}/{bname}/upload"] = _resident(ctx, range(6), G)
            ctx.refit(moved)
            out[f"{name}/{bname}/refit"] = _resident(ctx, range(6), G)
            out[f"{name}/{bname}/refit"]["grid_resident"] = int(ctx.refit_info().grid_resident)
            for route, kw in RENDERS.items():
                ctx.render(sc, rtow.make_config(2, 2, 1, 1, 4, seed=3, **kw))
                # (a lean upload without RTOW_F32 leaves no binary32 image: 2 and 3 are read only where they are built)
                out[f"{name}/{bname}/{route}"] = _resident(ctx, range(6) if route == "render_f32" else (0, 1, 4, 5), G)
        finally:
            ctx.close()
    return out


def record():
    out = {}
    for name in SCENES:
        out.update(record_scene(name))
    for knob, value in KNOBS.items():
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--scene", "suzanne"], capture_output=True,
                           text=True, env={**os.environ, knob: value})
        assert r.returncode == 0, (knob, r.stdout[-500:], r.stderr[-2000:])
        out.update({f"{knob}/{k}": v for k, v in json.loads(r.stdout).items()})
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    got = record_scene(args[1]) if args[:1] == ["--scene"] else record()
    text = json.dumps(got, indent=1, sort_keys=True) + "\n"
    if args and args[0] != "--scene":
        Path(args[0]).write_text(text)
    else:
        sys.stdout.write(text)
