#!/usr/bin/env python3
"""Throughput of the closest-hit query kernel alone (rtow_intersect_device): the walk without the render's new-ray
stage, on three ray sets of >= 8 M rays per scene:
   primary  camera rays of the scene's camera (pinhole, pixel centres), computed in numpy, in pixel order;
   logged   every segment of a small single-threaded oracle render (orc_set_raylog), tiled;
   random   origins uniform in the scene's box (the box of its small primitives), directions uniform on the sphere.
Per scene, set and kernel: Grays/s from the query kernel's HIP events (stats.kernel_ms, best of the repeats) and from a
host clock around `repeats` back-to-back calls closed by one synchronising call; beside them the render's own segments
per second (stats.segments / kernel_ms of one frame, AUTO kernel).  The bytes model: 64 B in + 72 B out per ray.

   python scripts/bench_query.py [--rays 8388608] [--precision fast|strict] [--scenes cover,moving,suzanne,mesh96k]
                                 [--repeats 5] [--json OUT]
"""
import argparse
import json
import math
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402  (device buffers; torch's runtime is loaded before librtow's, see rtow.lib)
import rtow  # noqa: E402
import orc  # noqa: E402

KERNELS = {"brute": rtow.KERNEL_BRUTE, "bvh": rtow.KERNEL_BVH, "grid": rtow.KERNEL_GRID, "bvh4": rtow.KERNEL_BVH4,
           "reftree": rtow.KERNEL_REFTREE}


def scene_of(name, tmpdir):
    if name in ("cover", "moving"):
        return rtow.HostScene.cover(11, 1.5, name == "moving"), 1.5
    if name == "suzanne":
        return rtow.HostScene.obj(ROOT / "tests/golden/suzanne.obj", 16 / 9), 16 / 9
    obj = Path(tmpdir) / "m10.obj"
    subprocess.run([sys.executable, str(ROOT / "scripts/make_mesh.py"), str(obj), "10"], check=True, capture_output=True)
    return rtow.HostScene.obj(obj, 16 / 9), 16 / 9


def primary_rays(scene, aspect, n):
    """Camera::get_ray at pixel centres without the lens (src/common-model.cpp:156-167), rows from the top."""
    cam = scene.c.camera
    H = max(2, int(math.sqrt(n / aspect)))
    W = -(-n // H)
    j = np.arange(W, dtype=np.float64)
    i = np.arange(H, dtype=np.float64)
    u = (j + 0.5) / (W - 1)
    v = ((H - 1 - i) + 0.5) / (H - 1)
    llc, hor, ver, org = (np.array(x[:]) for x in (cam.lower_left_corner, cam.horizontal, cam.vertical, cam.origin))
    d = llc[None, None, :] + u[None, :, None] * hor[None, None, :] + v[:, None, None] * ver[None, None, :] - org
    r = np.empty(W * H, dtype=rtow.RAY_DTYPE)
    r["origin"] = org
    r["direction"] = d.reshape(-1, 3)
    r["time"] = cam.t0
    r["tmax"] = np.inf
    return r[:n]


def logged_rays(name, scene, n):
    """The segments of a small oracle render, tiled to n."""
    mesh = name == "mesh96k"
    cfg = rtow.make_config(64 if mesh else 120, 36 if mesh else 80, 2 if mesh else 4, 1, 20 if name != "cover" and
                           name != "moving" else 50, seed=31, precision=rtow.F64_STRICT)
    import ctypes as C

    cap = 1_500_000
    buf = np.zeros((cap, 12))
    L = orc.lib()
    pd = C.POINTER(C.c_double)
    L.orc_set_raylog.argtypes = [pd, C.c_uint64]
    L.orc_set_raylog.restype = None
    L.orc_raylog_count.restype = C.c_uint64
    L.orc_set_raylog(buf.ctypes.data_as(pd), cap)
    try:
        orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=1, accel=mesh)
        k = int(L.orc_raylog_count())
    finally:
        L.orc_set_raylog(None, 0)
    log = np.tile(buf[:k], (-(-n // k), 1))[:n]
    r = np.empty(n, dtype=rtow.RAY_DTYPE)
    r["origin"], r["direction"], r["time"], r["tmax"] = log[:, 3:6], log[:, 6:9], log[:, 9], np.inf
    return r


def random_rays(scene, n, seed=7):
    a = orc.scene_arrays(scene.c)
    pts = []
    sph = a["sphere_geom"].reshape(-1, 4)
    small = sph[np.abs(sph[:, 3]) < 100.0]  # (not the cover scene's ground sphere)
    pts += [small[:, :3] - np.abs(small[:, 3:4]), small[:, :3] + np.abs(small[:, 3:4])]
    mov = a["moving_geom"].reshape(-1, 8)
    pts += [mov[:, 0:3] - mov[:, 6:7], mov[:, 3:6] + mov[:, 6:7]]
    pts.append(a["triangle_geom"].reshape(-1, 3))
    pts = np.concatenate([p for p in pts if len(p)])
    lo, hi = pts.min(0), pts.max(0)
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    r = np.empty(n, dtype=rtow.RAY_DTYPE)
    r["origin"] = lo + (hi - lo) * g.random((n, 3))
    r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r["time"] = g.random(n)
    r["tmax"] = np.inf
    return r


def render_segments_per_s(ctx, name, aspect):
    W = 480 if name in ("cover", "moving") else 640
    H = rtow.image_height(W, aspect)
    spp = 16
    cfg = rtow.make_config(W, H, spp, 2, 50 if name in ("cover", "moving") else 20, seed=1, precision=rtow.F64_FAST)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(cfg, out.data_ptr(), 0, True)
    best = None
    for _ in range(3):
        st = ctx.render_device(cfg, out.data_ptr(), 0, True)
        rate = st.segments / (st.kernel_ms * 1e-3) / 1e9
        best = rate if best is None else max(best, rate)
    return best, st.kernel_used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8 << 20)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--kernels", default="", help="comma list (default: grid,bvh for sphere scenes, bvh4,bvh for meshes)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    prec = rtow.F64_FAST if a.precision == "fast" else rtow.F64_STRICT
    n = a.rays
    ctx = rtow.Context(0)
    rows = []
    d_hits = torch.empty(n * 72, dtype=torch.uint8, device="cuda")
    print(f"# {n} rays per set, precision {a.precision}; Grays/s kernel-event (best of {a.repeats}) | end-to-end host "
          f"clock ({a.repeats} calls + 1 synchronising) | node / prim tests per ray | render segments/s (AUTO, event)")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            render_rate, render_kernel = render_segments_per_s(ctx, name, aspect)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            kernels = a.kernels.split(",") if a.kernels else (["bvh4", "bvh"] if mesh else ["grid", "bvh"])
            sets = {"primary": primary_rays(scene, aspect, n), "logged": logged_rays(name, scene, n),
                    "random": random_rays(scene, n)}
            for set_name, rays in sets.items():
                d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda")
                for kn in kernels:
                    k = KERNELS[kn]
                    for _ in range(a.warmup):
                        st = ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True)
                    ev = []
                    for _ in range(a.repeats):
                        st = ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True)
                        ev.append(st.kernel_ms)
                    t0 = time.perf_counter()
                    for _ in range(a.repeats):
                        ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, False)
                    st = ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True)
                    e2e_ms = (time.perf_counter() - t0) * 1e3 / (a.repeats + 1)
                    hits = d_hits[: min(n, 1 << 20) * 72].cpu().numpy().view(rtow.HIT_DTYPE)
                    row = dict(scene=name, set=set_name, kernel=kn, kernel_used=int(st.kernel_used), rays=n,
                               kernel_ms=min(ev), e2e_ms=e2e_ms, grays_event=n / min(ev) / 1e6,
                               grays_e2e=n / e2e_ms / 1e6, node_per_ray=st.node_tests / n, prim_per_ray=st.prim_tests / n,
                               hit_frac=float(np.isfinite(hits["t"]).mean()), render_gsegs=render_rate,
                               render_kernel=int(render_kernel))
                    rows.append(row)
                    print(f"{name:8s} {set_name:8s} {kn:5s}(ran {row['kernel_used']}) "
                          f"{row['grays_event']:7.3f} Grays/s event | {row['grays_e2e']:7.3f} end-to-end | "
                          f"{row['node_per_ray']:6.1f} nodes {row['prim_per_ray']:6.1f} prims/ray | hits {row['hit_frac']:.3f} | "
                          f"render {render_rate:6.3f} Gseg/s (kernel {render_kernel})", flush=True)
                del d_rays
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
