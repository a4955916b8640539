#!/usr/bin/env python3
"""In-place refit (rtow_scene_refit) against a fresh rtow_scene_upload, per scene.

   cost   one refit of the next frame of a deformation (host wall time of the call and the device time of its kernels and
          copies, rtow_refit_info) against rtow_scene_upload of the same scene with the host builder and with the device
          builder (host wall time of the call, synchronised); medians of `repeats` after `warmup`.
   walk   16 frames of a travelling sine wave along x (y displaced by 5 % of the extent), refitted one after another; then
          the closest-hit query (rtow_intersect_device, fast build, AUTO strategy) on primary rays: Grays/s from the kernel's
          HIP events (best of `repeats`) and node tests per ray, against a fresh upload (host builder) of the last frame.
          bvh_area_ratio (rtow_refit_info) is reported beside them.

   python scripts/bench_refit.py [--scenes moving,suzanne,mesh96k] [--rays 4194304] [--warmup 2] [--repeats 7] [--json OUT]
"""
import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import primary_rays, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
import orc  # noqa: E402


class Frames:
    """The scene's geometry under the wave, frame by frame: rtow.Scene structs sharing everything but the geometry."""

    def __init__(self, scene):
        self.base = scene
        a = orc.scene_arrays(scene.c)
        self.sph = a["sphere_geom"].reshape(-1, 4).copy()
        self.mov = a["moving_geom"].reshape(-1, 8).copy()
        self.tri = a["triangle_geom"].reshape(-1, 9).copy()
        small = self.sph[np.abs(self.sph[:, 3]) < 100.0]  # (the wave spans the small primitives, not a ground sphere)
        pts = [small[:, :3], self.mov[:, :3], self.mov[:, 3:6]] + [self.tri[:, 3 * v:3 * v + 3] for v in range(3)]
        pts = np.concatenate([p for p in pts if len(p)])
        self.lo, self.ext = pts.min(0), float(np.max(pts.max(0) - pts.min(0)))
        self.keep = []

    def scene(self, frame, frames=16, amp=0.05):
        def f(p):
            ph = 2 * np.pi * frame / frames
            q = p.copy()
            q[:, 1] += amp * self.ext * np.sin(2 * np.pi * (p[:, 0] - self.lo[0]) / self.ext + ph) * (frame > 0)
            return q
        ground = np.abs(self.sph[:, 3]) >= 100.0
        s = self.sph.copy()
        s[~ground, :3] = f(self.sph[~ground, :3])
        m = self.mov.copy()
        m[:, 0:3], m[:, 3:6] = f(self.mov[:, 0:3]), f(self.mov[:, 3:6])
        t = self.tri.copy()
        for v in range(3):
            t[:, 3 * v:3 * v + 3] = f(self.tri[:, 3 * v:3 * v + 3])
        sc = rtow.Scene.from_buffer_copy(self.base.c)  # (counts, materials, camera, insertion order)
        dp = C.POINTER(C.c_double)
        arrs = [np.ascontiguousarray(x) for x in (s, m, t)]
        sc.sphere_geom, sc.moving_geom, sc.triangle_geom = (x.ctypes.data_as(dp) for x in arrs)
        self.keep = (self.keep + [arrs])[-4:]
        return sc


def median(xs):
    return float(np.median(np.asarray(xs)))


def query_rate(ctx, d_rays, n, d_hits, repeats):
    best, nodes = 0.0, 0.0
    for _ in range(repeats):
        st = ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST, rtow.KERNEL_AUTO, want_stats=True)
        best = max(best, n / (st.kernel_ms * 1e-3) / 1e9)
        nodes = st.node_tests / n
        kernel = st.kernel_used
    return best, nodes, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="moving,suzanne,mesh96k")
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []
    ctx = rtow.Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            fr = Frames(scene)
            row = {"scene": name, "prims": scene.c.n_prims}
            # ---- cost: upload (both builders) against refit
            for bname, b in (("host", rtow.BUILDER_HOST_SAH), ("device", rtow.BUILDER_DEVICE_LBVH)):
                ctx.set_builder(b)
                ts = []
                for i in range(a.warmup + a.repeats):
                    sc = fr.scene(i % 16)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.upload(sc)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                row[f"upload_{bname}_ms"] = median(ts[a.warmup:])
            ctx.set_builder(rtow.BUILDER_HOST_SAH)
            ctx.upload(fr.scene(0))
            host_ms, dev_ms, wall_ms = [], [], []
            for i in range(1, a.warmup + a.repeats + 1):
                sc = fr.scene(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.refit(sc)
                ri = ctx.refit_info()
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                host_ms.append(ri.refit_ms)
                dev_ms.append(ri.device_ms)
            row["refit_ms"] = median(host_ms[a.warmup:])
            row["refit_device_ms"] = median(dev_ms[a.warmup:])
            row["refit_synced_ms"] = median(wall_ms[a.warmup:])
            # ---- walk: 16 refitted frames against a fresh upload of the last one
            rays = primary_rays(scene, aspect, a.rays)
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
            d_hits = torch.empty(len(rays) * 72, dtype=torch.uint8, device="cuda:0")
            ctx.upload(fr.scene(0))
            for f in range(1, 17):
                last = fr.scene(f)
                ctx.refit(last)
            ri = ctx.refit_info()
            query_rate(ctx, d_rays, len(rays), d_hits, a.warmup)
            r_gr, r_nodes, r_k = query_rate(ctx, d_rays, len(rays), d_hits, a.repeats)
            ctx.upload(last)
            query_rate(ctx, d_rays, len(rays), d_hits, a.warmup)
            u_gr, u_nodes, u_k = query_rate(ctx, d_rays, len(rays), d_hits, a.repeats)
            row.update({"kernel": r_k, "kernel_fresh": u_k, "refit_grays": r_gr, "fresh_grays": u_gr,
                        "refit_nodes_per_ray": r_nodes, "fresh_nodes_per_ray": u_nodes,
                        "bvh_area_ratio": ri.bvh_area_ratio, "grid_resident": ri.grid_resident})
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    if a.json:
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
