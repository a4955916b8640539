#!/usr/bin/env python3
"""The ambient query (rtow_ambient_device) against the any-hit query (rtow_occluded_device) on the very rays it exported,
per scene, point set and strategy: the existing kernel on the same work, fed from memory, is the baseline.

Points: hit points and hit normals (turned to face the arriving ray) of the segments of a small oracle render, seeded;
two sets per scene: `ao` with max_dist = 5 % of the scene's extent and `sky` with max_dist = inf.
Per row: Grays/s of each query from its kernel's HIP events (stats.kernel_ms, best of `repeats` after `warmup`; the worst
beside it), their ratio, the node and primitive tests per ray of each, the open share, and the fused records compared
with the fold of the occlusion bytes (`differ`: points whose `open` is not the count of unoccluded rays — 0 in the
strict build; the fast build's band apart).

   python scripts/bench_ambient.py [--points 131072] [--samples 64] [--precision fast|strict]
                                   [--scenes cover,moving,suzanne,mesh96k] [--kernels grid,bvh] [--warmup 2]
                                   [--repeats 5] [--json OUT]
"""
import argparse
import json
import math
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import KERNELS, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
from bench_occlusion import scene_extent, timed  # noqa: E402
import orc  # noqa: E402


def surface_points(ctx, name, scene, n, seed=41):
    """n seeded (point, normal facing the arriving ray, time) of the resident scene: strict closest hits of the segments
    of a small oracle render."""
    import ctypes as C

    mesh = name == "mesh96k"
    cfg = rtow.make_config(64 if mesh else 120, 36 if mesh else 80, 2 if mesh else 4, 1,
                           50 if name in ("cover", "moving") else 20, seed=31, precision=rtow.F64_STRICT)
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
    log = buf[:k]
    log = log[np.isfinite(log[:, 10])]
    rows = log[np.random.default_rng(seed).integers(0, len(log), n)]
    rays = rtow.make_rays(rows[:, 3:6], rows[:, 6:9], time=rows[:, 9])
    hits = ctx.intersect(rays, rtow.F64_STRICT, rtow.KERNEL_AUTO)
    ok = np.isfinite(hits["t"])
    nrm = hits["normal"][ok]
    away = (nrm * rays["direction"][ok]).sum(axis=1) > 0.0
    nrm[away] = -nrm[away]
    return hits["point"][ok], nrm, rays["time"][ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 17)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--kernels", default="", help="comma list (default: grid,bvh for sphere scenes, bvh4,bvh for meshes)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    prec = rtow.F64_FAST if a.precision == "fast" else rtow.F64_STRICT
    samples, seed = a.samples, 7
    ctx = rtow.Context(0)
    rows = []
    print(f"# {a.points} points x {samples} samples, precision {a.precision}; Grays/s from kernel events (best of "
          f"{a.repeats} after {a.warmup}; worst in brackets): ambient vs occluded on the exported rays")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, _ = scene_of(name, tmp)
            ctx.upload(scene)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            kernels = a.kernels.split(",") if a.kernels else (["bvh4", "bvh"] if mesh else ["grid", "bvh"])
            p, nrm, tm = surface_points(ctx, name, scene, a.points)
            n = len(p)
            lo, hi = scene_extent(scene)
            ext = float(np.max(hi - lo))
            d_out = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
            d_rays = torch.empty(n * samples * 64, dtype=torch.uint8, device="cuda")
            d_occ = torch.empty(n * samples, dtype=torch.bool, device="cuda")
            for set_name, max_dist in (("ao", 0.05 * ext), ("sky", math.inf)):
                pts = rtow.make_surface_points(p, nrm, time=tm, max_dist=max_dist)
                d_pts = torch.from_numpy(pts.view(np.uint8)).to("cuda")
                for kn in kernels:
                    k = KERNELS[kn]
                    # the export run (not timed) leaves the rays the timed occlusion calls read
                    ctx.ambient_device(d_pts.data_ptr(), n, 0, d_out.data_ptr(), samples, d_rays.data_ptr(), seed, 0, prec,
                                       k, 0, True)
                    a_best, a_worst, a_st = timed(
                        lambda: ctx.ambient_device(d_pts.data_ptr(), n, 0, d_out.data_ptr(), samples, 0, seed, 0, prec, k,
                                                   0, True), a.warmup, a.repeats)
                    o_best, o_worst, o_st = timed(
                        lambda: ctx.occluded_device(d_rays.data_ptr(), n * samples, d_occ.data_ptr(), prec, k, 0, True),
                        a.warmup, a.repeats)
                    out = d_out.cpu().numpy().view(rtow.AMBIENT_DTYPE)
                    occ = d_occ.cpu().numpy().reshape(n, samples)
                    differ = int((out["open"] != (~occ).sum(axis=1)).sum())
                    nr = n * samples
                    row = dict(scene=name, set=set_name, kernel=kn, kernel_used=int(a_st.kernel_used), points=n,
                               samples=samples, rays=nr, precision=a.precision,
                               amb_ms=a_best, amb_ms_worst=a_worst, amb_grays=nr / a_best / 1e6,
                               amb_grays_worst=nr / a_worst / 1e6, amb_node_per_ray=a_st.node_tests / nr,
                               amb_prim_per_ray=a_st.prim_tests / nr,
                               occ_ms=o_best, occ_ms_worst=o_worst, occ_grays=nr / o_best / 1e6,
                               occ_grays_worst=nr / o_worst / 1e6, occ_node_per_ray=o_st.node_tests / nr,
                               occ_prim_per_ray=o_st.prim_tests / nr,
                               ratio=o_best / a_best, open=float(out["open"].sum() / nr), differ=differ)
                    rows.append(row)
                    print(f"{name:8s} {set_name:4s} {kn:5s}(ran {row['kernel_used']}) open {row['open']:.3f} | "
                          f"ambient {row['amb_grays']:7.3f} ({row['amb_grays_worst']:7.3f}) Grays/s "
                          f"{row['amb_node_per_ray']:6.1f} nodes {row['amb_prim_per_ray']:6.1f} prims | "
                          f"occluded {row['occ_grays']:7.3f} ({row['occ_grays_worst']:7.3f}) Grays/s "
                          f"{row['occ_node_per_ray']:6.1f} nodes {row['occ_prim_per_ray']:6.1f} prims | "
                          f"x{row['ratio']:.2f} | differ {differ}", flush=True)
                del d_pts
            del d_out, d_rays, d_occ
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
