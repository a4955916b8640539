#!/usr/bin/env python3
"""The any-hit query (rtow_occluded_device) against the closest-hit query (rtow_intersect_device) on the same rays, per
scene, ray set and strategy.  Three seeded ray sets of >= 8 M rays per scene:
   shadow   from the hit points of a small oracle render's logged segments (o + t_hit d) toward a fixed point light
            above the scene: d = L - p, tmax = 1;
   ao       from the same points along seeded uniform directions, tmax = 5 % of the scene's extent;
   primary  camera rays (pixel centres), tmax = inf: occlusion is "hits anything".
Per row: Grays/s of each query from its kernel's HIP events (stats.kernel_ms, best of `repeats` after `warmup`), the
node and primitive tests per ray of each, the occluded share, and the two answers compared (they must agree: strict
build exactly; the fast build outside a 1e-9 rounding band around tmax, counted in `differ`).

   python scripts/bench_occlusion.py [--rays 8388608] [--precision fast|strict] [--scenes cover,moving,suzanne,mesh96k]
                                     [--kernels grid,bvh] [--warmup 2] [--repeats 5] [--json OUT]
"""
import argparse
import ctypes as C
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import KERNELS, primary_rays, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
import orc  # noqa: E402


def hit_points(name, scene, n, seed=41):
    """(points, times) of n hit points drawn from the segments of a small oracle render (seeded)."""
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
    return rows[:, 3:6] + rows[:, 10:11] * rows[:, 6:9], rows[:, 9]


def scene_extent(scene):
    a = orc.scene_arrays(scene.c)
    sph = a["sphere_geom"].reshape(-1, 4)
    small = sph[np.abs(sph[:, 3]) < 100.0]  # (not the cover scene's ground sphere)
    mov = a["moving_geom"].reshape(-1, 8)
    pts = [small[:, :3] - np.abs(small[:, 3:4]), small[:, :3] + np.abs(small[:, 3:4]), mov[:, 0:3] - mov[:, 6:7],
           mov[:, 3:6] + mov[:, 6:7], a["triangle_geom"].reshape(-1, 3)]
    pts = np.concatenate([p for p in pts if len(p)])
    return pts.min(0), pts.max(0)


def ray_sets(name, scene, aspect, n):
    lo, hi = scene_extent(scene)
    ext = float(np.max(hi - lo))
    light = 0.5 * (lo + hi) + np.array([0.2 * ext, 1.5 * ext, 0.1 * ext])
    p, tm = hit_points(name, scene, n)
    g = np.random.default_rng(43)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return {"shadow": rtow.make_rays(p, light[None, :] - p, time=tm, tmax=1.0),
            "ao": rtow.make_rays(p, u, time=tm, tmax=0.05 * ext),
            "primary": primary_rays(scene, aspect, n)}


def timed(call, warmup, repeats):
    for _ in range(warmup):
        call()
    sts = [call() for _ in range(repeats)]
    ms = [s.kernel_ms for s in sts]
    return min(ms), max(ms), sts[-1]


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
    d_occ = torch.empty(n, dtype=torch.bool, device="cuda")
    print(f"# {n} rays per set, precision {a.precision}; Grays/s from kernel events (best of {a.repeats} after "
          f"{a.warmup}; worst in brackets), node / prim tests per ray: occlusion vs closest hit")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            kernels = a.kernels.split(",") if a.kernels else (["bvh4", "bvh"] if mesh else ["grid", "bvh"])
            for set_name, rays in ray_sets(name, scene, aspect, n).items():
                d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda")
                for kn in kernels:
                    k = KERNELS[kn]
                    o_best, o_worst, o_st = timed(
                        lambda: ctx.occluded_device(d_rays.data_ptr(), n, d_occ.data_ptr(), prec, k, 0, True),
                        a.warmup, a.repeats)
                    i_best, i_worst, i_st = timed(
                        lambda: ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True),
                        a.warmup, a.repeats)
                    occ = d_occ.cpu().numpy()
                    t = d_hits.cpu().numpy().view(rtow.HIT_DTYPE)["t"]
                    with np.errstate(invalid="ignore"):  # (inf - inf: a miss with tmax = inf is not near)
                        near = np.abs(t - rays["tmax"]) <= 1e-9 * np.maximum(1.0, rays["tmax"])
                    differ = int(((occ != np.isfinite(t)) & ~near).sum())
                    row = dict(scene=name, set=set_name, kernel=kn, kernel_used=int(o_st.kernel_used), rays=n,
                               occ_ms=o_best, occ_ms_worst=o_worst, occ_grays=n / o_best / 1e6,
                               occ_grays_worst=n / o_worst / 1e6, occ_node_per_ray=o_st.node_tests / n,
                               occ_prim_per_ray=o_st.prim_tests / n, int_ms=i_best, int_ms_worst=i_worst,
                               int_grays=n / i_best / 1e6, int_grays_worst=n / i_worst / 1e6,
                               int_node_per_ray=i_st.node_tests / n, int_prim_per_ray=i_st.prim_tests / n,
                               occluded=float(occ.mean()), differ=differ)
                    rows.append(row)
                    print(f"{name:8s} {set_name:8s} {kn:5s}(ran {row['kernel_used']}) occluded {row['occluded']:.3f} | "
                          f"occlusion {row['occ_grays']:7.3f} ({row['occ_grays_worst']:7.3f}) Grays/s "
                          f"{row['occ_node_per_ray']:6.1f} nodes {row['occ_prim_per_ray']:6.1f} prims | "
                          f"closest hit {row['int_grays']:7.3f} ({row['int_grays_worst']:7.3f}) Grays/s "
                          f"{row['int_node_per_ray']:6.1f} nodes {row['int_prim_per_ray']:6.1f} prims | "
                          f"x{row['occ_grays'] / row['int_grays']:.2f} | differ {differ}", flush=True)
                del d_rays
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
