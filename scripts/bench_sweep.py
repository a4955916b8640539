#!/usr/bin/env python3
"""The swept-sphere query (rtow_sweep_device) against the first-hit ray query (rtow_first_hits_device, max_hits = 1) on
the same segments, per scene, radius, strategy and build: the thinnest existing walk over the same work is the baseline.

Segments: those of a small oracle render (bench_query.logged_rays), tiled to the count; the sweep takes each ray's origin,
direction and time with tmax = inf and a radius of 0, 1 % and 5 % of the scene's extent.
Per row: Msweeps/s from the kernel's HIP events (stats.kernel_ms, best of `repeats` after `warmup`; the worst beside it),
node and primitive tests per sweep, the share that hit and that started in overlap, and the baseline's rate and tests on
the same segments in the same run with their ratio.  A record, not a gate.

   python scripts/bench_sweep.py [--sweeps 1048576] [--scenes cover,moving,suzanne,mesh96k] [--kernels bvh,bvh4]
                                 [--precisions fast,strict] [--radii 0,0.01,0.05] [--warmup 2] [--repeats 5] [--json OUT]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import KERNELS, logged_rays, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
from bench_occlusion import scene_extent, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--kernels", default="bvh,bvh4")
    ap.add_argument("--precisions", default="fast,strict")
    ap.add_argument("--radii", default="0,0.01,0.05", help="fractions of the scene's extent")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "sweep_bench.json"))
    a = ap.parse_args()
    n = a.sweeps
    ctx = rtow.Context(0)
    rows = []
    print(f"# {n} segments of a logged render; Msweeps/s from kernel events (best of {a.repeats} after {a.warmup}; worst in "
          f"brackets): sweep vs first_hits(max_hits = 1) on the same segments")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, _ = scene_of(name, tmp)
            ctx.upload(scene)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            lo, hi = scene_extent(scene)
            ext = float(np.max(hi - lo))
            rays = logged_rays(name, scene, n)
            d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda")
            d_fh = torch.empty(n * rtow.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_hits = torch.empty(n * rtow.SWEEP_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            for pname in a.precisions.split(","):
                prec = rtow.F64_FAST if pname == "fast" else rtow.F64_STRICT
                for kn in a.kernels.split(","):
                    if kn == "bvh4" and not mesh:
                        continue  # (the 4-wide image exists for triangle meshes only: the request would run BVH again)
                    k = KERNELS[kn]
                    b_best, b_worst, b_st = timed(
                        lambda: ctx.first_hits_device(d_rays.data_ptr(), n, 1, d_fh.data_ptr(), 0, prec, k, 0, True),
                        a.warmup, a.repeats)
                    for frac in (float(x) for x in a.radii.split(",")):
                        q = rtow.make_sweeps(rays["origin"], rays["direction"], frac * ext, time=rays["time"])
                        d_q = torch.from_numpy(q.view(np.uint8)).to("cuda")
                        s_best, s_worst, s_st = timed(
                            lambda: ctx.sweep_device(d_q.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True),
                            a.warmup, a.repeats)
                        h = d_hits.cpu().numpy().view(rtow.SWEEP_HIT_DTYPE)
                        row = dict(scene=name, kernel=kn, kernel_used=int(s_st.kernel_used), precision=pname, sweeps=n,
                                   radius_fraction=frac, radius=frac * ext,
                                   sweep_ms=s_best, sweep_ms_worst=s_worst, sweep_mps=n / s_best / 1e3,
                                   sweep_mps_worst=n / s_worst / 1e3, sweep_node_per=s_st.node_tests / n,
                                   sweep_prim_per=s_st.prim_tests / n, hit=float((h["prim"] >= 0).mean()),
                                   start_overlap=float(h["start_overlap"].mean()),
                                   first_hits_ms=b_best, first_hits_ms_worst=b_worst, first_hits_mps=n / b_best / 1e3,
                                   first_hits_node_per=b_st.node_tests / n, first_hits_prim_per=b_st.prim_tests / n,
                                   ratio=s_best / b_best)
                        rows.append(row)
                        print(f"{name:8s} {pname:6s} {kn:5s}(ran {row['kernel_used']}) r {frac:4.2f} | sweep "
                              f"{row['sweep_mps']:8.2f} ({row['sweep_mps_worst']:8.2f}) M/s {row['sweep_node_per']:6.1f} nodes "
                              f"{row['sweep_prim_per']:6.1f} prims hit {row['hit']:.3f} overlap {row['start_overlap']:.3f} | "
                              f"first_hits {row['first_hits_mps']:8.2f} M/s {row['first_hits_node_per']:6.1f} nodes "
                              f"{row['first_hits_prim_per']:6.1f} prims | x{row['ratio']:.2f} the time", flush=True)
                        del d_q
            del d_rays, d_fh, d_hits
            if a.json:  # (after every scene: a run that is cut short keeps what it measured)
                Path(a.json).parent.mkdir(parents=True, exist_ok=True)
                Path(a.json).write_text(json.dumps(rows, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
