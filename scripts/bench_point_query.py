#!/usr/bin/env python3
"""The closest-point query (rtow_closest_point_device) per scene, point set and strategy.  Three seeded point sets per
scene:
   near     hit points of a small oracle render's logged segments (o + t_hit d) offset by up to 2 % of the scene's
            extent, max_dist = 5 % of the extent (proximity / collision tests);
   volume   a lattice over the scene's box in lattice order, max_dist = inf (a distance-field pass);
   random   uniform in the box, shuffled, max_dist = inf (picking / worst-case coherence).
Per row: Gqueries/s from the kernel's HIP events (stats.kernel_ms, best of `repeats` after `warmup`, and the spread of
the timed runs), node and primitive tests per query, and the hit share.  BRUTE runs on the small scenes only.

   python scripts/bench_point_query.py [--points 1048576] [--precision fast|strict] [--scenes cover,moving,suzanne,mesh96k]
                                       [--kernels brute,bvh,bvh4] [--warmup 2] [--repeats 5] [--json OUT]
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
from bench_occlusion import hit_points, scene_extent  # noqa: E402


def point_sets(name, scene, n):
    lo, hi = scene_extent(scene)
    ext = float(np.max(hi - lo))
    g = np.random.default_rng(47)
    p, tm = hit_points(name, scene, n)
    near = rtow.make_point_queries(p + g.uniform(-0.02, 0.02, size=p.shape) * ext, tm, 0.05 * ext)
    k = max(2, int(round(n ** (1 / 3))))
    ax = [np.linspace(lo[j], hi[j], k) for j in range(3)]
    lattice = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    volume = rtow.make_point_queries(lattice, 0.5, math.inf)
    random = rtow.make_point_queries(g.uniform(lo, hi, size=(n, 3)), g.uniform(0, 1, n), math.inf)
    return {"near": near, "volume": volume, "random": random}


def run(ctx, q, prec, kernel, warmup, repeats):
    n = len(q)
    dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    dh = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    for _ in range(warmup):
        ctx.closest_point_device(dq.data_ptr(), n, dh.data_ptr(), prec, kernel, want_stats=True)
    ms, st = [], None
    for _ in range(repeats):
        st = ctx.closest_point_device(dq.data_ptr(), n, dh.data_ptr(), prec, kernel, want_stats=True)
        ms.append(st.kernel_ms)
    h = dh.cpu().numpy().view(rtow.POINT_HIT_DTYPE)
    best = min(ms)
    return {"gq_per_s": n / best / 1e6, "spread": (max(ms) - best) / best, "kernel_ms": best,
            "nodes_per_q": st.node_tests / n, "prims_per_q": st.prim_tests / n,
            "hit_share": float((h["prim"] >= 0).mean()), "kernel_used": st.kernel_used}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--kernels", default="brute,bvh,bvh4")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    prec = rtow.F64_FAST if a.precision == "fast" else rtow.F64_STRICT
    ctx = rtow.Context(0)
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for name in a.scenes.split(","):
            scene, _ = scene_of(name, td)
            ctx.upload(scene.c)
            for sname, q in point_sets(name, scene, a.points).items():
                for kname in a.kernels.split(","):
                    if kname == "brute" and name == "mesh96k":
                        continue  # (96.8k primitives per query: not measured)
                    r = run(ctx, q, prec, KERNELS[kname], a.warmup, a.repeats)
                    r.update(scene=name, points=sname, kernel=kname, n=len(q))
                    rows.append(r)
                    print(f"{name:8s} {sname:7s} {kname:6s} used {r['kernel_used']}  {r['gq_per_s']:8.4f} Gq/s "
                          f"(+{100 * r['spread']:.1f} %)  nodes/q {r['nodes_per_q']:8.1f}  prims/q {r['prims_per_q']:9.1f}"
                          f"  hits {r['hit_share']:.3f}", flush=True)
            scene.close()
    ctx.close()
    if a.json:
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
