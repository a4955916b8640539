#!/usr/bin/env python3
"""The k-nearest query (rtow_nearest_device) beside the closest-point query on the same queries, per scene, point set
and strategy.  The scenes and the three seeded point sets (near, volume, random) are those of bench_point_query.py.
Per row: the closest-point query, then k = 1, 4, 8 — Gqueries/s from the kernel's HIP events (stats.kernel_ms, best of
`repeats` after `warmup`), the slowest timed call, node and primitive tests per query and the mean count — and, for
k = 1, its rate relative to the closest-point query's of the same run, next to that query's own run-to-run spread.
BRUTE runs on the small scenes only.

   python scripts/bench_nearest.py [--points 1048576] [--precision fast|strict] [--scenes cover,moving,suzanne,mesh96k]
                                   [--kernels brute,bvh,bvh4] [--warmup 2] [--repeats 5] [--json OUT]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import KERNELS, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
from bench_point_query import point_sets  # noqa: E402
from bench_point_query import run as run_closest  # noqa: E402

KS = (1, 4, 8)


def run(ctx, q, k, prec, kernel, warmup, repeats):
    n = len(q)
    dq = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    dh = torch.empty(n * k * 48, dtype=torch.uint8, device="cuda")
    dc = torch.empty(n, dtype=torch.int32, device="cuda")
    for _ in range(warmup):
        ctx.nearest_device(dq.data_ptr(), n, k, dh.data_ptr(), dc.data_ptr(), prec, kernel, want_stats=True)
    ms, st = [], None
    for _ in range(repeats):
        st = ctx.nearest_device(dq.data_ptr(), n, k, dh.data_ptr(), dc.data_ptr(), prec, kernel, want_stats=True)
        ms.append(st.kernel_ms)
    best = min(ms)
    return {"gq_per_s": n / best / 1e6, "spread": (max(ms) - best) / best, "kernel_ms": best, "slowest_ms": max(ms),
            "nodes_per_q": st.node_tests / n, "prims_per_q": st.prim_tests / n,
            "mean_count": float(dc.cpu().numpy().mean()), "kernel_used": st.kernel_used}


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
                    cp = run_closest(ctx, q, prec, KERNELS[kname], a.warmup, a.repeats)
                    cp.update(scene=name, points=sname, kernel=kname, n=len(q), k=0)
                    rows.append(cp)
                    print(f"{name:8s} {sname:7s} {kname:6s} used {cp['kernel_used']}  closest {cp['gq_per_s']:8.4f} Gq/s "
                          f"(+{100 * cp['spread']:.1f} %)  nodes/q {cp['nodes_per_q']:8.1f}  prims/q "
                          f"{cp['prims_per_q']:9.1f}", flush=True)
                    for k in KS:
                        r = run(ctx, q, k, prec, KERNELS[kname], a.warmup, a.repeats)
                        r.update(scene=name, points=sname, kernel=kname, n=len(q), k=k, vs_closest=r["gq_per_s"] / cp["gq_per_s"])
                        rows.append(r)
                        print(f"{'':8s} {'':7s} {'':6s} k = {k}       {r['gq_per_s']:8.4f} Gq/s (+{100 * r['spread']:.1f} %, "
                              f"slowest {r['slowest_ms']:.3f} ms)  nodes/q {r['nodes_per_q']:8.1f}  prims/q "
                              f"{r['prims_per_q']:9.1f}  count {r['mean_count']:.2f}  x{r['vs_closest']:.3f} of closest",
                              flush=True)
            scene.close()
    ctx.close()
    if a.json:
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
