#!/usr/bin/env python3
"""The first-k-hits query (rtow_first_hits_device) for max_hits 1, 4 and 8 against the closest-hit query
(rtow_intersect_device) on the same rays in the same process, per scene, ray set and strategy.  The scenes and the
seeded ray sets are those of scripts/bench_occlusion.py:
   primary  camera rays (pixel centres), tmax = inf;
   ao       from the hit points of a small oracle render along seeded uniform directions, tmax = 5 % of the extent.
Per row: Grays/s of each query from its kernel's HIP events (stats.kernel_ms, best of `repeats` after `warmup`, the
worst in brackets), node and primitive tests per ray, and the mean count.  No pass / fail threshold; the one
expectation checked against the table: with a finite tmax (the ao set) max_hits = 1 runs no more node and primitive
tests per ray than rtow_intersect (its walks are seeded with tmax) — printed as `seeded<=` yes / NO on those rows.

   python scripts/bench_first_hits.py [--rays 4194304] [--precision fast|strict] [--scenes cover,moving,suzanne,mesh96k]
                                      [--kernels grid,bvh] [--sets primary,ao] [--warmup 2] [--repeats 5] [--json OUT]
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
from bench_occlusion import ray_sets, timed  # noqa: E402

MAX_HITS = (1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4 << 20)
    ap.add_argument("--precision", default="fast", choices=["fast", "strict"])
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--kernels", default="", help="comma list (default: grid,bvh for sphere scenes, bvh4,bvh for meshes)")
    ap.add_argument("--sets", default="primary,ao")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    prec = rtow.F64_FAST if a.precision == "fast" else rtow.F64_STRICT
    n = a.rays
    ctx = rtow.Context(0)
    rows = []
    d_hits = torch.empty(n * max(MAX_HITS) * 72, dtype=torch.uint8, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    print(f"# {n} rays per set, precision {a.precision}; Grays/s from kernel events (best of {a.repeats} after "
          f"{a.warmup}; worst in brackets); nodes / prims: tests per ray")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            kernels = a.kernels.split(",") if a.kernels else (["bvh4", "bvh"] if mesh else ["grid", "bvh"])
            sets = ray_sets(name, scene, aspect, n)
            for set_name in a.sets.split(","):
                rays = sets[set_name]
                d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda")
                for kn in kernels:
                    k = KERNELS[kn]
                    i_best, i_worst, i_st = timed(
                        lambda: ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), prec, k, 0, True),
                        a.warmup, a.repeats)
                    row = dict(scene=name, set=set_name, kernel=kn, kernel_used=int(i_st.kernel_used), rays=n,
                               int_ms=i_best, int_ms_worst=i_worst, int_grays=n / i_best / 1e6,
                               int_grays_worst=n / i_worst / 1e6, int_node_per_ray=i_st.node_tests / n,
                               int_prim_per_ray=i_st.prim_tests / n)
                    line = (f"{name:8s} {set_name:8s} {kn:5s}(ran {row['kernel_used']}) | closest hit "
                            f"{row['int_grays']:7.3f} ({row['int_grays_worst']:7.3f}) Grays/s "
                            f"{row['int_node_per_ray']:6.1f} nodes {row['int_prim_per_ray']:6.1f} prims")
                    for m in MAX_HITS:
                        best, worst, st = timed(
                            lambda: ctx.first_hits_device(d_rays.data_ptr(), n, m, d_hits.data_ptr(), d_cnt.data_ptr(),
                                                          prec, k, 0, True), a.warmup, a.repeats)
                        mean = float(d_cnt.cpu().numpy().mean())
                        row.update({f"k{m}_ms": best, f"k{m}_ms_worst": worst, f"k{m}_grays": n / best / 1e6,
                                    f"k{m}_grays_worst": n / worst / 1e6, f"k{m}_node_per_ray": st.node_tests / n,
                                    f"k{m}_prim_per_ray": st.prim_tests / n, f"k{m}_mean_count": mean})
                        line += (f" | k={m} {n / best / 1e6:7.3f} ({n / worst / 1e6:7.3f}) {st.node_tests / n:6.1f} nodes "
                                 f"{st.prim_tests / n:6.1f} prims count {mean:.2f}")
                    if np.isfinite(rays["tmax"]).all():  # (the expectation is about a finite tmax)
                        row["k1_no_more_tests"] = bool(row["k1_node_per_ray"] <= row["int_node_per_ray"] and
                                                       row["k1_prim_per_ray"] <= row["int_prim_per_ray"])
                        line += f" | seeded<= {'yes' if row['k1_no_more_tests'] else 'NO'}"
                    rows.append(row)
                    print(line, flush=True)
                del d_rays
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
