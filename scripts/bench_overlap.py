#!/usr/bin/env python3
"""The box-overlap query (rtow_overlap_device) against the k-nearest query (rtow_nearest_device, k = 8) at the box centres
with max_dist = the half-diagonal — the only region question the code could answer before — per scene, edge length,
strategy and build.  The two answer different questions (a box against a ball that holds it; every primitive counted
against eight kept, with their records), so no ratio is demanded: a record, not a gate.

Boxes: the voxels of a grid over the scene's box (the cover scenes without the ground sphere: a slab one sphere high) at
three edge lengths, 1/64, 1/32 and 1/16 of the extent, in x-major order, tiled to the count.  Overlap runs counts only and
with eight ids.  Per row: the kernel's HIP-event time (stats.kernel_ms) as median, least and greatest of `repeats` after
`warmup`, Mboxes/s at the median, node and primitive tests per box, the share of occupied voxels and the mean and greatest
count; and the same for nearest on the same centres in the same run.

   python scripts/bench_overlap.py [--boxes 262144] [--scenes cover,suzanne,mesh96k] [--kernels bvh,bvh4]
                                   [--precisions fast,strict] [--edges 64,32,16] [--warmup 2] [--repeats 7] [--json OUT]
"""
import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from bench_query import KERNELS, rtow, scene_of, torch  # noqa: E402  (torch first: see rtow.lib)
from bench_occlusion import scene_extent  # noqa: E402


def voxels(lo, hi, per_axis, n):
    """n boxes: the cubic voxels of edge max(hi - lo) / per_axis that cover [lo, hi], x-major, tiled to n."""
    edge = float(np.max(hi - lo)) / per_axis
    dims = np.maximum(np.ceil((hi - lo) / edge).astype(np.int64), 1)
    idx = np.arange(n) % int(np.prod(dims))
    ijk = np.stack([idx // (dims[1] * dims[2]), (idx // dims[2]) % dims[1], idx % dims[2]], axis=1)
    vlo = lo + ijk * edge
    return rtow.make_boxes(vlo, vlo + edge, 0.5), edge


def timed(call, warmup, repeats):
    for _ in range(warmup):
        call()
    sts = [call() for _ in range(repeats)]
    ms = [s.kernel_ms for s in sts]
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms)), sts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 18)
    ap.add_argument("--scenes", default="cover,suzanne,mesh96k")
    ap.add_argument("--kernels", default="bvh,bvh4")
    ap.add_argument("--precisions", default="fast,strict")
    ap.add_argument("--edges", default="64,32,16", help="voxels per longest axis")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "overlap_bench.json"))
    a = ap.parse_args()
    n = a.boxes
    ctx = rtow.Context(0)
    rows = []
    print(f"# {n} voxels per row; kernel-event ms, median [least, greatest] of {a.repeats} after {a.warmup}: overlap (counts, "
          f"ids) vs nearest(k = 8, max_dist = half-diagonal) at the centres")
    d_counts = torch.empty(n, dtype=torch.int32, device="cuda")
    d_ids = torch.empty(n * 8, dtype=torch.int32, device="cuda")
    d_hits = torch.empty(n * 8 * rtow.POINT_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, _ = scene_of(name, tmp)
            ctx.upload(scene)
            mesh = scene.c.n_spheres + scene.c.n_moving == 0
            lo, hi = scene_extent(scene)
            for per_axis in (int(x) for x in a.edges.split(",")):
                q, edge = voxels(lo, hi, per_axis, n)
                centres = 0.5 * (q["lo"] + q["hi"])
                pq = rtow.make_point_queries(centres, 0.5, 0.5 * edge * np.sqrt(3.0))
                d_q = torch.from_numpy(q.view(np.uint8)).to("cuda")
                d_pq = torch.from_numpy(pq.view(np.uint8)).to("cuda")
                for pname in a.precisions.split(","):
                    prec = rtow.F64_FAST if pname == "fast" else rtow.F64_STRICT
                    for kn in a.kernels.split(","):
                        if kn == "bvh4" and not mesh:
                            continue  # (the 4-wide image exists for triangle meshes only: the request would run BVH again)
                        k = KERNELS[kn]
                        t_c, s_c = timed(lambda: ctx.overlap_device(d_q.data_ptr(), n, d_counts.data_ptr(), 0, 8, prec, k, 0, True),
                                         a.warmup, a.repeats)
                        t_i, s_i = timed(lambda: ctx.overlap_device(d_q.data_ptr(), n, d_counts.data_ptr(), d_ids.data_ptr(), 8,
                                                                    prec, k, 0, True), a.warmup, a.repeats)
                        counts = d_counts.cpu().numpy()
                        t_n, s_n = timed(lambda: ctx.nearest_device(d_pq.data_ptr(), n, 8, d_hits.data_ptr(), d_counts.data_ptr(),
                                                                    prec, k, 0, True), a.warmup, a.repeats)
                        kept = d_counts.cpu().numpy()
                        row = dict(scene=name, kernel=kn, kernel_used=int(s_c.kernel_used), precision=pname, boxes=n,
                                   voxels_per_axis=per_axis, edge=edge,
                                   overlap_counts=dict(t_c, mboxes_per_s=n / t_c["ms_median"] / 1e3, node_per=s_c.node_tests / n,
                                                       prim_per=s_c.prim_tests / n),
                                   overlap_ids=dict(t_i, mboxes_per_s=n / t_i["ms_median"] / 1e3, node_per=s_i.node_tests / n,
                                                    prim_per=s_i.prim_tests / n),
                                   nearest8=dict(t_n, mpoints_per_s=n / t_n["ms_median"] / 1e3, node_per=s_n.node_tests / n,
                                                 prim_per=s_n.prim_tests / n, kept_mean=float(kept.mean())),
                                   occupied=float((counts > 0).mean()), count_mean=float(counts.mean()), count_max=int(counts.max()),
                                   beyond_eight=float((counts > 8).mean()))
                        rows.append(row)
                        oc, oi, nn = row["overlap_counts"], row["overlap_ids"], row["nearest8"]
                        print(f"{name:8s} {pname:6s} {kn:5s}(ran {row['kernel_used']}) 1/{per_axis:<3d}| counts {oc['ms_median']:7.3f} "
                              f"[{oc['ms_min']:.3f}, {oc['ms_max']:.3f}] ms {oc['node_per']:6.1f} nodes {oc['prim_per']:6.1f} prims | ids "
                              f"{oi['ms_median']:7.3f} [{oi['ms_min']:.3f}, {oi['ms_max']:.3f}] ms | nearest8 {nn['ms_median']:7.3f} "
                              f"[{nn['ms_min']:.3f}, {nn['ms_max']:.3f}] ms {nn['node_per']:6.1f} nodes {nn['prim_per']:6.1f} prims | "
                              f"occupied {row['occupied']:.3f} mean {row['count_mean']:.2f} max {row['count_max']} >8 {row['beyond_eight']:.3f}",
                              flush=True)
                del d_q, d_pq
            if a.json:  # (after every scene: a run that is cut short keeps what it measured)
                Path(a.json).parent.mkdir(parents=True, exist_ok=True)
                Path(a.json).write_text(json.dumps(rows, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
