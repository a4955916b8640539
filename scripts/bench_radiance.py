#!/usr/bin/env python3
"""Throughput of the radiance query (rtow_radiance_device) beside the render's, fast build, AUTO kernel.

Per scene (cover, moving cover, suzanne, the 96.8k-triangle mesh): the W x H primary rays of the scene's camera (pinhole,
pixel centres, computed in numpy, in pixel order) with samples_per_ray = 16 and max_child_rays = 50.  Gsamples/s =
samples / stats.kernel_ms (HIP events around the query kernel), best of `--repeats` calls after `--warmup`, with the
slowest-to-fastest range; beside it the kernel_ms of rtow_render_device for the same W x H x 16 spp in the same process,
and for both the segments per sample and the (node + primitive) tests per segment.  The two trace different paths (the
render jitters its primaries and has a lens), so the per-sample counters say how far the workloads are comparable.

   python scripts/bench_radiance.py [--width 1200] [--spr 16] [--depth 50] [--scenes cover,moving,suzanne,mesh96k]
                                    [--warmup 2] [--repeats 5] [--split 1] [--json OUT]

--split S traces the same samples as S x as many work items: every ray is repeated S times with the identities
(i, k * spr / S), k < S, and spr / S samples each (what include/rtow.h suggests to a caller who wants more parallelism
than one lane per ray; the sums of a ray's S results are its spr samples).
"""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))
import torch  # noqa: E402  (device buffers; torch's runtime is loaded before librtow's, see rtow.lib)
import rtow  # noqa: E402


def scene_of(name, tmpdir):
    if name in ("cover", "moving"):
        return rtow.HostScene.cover(11, 1.5, name == "moving"), 1.5
    if name == "suzanne":
        return rtow.HostScene.obj(ROOT / "tests/golden/suzanne.obj", 16 / 9), 16 / 9
    obj = Path(tmpdir) / "m10.obj"
    subprocess.run([sys.executable, str(ROOT / "scripts/make_mesh.py"), str(obj), "10"], check=True, capture_output=True)
    return rtow.HostScene.obj(obj, 16 / 9), 16 / 9


def primary_rays(scene, W, H):
    """Camera::get_ray at pixel centres without the lens (src/common-model.cpp:156-167), rows from the top."""
    cam = scene.c.camera
    j = np.arange(W, dtype=np.float64)
    i = np.arange(H, dtype=np.float64)
    u = (j + 0.5) / (W - 1)
    v = ((H - 1 - i) + 0.5) / (H - 1)
    llc, hor, ver, org = (np.array(x[:]) for x in (cam.lower_left_corner, cam.horizontal, cam.vertical, cam.origin))
    d = llc[None, None, :] + u[None, :, None] * hor[None, None, :] + v[:, None, None] * ver[None, None, :] - org
    r = np.empty(W * H, dtype=rtow.RAY_DTYPE)
    r["origin"] = org
    r["direction"] = d.reshape(-1, 3)
    r["time"] = 0.5 * (cam.t0 + cam.t1)
    r["tmax"] = np.inf
    return r


def best_of(call, warmup, repeats):
    for _ in range(warmup):
        call()
    runs = [call() for _ in range(repeats)]
    ms = [st.kernel_ms for st in runs]
    return runs[int(np.argmin(ms))], min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spr", type=int, default=16)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--split", type=int, default=1)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.split < 1 or a.spr % a.split:
        ap.error("--split must divide --spr")
    ctx = rtow.Context(0)
    rows = []
    print(f"# fast build, AUTO kernel, {a.spr} samples per ray / pixel, depth {a.depth}; Gsamples/s from kernel events, best of "
          f"{a.repeats} after {a.warmup} (slowest..fastest ms) | segments per sample | tests per segment")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            W = a.width
            H = rtow.image_height(W, aspect)
            n = W * H
            rays = np.repeat(primary_rays(scene, W, H), a.split)
            nq, spr = n * a.split, a.spr // a.split
            d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda")
            d_rgb = torch.zeros((nq, 3), dtype=torch.float64, device="cuda")
            d_ids = None
            if a.split > 1:
                ids = np.stack([np.repeat(np.arange(n), a.split), np.tile(np.arange(a.split) * spr, n)], axis=1)
                d_ids = torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to("cuda")
            q, q_ms, q_max = best_of(lambda: ctx.radiance_device(d_rays.data_ptr(), nq, d_ids.data_ptr() if a.split > 1 else 0,
                                                                 d_rgb.data_ptr(), spr, a.depth, 1, 0, rtow.F64_FAST,
                                                                 rtow.KERNEL_AUTO, 0, True), a.warmup, a.repeats)
            finite = bool(torch.isfinite(d_rgb).all().item())
            cfg = rtow.make_config(W, H, a.spr, 1, a.depth, seed=1, precision=rtow.F64_FAST)
            out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
            r, r_ms, r_max = best_of(lambda: ctx.render_device(cfg, out.data_ptr(), 0, True), a.warmup, a.repeats)
            row = dict(scene=name, width=W, height=H, rays=nq, split=a.split, samples=int(q.samples), kernel_used=int(q.kernel_used),
                       query_ms=q_ms, query_ms_max=q_max, query_gsamples=q.samples / q_ms / 1e6,
                       query_seg_per_sample=q.segments / q.samples,
                       query_tests_per_seg=(q.node_tests + q.prim_tests) / max(q.segments, 1),
                       render_kernel=int(r.kernel_used), render_ms=r_ms, render_ms_max=r_max,
                       render_gsamples=r.samples / r_ms / 1e6, render_seg_per_sample=r.segments / r.samples,
                       render_tests_per_seg=(r.node_tests + r.prim_tests) / max(r.segments, 1), finite=finite)
            row["ratio"] = row["query_gsamples"] / row["render_gsamples"]
            rows.append(row)
            print(f"{name:8s} {W}x{H} kernel {row['kernel_used']} | query {row['query_gsamples']:6.3f} Gsamples/s "
                  f"({q_max:.3f}..{q_ms:.3f} ms) {row['query_seg_per_sample']:.3f} seg/sample "
                  f"{row['query_tests_per_seg']:.1f} tests/seg | render {row['render_gsamples']:6.3f} Gsamples/s "
                  f"({r_max:.3f}..{r_ms:.3f} ms) {row['render_seg_per_sample']:.3f} seg/sample "
                  f"{row['render_tests_per_seg']:.1f} tests/seg | query / render {row['ratio']:.2f}", flush=True)
            del d_rays, d_rgb, d_ids, out
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
