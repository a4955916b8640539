#!/usr/bin/env python3
"""Throughput of the path-step query (rtow_path_step_device) driven as a wavefront loop, fast build, AUTO kernel.

Per scene (cover, moving cover, suzanne, the 96.8k-triangle mesh): the W x H primary rays of the scene's camera (pinhole,
pixel centres, bench_radiance.py's) are stepped depth + 1 times IN PLACE (d_next = d_rays, no compaction: dead rays are
skipped by the kernel), one sample per ray.  Reported, best of `--repeats` loops after `--warmup`:

  per launch   Gsegments/s of the first launch (every ray live) and of the whole loop's launches taken one by one:
               live rays / stats.kernel_ms (HIP events around the kernel; each call synchronises);
  whole loop   Gsegments/s of the depth + 1 launches enqueued back to back without stats, between two events on the
               stream: all live segments / elapsed — what a wavefront caller gets, launch gaps and dead lanes included;
  beside them, in the same process: rtow_intersect_device on the same first-segment rays (kernel_ms) and
  rtow_radiance_device with one sample per ray and the same depth on the same primaries (kernel_ms, its own segment
  counter), and the two ratios first launch / intersect and whole loop / radiance.

   python scripts/bench_step.py [--width 1200] [--depth 50] [--scenes cover,moving,suzanne,mesh96k]
                                [--warmup 2] [--repeats 5] [--json OUT]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import torch  # noqa: E402  (device buffers; torch's runtime is loaded before librtow's, see rtow.lib)
import rtow  # noqa: E402
from bench_radiance import best_of, primary_rays, scene_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    ctx = rtow.Context(0)
    steps = a.depth + 1
    rows = []
    print(f"# fast build, AUTO kernel, 1 sample per ray, {steps} in-place launches; best of {a.repeats} after {a.warmup}")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            W = a.width
            H = rtow.image_height(W, aspect)
            n = W * H
            d_rays = torch.from_numpy(primary_rays(scene, W, H).view(np.uint8)).to("cuda")
            d_work = torch.empty_like(d_rays)
            d_att = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_hits = torch.zeros(n * 72, dtype=torch.uint8, device="cuda")
            d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")

            def step(b, stats):
                return ctx.path_step_device(d_work.data_ptr(), n, 0, d_work.data_ptr(), d_att.data_ptr(), d_st.data_ptr(), 0,
                                            b, 1, 0, rtow.F64_FAST, rtow.KERNEL_AUTO, 0, stats)

            # one counting pass: live rays and kernel time of every launch
            d_work.copy_(d_rays)
            live, launch_ms, kernel_used = [], [], 0
            for b in range(steps):
                st = step(b, True)
                kernel_used = int(st.kernel_used)
                live.append(int((d_st != rtow.STEP_SKIPPED).sum().item()))
                launch_ms.append(st.kernel_ms)
            segments = sum(live)

            def first_launch():
                d_work.copy_(d_rays)
                return step(0, True)

            _, first_ms, first_max = best_of(first_launch, a.warmup, a.repeats)

            def whole_loop():
                d_work.copy_(d_rays)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for b in range(steps):
                    step(b, False)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(a.warmup):
                whole_loop()
            loop = [whole_loop() for _ in range(a.repeats)]
            loop_ms, loop_max = min(loop), max(loop)

            _, i_ms, i_max = best_of(lambda: ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST,
                                                                  rtow.KERNEL_AUTO, 0, True), a.warmup, a.repeats)
            r, r_ms, r_max = best_of(lambda: ctx.radiance_device(d_rays.data_ptr(), n, 0, d_rgb.data_ptr(), 1, a.depth, 1, 0,
                                                                 rtow.F64_FAST, rtow.KERNEL_AUTO, 0, True), a.warmup, a.repeats)
            row = dict(scene=name, width=W, height=H, rays=n, kernel_used=kernel_used, launches=steps, segments=segments,
                       live_per_launch=live, launch_ms=launch_ms,
                       first_ms=first_ms, first_ms_max=first_max, first_gseg=n / first_ms / 1e6,
                       launches_gseg=segments / sum(launch_ms) / 1e6,
                       loop_ms=loop_ms, loop_ms_max=loop_max, loop_gseg=segments / loop_ms / 1e6,
                       intersect_ms=i_ms, intersect_ms_max=i_max, intersect_gseg=n / i_ms / 1e6,
                       radiance_ms=r_ms, radiance_ms_max=r_max, radiance_segments=int(r.segments),
                       radiance_gseg=r.segments / r_ms / 1e6)
            row["first_over_intersect"] = row["first_gseg"] / row["intersect_gseg"]
            row["loop_over_radiance"] = row["loop_gseg"] / row["radiance_gseg"]
            rows.append(row)
            print(f"{name:8s} {W}x{H} kernel {kernel_used} | {segments} segments in {steps} launches (radiance counts "
                  f"{row['radiance_segments']}) | first launch {row['first_gseg']:6.3f} Gseg/s ({first_max:.3f}..{first_ms:.3f} ms)"
                  f" | launches one by one {row['launches_gseg']:6.3f} Gseg/s | whole loop {row['loop_gseg']:6.3f} Gseg/s "
                  f"({loop_max:.3f}..{loop_ms:.3f} ms) | intersect {row['intersect_gseg']:6.3f} Gseg/s ({i_max:.3f}..{i_ms:.3f} ms)"
                  f" | radiance {row['radiance_gseg']:6.3f} Gseg/s ({r_max:.3f}..{r_ms:.3f} ms) | first / intersect "
                  f"{row['first_over_intersect']:.2f} | loop / radiance {row['loop_over_radiance']:.2f}", flush=True)
            del d_rays, d_work, d_att, d_st, d_hits, d_rgb
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
