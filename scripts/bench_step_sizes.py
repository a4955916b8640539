#!/usr/bin/env python3
"""What one launch of the path-step query costs against the ray count, fast build, AUTO kernel.

Cover scene and suzanne: the first n of the 1200-wide pinhole primaries (bench_radiance.py's), n = 64 .. the whole frame,
as they are (live) and with tmax = -1 (dead: the kernel skips the walk); per n the best stats.kernel_ms of five calls after
two warm-ups of rtow_path_step_device (out of place, no hit records) and of rtow_intersect_device on the same rays.

   python scripts/bench_step_sizes.py
"""
import sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import torch
import rtow
from bench_radiance import primary_rays, scene_of

ctx = rtow.Context(0)
for name in ("cover", "suzanne"):
    scene, aspect = scene_of(name, "/tmp")
    ctx.upload(scene)
    W = 1200
    H = rtow.image_height(W, aspect)
    rays = primary_rays(scene, W, H)
    dead = rays.copy()
    dead["tmax"] = -1.0
    for n in (64, 1024, 16384, 131072, len(rays)):
        row = [name, n]
        for label, src in (("live", rays), ("dead", dead)):
            d_src = torch.from_numpy(src[:n].view(np.uint8).copy()).to("cuda")
            d_next = torch.empty_like(d_src)
            d_att = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_hits = torch.zeros(n * 72, dtype=torch.uint8, device="cuda")
            ms = [ctx.path_step_device(d_src.data_ptr(), n, 0, d_next.data_ptr(), d_att.data_ptr(), d_st.data_ptr(), 0, 0, 1, 0,
                                       rtow.F64_FAST, rtow.KERNEL_AUTO, 0, True).kernel_ms for _ in range(7)][2:]
            mi = [ctx.intersect_device(d_src.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST, rtow.KERNEL_AUTO, 0, True).kernel_ms
                  for _ in range(7)][2:]
            row += [label, f"step {min(ms):.4f} ms", f"intersect {min(mi):.4f} ms"]
        print(*row, flush=True)
ctx.close()
