#!/usr/bin/env python3
"""Device time of the first-hit guide buffers (rtow_guides_device) beside the two ways a caller had before, fast build,
AUTO kernel.

Per scene (cover, moving cover, suzanne, the 96.8k-triangle mesh) at W x H x spp, in one process on one context:
  guides      rtow_guides_device: camera, walk and fold fused, 64 bytes written per pixel;
  rays + hit  rtow_camera_rays_device (W H spp rays of 64 bytes written) followed by rtow_intersect_device on the same
              primaries (read again, W H spp hit records of 72 bytes written) — the composition a caller builds from the
              other entry points, without the gather and the fold it would still have to run;
  render d0   rtow_render_device with max_child_rays = 0: the render's own first segment (camera, walk, sky);
  hit, tiled  rtow_intersect_device on the same primaries put into the guides kernel's bundle order — a wave's 64 rays are
              one sample of each pixel of an 8 x 8 tile instead of the 16 samples of 4 neighbouring pixels — which tells
              how much of a difference between the first two is the shape of the bundle a wave walks with.
Times are stats.kernel_ms (HIP events around the kernel), best of `--repeats` calls after `--warmup`, with the slowest;
rtow_camera_rays_device takes no stats and is timed with an event pair around the call on the same stream (its counter
memset included).  The node + primitive tests per primary say how far the walks are comparable.

   python scripts/bench_guides.py [--width 1200] [--spp 16] [--scenes cover,moving,suzanne,mesh96k] [--warmup 2]
                                  [--repeats 5] [--json OUT]
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


class Ms:
    def __init__(self, ms):
        self.kernel_ms = ms


def best_of(call, warmup, repeats):
    for _ in range(warmup):
        call()
    runs = [call() for _ in range(repeats)]
    ms = [st.kernel_ms for st in runs]
    return runs[int(np.argmin(ms))], min(ms), max(ms)


def tile_order(W, H, spp):
    """Ray indices (pixel-major, sample-minor) in the guides kernel's bundle order: tiles of 8 x 8 pixels row-major, inside a
    tile sample-major, the tile's pixels row-major."""
    ty, tx = (H + 7) // 8, (W + 7) // 8
    y = (np.arange(ty)[:, None, None, None, None] * 8 + np.arange(8)[None, None, None, :, None])
    x = (np.arange(tx)[None, :, None, None, None] * 8 + np.arange(8)[None, None, None, None, :])
    s = np.arange(spp)[None, None, :, None, None]
    ok = np.broadcast_to((y < H) & (x < W), (ty, tx, spp, 8, 8))
    idx = np.broadcast_to((y * W + x) * spp + s, (ty, tx, spp, 8, 8))
    return idx[ok].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--scenes", default="cover,moving,suzanne,mesh96k")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    ctx = rtow.Context(0)
    rows = []
    print(f"# fast build, AUTO kernel, {a.spp} spp; kernel ms, best of {a.repeats} after {a.warmup} (slowest) | tests per primary")
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            scene, aspect = scene_of(name, tmp)
            ctx.upload(scene)
            W = a.width
            H = rtow.image_height(W, aspect)
            n = W * H * a.spp
            cfg = rtow.make_config(W, H, a.spp, 1, 0, seed=1, precision=rtow.F64_FAST)
            d_g = torch.zeros((H * W, 8), dtype=torch.float64, device="cuda")
            d_rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
            d_ids = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
            d_hits = torch.zeros((n, 9), dtype=torch.float64, device="cuda")
            out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def camera():
                e0.record()
                ctx.camera_rays_device(cfg, d_rays.data_ptr(), d_ids.data_ptr(), 0)
                e1.record()
                e1.synchronize()
                return Ms(e0.elapsed_time(e1))

            g, g_ms, g_max = best_of(lambda: ctx.guides_device(cfg, d_g.data_ptr(), 0, True), a.warmup, a.repeats)
            _, c_ms, c_max = best_of(camera, a.warmup, a.repeats)
            q, q_ms, q_max = best_of(lambda: ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST,
                                                                  rtow.KERNEL_AUTO, 0, True), a.warmup, a.repeats)
            r, r_ms, r_max = best_of(lambda: ctx.render_device(cfg, out.data_ptr(), 0, True), a.warmup, a.repeats)
            order = torch.from_numpy(tile_order(W, H, a.spp)).to("cuda")
            assert order.numel() == n
            d_tiled = d_rays[order].contiguous()
            del order
            t, t_ms, t_max = best_of(lambda: ctx.intersect_device(d_tiled.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST,
                                                                  rtow.KERNEL_AUTO, 0, True), a.warmup, a.repeats)
            q = ctx.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), rtow.F64_FAST, rtow.KERNEL_AUTO, 0, True)
            # the same primaries: the guides' hit counts are the intersect's hits per pixel
            hits_g = float(d_g[:, 7].sum().item())
            hits_q = int(torch.isfinite(d_hits[:, 0]).sum().item())
            row = dict(scene=name, width=W, height=H, spp=a.spp, primaries=n, kernel_used=int(g.kernel_used),
                       guides_ms=g_ms, guides_ms_max=g_max, camera_rays_ms=c_ms, camera_rays_ms_max=c_max,
                       intersect_ms=q_ms, intersect_ms_max=q_max, composed_ms=c_ms + q_ms,
                       intersect_tiled_ms=t_ms, intersect_tiled_ms_max=t_max,
                       intersect_tiled_tests_per_primary=(t.node_tests + t.prim_tests) / n,
                       render_d0_ms=r_ms, render_d0_ms_max=r_max, render_kernel=int(r.kernel_used),
                       guides_tests_per_primary=(g.node_tests + g.prim_tests) / n,
                       intersect_tests_per_primary=(q.node_tests + q.prim_tests) / n,
                       render_tests_per_primary=(r.node_tests + r.prim_tests) / max(r.segments, 1),
                       hits_guides=hits_g, hits_intersect=hits_q, finite=bool(torch.isfinite(d_g).all().item()))
            row["guides_over_composed"] = g_ms / (c_ms + q_ms)
            row["guides_over_render_d0"] = g_ms / r_ms
            rows.append(row)
            print(f"{name:8s} {W}x{H} kernel {row['kernel_used']} | guides {g_ms:7.3f} ms ({g_max:.3f}) "
                  f"{row['guides_tests_per_primary']:.1f} tests | camera_rays {c_ms:7.3f} ms ({c_max:.3f}) + intersect "
                  f"{q_ms:7.3f} ms ({q_max:.3f}) {row['intersect_tests_per_primary']:.1f} tests = {c_ms + q_ms:7.3f} ms | "
                  f"render d0 {r_ms:7.3f} ms ({r_max:.3f}) {row['render_tests_per_primary']:.1f} tests | guides / composed "
                  f"{row['guides_over_composed']:.2f}, guides / render d0 {row['guides_over_render_d0']:.2f} | intersect in "
                  f"tile order {t_ms:7.3f} ms ({t_max:.3f}) | hits {hits_g:.0f} / {hits_q}", flush=True)
            del d_g, d_rays, d_ids, d_hits, d_tiled, out
    ctx.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
