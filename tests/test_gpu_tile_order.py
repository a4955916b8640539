"""The queue order of the tiles is a hint (GPU): tracing the empty tiles last, and buying them several levels at a time,
changes when a pixel is traced and never what is rendered.  Every build's image and the launch counters are compared,
array for array, between a context with the ordering on (the default) and one with RTOW_TILE_ORDER=0 — one queue
segment, the row order alone — and the strict image with the oracle's.  The frame (480x320, 20 spp: 2,400 tiles, a
few hundred of them empty in the cover scene, two levels in the fast builds) gives the empty segment more batches
than one wave takes.  A refit that moves geometry into tiles that were empty must drop the cached table.

(Status: not yet run on a GPU; the host-side half of the same claims is tests/test_tile_order_host.py.)"""
import numpy as np
import pytest
import torch

import orc
import rtow
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

W, H, SPP = 480, 320, 20


def _scene(name):
    if name == "suzanne":
        return rtow.HostScene.obj(GOLDEN / "suzanne.obj", W / H)
    return rtow.HostScene.cover(11, W / H, name == "cover_moving")


def _contexts(monkeypatch, **env):
    """(ordering on, ordering off): the knobs are read when a context is created."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("RTOW_TILE_ORDER", raising=False)
    on = rtow.Context(0)
    monkeypatch.setenv("RTOW_TILE_ORDER", "0")
    off = rtow.Context(0)
    monkeypatch.delenv("RTOW_TILE_ORDER")
    return on, off


@pytest.mark.parametrize("name", ["cover", "cover_moving", "suzanne"])
@pytest.mark.parametrize("nranks,rank,tile_rows", [(1, 0, 8), (8, 3, 8), (8, 3, 4)])
def test_ordering_on_equals_ordering_off_in_every_build(monkeypatch, name, nranks, rank, tile_rows):
    scene = _scene(name)
    on, off = _contexts(monkeypatch)
    try:
        for precision in (rtow.F64_STRICT, rtow.F64_FAST, rtow.F32):
            cfg = rtow.make_config(W, H, SPP, 2, 50, seed=7, precision=precision, rank=rank, nranks=nranks,
                                   tile_rows=tile_rows)
            a, sa = on.render(scene, cfg)
            b, sb = off.render(scene, cfg)
            assert np.array_equal(a, b), (name, precision)
            assert (sa.samples, sa.segments) == (sb.samples, sb.segments), (name, precision)
            assert sa.samples == len(rtow.local_rows(cfg)) * W * SPP
            if precision == rtow.F64_STRICT:
                ref, ost = orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=8, accel=name == "suzanne")
                assert np.array_equal(a, ref), name
                assert sa.segments == ost.segments
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("levels", ["1", "2", "5", "16"])
def test_levels_bought_at_once_do_not_change_the_image(monkeypatch, levels):
    """RTOW_EMPTY_LEVELS: the size of a batch in the empty segment, up to more levels than the launch has."""
    scene = _scene("cover")
    on, off = _contexts(monkeypatch, RTOW_EMPTY_LEVELS=levels)
    try:
        for precision, spp in ((rtow.F64_FAST, 60), (rtow.F64_STRICT, 20)):
            cfg = rtow.make_config(W, H, spp, 2, 50, seed=3, precision=precision)
            a, sa = on.render(scene, cfg)
            b, sb = off.render(scene, cfg)
            assert np.array_equal(a, b) and (sa.samples, sa.segments) == (sb.samples, sb.segments)
    finally:
        on.close()
        off.close()


def test_refit_into_empty_tiles_drops_the_cached_order():
    """Resident scene: render, move the small spheres up into what was sky, refit, render again — the second image is the
    image a fresh context makes of the moved scene (the table of the first render would trace those tiles in the empty
    segment; the image must not care, and the table must be rebuilt: both orders give this image)."""
    scene = rtow.HostScene.cover(11, W / H, False)
    cfg = rtow.make_config(W, H, SPP, 2, 50, seed=5, precision=rtow.F64_FAST)
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    ctx, fresh = rtow.Context(0), rtow.Context(0)
    try:
        ctx.upload(scene)
        ctx.render_device(cfg, buf.data_ptr())
        torch.cuda.synchronize()
        first = buf.cpu().numpy().copy()
        ctx.render_device(cfg, buf.data_ptr())  # (the cached table)
        torch.cuda.synchronize()
        assert np.array_equal(first, buf.cpu().numpy())
        s = scene.c
        for i in range(1, s.n_spheres):
            if abs(s.sphere_geom[4 * i + 3]) < 0.5:
                s.sphere_geom[4 * i + 1] += 2.5 + 0.01 * (i % 50)
        ctx.refit(scene)
        st = ctx.render_device(cfg, buf.data_ptr(), want_stats=True)
        torch.cuda.synchronize()
        second = buf.cpu().numpy().copy()
        ref, rst = fresh.render(scene, cfg)
        assert not np.array_equal(first, second)
        assert np.array_equal(second, ref)
        assert (st.samples, st.segments) == (rst.samples, rst.segments)
    finally:
        ctx.close()
        fresh.close()
