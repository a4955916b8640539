"""T3 on the device: the images the kernels render against the reference's mt19937 stream (GPU).

Everything per ray is held to exact references elsewhere; this module holds the DISTRIBUTION — the samplers' lattices, the
degree-9 sine, the coin, in the build the benchmark times and in the strict one — to the reference's own random stream,
with the statistic of tests/t3_stats.py (derived there; its self-test and the mutants it refuses are
tests/test_t3_stats_host.py).

Reference: 16 batches of 256 spp of the oracle's mt19937 policy per scene at 60x40 (tests/t3_ref.py), one CPU core,
8-16 s per scene, computed once per scene and shared.  Device: 16 batches of 4096 spp, batch b = streams [64 b, 64 b +
64) of a render over 1024 streams, rendered in place with rtow_render_device — 157 M samples per case, tens of
milliseconds of trace kernels in the fast build and about a tenth of a second in the strict one.  Each launch must count
pixels x spp samples and leave the dropped-sample word clear.

The smallest bias of an image mean a case refuses is q_t SE, printed per case: about 1.5e-4 of linear radiance, 0.04 / 255
(DESIGN.md section 3 has the figures of every case).
"""
import numpy as np
import pytest
import torch

import rtow
import t3_ref as tr
import t3_stats as ts
from support_tables import BUILDERS, KERNELS

pytestmark = pytest.mark.gpu

PRECISIONS = {"fast": rtow.F64_FAST, "strict": rtow.F64_STRICT}
KERNEL_OF = dict(KERNELS, auto=rtow.KERNEL_AUTO)
# (scene, kernel, builder): AUTO and one forced walk per scene on the host builder's images, and the device builder's once
CASES = [("static", "auto", "host"), ("static", "bvh", "host"), ("moving", "auto", "host"), ("moving", "bvh", "host"),
         ("suzanne", "auto", "host"), ("suzanne", "bvh", "host"), ("suzanne", "auto", "device")]


@pytest.fixture(scope="module")
def tctx():
    c = rtow.Context(0)
    yield c
    c.close()


def resident(ctx, kind, builder):
    ctx.set_builder(BUILDERS[builder])
    ctx.upload(tr.host_scene(kind))
    assert ctx.build_info().builder == BUILDERS[builder]


def frame(ctx, cfg, buf):
    """(sums [H, W, 3], Stats) of one rtow_render_device call into `buf`; waits for it (a dropped sample is an error)."""
    buf.zero_()
    st = ctx.render_device(cfg, buf.data_ptr(), 0, True)
    return buf.cpu().numpy(), st


def checked(ctx, what, kind, dev, spp, kernel_ms, used):
    ctx.profile_collect()  # raises if any launch since the last collect dropped samples
    try:
        fig = ts.check(tr.mt_batches(kind), dev, what, tr.MT_SPP, spp)
    except ts.T3Error as e:
        if e.figures:
            print(ts.describe(what + " (REFUSED)", e.figures))
        raise
    print(ts.describe(what, fig) + f"; kernel {used}, {kernel_ms:.1f} ms of trace kernels")
    return fig


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("kind,kernel,builder", CASES, ids=["-".join(c) for c in CASES])
def test_device_batches_against_the_mt19937_stream(tctx, kind, kernel, builder, precision):
    resident(tctx, kind, builder)
    buf = torch.zeros((tr.H, tr.W, 3), dtype=torch.float64, device="cuda:0")
    dev, ms, used = np.empty((tr.B, tr.H, tr.W, 3)), 0.0, set()
    for b in range(tr.B):
        cfg = tr.batch_cfg(kind, tr.DEVICE_SPP, b, tr.DEVICE_STREAMS, precision=PRECISIONS[precision],
                           kernel=KERNEL_OF[kernel])
        img, st = frame(tctx, cfg, buf)
        assert st.samples == tr.W * tr.H * tr.DEVICE_SPP, (b, st.samples)
        dev[b] = img / tr.DEVICE_SPP
        ms += st.kernel_ms
        used.add(st.kernel_used)
    assert len(used) == 1 and (kernel == "auto" or used == {KERNEL_OF[kernel]}), used
    checked(tctx, f"{kind}, {kernel}, {builder} builder, {precision}", kind, dev, tr.DEVICE_SPP, ms, used.pop())


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_ragged_frames_folded_by_the_caller(tctx, precision):
    """The frame of 4096 spp over 3 streams — 1365 samples each, one left over: a stream is many levels of the fast
    build's plan with a ragged last one — as two calls of unequal stream ranges whose sums the caller adds; sixteen such
    frames with seeds of their own are the batches."""
    kind = "static"
    resident(tctx, kind, "host")
    spp = tr.RAGGED_SPP // tr.RAGGED_STREAMS * tr.RAGGED_STREAMS
    assert spp == 4095
    buf = torch.zeros((tr.H, tr.W, 3), dtype=torch.float64, device="cuda:0")
    dev, ms, used = np.empty((tr.B, tr.H, tr.W, 3)), 0.0, set()
    for b in range(tr.B):
        first, rest = tr.ragged_cfgs(kind, b, precision=PRECISIONS[precision])
        assert rtow.spp_effective(first) == spp
        a, sa = frame(tctx, first, buf)
        c, sc = frame(tctx, rest, buf)
        assert (sa.samples, sc.samples) == (tr.W * tr.H * spp // 3, tr.W * tr.H * spp * 2 // 3)
        dev[b] = (a + c) / spp
        ms += sa.kernel_ms + sc.kernel_ms
        used |= {sa.kernel_used, sc.kernel_used}
    assert len(used) == 1
    checked(tctx, f"{kind}, ragged 3 x 1365, {precision}", kind, dev, spp, ms, used.pop())
