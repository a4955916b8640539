"""The batches of the device T3 (tests/t3_stats.py): per-batch pixel means of the three scenes at 60x40 under the
reference's mt19937 stream and under the oracle's Philox policy — test infrastructure (numpy + the CPU oracle, no GPU;
importing it loads no library).

mt19937 side.  The mt19937 policy is the one tests/test_oracle_golden.py pins byte for byte to the reference's images.
A batch is one orc.render of MT_SPP samples per pixel with the checker's tree (accel: the same image, bit for bit,
tests/test_oracle_units.py); the generator is process-global and a second render goes on where the first stopped, so B
consecutive renders are B independent batches of one stream, and B more from where they ended (`mt_second`) are a second
set, independent of the first.  The generator is sequential — one thread, 8-16 s
per scene — so every set of batches is computed once per process and shared read-only (`mt_batches`).

Philox side.  One render of B x spp samples over nstreams = B, batch b = stream b alone (stream_first = b,
stream_count = 1), as tests/sample_audit.py selects its samples: `batch_cfg`.  The device's batches are selected the
same way at its own spp, 64 consecutive streams to a batch.
"""
from __future__ import annotations

import functools

import numpy as np

import orc
import rtow
from conftest import GOLDEN

B = 16             # batches per side (tests/t3_stats.py is derived for this number)
W, H = 60, 40
SEED = 31
MT_SPP = 256       # per mt19937 batch
ORACLE_SPP = 1024  # per batch of the Philox oracle (host test)
DEVICE_SPP = 4096  # per device batch (GPU test) ...
DEVICE_STREAMS = 64  # ... as 64 streams of 64
RAGGED_SPP, RAGGED_STREAMS = 4096, 3  # the ragged frame: 3 streams of 1365, one sample of the 4096 left over
KINDS = ("static", "moving", "suzanne")
DEPTH = {"static": 50, "moving": 50, "suzanne": 20}


def oracle_scene(kind, burn=0):
    """The scene through the oracle's own script: resets the global mt19937 and draws the scene from it."""
    if kind == "suzanne":
        s = orc.OrcScene.obj(GOLDEN / "suzanne.obj", 1.5)
    else:
        s = orc.OrcScene.cover(11, 1.5, kind == "moving")
    if burn:
        orc.lib().orc_mt_burn(burn)
    return s


def host_scene(kind):
    """The same scene through the product's host script (the device's input)."""
    if kind == "suzanne":
        return rtow.HostScene.obj(GOLDEN / "suzanne.obj", 1.5)
    return rtow.HostScene.cover(11, 1.5, kind == "moving")


def batch_cfg(kind, spp, b, streams=1, nbatches=B, seed=SEED, **kw):
    """Batch b of nbatches: `streams` consecutive streams of a render of nbatches x spp samples per pixel over nbatches x
    streams streams.  (The strict build traces a stream of a pixel in one thread: 64 streams per batch are 153,600 threads
    of 64 samples where one stream would be 2,400 threads of 4,096.)"""
    assert spp % streams == 0
    return rtow.make_config(W, H, nbatches * spp, nbatches * streams, DEPTH[kind], seed=seed, stream_first=b * streams,
                            stream_count=streams, **kw)


@functools.lru_cache(maxsize=None)
def mt_stream(kind, burn=0):
    """([B, H, W, 3] per-batch pixel means under the reference's mt19937 stream, the doubles the B renders drew, the
    next double of the stream); once per process, read-only."""
    scene = oracle_scene(kind, burn)
    cfg = rtow.make_config(W, H, MT_SPP, 1, DEPTH[kind], seed=SEED)
    out = np.empty((B, H, W, 3))
    draws = 0
    for b in range(B):
        img, st = orc.render(scene, cfg, orc.RNG_MT19937, accel=True)
        assert st.samples == W * H * MT_SPP
        out[b] = img / MT_SPP
        draws += st.rng_doubles
    out.setflags(write=False)
    return out, draws, orc.lib().orc_mt_random_double(0.0, 1.0)


def mt_batches(kind):
    return mt_stream(kind)[0]


def mt_second(kind):
    """A second, independent set of batches: the stream from where the first set ended.  (A burn shorter than what the
    first set draws is NOT independent of it: the second stream is then the first one displaced, the displacement does a
    random walk as the two take different numbers of draws per sample, and once it reaches zero at a sample's start the
    two renders are the same from there on — with the 12,345 draws of tests/test_oracle_units.py the moving cover's two
    streams at this size meet in batch 11 and the last four batches are equal bit for bit.)"""
    return mt_stream(kind, mt_stream(kind)[1])[0]


@functools.lru_cache(maxsize=None)
def philox_batches(kind, spp=ORACLE_SPP, nthreads=8):
    """[B, H, W, 3] per-batch pixel means of the Philox oracle; once per process, read-only."""
    scene = oracle_scene(kind)
    out = np.empty((B, H, W, 3))
    for b in range(B):
        img, st = orc.render(scene, batch_cfg(kind, spp, b, precision=rtow.F64_STRICT), orc.RNG_PHILOX,
                             nthreads=nthreads, accel=True)
        assert st.samples == W * H * spp
        out[b] = img / spp
    out.setflags(write=False)
    return out


def ragged_cfgs(kind, b, **kw):
    """Batch b of the ragged frame: RAGGED_SPP samples asked over RAGGED_STREAMS streams (4095 traced), its own seed, as
    two calls of unequal stream ranges — stream 0 alone, then streams 1 and 2 — whose sums the caller adds."""
    mk = lambda first, count: rtow.make_config(W, H, RAGGED_SPP, RAGGED_STREAMS, DEPTH[kind], seed=SEED + 1 + b,  # noqa: E731
                                               stream_first=first, stream_count=count, **kw)
    return mk(0, 1), mk(1, RAGGED_STREAMS - 1)
