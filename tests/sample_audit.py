"""Sample audit: a rendered frame against its own samples, one sample at a time — test infrastructure (numpy + ctypes,
importable without a GPU).

A render of a stream range traces "the sample indices and random numbers of the full render" (include/rtow.h).  With
nstreams = spp_eff, stream_first = j, stream_count = 1 every build's schedule is one level of one sample at index j
(`sample_cfg`), so the image of that call is the colour c_j of sample j of every pixel, made by the kernel instantiation
that traces the full frame.  The full frame is by contract a fixed-order fold of those colours (`fold`):

    level k = (first, count):  s_k = +0.0;  s_k = s_k + c_j   for j = first .. first + count - 1
    pixel:                     g = +0.0;    g = s_k + g       for k ascending

(csrc/rtow_trace_body.h: an item's sum is sequential, donated colours are added in sample order; csrc/rtow_reduce.hip:
g = partial[k] + g).  So a frame can be compared with the fold of its samples bit for bit, pixel for pixel, and the
samples of two builds can be compared identity by identity (`census`).

`contracted_oracle` is the unchanged oracle source built with -ffp-contract=fast -mfma: the reference's algorithm under
FMA contraction on the CPU, a reference-side measure of how many samples rounding alone moves (`reference_census`).
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import orc
import rtow
from conftest import GOLDEN

_pd = C.POINTER(C.c_double)
CONTRACTED_LIB = orc.ORC_DIR / "liboracle_contracted.so"
# the project's thresholds for "the same value" between the strict and the fast build (tests/test_gpu_parity.py)
TIGHT_RTOL, TIGHT_ATOL = 1e-9, 1e-12
LOOSE_ABS = 1e-3

# the frames whose samples the fast build is compared with the strict build's, and the contracted oracle with the
# oracle's: name -> (scene, width, height, spp, max_child_rays, seed)
FRAMES = {
    "cover": (lambda: rtow.HostScene.cover(11, 1.5, False), 240, 160, 24, 50, 7),
    "cover_moving": (lambda: rtow.HostScene.cover(11, 1.5, True), 240, 160, 24, 50, 7),
    "suzanne": (lambda: rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9), 320, 180, 16, 20, 7),
    # (the query API against the render: smaller frames)
    "cover_small": (lambda: rtow.HostScene.cover(11, 1.5, False), 120, 80, 24, 50, 7),
    "suzanne_small": (lambda: rtow.HostScene.obj(GOLDEN / "suzanne.obj", 1.5), 120, 80, 24, 20, 7),
}


def frame(name, precision=rtow.F64_FAST, kernel=rtow.KERNEL_AUTO):
    """(scene, cfg) of FRAMES[name]."""
    mk, w, h, spp, depth, seed = FRAMES[name]
    return mk(), rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=precision, kernel=kernel)


def copy_cfg(cfg, **changes):
    out = rtow.Config.from_buffer_copy(cfg)
    for k, v in changes.items():
        setattr(out, k, v)
    return out


def sample_cfg(cfg, j):
    """The config of sample j of `cfg` alone: one stream per sample, stream j only; everything else unchanged."""
    spp_eff = rtow.spp_effective(cfg)
    assert 0 <= j < spp_eff
    return copy_cfg(cfg, nstreams=spp_eff, samples_per_pixel=spp_eff, stream_first=j, stream_count=1)


def levels(ctx, cfg):
    """The (first sample, count) pairs of rtow_debug_schedule.  `ctx`: a Context (its knobs, and the item length of the
    class of its RESIDENT scene: upload first) or None (a new context's table, pure host arithmetic)."""
    cap = 4096
    pairs = (C.c_uint32 * (2 * cap))()
    n = rtow.lib().rtow_debug_schedule(ctx._h if ctx is not None else None, C.byref(cfg), pairs, cap)
    if n < 0:
        rtow.check(n, "rtow_debug_schedule")
    assert n <= cap
    return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(n)]


def covers(lv, n):
    """Do the levels cut [0, n) into contiguous ascending ranges?"""
    at = 0
    for first, count in lv:
        if first != at or count <= 0:
            return False
        at += count
    return at == n


def fold(lv, c):
    """The device's sum of the colours c [spp_eff, rows, W, 3] under the levels `lv`: level sums in sample order from
    +0.0, then g = s_k + g over the levels in the order given, from +0.0."""
    c = np.asarray(c, dtype=np.float64)
    g = np.zeros(c.shape[1:])
    for first, count in lv:
        s = np.zeros(c.shape[1:])
        for j in range(first, first + count):
            s = s + c[j]
        g = s + g
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differing_pixels(a, b):
    """[rows, W] bool: pixels whose three sums do not all have the same bits."""
    return (bits(a) != bits(b)).any(axis=-1)


Census = collections.namedtuple("Census", "n equal tight loose tight_mask loose_mask max_abs")


def census(a, b):
    """Samples of `a` against the same samples of the reference `b` ([..., 3] each), in three classes: equal bits on all
    three channels; tight: not isclose(rtol=1e-9, atol=1e-12) on all three; loose: some channel with |a - b| > 1e-3 (a
    channel that is not finite counts as loose).  The masks have the shape of a[..., 0]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.shape[-1] == 3
    equal = (bits(a) == bits(b)).all(axis=-1)
    tight = ~np.isclose(a, b, rtol=TIGHT_RTOL, atol=TIGHT_ATOL).all(axis=-1)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
        loose = (~(d <= LOOSE_ABS)).any(axis=-1)
    return Census(equal.size, int(equal.sum()), int(tight.sum()), int(loose.sum()), tight, loose,
                  float(np.nanmax(d)) if d.size else 0.0)


def describe_loose(cen, a, b, limit=1000):
    """One line per loose sample: (sample, row, column) and both colours."""
    out = []
    for idx in np.argwhere(cen.loose_mask)[:limit]:
        t = tuple(int(i) for i in idx)
        out.append(f"  loose at {t}: {a[t].tolist()} against {b[t].tolist()}")
    return "\n".join(out)


# ------------------------------------------------------------------------------------------ the oracle's samples ---
def host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma" in line
    except OSError:
        pass
    return False


_contracted = None


def contracted_oracle():
    """ctypes handle of oracle/liboracle_contracted.so (built on demand, like orc.lib()): orc_render_ex and
    orc_scatter."""
    global _contracted
    if _contracted is not None:
        return _contracted
    if not host_has_fma():
        raise RuntimeError("the contracted oracle needs a host CPU with FMA (no `fma` among the flags of /proc/cpuinfo): "
                           "the reference-side census cannot be taken on this machine")
    srcs = [orc.ORC_DIR / f for f in ("rtow_oracle.cpp", "rtow_oracle.h", "Makefile")]
    if not CONTRACTED_LIB.exists() or any(s.stat().st_mtime > CONTRACTED_LIB.stat().st_mtime for s in srcs):
        subprocess.run(["make", "-C", str(orc.ORC_DIR), CONTRACTED_LIB.name], check=True, capture_output=True)
    L = C.CDLL(str(CONTRACTED_LIB))
    L.orc_render_ex.argtypes = [C.POINTER(rtow.Scene), C.POINTER(rtow.Config), C.c_int, C.c_int, C.c_int, _pd,
                                C.POINTER(orc.OrcStats)]
    orc.bind_scatter(L)
    _contracted = L
    return L


def cpu_threads():
    return max(1, min(16, os.cpu_count() or 1))


def oracle_render(scene, cfg, contracted=False, accel=True):
    """(sums [rows, W, 3], OrcStats) of the oracle (Philox), or of its contracted build."""
    if not contracted:
        return orc.render(scene, cfg, orc.RNG_PHILOX, nthreads=cpu_threads(), accel=accel)
    out = np.zeros((len(rtow.local_rows(cfg)), cfg.image_width, 3))
    st = orc.OrcStats()
    rc = contracted_oracle().orc_render_ex(C.byref(scene.c), C.byref(cfg), orc.RNG_PHILOX, cpu_threads(), int(accel),
                                           out.ctypes.data_as(_pd), C.byref(st))
    if rc != 0:
        raise RuntimeError(f"orc_render_ex (contracted) failed: {rc}")
    return out, st


def oracle_samples(scene, cfg, contracted=False):
    """(c [spp_eff, rows, W, 3], total segments): the oracle's one-sample frames of `cfg`."""
    c, segments = [], 0
    for j in range(rtow.spp_effective(cfg)):
        img, st = oracle_render(scene, sample_cfg(cfg, j), contracted)
        assert st.samples == img.shape[0] * img.shape[1]
        c.append(img)
        segments += st.segments
    return np.stack(c), segments


@functools.lru_cache(maxsize=None)
def oracle_stack(name, contracted=False):
    """FRAMES[name]: (c [spp, H, W, 3], total segments) of the oracle's (or the contracted oracle's) one-sample frames —
    computed once per process and shared; read-only."""
    scene, cfg = frame(name, rtow.F64_STRICT)
    c, seg = oracle_samples(scene, cfg, contracted)
    c.setflags(write=False)
    return c, seg


def reference_census(name):
    """FRAMES[name]: (census of the contracted oracle's samples against the oracle's, segments of either) — taken on the
    CPU, never from the code under test."""
    plain, seg = oracle_stack(name)
    fused, fseg = oracle_stack(name, True)
    return census(fused, plain), seg, fseg


# ------------------------------------------------------------------------------------------------ the fold check ---
class AuditError(AssertionError):
    pass


def check_fold(full, lv, c, what=""):
    """`full` [rows, W, 3] must be the fold of its samples `c` under the levels `lv`, which must cut [0, len(c)) into
    contiguous ranges — every bit of every pixel.  Raises AuditError naming the first pixels that differ."""
    if not covers(lv, len(c)):
        raise AuditError(f"{what}: the levels {lv} do not cut [0, {len(c)}) into contiguous ranges")
    want = fold(lv, c)
    if want.shape != np.shape(full):
        raise AuditError(f"{what}: frame {np.shape(full)} against samples {want.shape}")
    bad = differing_pixels(full, want)
    if bad.any():
        first = [tuple(int(i) for i in p) for p in np.argwhere(bad)[:5]]
        raise AuditError(f"{what}: {int(bad.sum())} of {bad.size} pixels are not the fold of their samples; first "
                         f"(row, column): {first}; e.g. {np.asarray(full)[first[0]].tolist()} against "
                         f"{want[first[0]].tolist()}")
