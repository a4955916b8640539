"""Ambient queries, host side (no GPU): the two entry points are exported and declared, the ABI version stays, the
records have their C layouts, the argument errors that need no device are reported, and the numpy mirror of the definition
(ambient_ref.py) samples what the definition says: a cosine-weighted hemisphere around an orthonormal frame."""
import ctypes as C
import math
import re

import numpy as np

import ambient_ref
import rtow
from conftest import REPO

NAMES = ("rtow_ambient", "rtow_ambient_device")


def test_ambient_symbols_are_exported_and_declared():
    L = rtow.lib()
    header = (REPO / "include" / "rtow.h").read_text()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for word in ("rtow_surface_point_t", "rtow_ambient_params_t", "rtow_ambient_t"):
        assert word in header
    assert re.search(r"#define\s+RTOW_MAX_AMBIENT_SAMPLES\s+65536\b", header)
    assert rtow.MAX_AMBIENT_SAMPLES == 65536


def test_abi_version_is_unchanged():
    assert rtow.lib().rtow_abi_version() == 9 == rtow.RTOW_ABI_VERSION
    assert hasattr(rtow.lib(), "rtow_ambient")


def test_record_layouts():
    assert (C.sizeof(rtow.SurfacePoint), C.sizeof(rtow.AmbientParams), C.sizeof(rtow.Ambient)) == (64, 16, 64)
    S, P, A = rtow.SurfacePoint, rtow.AmbientParams, rtow.Ambient
    assert (S.point.offset, S.time.offset, S.normal.offset, S.max_dist.offset) == (0, 24, 32, 56)
    assert (P.seed.offset, P.samples.offset, P.sample_first.offset) == (0, 8, 12)
    assert (A.open.offset, A.bent.offset, A.sky.offset, A.samples.offset) == (0, 8, 32, 56)
    assert rtow.SURFACE_POINT_DTYPE.itemsize == 64 and rtow.AMBIENT_DTYPE.itemsize == 64
    # the layout of rtow_ray_t: point / origin, time, normal / direction, max_dist / tmax
    assert [rtow.SURFACE_POINT_DTYPE.fields[k][1] for k in ("point", "time", "normal", "max_dist")] == \
        [rtow.RAY_DTYPE.fields[k][1] for k in ("origin", "time", "direction", "tmax")]
    q = rtow.make_surface_points([[1, 2, 3], [4, 5, 6]], [[0, 0, 2], [0, -1, 0]], time=[0.25, 0.5], max_dist=2.0)
    assert q.dtype == rtow.SURFACE_POINT_DTYPE and q.shape == (2,)
    assert q["point"][1].tolist() == [4, 5, 6] and q["normal"][0].tolist() == [0, 0, 2]
    assert q["time"].tolist() == [0.25, 0.5] and q["max_dist"].tolist() == [2.0, 2.0]
    assert math.isinf(rtow.make_surface_points([[0, 0, 0]], [[0, 1, 0]])["max_dist"][0])


def test_argument_errors_without_a_device():
    L = rtow.lib()
    pts = rtow.make_surface_points([[0, 0, 0]], [[0, 1, 0]])
    out = np.zeros(1, dtype=rtow.AMBIENT_DTYPE)
    prm = rtow.AmbientParams(1, 4, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.rtow_ambient(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), p(pts), 1, None, p(out), None, None)
    assert rc == rtow.RTOW_EINVAL and b"ctx is NULL" in L.rtow_last_error()
    rc = L.rtow_ambient_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), None, 0, None, None, None, None, None)
    assert rc == rtow.RTOW_EINVAL and b"ctx is NULL" in L.rtow_last_error()


# ------------------------------------------------------------------------------------- the mirror's sampling ---
def test_mirror_samples_a_cosine_weighted_hemisphere():
    """2^16 seeded samples around one tilted normal: every direction lies in the normal's hemisphere, the mean of d . n
    is the cosine-weighted 2/3 (variance 1/2 - 4/9 = 1/18) within four standard errors, and |d| is 1 to the sine
    polynomial's 2e-8."""
    n_samples = 1 << 16
    N = np.array([[0.3, -1.7, 0.9]])
    pts = rtow.make_surface_points([[0.5, 0.25, -1.0]], N, time=0.5, max_dist=3.0)
    r = ambient_ref.rays(pts, n_samples, seed=20261021, ids=[[77, 5]], sample_first=11)
    assert r.shape == (1, n_samples)
    d = r["direction"][0]
    nh = ambient_ref.unit_normal(N)[0]
    cos = d @ nh
    assert np.all(cos >= 0.0)
    assert abs(cos.mean() - 2.0 / 3.0) <= 4.0 * math.sqrt(1.0 / 18.0 / n_samples), cos.mean()
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 2e-8
    # the rest of the ray is the point's
    assert np.all(r["origin"] == pts["point"][0]) and np.all(r["time"] == 0.5) and np.all(r["tmax"] == 3.0)
    # the identity: the same samples through ids and through sample_first
    again = ambient_ref.rays(pts, 16, seed=20261021, ids=[[77, 10]], sample_first=6)
    assert again.tobytes() == r[:, :16].tobytes()


def test_mirror_frame_is_orthonormal():
    """(t, b, n) of 10^4 seeded unit normals, the poles and normals with -0.0 components: unit length and mutually
    orthogonal to 1e-15."""
    g = np.random.default_rng(5)
    N = g.normal(size=(10000, 3))
    special = np.array([[0, 0, 1], [0, 0, -1], [-0.0, 0.0, 1], [0.0, -0.0, -1], [1, 0, 0.0], [1, 0, -0.0], [0, -1, -0.0],
                        [-0.0, -0.0, 1], [0.6, -0.0, -0.8], [-0.0, 0.6, 0.8]], dtype=np.float64)
    nh = ambient_ref.unit_normal(np.concatenate([special, N]))
    t, b = ambient_ref.frame(nh)
    assert np.all(np.isfinite(t)) and np.all(np.isfinite(b))
    dot = lambda u, v: (u * v).sum(axis=1)  # noqa: E731
    for u, v, want in ((t, t, 1.0), (b, b, 1.0), (nh, nh, 1.0), (t, b, 0.0), (t, nh, 0.0), (b, nh, 0.0)):
        assert np.abs(dot(u, v) - want).max() <= 1e-15


def test_mirror_skips_and_folds():
    """A zero, NaN or infinite normal and a max_dist that is NaN or below 0.001 give dead rays and a zero record; the
    fold adds the unoccluded samples in order."""
    pts = rtow.make_surface_points(np.zeros((7, 3)), [[0, 1, 0], [0, 0, 0], [math.nan, 1, 0], [math.inf, 0, 0], [0, 1, 0],
                                                      [0, 1, 0], [0, 1, 0]],
                                   max_dist=[1.0, 1.0, 1.0, 1.0, math.nan, 0.0009, -1.0])
    assert ambient_ref.skipped(pts).tolist() == [False] + [True] * 6
    # a subnormal normal . normal (lengths 1e-155 to 1e-161) is skipped; 2e-154, whose square is a normal binary64, is live
    small = rtow.make_surface_points(np.zeros((6, 3)), [[1e-155, 0, 0], [0, -1e-158, 0], [0, 0, 1e-160], [-1e-161, 0, 0],
                                                        [0, 2e-154, 0], [2.0 ** -511, 0, 0]])
    assert ambient_ref.skipped(small).tolist() == [True] * 4 + [False] * 2
    rs = ambient_ref.rays(small, 3, seed=4)
    assert np.all(rs["tmax"][:4] == -1.0) and not rs["direction"][:4].any()
    assert np.abs(np.sqrt((rs["direction"][4:] ** 2).sum(axis=2)) - 1.0).max() <= 2e-8
    r = ambient_ref.rays(pts, 3, seed=4)
    assert np.all(r["tmax"][1:] == -1.0) and np.all(r["tmax"][0] == 1.0)
    dead = r[1:].copy()
    dead["tmax"] = 0.0
    assert not dead.view(np.uint8).any()
    occ = np.array([[False, True, False]] * 7)
    rec = ambient_ref.fold(pts, r, occ)
    assert not rec[1:].view(np.uint8).any()
    assert rec["open"][0] == 2.0 and rec["samples"][0] == 3.0
    assert np.array_equal(rec["bent"][0], (0.0 + r["direction"][0, 0]) + r["direction"][0, 2])
