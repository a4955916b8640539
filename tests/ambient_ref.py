"""The ambient query's definition (include/rtow.h, csrc/rtow_ambient.h) in numpy, in the written operand order: every
operation below is one binary64 operation that rounds once, like the strict build's.

Per sample: the Philox block of request 0 (scatter_exact.philox_words, which takes arrays as well as numbers), the lens
point of that block (csrc/rtow_trace_rng.h lens_from_block, with the sine polynomial test_oracle_units.py pins against the
oracle), the height over the disk, the unit normal, Duff et al.'s frame and the direction.  Given one occlusion byte per
ray (rtow_occluded on the exported rays), `fold` adds a point's unoccluded samples in sample order.

Importing this module loads no library.
"""
import numpy as np

import rtow
from scatter_exact import philox_words
from support_oracle import sky_of_strict

HALF_PI = 1.5707963267948966
SIN_C = [float.fromhex(h) for h in ("0x1.ffffffdb33084p-1", "-0x1.555549a9260fdp-3", "0x1.110eb1f04c8ffp-7",
                                     "-0x1.9f6d0201a288bp-13", "0x1.5da8d4e70fe23p-19")]
TMIN = 0.001


def sin_quarter(x):
    x2 = x * x
    return x * (SIN_C[0] + x2 * (SIN_C[1] + x2 * (SIN_C[2] + x2 * (SIN_C[3] + x2 * SIN_C[4]))))


def identities(n, samples, ids=None, sample_first=0):
    """(pixel, sample), each uint64 [n, samples] below 2^32: (ids[i][0], ids[i][1] + sample_first + j), or (i,
    sample_first + j)."""
    if ids is None:
        pixel, first = np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    else:
        ids = np.asarray(ids, dtype=np.uint64).reshape(n, 2)
        pixel, first = ids[:, 0], ids[:, 1]
    sample = (first[:, None] + np.uint64(sample_first) + np.arange(samples, dtype=np.uint64)[None, :]) & np.uint64(0xffffffff)
    return np.broadcast_to(pixel[:, None], sample.shape).copy(), sample


def disk_points(seed, pixel, sample):
    """(px, py) of request 0 of every identity: uniform on the unit disk."""
    w0, w1, w2, w3 = (np.asarray(w, dtype=np.uint64) for w in philox_words(int(seed), pixel, sample, 0))
    b = (w0 & np.uint64(0x7ff)) | ((w1 & np.uint64(0x7ff)) << np.uint64(11)) | ((w2 & np.uint64(0x3ff)) << np.uint64(22))
    rho = np.sqrt(w3.astype(np.float64) * 2.0**-32)
    th = (b & np.uint64(0x3fffffff)).astype(np.float64) * (2.0**-30 * HALF_PI)
    sn, cs = sin_quarter(th), sin_quarter(HALF_PI - th)
    q = b >> np.uint64(30)
    odd = (q & np.uint64(1)) != 0
    cx, sy = np.where(odd, sn, cs), np.where(odd, cs, sn)
    px = rho * np.where((q == 1) | (q == 2), -cx, cx)
    py = rho * np.where(q >= 2, -sy, sy)
    return px, py


def skipped(points):
    """The points that do no walk: normal . normal is 0, subnormal (below 2^-1022), NaN or infinite, or max_dist is NaN
    or below 0.001."""
    N = points["normal"]
    with np.errstate(all="ignore"):
        nn = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        return ~((nn >= 2.0 ** -1022) & (nn < np.inf) & (points["max_dist"] >= TMIN))


def unit_normal(N):
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    return N / length[:, None]


def frame(nh):
    """(t, b) [n, 3] of unit normals nh [n, 3]: Duff et al., "Building an orthonormal basis, revisited"."""
    x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
    s = np.copysign(1.0, z)
    a = -1.0 / (s + z)
    c = (x * y) * a
    sx = s * x
    t = np.stack([1.0 + (sx * x) * a, s * c, -sx], axis=1)
    b = np.stack([c, s + ((y * y) * a), -y], axis=1)
    return t, b


def hemisphere_dirs(nh, px, py):
    """d [n, samples, 3] for unit normals nh [n, 3] and disk points [n, samples]."""
    pz = np.sqrt(np.maximum(1.0 - (px * px + py * py), 0.0))
    t, b = frame(nh)
    return np.stack([(t[:, None, k] * px + b[:, None, k] * py) + nh[:, None, k] * pz for k in range(3)], axis=2)


def rays(points, samples, seed=1, ids=None, sample_first=0):
    """The rays the query walks, a RAY_DTYPE array [n, samples]: (point, d, time, max_dist); the dead ray (all fields 0,
    tmax = -1) in every slot of a skipped point."""
    points = np.ascontiguousarray(points, dtype=rtow.SURFACE_POINT_DTYPE).reshape(-1)
    n = len(points)
    out = np.zeros((n, samples), dtype=rtow.RAY_DTYPE)
    out["tmax"] = -1.0
    live = np.nonzero(~skipped(points))[0]
    if len(live) == 0:
        return out
    pixel, sample = identities(n, samples, ids, sample_first)
    px, py = disk_points(seed, pixel[live], sample[live])
    d = hemisphere_dirs(unit_normal(points["normal"][live]), px, py)
    p = points[live]
    out["origin"][live] = p["point"][:, None, :]
    out["time"][live] = p["time"][:, None]
    out["direction"][live] = d
    out["tmax"][live] = p["max_dist"][:, None]
    return out


def fold(points, ray_array, occluded):
    """The records (an AMBIENT_DTYPE array [n]) of rays [n, samples] given one occlusion answer per ray: the unoccluded
    samples added in sample order from +0.0; a skipped point's record is all +0.0."""
    points = np.ascontiguousarray(points, dtype=rtow.SURFACE_POINT_DTYPE).reshape(-1)
    n, samples = ray_array.shape
    occ = np.asarray(occluded, dtype=bool).reshape(n, samples)
    live = ~skipped(points)
    out = np.zeros(n, dtype=rtow.AMBIENT_DTYPE)
    opened = np.zeros(n)
    bent, sky = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for j in range(samples):
            d = ray_array["direction"][:, j]
            take = live & ~occ[:, j]
            opened = np.where(take, opened + 1.0, opened)
            bent = np.where(take[:, None], bent + d, bent)
            sky = np.where(take[:, None], sky + sky_of_strict(d), sky)
    out["open"], out["bent"], out["sky"] = opened, bent, sky
    out["samples"] = np.where(live, float(samples), 0.0)
    return out
