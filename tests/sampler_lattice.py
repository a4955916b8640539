"""The Philox policy's samplers restated in numpy, field by field — test infrastructure (no GPU, no library at import).

One request is one Philox block of four 32-bit words (oracle/rtow_oracle.cpp PhiloxDraw, csrc/rtow_trace_rng.h).  The
functions below take the integer FIELDS of a block and return the values the oracle computes from them, operation for
operation in binary64 (numpy rounds every operation once, like the strict build), on arrays:

  block of a new sample:  ju, jv, time = top 21 bits of words 0, 1, 2;  lens_a = word 3;  lens_b = the 11 + 11 + 10 low
                          bits of words 0, 1, 2
  block of a bounce:      kz = top 24 bits of word 0;  kphi = top 24 bits of word 1;  m = the largest of the two halves
                          of word 2 and the low half of word 3;  coin = high half of word 3, low bytes of words 0 and 1

tests/test_sampler_lattices_host.py pins them to orc_philox_request on random blocks and then ENUMERATES the lattices;
tests/test_oracle_units.py::test_philox_requests pins the same layout by hand.
"""
import numpy as np

# the samplers' sine polynomial, operation for operation (oracle sin_quarter, csrc/rtow_trace_rng.h): a Python float or
# a numpy array of binary64, every operation rounding once like the strict build's — one definition for the suite
from ambient_ref import HALF_PI, SIN_C, sin_quarter  # noqa: F401

SIN_ERR = 7e-9  # |sin_quarter(x) - sin x| on [0, pi / 2] (asserted in both test modules)


def sample_fields(w):
    """(ju, jv, time, lens_a, lens_b) of the blocks w [n, 4] uint32."""
    w = np.asarray(w, dtype=np.uint32).reshape(-1, 4).astype(np.uint64)
    low = (w[:, 0] & 0x7ff) | ((w[:, 1] & 0x7ff) << 11) | ((w[:, 2] & 0x3ff) << 22)
    return w[:, 0] >> 11, w[:, 1] >> 11, w[:, 2] >> 11, w[:, 3], low


def bounce_fields(w):
    """(kz, kphi, m, coin) of the blocks w [n, 4] uint32."""
    w = np.asarray(w, dtype=np.uint32).reshape(-1, 4).astype(np.uint64)
    m = np.maximum(np.maximum(w[:, 2] & 0xffff, w[:, 2] >> 16), w[:, 3] & 0xffff)
    coin = ((w[:, 3] >> 16) << 16) | ((w[:, 0] & 0xff) << 8) | (w[:, 1] & 0xff)
    return w[:, 0] >> 8, w[:, 1] >> 8, m, coin


def unit21(k):
    return np.asarray(k, dtype=np.float64) * 2.0**-21


def coin_value(c):
    return np.asarray(c, dtype=np.float64) * 2.0**-32


def radius(m):
    return np.asarray(m, dtype=np.float64) * 2.0**-16


def height(kz):
    return np.asarray(kz, dtype=np.float64) * 2.0**-24


def azimuth(kphi):
    """(cos, sin) of the azimuth kphi * 2^-24 * pi / 2."""
    phi = np.asarray(kphi, dtype=np.float64) * (2.0**-24 * HALF_PI)
    return sin_quarter(HALF_PI - phi), sin_quarter(phi)


def ball_point(kz, kphi, m):
    """The point of the unit ball's positive octant: [n, 3]."""
    z, r = height(kz), radius(m)
    cs, sn = azimuth(kphi)
    rs = r * np.sqrt(1.0 - z * z)
    return np.stack([rs * cs, rs * sn, r * z], axis=-1)


def lens_angle(k30):
    """(cos, sin) of the angle k30 * 2^-30 * pi / 2 inside its quadrant."""
    th = np.asarray(k30, dtype=np.float64) * (2.0**-30 * HALF_PI)
    return sin_quarter(HALF_PI - th), sin_quarter(th)


def lens_point(a, b):
    """The point of the unit disk: [n, 2]; a the radius word, b the angle word (top two bits: the quadrant)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    rho = np.sqrt(a.astype(np.float64) * 2.0**-32)
    cs, sn = lens_angle(b & 0x3fffffff)
    q = b >> 30
    odd = (q & 1) == 1
    cx, sy = np.where(odd, sn, cs), np.where(odd, cs, sn)
    return np.stack([rho * np.where((q == 1) | (q == 2), -cx, cx), rho * np.where(q >= 2, -sy, sy)], axis=-1)
