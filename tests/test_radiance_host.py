"""Radiance queries, host side (no GPU): the two entry points are exported and declared, the ABI version stays, the
parameter block has its C layout, and a NULL context is refused."""
import ctypes as C
import re

import numpy as np

import rtow
from conftest import REPO

NAMES = ("rtow_radiance", "rtow_radiance_device")


def test_radiance_symbols_are_exported_and_declared():
    L = rtow.lib()
    header = (REPO / "include" / "rtow.h").read_text()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "rtow_radiance_params_t" in header


def test_abi_version_is_unchanged():
    assert rtow.lib().rtow_abi_version() == 9 == rtow.RTOW_ABI_VERSION


def test_params_layout():
    assert C.sizeof(rtow.RadianceParams) == 24
    P = rtow.RadianceParams
    assert (P.seed.offset, P.samples_per_ray.offset, P.max_child_rays.offset, P.sample_first.offset, P.pad_.offset) == \
        (0, 8, 12, 16, 20)


def test_null_context_is_einval():
    L = rtow.lib()
    rays = rtow.make_rays([[0, 0, 0]], [[0, 0, -1]])
    out = np.zeros((1, 3))
    prm = rtow.RadianceParams(1, 1, 50, 0, 0)
    rc = L.rtow_radiance(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), rays.ctypes.data_as(C.c_void_p), 1, None,
                         out.ctypes.data_as(C.c_void_p), None)
    assert rc == rtow.RTOW_EINVAL
    assert b"ctx is NULL" in L.rtow_last_error()
    rc = L.rtow_radiance_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), None, 0, None, None, None, None)
    assert rc == rtow.RTOW_EINVAL
    assert b"ctx is NULL" in L.rtow_last_error()
