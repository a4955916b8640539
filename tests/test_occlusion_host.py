"""Occlusion queries, host side (no GPU): the two entry points are exported and refuse a NULL context; ABI 9."""
import ctypes as C

import numpy as np

import rtow


def test_occlusion_symbols_are_exported():
    L = rtow.lib()
    for name in ("rtow_occluded", "rtow_occluded_device"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS


def test_null_context_is_einval():
    L = rtow.lib()
    rays = rtow.make_rays([[0, 0, 0]], [[0, 0, -1]], tmax=1.0)
    out = np.full(1, 0xAB, dtype=np.uint8)
    rc = L.rtow_occluded(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, rays.ctypes.data_as(C.c_void_p), 1,
                         out.ctypes.data_as(C.c_void_p), None)
    assert rc == rtow.RTOW_EINVAL
    assert b"NULL" in L.rtow_last_error()
    assert out[0] == 0xAB
    rc = L.rtow_occluded_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, None, 0, None, None, None)
    assert rc == rtow.RTOW_EINVAL
    assert b"NULL" in L.rtow_last_error()


def test_abi_version_is_9():
    assert rtow.RTOW_ABI_VERSION == 9
    assert rtow.lib().rtow_abi_version() == 9
