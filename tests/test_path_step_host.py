"""Path-step queries, host side (no GPU): the two entry points are exported and declared, the ABI version stays, the
parameter block has its C layout, and a NULL context is refused."""
import ctypes as C
import re

import numpy as np

import rtow
from conftest import REPO

NAMES = ("rtow_path_step", "rtow_path_step_device")


def test_path_step_symbols_are_exported_and_declared():
    L = rtow.lib()
    header = (REPO / "include" / "rtow.h").read_text()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "rtow_step_params_t" in header
    for word, value in (("MISS", 0), ("SCATTERED", 1), ("ABSORBED", 2), ("SKIPPED", 3)):
        assert re.search(rf"#define\s+RTOW_STEP_{word}\s+{value}\b", header), word
        assert getattr(rtow, "STEP_" + word) == value


def test_abi_version_is_unchanged():
    assert rtow.lib().rtow_abi_version() == 9 == rtow.RTOW_ABI_VERSION
    assert hasattr(rtow.lib(), "rtow_path_step")


def test_params_layout():
    assert C.sizeof(rtow.StepParams) == 16
    P = rtow.StepParams
    assert (P.seed.offset, P.bounce.offset, P.sample_first.offset) == (0, 8, 12)


def test_null_context_is_einval():
    L = rtow.lib()
    rays = rtow.make_rays([[0, 0, 0]], [[0, 0, -1]])
    nxt = np.zeros(1, dtype=rtow.RAY_DTYPE)
    atten = np.zeros((1, 3))
    status = np.zeros(1, dtype=np.int32)
    prm = rtow.StepParams(1, 0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.rtow_path_step(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), p(rays), 1, None, p(nxt), p(atten),
                          p(status), None, None)
    assert rc == rtow.RTOW_EINVAL
    assert b"ctx is NULL" in L.rtow_last_error()
    rc = L.rtow_path_step_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, C.byref(prm), None, 0, None, None, None, None,
                                 None, None, None)
    assert rc == rtow.RTOW_EINVAL
    assert b"ctx is NULL" in L.rtow_last_error()
