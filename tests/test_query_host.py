"""Ray queries, host side (no GPU): the two entry points are exported, refuse a NULL context, and the ctypes and numpy
views of rtow_ray_t / rtow_hit_t have the C layouts of include/rtow.h."""
import ctypes as C

import numpy as np

import rtow


def test_query_symbols_are_exported():
    L = rtow.lib()
    for name in ("rtow_intersect", "rtow_intersect_device"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS


def test_null_context_is_einval():
    L = rtow.lib()
    rays = rtow.make_rays([[0, 0, 0]], [[0, 0, -1]])
    hits = np.zeros(1, dtype=rtow.HIT_DTYPE)
    rc = L.rtow_intersect(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, rays.ctypes.data_as(C.c_void_p), 1,
                          hits.ctypes.data_as(C.c_void_p), None)
    assert rc == rtow.RTOW_EINVAL
    rc = L.rtow_intersect_device(None, rtow.F64_STRICT, rtow.KERNEL_AUTO, None, 0, None, None, None)
    assert rc == rtow.RTOW_EINVAL
    assert b"NULL" in L.rtow_last_error()


def test_ray_and_hit_layouts():
    assert C.sizeof(rtow.Ray) == rtow.RAY_DTYPE.itemsize == 64
    assert C.sizeof(rtow.Hit) == rtow.HIT_DTYPE.itemsize == 72
    for struct, dtype in ((rtow.Ray, rtow.RAY_DTYPE), (rtow.Hit, rtow.HIT_DTYPE)):
        assert [f[0] for f in struct._fields_] == list(dtype.names)
        for name in dtype.names:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
            assert getattr(struct, name).size == dtype.fields[name][0].itemsize, name
    # the C offsets of include/rtow.h
    assert rtow.Ray.direction.offset == 32 and rtow.Ray.tmax.offset == 56
    assert rtow.Hit.prim.offset == 56 and rtow.Hit.front_face.offset == 68


def test_make_rays_fills_every_field():
    r = rtow.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [1, 0, 0]], time=0.5, tmax=[1.0, 2.0])
    assert r.dtype == rtow.RAY_DTYPE and len(r) == 2
    assert np.array_equal(r["origin"][1], [4, 5, 6]) and np.array_equal(r["direction"][0], [0, 0, 1])
    assert np.array_equal(r["time"], [0.5, 0.5]) and np.array_equal(r["tmax"], [1.0, 2.0])
