"""The camera stage's host side (rtow_camera_rays*, rtow_guides*): exports, record sizes, rtow_camera_ray_count and the
argument checks that need no GPU."""
import ctypes as C
import re

import rtow
from conftest import REPO


def test_exports_and_abi():
    L = rtow.lib()
    for name in ("rtow_camera_rays_device", "rtow_camera_rays", "rtow_camera_ray_count", "rtow_guides_device",
                 "rtow_guides"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS
    assert L.rtow_abi_version() == 9


def test_guide_record_is_64_bytes():
    assert rtow.GUIDE_DTYPE.itemsize == 64
    assert C.sizeof(rtow.Guide) == 64
    assert [rtow.GUIDE_DTYPE.fields[f][1] for f in ("albedo", "normal", "depth", "hits")] == [0, 24, 48, 56]
    # the C declaration: eight doubles, nothing else (sizeof(rtow_guide_t) == 64 is a static_assert of the build)
    header = (REPO / "include" / "rtow.h").read_text()
    body = re.search(r"typedef struct rtow_guide_t \{(.*?)\} rtow_guide_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["double albedo[3]", "double normal[3]", "double depth", "double hits"]


def _count(cfg):
    return rtow.lib().rtow_camera_ray_count(C.byref(cfg))


def _rows(cfg):
    return rtow.lib().rtow_local_rows(C.byref(cfg))


def test_camera_ray_count():
    # spp 5 over 2 streams: 2 samples per stream, 4 effective samples
    cfg = rtow.make_config(48, 27, 5, nstreams=2)
    assert _rows(cfg) == 27 and _count(cfg) == 27 * 48 * 4
    # a stream range: stream 1 of 2
    cfg = rtow.make_config(48, 27, 5, nstreams=2, stream_first=1, stream_count=1)
    assert _count(cfg) == 27 * 48 * 2
    # three ranks, strips of 4 rows, H = 27: 11 + 8 + 8 rows
    total = 0
    for rank, rows in enumerate((11, 8, 8)):
        cfg = rtow.make_config(48, 27, 4, nstreams=1, rank=rank, nranks=3, tile_rows=4)
        assert _rows(cfg) == rows
        assert _count(cfg) == rows * 48 * 4
        total += _count(cfg)
    assert total == 27 * 48 * 4
    # fewer samples than streams: no effective samples
    assert _count(rtow.make_config(48, 27, 1, nstreams=2)) == 0
    # RTOW_F32 and an invalid config are refused
    assert _count(rtow.make_config(48, 27, 4, precision=rtow.F32)) == rtow.RTOW_EINVAL
    assert _count(rtow.make_config(0, 27, 4)) == rtow.RTOW_EINVAL


def test_null_arguments():
    L = rtow.lib()
    cfg = rtow.make_config(8, 8, 1)
    assert L.rtow_camera_ray_count(None) == rtow.RTOW_EINVAL
    assert L.rtow_camera_rays(None, C.byref(cfg), None, None) == rtow.RTOW_EINVAL
    assert L.rtow_camera_rays_device(None, C.byref(cfg), None, None, None) == rtow.RTOW_EINVAL
    assert L.rtow_guides(None, C.byref(cfg), None, None) == rtow.RTOW_EINVAL
    assert L.rtow_guides_device(None, C.byref(cfg), None, None, None) == rtow.RTOW_EINVAL
    assert L.rtow_camera_rays(None, None, None, None) == rtow.RTOW_EINVAL
    assert L.rtow_guides(None, None, None, None) == rtow.RTOW_EINVAL
