"""In-place refit, host side (no GPU): both entry points are exported and refuse NULL arguments; RefitInfo has the C
layout of rtow_refit_info_t; the ABI stays 9 (the change is additive)."""
import ctypes as C
import shutil
import subprocess

import rtow
from conftest import REPO


def test_refit_symbols_are_exported():
    L = rtow.lib()
    for name in ("rtow_scene_refit", "rtow_refit_info"):
        assert hasattr(L, name), name
        assert name in rtow.EXPORTS


def test_null_arguments_are_einval():
    L = rtow.lib()
    scene = rtow.HostScene.cover(2, 1.5, False)
    try:
        assert L.rtow_scene_refit(None, C.byref(scene.c)) == rtow.RTOW_EINVAL
        assert b"NULL" in L.rtow_last_error()
        assert L.rtow_scene_refit(None, None) == rtow.RTOW_EINVAL
        assert b"NULL" in L.rtow_last_error()
        info = rtow.RefitInfo()
        assert L.rtow_refit_info(None, C.byref(info)) == rtow.RTOW_EINVAL
        assert b"NULL" in L.rtow_last_error()
        assert L.rtow_refit_info(None, None) == rtow.RTOW_EINVAL
    finally:
        scene.close()


def test_refit_info_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in rtow.RefitInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtow.h"\nint main(void) {\n'
                   + "".join(f'  printf("%zu\\n", offsetof(rtow_refit_info_t, {f}));\n' for f in fields)
                   + '  printf("%zu\\n", sizeof(rtow_refit_info_t));\n  return 0;\n}\n')
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    exe = tmp_path / "layout"
    lang = ["-x", "c"] if not cc.endswith("g++") else ["-x", "c++"]
    subprocess.run([cc, *lang, str(src), "-I", str(REPO / "include"), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(rtow.RefitInfo, f).offset for f in fields] + [C.sizeof(rtow.RefitInfo)]
    assert got == want
    assert want == [0, 4, 8, 16, 24, 32]


def test_abi_version_stays_9():
    assert rtow.RTOW_ABI_VERSION == 9
    assert rtow.lib().rtow_abi_version() == 9
