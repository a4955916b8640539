"""The constants block of the GRID walk (csrc/rtow_walk_consts.h) against the kernel's formulas, CPU only.

The specialised trace kernels no longer read the grid image's header: the host derives the near and far planes, the
clamps, the strides and the list offsets from the header of the resident image and hands them over as one block of
kernel arguments.  The header is plain C++, so the very function the host calls is compiled with the host compiler
(tests/tools/walk_consts_check.cpp) and every word is compared with what the generic walk of rtow_trace_grid.h computes
from the same header — the far planes bit for bit against n * c + g rounded ONCE (binary128 sum, exact, then one
rounding: what v_fma_f32 does).  Cases: the host-built grids of both cover scenes (tests/tools/dump_host_images.cpp),
a grid with three layers in y, a grid far from the origin, one cell and 128 cells per axis."""
import re
import shutil
import subprocess

import numpy as np
import pytest

import accel_images as ai
import rtow
from conftest import REPO

SYNTHETIC = {"three_layers": (11, 3, 11), "far_from_origin": (35, 1, 35), "far_from_origin_3d": (19, 7, 23),
             "one_cell": (1, 1, 1), "cells_128": (128, 128, 128), "cells_128_1_1": (128, 1, 1), "cells_1_128_37": (1, 128, 37)}


def _compile(tmp, name, extra=()):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed to build " + name)
    exe = tmp / name
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *extra,
                        str(REPO / "tests" / "tools" / (name + ".cpp")), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cover_grids(tmp_path_factory):
    """The host builder's grid images of the static and the moving cover scene, as files."""
    tmp = tmp_path_factory.mktemp("walk_consts")
    dumper = _compile(tmp, "dump_host_images", ("-pthread",))
    paths = []
    for moving in (False, True):
        hs = rtow.HostScene.cover(11, 1.5, moving)
        G = ai.Geometry.of_scene(hs.c)
        hs.close()
        out = tmp / ("moving" if moving else "static")
        out.mkdir()
        with open(out / "scene.bin", "wb") as fh:
            fh.write(np.array([G.ns, G.nm, G.nt, len(G.mats)], "<i4").tobytes())
            fh.write(G.cam.astype("<f8").tobytes())
            for a in (G.sph, G.mov, G.tri):
                fh.write(np.ascontiguousarray(a, "<f8").tobytes())
            fh.write(G.pmat.astype("<i4").tobytes())
            fh.write(G.mat_records())
        r = subprocess.run([str(dumper), str(out / "scene.bin"), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
        assert (out / "image1.bin").stat().st_size > 64, "the cover scene has a grid image"
        paths.append(out / "image1.bin")
    return tmp, paths


def test_block_matches_the_kernels_formulas(cover_grids):
    tmp, images = cover_grids
    checker = _compile(tmp, "walk_consts_check", ("-Werror",))
    r = subprocess.run([str(checker)] + [str(p) for p in images], capture_output=True, text=True)
    print(r.stdout)
    m = re.search(r"^(\d+) cases, (\d+) mismatches, (\d+) far planes where two roundings would differ$", r.stdout, re.M)
    assert m, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    cases, bad, fused_differs = (int(x) for x in m.groups())
    assert bad == 0 and r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for line in r.stdout.splitlines():
        c = re.match(r"(\w+): n (\d+) (\d+) (\d+) h \S+ \S+ \S+ (ok|BAD)$", line)
        if c:
            seen[c.group(1)] = (tuple(int(c.group(k)) for k in (2, 3, 4)), c.group(5))
    assert cases == len(seen) == 2 + len(SYNTHETIC)
    assert all(v[1] == "ok" for v in seen.values()), seen
    # the two cover grids are the one-layer grids the benchmark walks ...
    for name in ("image1", "image2"):
        n = seen[name][0]
        assert n[1] == 1 and n[0] > 8 and n[2] > 8, (name, n)
    # ... and the synthetic headers have the cell counts they were made for
    for name, n in SYNTHETIC.items():
        assert seen[name][0] == n, (name, seen[name])
    # the cases can tell a fused multiply-add from a product rounded on its own
    assert fused_differs > 0
