"""The two-axis cell crossing of the GRID walk against the 3D one, CPU only: csrc/rtow_dda_step.h is plain C++, so the
very functions the kernels inline are compiled with the host compiler (tests/tools/flat_dda_check.cpp) and stepped side
by side from the same states of a grid with one layer in y — every ordering and equality of (tmx, ty_exit, tmz, tmax),
clamped +-1e30 reciprocals, infinities, rem = 0 on either axis, both signs of every direction component, and seeded
random walks.  Same cells in the same order, the same last step, the same t_entry bits."""
import re
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed to build the DDA step checker")
    exe = tmp_path_factory.mktemp("dda") / "flat_dda_check"
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        str(REPO / "tests" / "tools" / "flat_dda_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("seed", [1, 20251])
def test_flat_step_walks_like_the_generic_step(checker, seed):
    r = subprocess.run([str(checker), str(seed)], capture_output=True, text=True)
    m = re.match(r"(\d+) walks, (\d+) steps, (\d+) mismatches", r.stdout)
    assert m, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    walks, steps, bad = (int(x) for x in m.groups())
    assert bad == 0 and r.returncode == 0, r.stderr[-2000:]
    # the enumerations (256 * 81 * 8 and 1000 * 12 * 8 walks) and the 6000 random ones all ran, and walked
    assert walks == 256 * 81 * 8 + 1000 * 12 * 8 + 6000
    assert steps > walks
