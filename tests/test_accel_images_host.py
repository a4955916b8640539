"""The image checker (tests/accel_images.py) on the host builders' images, CPU only: the SAH BVH2 image, the 4-wide
image with both node formats and the uniform grid of rtow_bvh.h / rtow_bvh4.h / rtow_grid.h, compiled without HIP
(tests/tools/dump_host_images.cpp), for the cover scenes, suzanne and the edge meshes — and the checker rejects
corrupted copies of them.  tests/test_gpu_accel_images.py runs the same checks on the images resident on the GPU."""
import shutil
import subprocess

import numpy as np
import pytest

import accel_images as ai
import rtow
from conftest import REPO
from support_scenes import suzanne_tris


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed to build the host-image dumper")
    exe = tmp_path_factory.mktemp("dump") / "dump_host_images"
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread",
                    str(REPO / "tests" / "tools" / "dump_host_images.cpp"), "-o", str(exe)], check=True, capture_output=True)
    return exe


def host_images(exe, G, tmp_path):
    inp = tmp_path / "scene.bin"
    with open(inp, "wb") as fh:
        fh.write(np.array([G.ns, G.nm, G.nt, len(G.mats)], "<i4").tobytes())
        fh.write(G.cam.astype("<f8").tobytes())
        for a in (G.sph, G.mov, G.tri):
            fh.write(np.ascontiguousarray(a, "<f8").tobytes())
        fh.write(G.pmat.astype("<i4").tobytes())
        fh.write(G.mat_records())
    r = subprocess.run([str(exe), str(inp), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
    rd = lambda name: (tmp_path / name).read_bytes() if (tmp_path / name).exists() else b""
    return {0: rd("image0.bin"), 1: rd("image1.bin")}, (rd("image4.bin"), rd("image5.bin")), (rd("image4h.bin"), rd("image5h.bin"))


def _check_all(exe, G, tmp_path):
    images, (b4, f4), (b4h, f4h) = host_images(exe, G, tmp_path)
    info = ai.check_resident(images, G)
    if G.ns == 0 and G.nm == 0:
        info["bvh4"] = ai.check_bvh4(b4, f4, G)
        info["bvh4h"] = ai.check_bvh4(b4h, f4h, G)
        assert not info["bvh4"]["half"] and info["bvh4h"]["half"]
    return images, info


@pytest.mark.parametrize("moving", [False, True])
def test_host_images_of_the_cover_scene(dumper, tmp_path, moving):
    hs = rtow.HostScene.cover(11, 1.5, moving)
    G = ai.Geometry.of_scene(hs.c)
    hs.close()
    _, info = _check_all(dumper, G, tmp_path)
    assert 0 in info and 1 in info and info[1]["n_large"] >= 1  # the r = 1000 ground sphere


@pytest.mark.parametrize("name", ["suzanne"] + list(ai.edge_meshes()))
def test_host_images_of_meshes(dumper, tmp_path, name):
    G = ai.mesh_geometry(suzanne_tris() if name == "suzanne" else ai.edge_meshes()[name])
    _check_all(dumper, G, tmp_path)


@pytest.mark.parametrize("name", list(ai.sphere_edge_scenes()))
def test_host_images_of_sphere_edge_scenes(dumper, tmp_path, name):
    _check_all(dumper, ai.sphere_edge_scenes()[name], tmp_path)


def test_the_checker_rejects_corrupted_host_images(dumper, tmp_path):
    """Each corruption of a real image fails for the reason it names (the GPU module does the same on device images)."""
    G = ai.mesh_geometry(suzanne_tris())
    images, (b4, f4), (b4h, f4h) = host_images(dumper, G, tmp_path)
    bad, i = ai.bvh2_plane_inward(images[0], G)
    with pytest.raises(ai.ImageError, match=rf"node {i} .*lo plane of axis 0 .* does not enclose"):
        ai.check_bvh2(bad, G)
    bad, i = ai.bvh2_leaf_count(images[0], G, +1)
    with pytest.raises(ai.ImageError, match=r"appears in 2 leaves"):
        ai.check_bvh2(bad, G)
    bad, i = ai.bvh2_leaf_count(images[0], G, -1)
    with pytest.raises(ai.ImageError, match=r"appears in 0 leaves"):
        ai.check_bvh2(bad, G)
    for blob, fr in ((b4, f4), (b4h, f4h)):
        bad, (i, c) = ai.bvh4_plane_inward(blob, fr, G)
        with pytest.raises(ai.ImageError, match=rf"node {i} slot {c} .*lo plane of axis 0 .* does not enclose"):
            ai.check_bvh4(bad, fr, G)
        bad, i = ai.bvh4_child_backwards(blob, fr, G)
        with pytest.raises(ai.ImageError, match=rf"node {i} slot \d: child link 0 does not point to a later node"):
            ai.check_bvh4(bad, fr, G)
    bad, c = ai.grid_drop_one(images[1], G)
    with pytest.raises(ai.ImageError, match=rf"is not listed in cell {c} "):
        ai.check_grid(bad, G)
