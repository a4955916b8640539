"""The large-list words of the GRID walk's constants block (csrc/rtow_walk_consts.h) against the image, CPU only.

The host puts the head of the always-test list — up to four static spheres, ids and record offsets — into the block,
and the trace kernels of the class with moving spheres test it from those wave-uniform values instead of reading the ids
from the image in every trip.  The block
is plain C++: the functions the host calls (make_grid_walk_consts, fill_large_head) are compiled with the host compiler
(tests/tools/walk_consts_large_check.cpp, which also carries the layout's static_asserts) and run on the host builder's
grid images of the scenes of tests/test_gpu_large_block.py (large lists of 0, 1, 3, 4, 5 and 7 entries in both scene
classes, and one that mixes a static and a moving sphere) and of both cover scenes.  Every new word must be what the header and the id section
of the image say, and every record offset must point at the record of the sphere the id names.  (The device builder
writes the same bytes — tests/test_gpu_scene_image_digests.py — and its images reach the block through the same two
functions; tests/test_gpu_large_block.py renders from them after a refit.)"""
import re
import shutil
import subprocess

import numpy as np
import pytest

import accel_images as ai
import rtow
import support_large_lists as sl
from conftest import REPO


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
def tools(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("walk_consts_large")
    return tmp, _compile(tmp, "dump_host_images", ("-pthread",)), _compile(tmp, "walk_consts_large_check", ("-Werror",))


def _cases():
    out = dict(sl.scenes())
    for name, moving in (("cover_static", False), ("cover_moving", True)):
        hs = rtow.HostScene.cover(11, 1.5, moving)
        out[name] = (ai.Geometry.of_scene(hs.c), 4, 4)  # the ground and the three big spheres, all static
        hs.close()
    return out


def _grid_image(tmp, dumper, name, G):
    out = tmp / name
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
    return out / "image1.bin"


def test_large_list_words_are_what_the_image_says(tools):
    tmp, dumper, checker = tools
    for name, (G, n_large, n_fast) in _cases().items():
        path = _grid_image(tmp, dumper, name, G)
        blob = path.read_bytes()
        assert len(blob) > 64, (name, "the scene has a grid image")
        P = ai.parse_grid(blob, G)
        assert P["n_large"] == n_large, (name, P["n_large"])  # the scene is the case it was made for
        assert P["off_fat"] != 0 and P["stride"] == (80 if G.nm else 48), (name, "the class kernels' list format")
        r = subprocess.run([str(checker), str(path), str(G.ns)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-1000:])
        m = re.match(r"n_large (\d+) large_first (\d+) n_large_fast (\d+) rec (\d+) (\d+) (\d+) (\d+) id (\d+) (\d+) (\d+) (\d+) "
                     r"size (\d+)$", r.stdout.strip())
        assert m, r.stdout
        v = [int(x) for x in m.groups()]
        got_fast, got_rec, got_id = v[2], v[3:7], v[7:11]
        want_fast, want_rec, want_id = sl.block_of_image(blob, G.ns)
        print(name, "n_large", v[0], "n_large_fast", got_fast, "rec", got_rec, "id", got_id)
        assert v[0] == n_large and v[1] == (P["off_large"] - P["off_ids"]) // 4 and v[11] == 192
        assert got_fast == want_fast == n_fast, (name, got_fast, want_fast, n_fast)
        assert got_rec == want_rec and got_id == want_id, (name, got_rec, want_rec, got_id, want_id)
        # every offset points at the record of the sphere its id names: centre and signed r * r (rtow_scene_records.h)
        recs = G.sph_records()
        for k in range(got_fast):
            assert got_id[k] < G.ns
            rec = np.frombuffer(blob, "<f8", 4, got_rec[k])
            assert np.array_equal(rec, recs[got_id[k]]), (name, k, rec, recs[got_id[k]])
        # the list is in id order, so the block's entries are its first ones, and a moving sphere ends the served head
        ids = np.frombuffer(blob, np.uint32, n_large, P["off_large"])
        assert list(ids[:got_fast]) == got_id[:got_fast]
        if got_fast < min(n_large, 4):
            assert ids[got_fast] >= G.ns
