"""GPU: every resident scene image, byte for byte, against digests recorded before the scene half of the C-ABI shim was
split into stages (csrc/rtow_scene.cpp).

tests/scene_digests.py makes a fixed list of small scenes resident by every route (rtow_scene_upload, the lean uploads
of rtow_render, rtow_scene_refit) with both builders, suzanne also under the knobs that change an image, and returns
the SHA-256 of each image of rtow_debug_image and the integer fields of rtow_build_info.  The fixture
tests/golden/scene_image_digests.json holds the same values, recorded twice (equal) with the library as it was before
the split.  Equality, no tolerance: the host code around the builders may be rearranged, the images may not move.
(One image is left out where it cannot be pinned: the device-built binary BVH image of the one- and two-triangle
meshes, whose alignment gap behind the material indices that builder does not write; scene_digests._resident.)
"""
import json

import pytest

import scene_digests
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_resident_images_and_build_info_equal_the_recorded_digests():
    want = json.loads((GOLDEN / "scene_image_digests.json").read_text())
    got = scene_digests.record()
    assert sorted(got) == sorted(want), "the cases differ from the fixture's"
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    lines = []
    for k, (g, w) in list(bad.items())[:8]:
        diff = {f"image {i}" for i in w["images"] if g["images"].get(i) != w["images"][i]}
        diff |= {f for f in w["build_info"] if g["build_info"].get(f) != w["build_info"][f]}
        diff |= {"grid_resident"} if g.get("grid_resident") != w.get("grid_resident") else set()
        lines.append(f"{k}: {', '.join(sorted(diff))}")
    assert not bad, f"{len(bad)} of {len(want)} cases differ from the recorded digests:\n  " + "\n  ".join(lines)
