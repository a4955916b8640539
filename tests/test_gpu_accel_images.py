"""GPU: the resident acceleration images checked against the exact bounds of their geometry (tests/accel_images.py).

Ray-independent: every node's planes must enclose every primitive below it with a margin, every grid cell must list
every primitive that touches it, and every record must be the scene's primitive bit for bit — so the closest hit
cannot depend on the tree for ANY ray, not only for the rays a camera happens to send.  Each scene is uploaded with
both builders (rtow_scene_upload builds every image), and every resident image (0-5 of rtow_debug_image) is checked.
"""
import pytest

import accel_images as ai
import rtow
from conftest import GOLDEN
from support_fixtures import mctx  # noqa: F401
from support_scenes import random_scene, resident_images, suzanne_tris, to_scene
from support_tables import BUILDERS as BUILDER_OF

pytestmark = pytest.mark.gpu

BUILDERS = list(BUILDER_OF.values())  # (the ids below are its names)


def upload_and_check(ctx, sc, G, builder, label=""):
    """upload with `builder`, then every resident image through the checker; returns the images."""
    assert tuple(sc.camera.origin) == tuple(G.cam) and sc.camera.t0 == 0.0 and sc.camera.t1 == 1.0
    ctx.set_builder(builder)
    ctx.upload(sc)
    bi = ctx.build_info()
    assert bi.builder == builder, label
    im = resident_images(ctx)
    assert im[0] and im[2], f"{label}: rtow_scene_upload builds the BVH images"
    assert bool(im[1]) == bool(bi.grid_image_bytes) and bool(im[1]) == bool(im[3]), label
    if bi.bvh4_nodes > 0:
        assert im[4] and len(im[5]) == 48, f"{label}: {bi.bvh4_nodes} 4-wide nodes but no 4-wide image read back"
        assert len(im[4]) == bi.bvh4_image_bytes and ai.parse_frame(im[5])["half"] == (bi.bvh4_node_bytes == 64)
    else:
        assert not im[4] and not im[5], label
    info = ai.check_resident(im, G)
    assert info[0]["n_nodes"] == bi.bvh_nodes, label
    if 4 in info:
        assert info[4]["n4"] == bi.bvh4_nodes, label
    return im, bi


# ---- sphere and mixed scenes ---------------------------------------------------------------------------------------
def _cover(moving, keep):
    hs = rtow.HostScene.cover(11, 1.5, moving)
    keep.append(hs)
    return hs.c


def _fuzz(shape, keep):
    return random_scene(17 + sum(shape), *shape, keep)


SCENES = {
    "cover_static": lambda keep: _cover(False, keep),
    "cover_moving": lambda keep: _cover(True, keep),
    "fuzz_s40_m10_t60": lambda keep: _fuzz((40, 10, 60), keep),
    "fuzz_s120_m40_t100": lambda keep: _fuzz((120, 40, 100), keep),
    "fuzz_s5_m5_t5": lambda keep: _fuzz((5, 5, 5), keep),
}


@pytest.mark.parametrize("builder", BUILDERS, ids=["host", "device"])
@pytest.mark.parametrize("name", list(SCENES))
def test_sphere_and_mixed_scene_images_enclose_their_geometry(mctx, name, builder):
    keep = []
    sc = SCENES[name](keep)
    G = ai.Geometry.of_scene(sc)
    im, bi = upload_and_check(mctx, sc, G, builder, name)
    if name.startswith("cover"):
        assert im[1], "the cover scene takes a grid"
        info = ai.check_grid(im[1], G)
        assert info["n_large"] >= 1  # the r = 1000 ground sphere


@pytest.mark.parametrize("builder", BUILDERS, ids=["host", "device"])
@pytest.mark.parametrize("name", list(ai.sphere_edge_scenes()))
def test_sphere_edge_scene_images_enclose_their_geometry(mctx, name, builder):
    keep = []
    G = ai.sphere_edge_scenes()[name]
    upload_and_check(mctx, to_scene(G, keep), G, builder, name)


# ---- triangle meshes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS, ids=["host", "device"])
def test_suzanne_images_enclose_their_geometry(mctx, builder):
    hs = rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)
    G = ai.Geometry.of_scene(hs.c)
    _, bi = upload_and_check(mctx, hs.c, G, builder, "suzanne")
    assert bi.bvh4_node_bytes == 128
    hs.close()


@pytest.mark.parametrize("builder", BUILDERS, ids=["host", "device"])
def test_meshes_around_the_lds_limit_images_enclose_their_geometry(mctx, builder):
    """The first 850 and 1,400 triangles of suzanne subdivided 2x2 (test_gpu_parity: both 4-wide node formats)."""
    tris = suzanne_tris(2)
    formats = set()
    for n in (850, 1400):
        keep = []
        G = ai.mesh_geometry(tris[:n])
        _, bi = upload_and_check(mctx, to_scene(G, keep), G, builder, f"first {n}")
        formats.add(bi.bvh4_node_bytes)
    assert formats == {64, 128}


@pytest.mark.parametrize("builder", BUILDERS, ids=["host", "device"])
@pytest.mark.parametrize("name", list(ai.edge_meshes()))
def test_edge_mesh_images_enclose_their_geometry(mctx, name, builder):
    keep = []
    G = ai.mesh_geometry(ai.edge_meshes()[name])
    _, bi = upload_and_check(mctx, to_scene(G, keep), G, builder, name)
    if G.nt >= 2000:
        assert bi.bvh4_node_bytes == 64, (name, bi.bvh4_node_bytes)


@pytest.fixture(scope="module")
def mesh100k():
    keep = []
    G = ai.mesh_geometry(suzanne_tris(10))
    assert G.nt == 96800
    return to_scene(G, keep), G, keep


@pytest.mark.parametrize("tree", ["host", "sah", "ploc16", "radix"])
def test_mesh100k_images_enclose_their_geometry(mesh100k, monkeypatch, tree):
    """96,800 triangles: 64-byte nodes; the host builder and the device builder's three trees (RTOW_DEVICE_TREE=sah,
    the default; PLOC with RTOW_PLOC_RADIUS=16; Karras' radix tree with RTOW_PLOC_RADIUS=0)."""
    sc, G, _ = mesh100k
    monkeypatch.delenv("RTOW_DEVICE_TREE", raising=False)
    monkeypatch.delenv("RTOW_PLOC_RADIUS", raising=False)
    if tree == "sah":
        monkeypatch.setenv("RTOW_DEVICE_TREE", "sah")
    elif tree != "host":
        monkeypatch.setenv("RTOW_PLOC_RADIUS", "16" if tree == "ploc16" else "0")
    c = rtow.Context(0)  # (the knobs are read at context creation)
    try:
        builder = rtow.BUILDER_HOST_SAH if tree == "host" else rtow.BUILDER_DEVICE_LBVH
        _, bi = upload_and_check(c, sc, G, builder, tree)
        assert bi.bvh4_node_bytes == 64 and bi.bvh4_nodes > 0
    finally:
        c.close()


# ---- determinism ---------------------------------------------------------------------------------------------------
def test_device_builds_are_deterministic(mesh100k):
    """DESIGN: the device SAH build uses integer sums, minima and maxima only.  Two fresh contexts, one build each:
    byte-identical images 0 and 4 for the 96.8k-triangle mesh and for suzanne."""
    hs = rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)
    for label, sc in (("mesh100k", mesh100k[0]), ("suzanne", hs.c)):
        out = []
        for _ in range(2):
            c = rtow.Context(0)
            try:
                c.set_builder(rtow.BUILDER_DEVICE_LBVH)
                c.upload(sc)
                out.append((c.debug_image(0), c.debug_image(4)))
            finally:
                c.close()
        assert out[0][1], label
        assert out[0][0] == out[1][0], f"{label}: image 0 differs between two device builds"
        assert out[0][1] == out[1][1], f"{label}: image 4 differs between two device builds"
    hs.close()


# ---- the AUTO builder and rtow_scene_upload ------------------------------------------------------------------------
def test_upload_after_an_auto_render_takes_the_host_builder(mesh100k):
    """include/rtow.h: rtow_scene_upload takes the host builder under AUTO, also after a render resolved AUTO to the
    device for a big mesh."""
    sc, G, _ = mesh100k
    c = rtow.Context(0)  # AUTO, the default of a new context
    try:
        c.render(sc, rtow.make_config(32, 18, 1, 1, 4, seed=3, precision=rtow.F64_FAST))
        assert c.build_info().builder == rtow.BUILDER_DEVICE_LBVH
        c.upload(sc)
        assert c.build_info().builder == rtow.BUILDER_HOST_SAH
        ai.check_resident(resident_images(c), G)
    finally:
        c.close()


# ---- the checker has teeth: corrupted copies of real images --------------------------------------------------------
def test_the_checker_rejects_corrupted_device_images(mctx):
    keep = []
    hs = rtow.HostScene.obj(GOLDEN / "suzanne.obj", 16 / 9)
    keep.append(hs)
    G = ai.Geometry.of_scene(hs.c)
    mctx.set_builder(rtow.BUILDER_DEVICE_LBVH)
    mctx.upload(hs.c)
    im = resident_images(mctx)
    half_G = ai.mesh_geometry(suzanne_tris(2)[:1400])
    sc = to_scene(half_G, keep)
    mctx.upload(sc)
    imh = resident_images(mctx)
    assert ai.parse_frame(imh[5])["half"] and not ai.parse_frame(im[5])["half"]
    cover = _cover(False, keep)
    Gc = ai.Geometry.of_scene(cover)
    mctx.upload(cover)
    imc = resident_images(mctx)
    for blob, G_ in ((im, G), (imh, half_G), (imc, Gc)):
        ai.check_resident(blob, G_)  # the real images pass
    # a plane moved inwards past the margin: binary32 (binary BVH and 128-byte nodes) and binary16 (one step)
    bad, i = ai.bvh2_plane_inward(im[0], G)
    with pytest.raises(ai.ImageError, match=rf"node {i} .*lo plane of axis 0 .* does not enclose"):
        ai.check_bvh2(bad, G)
    for imgs, G_ in ((im, G), (imh, half_G)):
        bad, (i, c) = ai.bvh4_plane_inward(imgs[4], imgs[5], G_)
        with pytest.raises(ai.ImageError, match=rf"node {i} slot {c} .*lo plane of axis 0 .* does not enclose"):
            ai.check_bvh4(bad, imgs[5], G_)
        # a 4-wide child link pointing backwards
        bad, i = ai.bvh4_child_backwards(imgs[4], imgs[5], G_)
        with pytest.raises(ai.ImageError, match=rf"node {i} slot \d: child link 0 does not point to a later node"):
            ai.check_bvh4(bad, imgs[5], G_)
    # a duplicated and a dropped leaf id
    bad, _ = ai.bvh2_leaf_count(im[0], G, +1)
    with pytest.raises(ai.ImageError, match=r"appears in 2 leaves"):
        ai.check_bvh2(bad, G)
    bad, _ = ai.bvh2_leaf_count(im[0], G, -1)
    with pytest.raises(ai.ImageError, match=r"appears in 0 leaves"):
        ai.check_bvh2(bad, G)
    # one id removed from one grid cell
    bad, c = ai.grid_drop_one(imc[1], Gc)
    with pytest.raises(ai.ImageError, match=rf"is not listed in cell {c} "):
        ai.check_grid(bad, Gc)
    # two binary32 record slots swapped
    bad, j = ai.image32_swap_records(im[2], im[0], G)
    with pytest.raises(ai.ImageError, match=rf"binary32 triangle record slot 0: .* rounded to nearest"):
        ai.check_bvh2_f32(bad, im[0], G)
