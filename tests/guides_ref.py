"""Helpers of the guide tests (test_gpu_guides.py, test_gpu_exact_guides.py, test_guides_exact_host.py): the logged
depth-0 renders, the row partition, the numpy statement of the guide fold (csrc/rtow_guides.h) — IEEE binary64, the
written operand order, samples added in order from zero — and what the exact checker (guides_exact.py) needs of a scene."""
import ctypes as C

import numpy as np
import pytest

import exact_hits as ex
import guides_exact as gx
import orc
import rtow
from support_oracle import logged_render, primaries, sum_in_order
from support_scenes import SceneView, cover, cover_moving, suzanne

# name: (scene, width, height, spp, seed).  The cover camera has a lens (radius 0.05: the origins differ per sample), the
# moving cover a shutter interval (the times differ per sample), suzanne is a triangle mesh.
SCENES = {"cover": (cover, 48, 32, 4, 21), "cover_moving": (cover_moving, 48, 32, 4, 22), "suzanne": (suzanne, 48, 27, 4, 23)}
CAP = 0.01  # the share of pixels that may hold an undecided sample


class Logged:
    """One oracle render at depth 0 with its log; `cfg` is the strict config the device calls take."""

    def __init__(self, mk, w, h, spp, seed):
        self.scene = mk() if callable(mk) else mk
        self.w, self.h, self.spp, self.seed = w, h, spp, seed
        self.cfg = self.config()
        self.image, self.log = logged_render(self.scene, self.cfg)
        assert len(self.log) == w * h * spp and np.all(self.log[:, 2] == 0)  # depth 0: every row is a primary
        self.rays, self.ids = primaries(self.log)
        # pixel-major, sample-minor
        assert np.array_equal(self.ids[:, 0], np.repeat(np.arange(w * h), spp))
        assert np.array_equal(self.ids[:, 1], np.tile(np.arange(spp), w * h))

    def config(self, precision=rtow.F64_STRICT, kernel=rtow.KERNEL_AUTO, **kw):
        kw.setdefault("nstreams", 1)
        return rtow.make_config(self.w, self.h, kw.pop("spp", self.spp), max_child_rays=0, seed=self.seed,
                                precision=precision, kernel=kernel, **kw)


@pytest.fixture(scope="module")
def logged():
    """name -> the three small oracle renders (computed once per importing module, never changed)."""
    return {name: Logged(*v) for name, v in SCENES.items()}


def row_list(cfg):
    """This rank's global rows, ascending (rtow_local_row_list)."""
    L = rtow.lib()
    n = L.rtow_local_rows(C.byref(cfg))
    rows = np.zeros(max(n, 1), dtype=np.int32)
    assert L.rtow_local_row_list(C.byref(cfg), rows.ctypes.data_as(C.POINTER(C.c_int32)), n) == n
    return rows[:n]


def attenuations(scene):
    """[n_materials, 3]: what the reference's scatter returns as attenuation — albedo, or (1, 1, 1) for a Dielectric."""
    m = orc.scene_arrays(scene.c)["materials"]
    att = m[:, 0:3].copy()
    att[m[:, 5] == rtow.MAT_DIELECTRIC] = 1.0
    return att


def fold_guides(rays, hits, sky, att, spp):
    """The guide sums of csrc/rtow_guides.h from pinned pieces: `hits` the strict closest hits of `rays` (HIT_DTYPE), `sky`
    [n, 3] the strict radiance of the rays at depth 0 (the sky on a miss, black on a hit), `att` attenuations().  Returns a
    GUIDE_DTYPE array [pixels].  A miss adds +0.0 where the kernel adds nothing: the same bits (no sum is ever -0.0)."""
    hit = np.isfinite(hits["t"])
    mat = np.where(hit, hits["material"], 0)
    albedo = np.where(hit[:, None], att[mat], sky)
    n = hits["normal"]
    tri = hits["kind"] == rtow.PRIM_TRIANGLE
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        unit = np.where(tri[:, None], n / s[:, None], n)
        d = rays["direction"]
        depth = hits["t"] * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    unit = np.where(hit[:, None], unit, 0.0)
    depth = np.where(hit, depth, 0.0)
    out = np.zeros(len(rays) // spp, dtype=rtow.GUIDE_DTYPE)
    out["albedo"] = sum_in_order(albedo, spp)
    out["normal"] = sum_in_order(unit, spp)
    out["depth"] = sum_in_order(depth, spp)
    out["hits"] = sum_in_order(hit.astype(np.float64), spp)
    return out


def guide_values(g):
    """[..., 8] float64 view of a GUIDE_DTYPE array: albedo, normal, depth, hits."""
    g = np.ascontiguousarray(g)
    return g.view(np.float64).reshape(g.shape + (8,))


def camera_ray_scales(scene, rays):
    """Per ray and component, the sum of the absolute values of the terms of Camera::get_ray: (S_origin [n, 3],
    S_direction [n, 3], S_time [n]).  origin = o + (u rdx + v rdy); direction = llc + s horizontal + t vertical - origin;
    time = jt (t1 - t0) + t0.  (rdx, rdy) and (s, t) are recovered from the strict ray by least squares."""
    cam = scene.c.camera
    o, cu, cv = (np.array(list(x)) for x in (cam.origin, cam.u, cam.v))
    hor, ver, llc = (np.array(list(x)) for x in (cam.horizontal, cam.vertical, cam.lower_left_corner))
    lens = (rays["origin"] - o) @ np.linalg.pinv(np.stack([cu, cv]))            # [n, 2] (rdx, rdy)
    s_off = np.abs(lens[:, 0:1] * cu) + np.abs(lens[:, 1:2] * cv)
    s_org = np.abs(o) + s_off
    st = (rays["direction"] + rays["origin"] - llc) @ np.linalg.pinv(np.stack([hor, ver]))
    s_dir = np.abs(llc) + np.abs(st[:, 0:1] * hor) + np.abs(st[:, 1:2] * ver) + s_org
    s_time = np.abs(rays["time"] - cam.t0) + abs(cam.t0)
    return s_org, s_dir, s_time


def moved_cover():
    """The moving cover with its spheres and its camera moved: what the refit tests refit over the unmoved scene."""
    moved = cover_moving()
    sc = moved.c
    for i in range(1, sc.n_spheres):  # (sphere 0 is the ground)
        sc.sphere_geom[4 * i + 0] += 0.05 * ((i % 5) - 2)
        sc.sphere_geom[4 * i + 1] += 0.02 * (i % 3)
    for i in range(sc.n_moving):
        sc.moving_geom[8 * i + 1] += 0.03 * (i % 4)
        sc.moving_geom[8 * i + 4] += 0.03 * (i % 4) + 0.1
    for k, d in enumerate((-0.75, 0.5, 0.25)):  # the camera, translated
        sc.camera.origin[k] += d
        sc.camera.lower_left_corner[k] += d
    return moved


class Parts:
    """What the exact checker needs of one host scene: its exact_hits.Scene and its attenuation table."""

    def __init__(self, scene):
        self.scene = scene
        self.exact = ex.Scene.of(SceneView(scene))
        self.att = attenuations(scene)

    def reference(self, rays, ids, spp, build, unit_cut=False):
        if build == gx.STRICT:
            return gx.GuideReference(rays, ids, self.exact, self.att, spp, gx.STRICT)
        s_org, s_dir, s_time = camera_ray_scales(self.scene, rays)
        omag, dmag = gx.ray_magnitudes(s_org, s_dir, list(self.scene.c.camera.origin))
        return gx.GuideReference(rays, ids, self.exact, self.att, spp, gx.FAST, unit_cut and len(self.exact.tri) > 0,
                                 omag, dmag, s_time)


def within_cap(what, stats):
    print(gx.report(str(what), stats))
    assert stats["undecided_pixels"] <= CAP * stats["pixels"], (what, stats)
