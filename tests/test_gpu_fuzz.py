"""GPU: random mixed scenes (spheres of very different sizes, moving spheres, triangles; all three
materials) through every kernel, both builders and the oracle.

The oracle walks the REFERENCE's tree and tests in insertion order; the device walks its own
structures.  The strict build must still return the same image bit for bit: the closest hit does
not depend on the acceleration structure.  (Insertion order = class-major order here, so prim_kind /
prim_index describe exactly the order the oracle's tree is built from.)
"""
import numpy as np
import pytest

import orc
import rtow
from support_scenes import random_scene

pytestmark = pytest.mark.gpu


SHAPES = [(30, 0, 0), (60, 20, 0), (0, 0, 80), (40, 10, 60), (200, 0, 0), (5, 5, 5), (120, 40, 100), (0, 0, 1500)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"s{a}_m{b}_t{c}" for a, b, c in SHAPES])
def test_random_scene_all_kernels_and_builders_match_the_oracle(ctx, shape):
    keep = []
    scene = random_scene(sum(shape) + 17, *shape, keep)
    cfg0 = rtow.make_config(72, 48, 4, 2, 12, seed=shape[0] + 3, precision=rtow.F64_STRICT)
    ref, ost = orc.render(scene, cfg0, orc.RNG_PHILOX, nthreads=4)
    dctx = rtow.Context(0)
    dctx.set_builder(rtow.BUILDER_DEVICE_LBVH)
    try:
        for c in (ctx, dctx):
            for kernel in (rtow.KERNEL_BRUTE, rtow.KERNEL_BVH, rtow.KERNEL_GRID, rtow.KERNEL_BVH4):  # (BVH4: triangle-only scenes, host builder; else the binary walk)
                cfg = rtow.make_config(72, 48, 4, 2, 12, seed=shape[0] + 3, precision=rtow.F64_STRICT, kernel=kernel)
                img, st = c.render(scene, cfg)
                if kernel == rtow.KERNEL_BVH4 and c is ctx and shape[0] == 0 and shape[1] == 0:
                    assert st.kernel_used == rtow.KERNEL_BVH4
                assert st.segments == ost.segments, (kernel, st.kernel_used)
                assert np.array_equal(img, ref), (kernel, st.kernel_used, int((img != ref).sum()))
            # the opt-in kernel that walks the reference's own tree: the oracle's walk, test for test
            rimg, rst = c.render(scene, rtow.make_config(72, 48, 4, 2, 12, seed=shape[0] + 3, precision=rtow.F64_STRICT,
                                                         kernel=rtow.KERNEL_REFTREE))
            assert rst.kernel_used == rtow.KERNEL_REFTREE and np.array_equal(rimg, ref) and rst.segments == ost.segments
            assert rst.node_tests == ost.node_tests and rst.prim_tests == ost.prim_tests
            # the fast and f32 builds: finite, close, and the same from both builders
            fa, _ = c.render(scene, rtow.make_config(72, 48, 16, 4, 12, seed=5, precision=rtow.F64_FAST))
            f3, _ = c.render(scene, rtow.make_config(72, 48, 16, 4, 12, seed=5, precision=rtow.F32))
            assert np.isfinite(fa).all() and np.isfinite(f3).all()
            assert np.abs(np.sqrt(np.clip(fa / 16, 0, 1)) - np.sqrt(np.clip(f3 / 16, 0, 1))).mean() < 2.0 / 255.0
    finally:
        dctx.close()
