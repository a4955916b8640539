"""The tmax-bounded walks (csrc/rtow_bounded_walks.h) pinned by their test counters.

`occluded` and `first_hits` share one BVH, one GRID and one BVH4 walk; what differs is a sink: any-hit ends a lane at its
first hit, first-hits never does and shrinks the bound from its list.  A wrong sink can get both wrong and still return
right answers, so this file pins what the answers do not show: the primitive and node tests of the strict build on
small fixed inputs equal the counts in tests/golden/bounded_walk_counters.json, which were recorded from the build
BEFORE the walks were shared (the copies in rtow_occlude.h and rtow_first_hits.h).  The counts are deterministic
integers — a wave takes 64 consecutive rays and its votes depend only on its own lanes, whatever the launch — so
equality is exact.  The results themselves are checked in test_gpu_occlusion.py and test_gpu_first_hits.py.
"""
import json

import numpy as np
import pytest

import rtow
from conftest import GOLDEN
from support_oracle import LOGGED, log_rays, rays_of, seeded_finite_tmax
from support_scenes import handmade_rays, handmade_scene
from support_tables import KERNELS as ALL_KERNELS

pytestmark = pytest.mark.gpu

S = rtow.F64_STRICT
KERNELS = {k: ALL_KERNELS[k] for k in ("bvh", "grid", "bvh4")}
QUERIES = ("occluded", "first_hits_1", "first_hits_8")
N_LOGGED = 4099  # 64 waves and a partial one
GOLD = json.loads((GOLDEN / "bounded_walk_counters.json").read_text())
# (scene, kernel) where the scene has that kernel resident; the goldens hold nothing else
CASES = sorted({tuple(k.split("/")[::2]) for k in GOLD})


def logged_rays(name, seed):
    """(scene, N_LOGGED seeded rows of the oracle's ray log of the small render of `name`, as rays)."""
    mk, w, h, spp, depth, rseed = LOGGED[name]
    scene = mk()
    log = log_rays(scene, rtow.make_config(w, h, spp, 1, depth, seed=rseed, precision=S))
    rows = log[np.sort(np.random.default_rng(seed).choice(len(log), size=N_LOGGED, replace=False))]
    return scene, rays_of(rows)


def make_inputs():
    """name -> (what Context.upload takes, {"inf": rays, "finite": rays}, whatever must stay alive)."""
    out = {}
    hand = handmade_scene()
    out["handmade"] = (hand.c, handmade_rays(), hand)
    for name, seed in (("cover_static", 71), ("suzanne", 72)):
        scene, rays = logged_rays(name, seed)
        out[name] = (scene, rays, scene)
    return {name: (up, {"inf": rays, "finite": seeded_finite_tmax(rays)}, keep) for name, (up, rays, keep) in out.items()}


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.fixture(scope="module")
def bctx():
    c = rtow.Context(0)
    c.set_builder(rtow.BUILDER_HOST_SAH)  # (the images the counts were recorded on)
    yield c
    c.close()


def measure(ctx, rays, kernel):
    """query -> [prim_tests, node_tests], and the kernel that ran (the same for the three queries)."""
    _, st = ctx.occluded(rays, S, kernel, want_stats=True)
    out, used = {"occluded": [int(st.prim_tests), int(st.node_tests)]}, {int(st.kernel_used)}
    for k in (1, 8):
        _, _, st = ctx.first_hits(rays, k, S, kernel, want_stats=True)
        out[f"first_hits_{k}"] = [int(st.prim_tests), int(st.node_tests)]
        used.add(int(st.kernel_used))
    assert len(used) == 1, used
    return out, used.pop()


def test_the_goldens_cover_every_walk():
    assert {("handmade", "bvh"), ("handmade", "grid"), ("cover_static", "bvh"), ("cover_static", "grid"),
            ("suzanne", "bvh"), ("suzanne", "grid"), ("suzanne", "bvh4")} <= set(CASES)
    for key, gold in GOLD.items():
        assert key.split("/")[1] in ("inf", "finite") and sorted(gold) == sorted(QUERIES), key


@pytest.mark.parametrize("name,kernel", CASES)
def test_counters_equal_those_of_the_separate_walks(name, kernel, inputs, bctx):
    upload, sets, _ = inputs[name]
    bctx.upload(upload)
    got = {}
    for what, rays in sets.items():
        assert len(rays) % 64 != 0
        got[what], used = measure(bctx, rays, KERNELS[kernel])
        assert used == KERNELS[kernel], (name, kernel, used)
        print(f"\n{name}/{what}/{kernel}: {got[what]}")
    for what in sets:
        assert got[what] == GOLD[f"{name}/{what}/{kernel}"], (name, what, kernel)
        # what makes the numbers meaningful: a lane that stops at its first hit walks no more than one that keeps the
        # closest, and that no more than one that keeps eight; a finite tmax prunes from the first node
        occ, one, eight = (got[what][q][1] for q in QUERIES)
        assert 0 < occ <= one <= eight, (name, what, kernel, occ, one, eight)
    assert got["finite"]["first_hits_8"][1] <= got["inf"]["first_hits_8"][1], (name, kernel)
