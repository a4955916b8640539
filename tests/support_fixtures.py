"""The pytest fixtures more than one test module uses, each defined once.  A test module imports the ones it needs by
name (`from support_fixtures import logged, qctx  # noqa: F401`); every scope is `module`, so each importing module gets
its own instance, set up once for that module.
"""
import pytest

import rtow
from support_oracle import LOGGED, log_rays
from support_scenes import SceneView, write_mesh_obj


def _context_fixture(name, doc=None):
    @pytest.fixture(scope="module", name=name)
    def context():
        c = rtow.Context(0)
        yield c
        c.close()

    context.__doc__ = doc
    return context


# a plain context of the module's own, under the name each module's tests ask for
qctx = _context_fixture("qctx")
pctx = _context_fixture("pctx")
fctx = _context_fixture("fctx")
octx = _context_fixture("octx")
mctx = _context_fixture("mctx")
rctx = _context_fixture("rctx")
fresh = _context_fixture("fresh", "A second context: the fresh uploads the refits are compared with.")


@pytest.fixture(scope="module")
def logged():
    """name -> (scene, view, log) of the three small renders."""
    out = {}
    for name, (mk, w, h, spp, depth, seed) in LOGGED.items():
        scene = mk()
        cfg = rtow.make_config(w, h, spp, 1, depth, seed=seed, precision=rtow.F64_STRICT)
        out[name] = (scene, SceneView(scene), log_rays(scene, cfg))
    return out


@pytest.fixture(scope="module")
def big_mesh(tmp_path_factory):
    """The 96,800-triangle mesh (scripts/make_mesh.py) and a 64x36x2 spp raylog of it (the checker's tree: the same
    hits as the reference's tree, ~100x faster)."""
    scene = rtow.HostScene.obj(write_mesh_obj(tmp_path_factory.mktemp("mesh")), 16 / 9)
    assert scene.c.n_triangles == 96800
    cfg = rtow.make_config(64, 36, 2, 1, 20, seed=24, precision=rtow.F64_STRICT)
    return scene, SceneView(scene), log_rays(scene, cfg, accel=True)
