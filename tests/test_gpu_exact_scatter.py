"""Path-step queries of both builds against the exact scatter reference (tests/scatter_exact.py) on the GPU.

Every strategy a build accepts (with the render's fallbacks) and both builders, in F64_STRICT and F64_FAST, on the
"material edge" scene with every ray family of tests/scatter_cases.py (and its triangle-only variant, which the BVH4
kernel walks) and on the logged rows of the three deep renders:
  * the step's hit records pass exact_hits.check (the first check of the fast step's records);
  * status, next ray and attenuation pass scatter_exact.check, and the undecided shares of scatter_cases.assert_shares
    hold for the reference of what ran;
  * strict build: the whole result equals orc_scatter fed with the step's own hit record, bit for bit, and GRID equals
    BRUTE bit for bit (on the mixed scene beyond LDS, which has no exact ties among its rows: BVH and BVH4 too);
  * want_hits=False and stepping in place give the bits of the checked result, in both builds.
Each test prints decided, undecided and the worst direction error over its bound, per family.

Measured on one MI355X ("Exact scatter") — worst |direction error| / bound over the decided rays, worst
of all strategies and both builders, strict / fast; undecided rays (scatter or hit) in brackets:
    edge (a) 0.373 (57) / 0.373 (75; GRID 65)    (b) 0.093 (60) / 0.023 (80)    (c) 0.066 (0) / 0.022 (0)
         (d) 0.155 (0) / 0.155 (0)               (e) 0.053 (0) / 0.048 (0)      (f) 0.000 (2) / 0.049 (2)
    triangle-only (a) 0.397 (5) / 0.369 (10; GRID 0), (d) 0.395 / 0.395, (e) 0.069 / 0.048, (b), (c), (f) as above
    rows: cover_d50 0.020 / 0.019, cover_moving_d50 0.006 / 0.008, suzanne_d20 0.277 / 0.274, none undecided
    the step's hit records: worst t error 0.036 / 0.059 of its bound
The undecided rays of (a) and (f) are the ones placed on a cut by construction, those of (b) have offsets below 1e-9; the
52 (strict) and 64 (fast) rays of (a) whose HIT is undecided pass as one of the outcomes their hit band leaves open.
REFTREE misses 53 of the 188 edge rays that end at a negative-radius sphere (the reference's inside-out box): see
scatter_cases.Case.without_reftree_blind_hits.
"""
import numpy as np
import pytest

import big_mixed as bm
import exact_hits as ex
import orc
import rtow
import scatter_cases as sc
import scatter_exact as sx
from exact_cases import BUILDS
from support_fixtures import qctx  # noqa: F401
from support_oracle import expected_kernel, same_bits
from support_tables import BUILDERS, KERNELS, WALKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def edge():
    return {c.name: c for c in (sc.edge_case(False), sc.edge_case(True))}


@pytest.fixture(scope="module")
def rows():
    """2,000 rows per render (every segment depth among them): the references of a case cost what its rays cost."""
    return {name: sc.logged_case(name, 2000) for name in sc.DEEP}


def step(ctx, case, prec, kernel, want_hits=True):
    """path_step over the case, one launch per bounce among its rays: (status, next, atten, hits, kernel used)."""
    n = len(case.rays)
    status = np.zeros(n, np.int32)
    nxt = np.zeros(n, rtow.RAY_DTYPE)
    atten = np.zeros((n, 3))
    hits = np.zeros(n, rtow.HIT_DTYPE) if want_hits else None
    used = set()
    for b in np.unique(case.bounce):
        s = np.nonzero(case.bounce == b)[0]
        st, nx, at, h, stats = ctx.path_step(case.rays[s], int(b), case.seed, case.ids[s], 0, prec, kernel, want_stats=True,
                                             want_hits=want_hits)
        status[s], nxt[s], atten[s] = st, nx, at
        if want_hits:
            hits[s] = h
        used.add(stats.kernel_used)
    assert len(used) == 1, used
    return status, nxt, atten, hits, used.pop()


def oracle_on_hits(case, status, hits):
    """orc_scatter fed with the step's own hit records: (indices of the rays that hit, status, next, atten)."""
    s_all = np.nonzero(hits["prim"] >= 0)[0]
    st = np.zeros(len(s_all), np.int32)
    nx = np.zeros(len(s_all), rtow.RAY_DTYPE)
    at = np.zeros((len(s_all), 3))
    for b in np.unique(case.bounce[s_all]):
        k = np.nonzero(case.bounce[s_all] == b)[0]
        s = s_all[k]
        st[k], nx[k], at[k] = orc.scatter(hits["point"][s], hits["normal"][s], hits["front_face"][s],
                                          case.rays["direction"][s], case.rays["time"][s], case.mats[hits["material"][s]],
                                          case.seed, case.ids[s], 1 + int(b))
    return s_all, st, nx, at


def run_case(ctx, whole, upload, view_like, resident=None, equal_brute=("grid",)):
    """resident(ctx, builder name): assertions on what the upload left resident; equal_brute: the strict walks whose whole
    result must equal strict BRUTE's bit for bit (a case without exact ties can name them all).
    REFTREE is checked on whole.without_reftree_blind_hits() (the reference's boxes of negative-radius spheres); its bits
    against orc_scatter on every ray."""
    lines = []
    results = {}
    for bname, builder in BUILDERS.items():
        ctx.set_builder(builder)
        try:
            ctx.upload(upload)
            if resident is not None:
                resident(ctx, bname)
            for build, prec in BUILDS.items():
                for kname, kernel in (KERNELS if build == ex.STRICT else WALKS).items():
                    if kname == "brute" and bname == "device":
                        continue  # (the brute force does not depend on the builder)
                    case = whole.without_reftree_blind_hits() if kname == "reftree" else whole
                    status, nxt, atten, hits, used = step(ctx, case, prec, kernel)
                    want = expected_kernel(view_like, kernel)
                    if want is not None:
                        assert used == want, (kname, used, want)
                    what = (case.name, bname, kname, build, used)
                    href, ref = case.ref(build, build == ex.FAST and used == rtow.KERNEL_GRID)
                    hs = ex.check(href, hits, None, what)
                    for name, idx in case.groups().items():
                        s = sx.check(ref, status, nxt, atten, hits, what=what + (name,), only=idx)
                        lines.append(f"  {bname:6s} {kname:7s}(used {used}) {build:6s} {name}: decided {s['decided']}, "
                                     f"undecided {s['undecided']} (hit {s['hit_undecided']}), worst direction error "
                                     f"{s['worst_dir_err']:.3f} of bound; hits: worst t err {hs['worst_t_err']:.3f}")
                    sc.assert_shares(case, ref, what)
                    if build == ex.STRICT:
                        s, ost, onx, oat = oracle_on_hits(case, status, hits)
                        assert same_bits(status[s], ost) and same_bits(nxt[s], onx) and same_bits(atten[s], oat), what
                        results[(bname, kname)] = (status, nxt, atten, hits)
                        if hasattr(case, "rows"):  # the rows are what the render traced: the log's own t, bit for bit
                            assert same_bits(hits["t"], case.rows[:, 10]), what
                        if case is not whole:  # the rays left out: whatever the tree found, scattered as the oracle does
                            status, nxt, atten, hits, used = step(ctx, whole, prec, kernel)
                            s, ost, onx, oat = oracle_on_hits(whole, status, hits)
                            assert same_bits(status[s], ost) and same_bits(nxt[s], onx) and same_bits(atten[s], oat), what
                            lines.append(f"  {bname:6s} {kname:7s}: {len(whole.rays) - len(case.rays)} rays at "
                                         f"negative-radius spheres left to the bit comparison, "
                                         f"{int((hits['prim'] < 0).sum())} misses in all")
        finally:
            ctx.set_builder(rtow.BUILDER_AUTO)
    # strict GRID (and the other walks of equal_brute) == strict BRUTE (the brute force ran under the host builder)
    for (bname, kname), got in results.items():
        if kname in equal_brute:
            for x, y in zip(got, results[("host", "brute")]):
                assert same_bits(x, y), (whole.name, bname, f"{kname} != brute")
    print(f"\n{whole.name}: {len(whole.rays)} rays\n" + "\n".join(lines))


@pytest.mark.parametrize("name", ["edge", "edge_tri"])
def test_edge_scene_families(qctx, edge, name):
    case = edge[name]
    keep = []
    run_case(qctx, case, case.es.upload(keep), case.scene)


@pytest.mark.parametrize("name", list(sc.DEEP))
def test_logged_rows(qctx, rows, name):
    case = rows[name]
    run_case(qctx, case, case.hs, case.hs)


def test_without_hits_and_in_place(qctx, edge):
    """want_hits=False and stepping in place (next = rays) give the bits of the result the other tests check."""
    import torch

    case = edge["edge"]
    keep = []
    qctx.upload(case.es.upload(keep))
    n = len(case.rays)
    for prec in BUILDS.values():
        status, nxt, atten, hits, _ = step(qctx, case, prec, rtow.KERNEL_AUTO)
        s2, n2, a2, h2, _ = step(qctx, case, prec, rtow.KERNEL_AUTO, want_hits=False)
        assert h2 is None and same_bits(s2, status) and same_bits(n2, nxt) and same_bits(a2, atten)
        d_rays = torch.from_numpy(case.rays.view(np.uint8).copy()).to("cuda:0")
        d_ids = torch.from_numpy(case.ids.view(np.int32).copy()).to("cuda:0")
        d_att = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda:0")
        d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        qctx.path_step_device(d_rays.data_ptr(), n, d_ids.data_ptr(), d_rays.data_ptr(), d_att.data_ptr(),
                              d_st.data_ptr(), 0, sc.BOUNCE, case.seed, 0, prec)
        torch.cuda.synchronize()
        assert same_bits(d_st.cpu().numpy(), status) and same_bits(d_att.cpu().numpy(), atten)
        assert same_bits(d_rays.cpu().numpy().view(rtow.RAY_DTYPE).reshape(-1), nxt)


# ---- the mixed scene beyond LDS (tests/big_mixed.py): the <BVH, false> and <GRID, false> forms ----
def test_big_mixed(qctx):
    """Rows of the scene's own log (all three materials, every segment depth); strict BVH, GRID and BVH4-as-BVH equal BRUTE
    bit for bit."""
    c = bm.case()
    run_case(qctx, bm.scatter_case(c), c.hs.c, c.view, resident=bm.resident, equal_brute=("bvh", "grid", "bvh4"))
