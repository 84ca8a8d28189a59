"""The general fused stage (csrc/general.hip, hfx_run_steps_blocks(..., fused = 4)) on last batches of fewer than 16 elements and in
every launch form: six compile-time size classes and the size-generic kernels, 3 / 4 / 8 flux waves, 4 / 8 update waves, batched
and looped staging, LDG corrections gathered in the flux kernel or written by face_delta_kernel, the folded and the unfolded
opp_2, the LES form.

Blocks of 1, 15, 17 and 33 elements come from tests/general_util.py (a seeded choice of a fixture's elements; the faces that lose a
side carry the six boundary kinds of hex_p2_bdy_walls) and are checked against the oracle ON THE SAME BLOCK
(tests/test_general_cut_blocks.py shows without a GPU that each of them is a sound input in which every element moves); uncut and
permuted blocks against the genuine reference's fixture states.  Every run is two time steps, and after each: the state relative
to max |u| (1e-11, the worst element reported), DIV_TCONF_UPTS of the step's last stage (5e-10), DISU_FPTS against opp_0 of the
new state (1e-12), the shock sensor (1e-10) and check_nan() == -1 -- the padded elements of a last batch hold a zero state, whose
point physics must reach neither the NaN flag nor memory.  hfx_general_plan shows that the form a test asks for is the one that ran."""
import numpy as np
import pytest

import hfx
import general_util as G
import mixed_util as MU
from ragged_partition import self_partition
from test_gpu_methods_vs_golden import build

pytestmark = pytest.mark.gpu

TOL_U, TOL_DIV, TOL_FPTS, TOL_SENSOR = 1e-11, 5e-10, 1e-12, 1e-10
DEFAULTS = {"general_waves": 0, "general_update_waves": 0, "fold_general": 1, "gather_delta": 1, "bdy_beside": 0}
SIZE_CLASS = {(4, 12): 0, (10, 24): 1, (20, 40): 2, (6, 18): 3, (18, 39): 4, (40, 68): 5}  # GENERAL_SIZES of csrc/general.hpp


@pytest.fixture(scope="module")
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def relerr(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


# ---- the plan a block must get, restated from the rules of csrc/general.hpp ------------------------------------------------------
def pad4(n):
    return (n + 3) & ~3


def staged(n, waves):
    return (n * 16 + 64 * waves - 1) // (64 * waves)


def expected_plan(d, options, les=False):
    nu, nfp = int(d["sizes"][1]), int(d["sizes"][2])
    o = dict(DEFAULTS, **dict(options))
    lds = 8 * 16 * (20 * pad4(nu) + 5 * pad4(nfp))
    viscous = int(np.ravel(d["viscous"])[0])
    p = {"size_class": SIZE_CLASS.get((nu, nfp), -1), "flux_lds": lds}
    p["flux_waves"] = o["general_waves"] or (4 if lds <= 80 * 1024 else 8)
    p["flux_batched"] = int(p["size_class"] >= 0 and (staged(pad4(nu), p["flux_waves"]) + staged(pad4(nfp), p["flux_waves"])) * 5 <= 30)
    interior = any(k.startswith("int") for k in d)  # partner words exist only where a pair lies inside the block
    p["gather"] = int(bool(o["gather_delta"]) and viscous and p["flux_batched"] and interior)
    p["les"] = int(les)
    p["update_waves"] = o["general_update_waves"] or (4 if staged(pad4(nfp), 4) * 5 <= 20 and staged(nu, 4) * 5 <= 15 else 8)
    p["fold"] = int(bool(o["fold_general"]))
    return p


class options:
    """options on the shared context for the length of a run, the defaults afterwards"""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, DEFAULTS[k])


def check_block(e, d, want_u, want_div, tag):
    """one block after a time step: state (worst element reported), divergence of the last stage, flux-point solution, NaN flag"""
    u = e.download(hfx.DISU_UPTS0)
    per_ele = np.abs(u - want_u).max(axis=(0, 2)) / np.abs(want_u).max()
    worst = int(per_ele.argmax())
    err_div = relerr(e.download(hfx.DIV_TCONF_UPTS), want_div) if want_div is not None else 0.0
    err_fpts = relerr(e.download(hfx.DISU_FPTS), np.einsum("fu,uen->fen", np.asarray(d["opp_0"]), u))
    bad = e.check_nan()
    print("%s: state %.2e (element %d of %d)  div %.2e  fpts %.2e  nan %d" % (tag, per_ele[worst], worst, len(per_ele), err_div, err_fpts, bad))
    assert per_ele[worst] < TOL_U, (tag, "element", worst, per_ele[worst])
    assert err_div < TOL_DIV, (tag, err_div)
    assert err_fpts < TOL_FPTS, (tag, err_fpts)
    assert bad == -1, (tag, bad)


def run_block(ctx, d, key, opts=(), fixture=None, keep=None):
    """two time steps of fused 4 on a single-class block against the oracle on the same block (and, where `fixture` holds them,
    the genuine reference's states of the elements `keep`) -> the plan that ran"""
    ref = G.reference(key, d)
    nstage = int(d["sizes"][7])
    with options(ctx, opts):
        e, faces = build(ctx, d)
        try:
            if int(np.ravel(d["dt_type"])[0]) != 0:
                e.set_h_ref(d["h_ref"])
                ctx.set_CFL(float(np.ravel(d["CFL"])[0]))
            for st in range(G.N_STEPS):
                hfx.run_steps_blocks([e], faces, 1, fused=4)
                tag = "%s step %d" % ("-".join(str(k) for k in key), st)
                check_block(e, d, ref[st]["u"], ref[st]["div"], tag)
                if ref[st]["sensor"] is not None:
                    err = relerr(e.download(hfx.SENSOR), ref[st]["sensor"])
                    print("%s: sensor %.2e" % (tag, err))
                    assert err < TOL_SENSOR, (tag, err)
                k = "u_step%d_stage%d" % (st, nstage - 1)
                if fixture is not None and k in fixture:
                    want = fixture[k] if keep is None else fixture[k][:, keep, :]
                    err = relerr(e.download(hfx.DISU_UPTS0), want)
                    print("%s: against the genuine reference %.2e" % (tag, err))
                    assert err < TOL_U, (tag, err)
            return e.general_plan()
        finally:
            for f in faces:
                f.close()
            e.close()


def is_les(d):
    return "LES" in d and int(np.ravel(d["LES"])[0]) != 0 and int(np.ravel(d["SGS_model"])[0]) != 3


# ---- a. every size class on 1, 15, 17 and 33 elements ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.COUNTS)
@pytest.mark.parametrize("cls", list(G.CLASSES))
def test_partial_batches(ctx, cls, n):
    """a batch of 1 (one lane column of every tile alive), 15 (one padded element), 16 + 1 and 32 + 1 elements on the six
    instantiated sizes and on P4 tetrahedra (35, 60: the size-generic kernels, an LDS image of 130 560 bytes, so 8 flux waves and
    the looped staging).  P3 prisms (40, 68) run 8 flux and 8 update waves; their staging is the looped one on 3 and 4 waves
    (test_launch_forms) and the batched one on 8 (general_flux_batched, csrc/general.hpp)."""
    d = G.class_block(cls, n)
    plan = run_block(ctx, d, ("class", cls, n))
    assert plan == expected_plan(d, ()), plan
    if cls == "tet_p4":
        assert (plan["size_class"], plan["flux_waves"], plan["flux_batched"], plan["flux_lds"]) == (-1, 8, 0, 130560)
    if cls == "pri_p3":
        assert (plan["size_class"], plan["flux_waves"], plan["update_waves"]) == (5, 8, 8)


# ---- b. every launch form on 17 elements ------------------------------------------------------------------------------------------
FORMS = {"flux_waves_3": {"general_waves": 3}, "flux_waves_4": {"general_waves": 4}, "flux_waves_8": {"general_waves": 8},
         "update_waves_4": {"general_update_waves": 4}, "update_waves_8": {"general_update_waves": 8},
         "unfolded": {"fold_general": 0}, "face_delta": {"gather_delta": 0}, "unfolded_face_delta": {"fold_general": 0, "gather_delta": 0},
         "bdy_beside": {"bdy_beside": 1}}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cls", list(G.CLASSES))
def test_launch_forms(ctx, cls, form):
    """16 + 1 elements through every form an option selects; the plan shows that the form ran (split_rounds deals the tiles of
    P1 and P4 differently for 3, 4 and 8 waves; P3 prisms on 3 and 4 flux waves and every class on the generic kernels stage in a
    loop; the update kernel on 4 waves stages P3 prisms in a loop).  No form is refused by the option parser or the LDS limit on
    these seven classes: nothing is skipped."""
    d = G.class_block(cls, 17)
    opts = FORMS[form]
    plan = run_block(ctx, d, ("class", cls, 17), opts)
    want = expected_plan(d, opts.items())
    assert plan == want, (plan, want)
    shown = {"general_waves": "flux_waves", "general_update_waves": "update_waves", "fold_general": "fold", "gather_delta": "gather"}
    for k, v in opts.items():  # what the option asked for, literally (bdy_beside changes a stream, not the plan)
        assert k not in shown or plan[shown[k]] == v, (k, v, plan)


# ---- c. the features on 17 elements ---------------------------------------------------------------------------------------------------
FEATURE_RUNS = [(f, 0) for f in G.FEATURES] + [(f, w) for f in ("tet_p2_les_wale", "pri_p2_les_wale") for w in (3, 8)]


@pytest.mark.parametrize("name,waves", FEATURE_RUNS)
def test_features_on_partial_batches(ctx, name, waves):
    """LES closures (the LESG form; WALE also on 3 and 8 flux waves), over-integration, shock capturing (the sensor too), a local
    time step (h_ref cut per element), RoeM with Sutherland's law, Rusanov with an off-centre LDG switch, and an inviscid run, each
    on 16 + 1 elements"""
    d = G.feature_block(name)
    opts = {"general_waves": waves} if waves else {}
    plan = run_block(ctx, d, ("feature", name, 17), opts)
    assert plan == expected_plan(d, opts.items(), les=is_les(d)), plan


# ---- d. whole blocks in a random element order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tet_p2_n2_deformed", "pri_p3_n2_deformed", "mixed_p3_channel"])
def test_permuted_blocks(ctx, name):
    """every element of the fixture, in a seeded random order: the partners of a batch's flux points lie in other batches -- on
    the mixed channel, each class permuted, in any batch of the other block; the states are the genuine reference's, permuted"""
    d, keep = G.permuted(name)
    if "classes" in d:
        plans = run_mixed(ctx, d, ("permuted", name), fixture=G.load(name), keep=keep)
        assert plans[2]["gather"] == 1 and plans[3]["gather"] == 1
        return
    assert not any(k.startswith("bdy") for k in d)
    run_block(ctx, d, ("permuted", name), fixture=G.load(name), keep=keep)


def run_mixed(ctx, d, key, fixture=None, keep=None):
    from test_mixed_mesh import build_gpu
    ref = G.reference(key, d)
    classes, E, F = build_gpu(ctx, d)
    per = MU.split(d)[1]
    nstage = int(d["c%d_sizes" % classes[0]][7])
    try:
        for st in range(G.N_STEPS):
            hfx.run_steps_blocks([E[c] for c in classes], F, 1, fused=4)
            for c in classes:
                tag = "%s class %d step %d" % ("-".join(str(k) for k in key), c, st)
                check_block(E[c], per[c], ref[st][c]["u"], ref[st][c]["div"], tag)
                k = "c%d_u_step%d_stage%d" % (c, st, nstage - 1)
                if fixture is not None and k in fixture:
                    err = relerr(E[c].download(hfx.DISU_UPTS0), fixture[k][:, keep[c], :])
                    print("%s: against the genuine reference %.2e" % (tag, err))
                    assert err < TOL_U, (tag, err)
        return {c: E[c].general_plan() for c in classes}
    finally:
        for f in F:
            f.close()
        for c in classes:
            E[c].close()


# ---- e. tails in both blocks of a mixed mesh ----------------------------------------------------------------------------------------------
def test_mixed_channel_with_tails_in_both_blocks(ctx):
    """23 tetrahedra (16 + 7) and 15 prisms: partner words cross the blocks, the fixture's walls stand beside the cut faces"""
    d = G.mixed_block()
    plans = run_mixed(ctx, d, ("mixed", "mixed_p3_channel", 38))
    assert (plans[2]["size_class"], plans[3]["size_class"]) == (2, 5)
    assert plans[2]["gather"] == 1 and plans[3]["gather"] == 1


# ---- f. partition faces on partial batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,n", [("tet_p2", 17), ("pri_p2", 15)])
def test_partitioned_partial_batches(ctx, cls, n):
    """hfx_run_steps_partitioned_blocks on the cut blocks: half of the interior faces that are left exchanged with the rank itself,
    the cut faces as boundary faces, against the oracle on the undivided cut block.  (Of the prisms only the triangular faces are
    partitioned: see test_simplex_les_on_partitioned_blocks in tests/test_mixed_mesh.py.)"""
    d = G.class_block(cls, n)
    ref = G.reference(("class", cls, n), d)
    c = int(d["sizes"][6])
    e, faces = build(ctx, d)
    bdy = [f for f in faces if isinstance(f, hfx.BdyInters)]
    for f in faces:
        if isinstance(f, hfx.IntInters):
            f.close()
    tabs = {t: (c, c, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d}
    cut = [tabs[t] for t in tabs if c != 3 or t == 1]
    rest, M = self_partition(ctx, {c: e}, cut)
    rest = rest + [tabs[t] for t in tabs if c == 3 and t != 1]
    assert bdy and len(M) >= 1
    F = [hfx.IntInters(ctx, e, e, L, R) for a, b, L, R in rest] + bdy
    comm = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    try:
        for st in range(G.N_STEPS):
            hfx.run_steps_partitioned_blocks([e], F, M, comm, 1)
            check_block(e, d, ref[st]["u"], ref[st]["div"], "partitioned %s-%d step %d" % (cls, n, st))
    finally:
        for f in F + M:
            f.close()
        comm.close()
        e.close()


# ---- g. hexahedra: any 3-D five-field block runs the size-generic kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex_p1_rk24", "hex_p2_n3_deformed", "hex_p2_bdy_walls"])
def test_hexahedra_through_the_generic_kernels(ctx, name):
    """general_build takes its operators from the dense form every block keeps (make_operator uploads it for the tensor-product
    classes too; padded_operator pads that), so 27 hexahedra (16 + 11) at P1 (8, 24) and P2 (27, 54) run the size-generic kernels:
    RK24 (the stage-dependent register reads of the update kernel), a periodic box, and all six boundary kinds, against the
    genuine reference"""
    d = G.load(name)
    plan = run_block(ctx, d, ("fixture", name), fixture=d)
    assert plan == expected_plan(d, ()) and plan["size_class"] == -1, plan


# ---- h. a class whose batch does not fit LDS ----------------------------------------------------------------------------------------------------
def test_block_too_large_for_lds_is_refused(ctx):
    """P5 tetrahedra (56, 84): a batch's image is 197 120 bytes, over the 160 kB of a CU -- refused before anything is launched"""
    import hfx_host as H
    b = G.load("tet_p2_n2_deformed")
    ne = 3
    S = H.Simplex(2, 5, b["shape"][:, :4, :ne], viscous=1)
    d = {k: S.array(k) for k in ["opp_0", "opp_3", "opp_6", "detjac_upts", "JGinv_upts", "detjac_fpts", "JGinv_fpts", "tdA_fpts", "norm_fpts"] +
         ["opp_%d_%d" % (w, dd) for w in (1, 2, 4, 5) for dd in range(3)]}
    S.close()
    assert d["opp_0"].shape == (84, 56) and 8 * 16 * (20 * 56 + 5 * 84) == 197120
    ctx.set_params(hfx.params_from(b))
    e = hfx.Eles(ctx, [ne, 56, 84, 5, 3], d, ele_type=2, order=5)
    u = np.zeros((56, ne, 5), order="F")
    u[:, :, 0], u[:, :, 4] = 1.0, 2.5
    e.upload(hfx.DISU_UPTS0, u)
    try:
        with pytest.raises(hfx.HfxError, match="does not fit LDS"):
            hfx.run_steps_blocks([e], [], 1, fused=4)
        with pytest.raises(hfx.HfxError, match="hfx_general_plan"):
            e.general_plan()
        assert np.array_equal(e.download(hfx.DISU_UPTS0), u)
    finally:
        e.close()
