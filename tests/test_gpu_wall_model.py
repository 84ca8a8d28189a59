"""The wall model on the device (Werner-Wengle, Breuer-Rodi; csrc/wall_model.hpp, csrc/kernels_bdy.hpp) against the genuine
reference's fixtures under tests/golden/wall_model (18 hexahedra / 12 quadrilaterals, two RK45 steps).

Bars, the ones the boundary sweeps and the step loops hold everywhere else in this suite: 1e-12 of the block's scale for
norm_tconf_fpts and delta_disu_fpts after the boundary sweeps, 1e-11 for the state after every stage / step.  That no path can
meet them by ignoring the model is shown in tests/test_wall_model_host.py (the state without the model is 5e-3 or more away).
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import bdy_util
import hfx
import wall_model_util as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wall_model")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "wm_*.npz")))
RTOL1, RTOLS = 1e-12, 1e-11
_cache = {}


def load(name):
    """the fixture and its restated input points, read once"""
    if name not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        upt, dist, _ = W.input_points(d)
        _cache[name] = (d, upt, dist)
    d, upt, dist = _cache[name]
    return dict(d), upt, dist


def relerr(a, b):
    scale = np.abs(b).max()
    return np.abs(a - b).max() / (scale if scale > 0 else 1.0)


def sc(d, k):
    return float(np.ravel(d[k])[0])


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def build(ctx, d, upt=None, dist=None, wall_model=None):
    """the fixture's block through the raw C ABI; wall_model None: the fixture's"""
    kk = W.meta_of(d)["keys"]
    ctx.set_params(hfx.params_from(d))
    model = kk["wall_model"] if wall_model is None else wall_model
    ctx.set_wall_model(model, sc(d, "prandtl_t") if "prandtl_t" in d else 0.9, sc(d, "Kappa") if "Kappa" in d else 0.41)
    sz = [int(v) for v in d["sizes"]]
    e = hfx.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    faces = []
    for t in range(3):
        if "int%d_L" % t in d:
            faces.append(hfx.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]))
    for t in range(3):
        if "bdy%d_L" % t in d:
            b = hfx.BdyInters(ctx, e, d["bdy%d_L" % t], d["bdy%d_id" % t], hfx.bc_records(d["bc_flags"], d["bc_params"]),
                              sc(d, "bc_R_ref"), int(sc(d, "ramp_counter")))
            if upt is not None:
                b.set_wall_model_points(upt, dist)
            faces.append(b)
    if "LES" in d and int(sc(d, "LES")):
        e.set_les(int(sc(d, "SGS_model")), sc(d, "C_s"), sc(d, "filter_ratio"), sc(d, "Kappa"), sc(d, "prandtl_t"), d["Jacobian_fpts"],
                  None, None)
    e.upload(hfx.DISU_UPTS0, d["u_init"])
    return e, faces


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


def final_state(d):
    steps = sorted({int(k.split("_")[1][4:]) for k in d if k.startswith("u_step")})
    return len(steps), d["u_step%d_stage%d" % (steps[-1], int(d["sizes"][7]) - 1)]


def model_points(d):
    L, _ = W.bdy_block(d)
    n_fpts = d["s0_disu_fpts"].shape[0]
    pts = L[:, W.model_faces(d)].ravel()
    return pts % n_fpts, pts // n_fpts


@pytest.mark.parametrize("name", NAMES)
def test_boundary_sweeps(ctx, name):
    """one residual call by call: the common flux after the inviscid sweep (slip mirror at the model faces), the LDG differences
    (wall-parallel velocity there), and the total common flux after the viscous sweep (the modelled stress there)"""
    d, upt, dist = load(name)
    e, faces = build(ctx, d, upt, dist)
    bdy = [f for f in faces if isinstance(f, hfx.BdyInters)]
    assert bdy[0].wall_model_faces() == len(W.model_faces(d)) > 0
    fm, em = model_points(d)
    les = "LES" in d and int(sc(d, "LES"))
    inner = [f for f in faces if isinstance(f, hfx.IntInters)]
    e.extrapolate_solution()
    e.calculate_gradient()
    e.evaluate_invFlux()
    for f in inner:
        f.calculate_common_invFlux()
    for f in bdy:
        f.evaluate_boundaryConditions_invFlux()
    got = e.download(hfx.NORM_TCONF_FPTS)
    err = relerr(got, d["s0_norm_tconf_fpts_inv"])
    print("%s: norm_tconf after the inviscid sweep %.2e" % (name, err))
    assert err < RTOL1
    e.correct_gradient()
    e.evaluate_viscFlux()
    if les:
        e.extrapolate_sgsFlux()  # src/solver.cpp:162-167
    e.extrapolate_totalFlux()
    e.calculate_divergence()
    for f in inner:
        f.calculate_common_viscFlux()
    for f in bdy:
        f.evaluate_boundaryConditions_viscFlux()
    delta = e.download(hfx.DELTA_DISU_FPTS)
    scale = np.abs(d["s0_delta_disu_fpts"]).max()
    err_d = np.abs(delta[fm, em, :] - d["s0_delta_disu_fpts"][fm, em, :]).max() / scale
    got = e.download(hfx.NORM_TCONF_FPTS)
    err = relerr(got, d["s0_norm_tconf_fpts"])
    err_m = np.abs(got[fm, em, :] - d["s0_norm_tconf_fpts"][fm, em, :]).max() / np.abs(d["s0_norm_tconf_fpts"]).max()
    print("%s: delta_disu at the model faces %.2e, norm_tconf after the viscous sweep %.2e (model faces %.2e)" % (name, err_d, err, err_m))
    assert relerr(delta, d["s0_delta_disu_fpts"]) < RTOL1 and err_d < RTOL1
    assert err < RTOL1 and err_m < RTOL1
    e.calculate_corrected_divergence()
    assert relerr(e.download(hfx.DIV_TCONF_UPTS), d["s0_div_tconf_upts"]) < 5e-11
    close(e, faces)


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_call_by_call(ctx, name):
    d, upt, dist = load(name)
    e, faces = build(ctx, d, upt, dist)
    nstage, adv = int(d["sizes"][7]), int(sc(d, "adv_type"))
    worst = 0.0
    for st in range(final_state(d)[0]):
        for rk in range(nstage):
            hfx.CalcResidual(e, faces)
            e.AdvanceSolution(rk, adv)
            err = relerr(e.download(hfx.DISU_UPTS0), d["u_step%d_stage%d" % (st, rk)])
            worst = max(worst, err)
            assert err < RTOLS, (st, rk, err)
    print("%s: every stage call by call %.2e" % (name, worst))
    assert e.check_nan() == -1
    close(e, faces)


# hfx_run_steps: per-method (0), the split fused stage (2, 3) and the general fused stage (4), with the viscous boundary kernels on
# the compute stream and (bdy_beside) on the side stream beside the interior-face kernel.  The general stage takes three-dimensional
# blocks, and an LES closure on tetrahedra and prisms only: it runs the three hexahedral fixtures without a closure
GENERAL = [n for n in NAMES if "hex" in n and "wale" not in n]
RUNS = [(n, f, b) for n in NAMES for f, b in ((0, 0), (2, 0), (2, 1), (3, 0), (3, 1))] + [(n, 4, b) for n in GENERAL for b in (0, 1)]


@pytest.mark.parametrize("name,fused,beside", RUNS)
def test_run_steps(ctx, name, fused, beside):
    d, upt, dist = load(name)
    ctx.set_option("bdy_beside", beside)
    e, faces = build(ctx, d, upt, dist)
    n_steps, want = final_state(d)
    hfx.run_steps(e, faces, n_steps, fused=fused)
    err = relerr(e.download(hfx.DISU_UPTS0), want)
    print("%s: hfx_run_steps fused %d, bdy_beside %d: %.2e" % (name, fused, beside, err))
    assert err < RTOLS
    assert e.check_nan() == -1
    close(e, faces)


def mirror_case(d, **kw):
    kk = W.meta_of(d)["keys"]
    over = dict(mu_gas=kk["mu_gas"], wall_model=kk["wall_model"])
    if kk.get("LES"):
        over.update(LES=1, SGS_model=kk["SGS_model"], C_s=kk["C_s"], filter_ratio=kk["filter_ratio"])
    over.update(kw)
    return bdy_util.case_from_fixture(d, **over)[0]


@pytest.mark.parametrize("mode", ["deferred", "calls"])
@pytest.mark.parametrize("name", NAMES)
def test_through_the_mirror(name, mode):
    """from the mesh and the input keys alone (hfxh_case_run): the mirror finds the input points and registers model and points;
    its calls run deferred (whole stages fused) and one by one"""
    d, _, _ = load(name)
    c = mirror_case(d)
    try:
        c.set_deferred(mode == "deferred")
        c.to_device(0)
        n_steps, want = final_state(d)
        c.run(n_steps)
        c.sync_host()
        err = relerr(c.array("disu_upts0"), want)
        print("%s: the mirror, %s: %.2e" % (name, mode, err))
        assert err < RTOLS
    finally:
        c.close()


@pytest.mark.parametrize("name", ["wm_hex_p2_ww", "wm_quad_p3_br"])
def test_self_partitioned(name):
    """the wrap-around faces of x as partition faces of the one rank: the partitioned step loop.  The input point lies in the
    face's own element, so nothing of the model crosses ranks"""
    d, _, _ = load(name)
    c = mirror_case_partitioned(d, W.meta_of(d))
    try:
        c.to_device(0)
        c.set_comm(hfx.comm_unique_id())
        n_steps, want = final_state(d)
        c.run_partitioned(n_steps)
        c.sync_host()
        err = relerr(c.array("disu_upts0"), want)
        print("%s: self-partitioned: %.2e" % (name, err))
        assert err < RTOLS
    finally:
        c.close()


def mirror_case_partitioned(d, meta):
    """bdy_util.case_from_fixture with the Case keyword self_partition (x)"""
    import hfx_host as H
    kk = meta["keys"]
    bcs, sides = bdy_util.groups_of(meta)
    n = list(meta["n"])
    kw = dict(dims=meta["dims"], order=kk["order"], adv_type=kk["adv_type"], riemann_solve_type=kk["riemann_solve_type"], viscous=kk["viscous"],
              ic_form=kk["ic_form"], fix_vis=kk["fix_vis"], T_c_ic=kk["T_c_ic"], rho_c_ic=kk["rho_c_ic"], dt=kk["dt"], Mach_c_ic=kk["Mach_c_ic"],
              mu_gas=kk["mu_gas"], wall_model=kk["wall_model"],
              upts_type=kk["upts_type_hexa" if meta["dims"] == 3 else "upts_type_quad"],
              vcjh_scheme=kk["vcjh_scheme_hexa" if meta["dims"] == 3 else "vcjh_scheme_quad"])
    return H.Case(n + [1] * (3 - len(n)), xv=d["xv"], bcs=bcs, sides=sides, self_partition=[1, 0, 0], **kw)


# ---- refusals and acceptances ------------------------------------------------------------------------------------------------
def test_use_wm_without_a_model_keeps_its_refusal(ctx):
    d, upt, dist = load("wm_quad_p3_ww")
    with pytest.raises(hfx.HfxError, match="uses the wall model, which is not part of this path"):
        build(ctx, d, wall_model=0)


def test_unknown_model_is_the_references_error(ctx):
    with pytest.raises(hfx.HfxError, match="Wall model not implemented!"):
        ctx.set_wall_model(3)


def test_viscous_sweep_without_points_is_refused_before_any_launch(ctx):
    d, upt, dist = load("wm_quad_p3_ww")
    e, faces = build(ctx, d)  # no points
    bdy = [f for f in faces if isinstance(f, hfx.BdyInters)][0]
    u0 = e.download(hfx.DISU_UPTS0)
    for call in (lambda: bdy.evaluate_boundaryConditions_viscFlux(), lambda: hfx.CalcResidual(e, faces), lambda: hfx.run_steps(e, faces, 1),
                 lambda: hfx.run_steps(e, faces, 1, fused=3), lambda: hfx.run_steps(e, faces, 1, fused=4)):
        with pytest.raises(hfx.HfxError, match="no input points"):
            call()
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u0)
    bad = upt.copy()
    bad[W.model_faces(d)[0]] = int(d["sizes"][1])  # n_upts: one past the last solution point
    with pytest.raises(hfx.HfxError, match="out of range"):
        bdy.set_wall_model_points(bad, dist)
    # entries of faces without a model are ignored, whatever they hold
    d2, upt2, dist2 = load("wm_hex_p2_ww_wale")
    close(e, faces)
    e, faces = build(ctx, d2)
    bdy = [f for f in faces if isinstance(f, hfx.BdyInters)][0]
    junk = upt2.copy()
    others = np.setdiff1d(np.arange(len(junk)), W.model_faces(d2))
    junk[others] = -7
    bdy.set_wall_model_points(junk, dist2)
    n_steps, want = final_state(d2)
    hfx.run_steps(e, faces, n_steps, fused=0)
    assert relerr(e.download(hfx.DISU_UPTS0), want) < RTOLS
    close(e, faces)


def test_inviscid_context_takes_the_slip_mirror(ctx):
    """an inviscid context accepts a use_wm group: its sol_spec 0 state is the slip wall's, bit for bit"""
    d, upt, dist = load("wm_quad_p3_ww")
    out = []
    for flag, use_wm in ((hfx.BC_ISOTHERM_WALL, 1), (hfx.BC_SLIP_WALL, 0)):
        d1 = dict(d)
        d1["viscous"] = np.array([0.0])
        fl = np.array(d["bc_flags"]).copy()
        walls = [g for g in range(fl.shape[1]) if fl[0, g] in (hfx.BC_ISOTHERM_WALL, hfx.BC_ADIABAT_WALL)]
        fl[0, walls], fl[2, walls] = flag, use_wm
        d1["bc_flags"] = fl
        e, faces = build(ctx, d1)
        bdy = [f for f in faces if isinstance(f, hfx.BdyInters)][0]
        e.extrapolate_solution()
        bdy.evaluate_boundaryConditions_invFlux()
        out.append(e.download(hfx.NORM_TCONF_FPTS))
        close(e, faces)
    fm, em = model_points(d)
    assert np.abs(out[0][fm, em, :]).max() > 0
    assert np.array_equal(out[0][fm, em, :], out[1][fm, em, :])


@pytest.mark.parametrize("fused", [0, 3])
def test_a_model_in_the_context_changes_nothing_without_use_wm(ctx, fused):
    """every group use_wm 0 under a context with a model: bit-identical to the same run without a model"""
    d, _, _ = load("wm_hex_p2_ww")
    d["bc_flags"] = np.array(d["bc_flags"]).copy()
    d["bc_flags"][2] = 0
    out = []
    for model in (0, 1, 2):
        e, faces = build(ctx, d, wall_model=model)
        assert [f for f in faces if isinstance(f, hfx.BdyInters)][0].wall_model_faces() == 0
        hfx.run_steps(e, faces, 1, fused=fused)
        out.append(e.download(hfx.DISU_UPTS0))
        close(e, faces)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
