"""Triangles on the device, against the genuine reference's fixtures under tests/golden/tris (tools/capture_tris.py): the per-method
path (fused 0), the 2-D simplex fused stage (csrc/simplex2d.hip; hfx_run_steps_blocks(..., fused = 4)) and the same stage behind the
deferred call sequence.

Bars, relative to the array's largest magnitude: 1e-12 for one residual's intermediates, 5e-11 for div_tconf_upts, 1e-11 for states
after whole steps, 1e-12 for disu_fpts against opp_0 of the new state.  Every fused run asserts hfx_simplex2d_plan, so a silent
per-method run cannot pass.  Blocks of 1, G - 1, G + 1 and 2 G + 1 elements (G = 32 at P3) come from tests/tri_util.py and are
checked against the oracle on the same block (tests/test_tris_oracle.py shows without a GPU that each is a sound input).

Without the stage every fused test here fails at general_prepare's "three-dimensional ... blocks only"; the per-method tests pass."""
import os

import numpy as np
import pytest

import hfx
import tri_util as T
from test_gpu_methods_vs_golden import build
from test_gpu_deferred import calc_residual_calls, tag

pytestmark = pytest.mark.gpu

TOL_1, TOL_DIV, TOL_U, TOL_FPTS = 1e-12, 5e-11, 1e-11, 1e-12
NAMES = T.names()
SIZES = {(3, 6): (0, 64), (6, 9): (1, 64), (10, 12): (2, 32), (15, 15): (3, 32), (21, 18): (4, 16)}  # SIMPLEX2D_SIZES of csrc/simplex2d.hpp
G_P3 = T.GROUP[3]
relerr = T.relerr


@pytest.fixture(scope="module")
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


def make(ctx, d):
    e, faces = build(ctx, d)
    if int(np.ravel(d["dt_type"])[0]) != 0:
        e.set_h_ref(d["h_ref"])
        ctx.set_CFL(float(np.ravel(d["CFL"])[0]))
    return e, faces


def expected_plan(d, gather=1):
    nu, nfp = int(d["sizes"][1]), int(d["sizes"][2])
    cls, g = SIZES[(nu, nfp)]
    interior = any(k.startswith("int") for k in d)
    return {"size_class": cls, "group": g, "waves": 4, "gather": int(bool(gather) and bool(int(np.ravel(d["viscous"])[0])) and interior),
            "element_lds": 8 * (4 * nu * nu + 6 * nu * nfp + (g + 1) * (12 * nu + 4 * nfp)),
            "update_lds": 8 * (2 * nu * nfp + (g + 1) * (4 * nu + 4 * nfp))}


def check_fpts_and_nan(e, d, what):
    u = e.download(hfx.DISU_UPTS0)
    err = relerr(e.download(hfx.DISU_FPTS), np.einsum("fu,uen->fen", np.asarray(d["opp_0"]), u))
    print("%s: disu_fpts against opp_0 u %.2e" % (what, err))
    assert err < TOL_FPTS, (what, err)
    assert e.check_nan() == -1, what


# ---- 1. the per-method path ------------------------------------------------------------------------------------------------------
def test_per_method_every_intermediate(ctx):
    d = T.load("tri_p2_n3_deformed")
    e, faces = make(ctx, d)
    got = {}
    e.extrapolate_solution(); got["s0_disu_fpts"] = e.download(hfx.DISU_FPTS)
    e.calculate_gradient(); got["s0_grad_disu_upts_ref"] = e.download(hfx.GRAD_DISU_UPTS)
    e.evaluate_invFlux(); got["s0_tdisf_upts_inv"] = e.download(hfx.TDISF_UPTS)
    for f in faces:
        f.calculate_common_invFlux()
    got["s0_norm_tconf_fpts_inv"] = e.download(hfx.NORM_TCONF_FPTS)
    got["s0_delta_disu_fpts"] = e.download(hfx.DELTA_DISU_FPTS)
    e.correct_gradient()
    got["s0_grad_disu_upts"] = e.download(hfx.GRAD_DISU_UPTS); got["s0_grad_disu_fpts"] = e.download(hfx.GRAD_DISU_FPTS)
    e.evaluate_viscFlux(); got["s0_tdisf_upts"] = e.download(hfx.TDISF_UPTS)
    e.extrapolate_totalFlux(); got["s0_norm_tdisf_fpts"] = e.download(hfx.NORM_TDISF_FPTS)
    e.calculate_divergence(); got["s0_div_tconf_upts_disc"] = e.download(hfx.DIV_TCONF_UPTS)
    for f in faces:
        f.calculate_common_viscFlux()
    got["s0_norm_tconf_fpts"] = e.download(hfx.NORM_TCONF_FPTS)
    e.calculate_corrected_divergence(); got["s0_div_tconf_upts"] = e.download(hfx.DIV_TCONF_UPTS)
    for k, v in got.items():
        err, bar = relerr(v, d[k]), TOL_DIV if "div_tconf" in k else TOL_1
        print("%-26s %.2e" % (k, err))
        assert err < bar, (k, err)
    assert e.check_nan() == -1
    close(e, faces)


@pytest.mark.parametrize("name", NAMES)
def test_per_method_states(ctx, name):
    """every dumped stage state, stage by stage: hfx_CalcResidual + hfx_eles_AdvanceSolution"""
    d = T.load(name)
    e, faces = make(ctx, d)
    nstage, adv, dt_type = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0]), int(np.ravel(d["dt_type"])[0])
    for st in range(max(T.stored_steps(d)) + 1):
        if dt_type != 0:
            p = hfx.params_from(d)
            p.dt = e.calc_dt_local(float(np.ravel(d["CFL"])[0]))
            assert abs(p.dt - float(np.ravel(d["dt_step%d" % st])[0])) <= 1e-11 * p.dt
            ctx.set_params(p)
        for rk in range(nstage):
            hfx.CalcResidual(e, faces)
            if st == 0 and rk == 0:
                assert relerr(e.download(hfx.DIV_TCONF_UPTS), d["s0_div_tconf_upts"]) < TOL_DIV
            e.AdvanceSolution(rk, adv)
            key = "u_step%d_stage%d" % (st, rk)
            if key in d:
                err = relerr(e.download(hfx.DISU_UPTS0), d[key])
                assert err < TOL_U, (key, err)
    assert e.check_nan() == -1
    close(e, faces)


# ---- 2. the fused stage ----------------------------------------------------------------------------------------------------------
def run_fused_steps(ctx, d, want, what, opts=(), grids=None):
    """one call of one step per entry of `want` (the state after that step, or None); -> the plan that ran (grids: a list that
    receives hfx.fused_launch_grids of the last stage)"""
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        e, faces = make(ctx, d)
        for st, w in enumerate(want):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            if w is not None:
                u = e.download(hfx.DISU_UPTS0)
                per_ele = np.abs(u - w["u"]).max(axis=(0, 2)) / np.abs(w["u"]).max()
                print("%s step %d: state %.2e (element %d of %d)" % (what, st, per_ele.max(), int(per_ele.argmax()), len(per_ele)))
                assert per_ele.max() < TOL_U, (what, st, int(per_ele.argmax()), per_ele.max())
                if w.get("div") is not None:
                    err = relerr(e.download(hfx.DIV_TCONF_UPTS), w["div"])
                    print("%s step %d: div_tconf_upts %.2e" % (what, st, err))
                    assert err < 10 * TOL_DIV, (what, st, err)  # (of the step's LAST stage: the bar of tests/test_gpu_general_batches.py)
            check_fpts_and_nan(e, d, "%s step %d" % (what, st))
        plan = e.simplex2d_plan()
        if grids is not None:
            grids.extend(hfx.fused_launch_grids(e.h))
        close(e, faces)
        return plan
    finally:
        for k, _ in opts:
            ctx.set_option(k, 1 if k == "gather_delta" else 0)


@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_fused_states(ctx, name, gather):
    """fused 4 on every fixture (boundaries and the cylinder included) against the genuine reference's state after every stored
    step; the LDG corrections gathered in the element kernel (the default) and written by face_delta_kernel<2>"""
    d = T.load(name)
    nstage = int(d["sizes"][7])
    steps = T.stored_steps(d)
    want = [({"u": d["u_step%d_stage%d" % (st, nstage - 1)]} if "u_step%d_stage%d" % (st, nstage - 1) in d else None) for st in range(max(steps) + 1)]
    assert want[-1] is not None
    plan = run_fused_steps(ctx, d, want, name, [("gather_delta", gather)])
    assert plan == expected_plan(d, gather), plan


@pytest.mark.parametrize("adv", [0, 1, 2, 4])
def test_fused_every_adv_type(ctx, adv):
    """tri_p2_n3_deformed's inputs with adv_type overridden (the fixture is RK45, adv_type 3), two steps against the oracle"""
    d = T.load("tri_p2_n3_deformed")
    d["adv_type"] = np.array([adv])
    d["sizes"] = np.array(list(d["sizes"][:7]) + [{0: 1, 1: 4, 2: 4, 4: 14}[adv]], dtype=np.int32)
    if adv == 4:  # (the fixture carries RK45's coefficients; RK414's are the reference's, from hex_p1_rk414)
        rk = np.load(os.path.join(os.path.dirname(T.GOLDEN), "hex_p1_rk414.npz"))
        d["RK_a"], d["RK_b"] = rk["RK_a"], rk["RK_b"]
    ref = T.reference(("adv", adv), d)
    assert all(r["bad"] == -1 for r in ref)
    run_fused_steps(ctx, d, ref, "adv_type %d" % adv)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("n", [1, G_P3 - 1, G_P3 + 1, 2 * G_P3 + 1])
def test_fused_group_edges(ctx, n, cap):
    """a last group of 1, G - 1 and 1 elements behind 0, 0, 1 and 2 whole ones; cap 1: ONE workgroup walks all groups"""
    d = T.block(n)
    ref = T.reference(("block", n), d)
    plan = run_fused_steps(ctx, d, ref, "block of %d" % n, [("persistent_grid_cap", cap)])
    assert plan["group"] == G_P3 and plan == expected_plan(d)


# ---- 3. the deferred call sequence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peek", [False, True])
def test_deferred_call_sequence(peek):
    """the reference's calls on tri_p3_n4_deformed with `deferred` 1: every whole stage runs as the 2-D simplex stage (n_fused), and
    the states equal the per-method ones; peek: a download of grad_disu_upts between two calls makes that record replay"""
    d = T.load("tri_p3_n4_deformed")
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    states = {}
    for mode in ("per_method", "deferred"):
        c = hfx.Context(0)
        c.set_option("deferred", int(mode == "deferred"))
        e, faces = make(c, d)
        tag(e, d)
        got = []
        for st in range(2):
            for rk in range(nstage):
                calc_residual_calls([e], faces, True, rk)
                if peek and mode == "deferred" and st == 0 and rk == 1:
                    g = e.download(hfx.GRAD_DISU_UPTS)
                    assert np.isfinite(g).all() and np.abs(g).max() > 0
                e.AdvanceSolution(rk, adv)
                got.append(e.download(hfx.DISU_UPTS0))
        if mode == "deferred":
            nf, nr, why = c.deferred_stats()
            print("deferred: %d fused, %d replayed (%s)" % (nf, nr, why))
            assert nf == 2 * nstage - (1 if peek else 0), (nf, nr, why)
            assert e.simplex2d_plan() == expected_plan(d)
        states[mode] = got
        close(e, faces)
        c.close()
    for i, (a, b) in enumerate(zip(states["deferred"], states["per_method"])):
        assert relerr(a, b) < TOL_U, (i, relerr(a, b))
        key = "u_step%d_stage%d" % (i // nstage, i % nstage)
        if key in d:
            assert relerr(a, d[key]) < TOL_U, key


# ---- 4. the per-step duties ------------------------------------------------------------------------------------------------------
def test_duties_in_the_fused_loop():
    """with the clock set: time averages and the residual history rows (res_norm_type 2, no forces) of a fused-4 loop equal those
    of the fused-0 loop at the bars of tests/test_gpu_time_average.py (1e-12 per field) and tests/test_gpu_history_rows.py (1e-11 on
    the norm)"""
    d = T.load("tri_p3_n4_deformed")
    fields = ["rho_average", "u_average", "v_average", "e_average"]
    out = {}
    for fused in (0, 4):
        c = hfx.Context(0)
        e, faces = make(c, d)
        e.set_average_fields(fields)
        c.set_history_monitor(2, False, 1, capacity=4)
        c.set_clock(0.25, 0)
        hfx.run_steps_blocks([e], faces, 3, fused=fused)
        times, steps, res, frc = e.read_history()
        out[fused] = (e.download_average(), c.get_clock(), np.array(times), np.array(steps), np.array(res))
        close(e, faces)
        c.close()
    a0, clock0, t0, s0, r0 = out[0]
    a4, clock4, t4, s4, r4 = out[4]
    assert clock0 == clock4 and list(s0) == [1, 2, 3] == list(s4) and np.array_equal(t0, t4)
    avg = max(np.abs(a4[:, :, i] - a0[:, :, i]).max() / np.abs(a0[:, :, i]).max() for i in range(a0.shape[2]))
    rows = float((np.abs(r4 - r0) / np.abs(r0)).max())
    print("averages %.2e, residual rows %.2e" % (avg, rows))
    assert avg <= 1e-12 and rows <= 1e-11


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def refused(e, blocks, faces, match):
    before = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match=match) as err:
        hfx.run_steps_blocks(blocks, faces, 1, fused=4)
    assert "fused 0" in str(err.value), str(err.value)
    assert np.array_equal(e.download(hfx.DISU_UPTS0), before)


def test_refusals(ctx):
    d = T.load("tri_p3_n4_deformed")
    # partition faces: the cut faces of a block as a partition-face block
    b = T.block(G_P3 - 1)
    e, faces = make(ctx, b)
    keep = [f for f in faces if isinstance(f, hfx.IntInters)]
    L = np.asarray(b["bdy0_L"])
    mpi = hfx.MpiInters(ctx, e, L, np.repeat(np.arange(L.shape[0], dtype=np.int32)[::-1, None], L.shape[1], axis=1))
    refused(e, [e], keep + [mpi], "partition faces")
    mpi.close()
    close(e, faces)
    # a registered LES closure, over-integration, shock capturing: the quad fixtures' registration data of the same order fit no
    # triangle, so each is registered with arrays of the right shape -- the refusal comes before anything reads them
    nu, ne = int(d["sizes"][1]), int(d["sizes"][0])
    e, faces = make(ctx, d)
    e.set_les(1, 0.325, 1.0, 0.41, 0.9, np.ones((2, 2, int(d["sizes"][2]), ne), order="F"))
    refused(e, [e], faces, "LES closure")
    close(e, faces)
    e, faces = make(ctx, d)
    e.set_over_int(np.zeros((nu + 2, nu), order="F"), np.zeros((nu, nu + 2), order="F"), np.ones((2, 2, nu + 2, ne), order="F"))
    refused(e, [e], faces, "over-integration")
    close(e, faces)
    e, faces = make(ctx, d)
    e.set_shock_capture(np.eye(nu, order="F"), np.eye(nu, order="F"), np.ones(nu), np.arange(nu - 1, nu, dtype=np.int32), 1.0, 0)
    refused(e, [e], faces, "shock capturing")
    close(e, faces)
    # several element blocks of which one is two-dimensional
    e, faces = make(ctx, d)
    e2, faces2 = make(ctx, d)
    refused(e, [e, e2], faces + faces2, "several element blocks")
    close(e2, faces2)
    # ... and the block runs once the closure is gone: a refusal leaves nothing behind
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage4"]) < TOL_U
    close(e, faces)


def test_quadrilaterals_stay_refused(ctx):
    q = dict(np.load(os.path.join(os.path.dirname(T.GOLDEN), "quad_p3_scrambled.npz")))
    e, faces = build(ctx, q)
    with pytest.raises(hfx.HfxError, match="three-dimensional"):
        hfx.run_steps_blocks([e], faces, 1, fused=4)
    close(e, faces)


def test_plan_is_refused_before_a_fused_call(ctx):
    e, faces = make(ctx, T.load("tri_p1_n4_deformed"))
    with pytest.raises(hfx.HfxError, match="no 2-D simplex fused stage has prepared"):
        e.simplex2d_plan()
    hfx.run_steps_blocks([e], faces, 1, fused=0)
    with pytest.raises(hfx.HfxError, match="no 2-D simplex fused stage has prepared"):
        e.simplex2d_plan()
    close(e, faces)


def test_timing_and_byte_queries(ctx):
    """hfx_time_general_kernels: four slots with the stage's kernel names; hfx_general_kernel_bytes: the plan's algorithmic bytes"""
    d = T.load("tri_p3_n4_deformed")
    e, faces = make(ctx, d)
    ms, names = hfx.time_general_kernels([e], faces, 2)
    assert names.split(",") == ["face_delta_kernel", "simplex2d_element_kernel", "face_flux2_kernel", "simplex2d_update_kernel"]
    assert e.simplex2d_plan()["gather"] == 1  # (slot 0 then holds no launch: the time between two events)
    assert all(m > 0.0 for m in ms[1:4]) and ms[0] < min(ms[1:4]) and not any(ms[4:])
    by = hfx.general_kernel_bytes([e])
    nu, nfp, nf, nd, ne = 10, 12, 4, 2, 32
    assert by[0] == 0.0 and not any(by[4:])
    assert by[1] == ne * (8.0 * (nu * nf + nu * nd * nd + nu * nf + nfp * nf) + 8.0 * (2 * nfp * nf + nu + nfp * (nd * nd + 1) + nfp * nd + nfp * nf) + 4.0 * nfp)
    assert by[3] == ne * 8.0 * (3 * nu * nf + nu + 2 * nfp * nf + 3 * nu * nf + nfp * nf)
    assert np.isfinite(e.download(hfx.DISU_UPTS0)).all()
    close(e, faces)
