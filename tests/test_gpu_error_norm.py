"""Exact-solution error norms on the device (hfx_eles_compute_error; eles::compute_error, src/eles.cpp:5076-5277) against the
yardstick of tests/error_norm_util.py: a numpy restatement in np.longdouble applied to exactly the arrays the device gets, at
the derived bar stated there (1e-12 of ||exact|| + ||interpolated||, in the norm asked for, both rows)."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
from error_norm_util import assert_at_the_bar, gauss_tensor_rule, yardstick
from test_gpu_methods_vs_golden import GOLDEN, build

pytestmark = pytest.mark.gpu

INTEGRALS = ["hex_p2_integrals", "quad_p3_integrals", "tet_p2_integrals", "pri_p2_integrals"]
TIME = 0.37
STALE = "was not materialised by the fused stage that ran last"


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def scalar(d, k):
    return float(np.ravel(d[k])[0])


def couette_of(d):
    """made-up walls, the fixture's bound pressure and gas constant (an inviscid fixture records no R_ref (NaN), which makes the exact
    solution NaN on both sides: it takes the two from the viscous fixture whose cubature it borrows)"""
    src = d if np.isfinite(scalar(d, "R_ref")) else load("tet_p2_integrals")
    return dict(u_wall=0.3, T_wall=1.1, p_bound=scalar(src, "p_c_ic"), R_ref=scalar(src, "R_ref"), T_ref=2.0)


def positions(d, cub=None):
    """opp_volume_cubpts @ pos_upts: any positions serve, device and yardstick get the same array"""
    opp = (cub or d)["opp_volume_cubpts"]
    return np.asfortranarray(np.einsum("jk,kid->jid", opp, d["pos_upts"]))


def register(e, d, cub=None):
    c = cub or d
    e.set_volume_cubpts(c["opp_volume_cubpts"], c["weight_volume_cubpts"], c["vol_detjac_vol_cubpts"])
    pos = positions(d, cub)
    e.set_error_points(pos)
    return pos


def want_of(d, pos, u, grad, test_case, norm, time=TIME, cub=None, viscous=None):
    c = cub or d
    return yardstick(c["opp_volume_cubpts"], c["weight_volume_cubpts"], c["vol_detjac_vol_cubpts"], pos, u, grad, test_case, norm,
                     time, scalar(d, "gamma"), viscous=int(scalar(d, "viscous")) if viscous is None else viscous,
                     couette=couette_of(d), prandtl=scalar(d, "prandtl"))


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


@pytest.mark.parametrize("name", INTEGRALS)
def test_vortex_error_on_every_element_class(ctx, name):
    """test case 1 in both norms at the bar; the gradient row is exactly zero"""
    d = load(name)
    e, faces = build(ctx, d)
    pos = register(e, d)
    ctx.set_exact_solution(1)
    for norm in (1, 2):
        got = e.compute_error(norm, TIME)
        want, scale = want_of(d, pos, d["u_init"], None, 1, norm)
        assert_at_the_bar(got[:1], want[:1], scale[:1], norm, name + " vortex")
        assert np.any(got[0] > 0)
        assert np.all(got[1] == 0.0)
    close(e, faces)


@pytest.mark.parametrize("name,cub", [(n, None) for n in INTEGRALS] + [("tet_p2_inviscid", "tet_p2_integrals")])
def test_couette_error_with_a_current_gradient(ctx, name, cub):
    """test case 5 after CalcResidual, both norms, both rows; an inviscid context gives a zero gradient row"""
    d = load(name)
    cub = load(cub) if cub else None
    viscous = int(scalar(d, "viscous"))
    assert viscous == (0 if cub else 1)
    e, faces = build(ctx, d)
    pos = register(e, d, cub)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS) if viscous else None
    ctx.set_exact_solution(5, **couette_of(d))
    for norm in (1, 2):
        got = e.compute_error(norm, TIME)
        want, scale = want_of(d, pos, d["u_init"], grad, 5, norm, cub=cub)
        assert_at_the_bar(got, want, scale, norm, name + " couette")
        assert np.any(got[0] > 0)
        if viscous:
            assert np.any(got[1] > 0)
        else:
            assert np.all(got[1] == 0.0)
    close(e, faces)


ELE_AXIS = {"detjac_upts": 1, "JGinv_upts": 3, "detjac_fpts": 1, "JGinv_fpts": 3, "tdA_fpts": 1, "norm_fpts": 1, "pos_upts": 1,
            "vol_detjac_vol_cubpts": 1}


@pytest.mark.parametrize("name", ["pri_p2_integrals", "hex_p2_integrals"])
def test_past_the_first_pass(ctx, name):
    """every workgroup walks at least three passes of its grid-stride loop: the elements are tiled until
    n_eles >= 3 n_groups eles_per_pass as hfx_eles_error_launch reports them, every copy with its own state (and a gradient
    of its own, uploaded).  The grid is held to 5 workgroups (option persistent_grid_cap, as the tests of the other persistent
    loops do), so that the tiled arrays stay small: the loop is the same whatever the grid.  Two calls are bit-equal."""
    d = load(name)
    ctx.set_option("persistent_grid_cap", 5)
    sz = [int(v) for v in d["sizes"]]
    e0, faces0 = build(ctx, d)
    register(e0, d)
    n_groups, epp = e0.error_launch()
    close(e0, faces0)
    assert n_groups == min(5, -(-sz[0] // epp))
    copies = -(-3 * 5 * epp // sz[0]) + 1
    t = dict(d)
    for k, ax in ELE_AXIS.items():
        t[k] = np.concatenate([d[k]] * copies, axis=ax)
    rng = np.random.default_rng(20260119)
    factor = rng.uniform(0.9, 1.1, copies)
    t["u_init"] = np.concatenate([d["u_init"] * f for f in factor], axis=1)
    sizes = np.array(d["sizes"]).copy()
    sizes[0] = sz[0] * copies
    t["sizes"] = sizes
    for k in [k for k in t if k.startswith("int") or k.startswith("bdy")]:
        del t[k]  # (no faces: nothing here runs a residual)
    e, faces = build(ctx, t)
    pos = register(e, t)
    n_groups, epp2 = e.error_launch()
    assert (n_groups, epp2) == (5, epp) and e.n_eles >= 3 * n_groups * epp
    grad = np.asfortranarray(rng.uniform(-1.0, 1.0, (e.n_upts, e.n_eles, e.n_fields, e.n_dims)))
    e.upload(hfx.GRAD_DISU_UPTS, grad)
    for tc in (1, 5):
        ctx.set_exact_solution(tc, **couette_of(d))
        for norm in (1, 2):
            got = e.compute_error(norm, TIME)
            again = e.compute_error(norm, TIME)
            assert np.array_equal(got, again)
            want, scale = want_of(t, pos, t["u_init"], grad, tc, norm)
            assert_at_the_bar(got, want, scale, norm, "%s tiled x%d, test case %d" % (name, copies, tc))
    close(e, faces)


def test_cubature_that_is_neither_the_solution_points_nor_whole_waves(ctx):
    """quad_p3_integrals with a hand-built 5 x 5 Gauss rule (25 points: not n_upts = 16, not a multiple of 64): the operator
    from the Lagrange basis on the fixture's solution points, the determinant from the derivatives of the interpolated
    positions, both by numpy"""
    d = load("quad_p3_integrals")
    loc, wt = gauss_tensor_rule(5, 2)
    P = np.polynomial.legendre

    def vander(r, s, dr=0, ds=0):
        cols = []
        for a in range(4):
            for b in range(4):
                ca, cb = np.eye(4)[a], np.eye(4)[b]
                cols.append(P.legval(r, P.legder(ca, dr) if dr else ca) * P.legval(s, P.legder(cb, ds) if ds else cb))
        return np.array(cols).T
    Vinv = np.linalg.inv(vander(d["loc_upts"][0], d["loc_upts"][1]))
    opp = vander(loc[0], loc[1]) @ Vinv
    Dr, Ds = vander(loc[0], loc[1], dr=1) @ Vinv, vander(loc[0], loc[1], ds=1) @ Vinv
    x, y = d["pos_upts"][:, :, 0], d["pos_upts"][:, :, 1]
    detjac = (Dr @ x) * (Ds @ y) - (Ds @ x) * (Dr @ y)
    assert opp.shape == (25, 16) and np.abs(opp.sum(axis=1) - 1).max() < 1e-12 and np.all(detjac > 0)
    cub = dict(opp_volume_cubpts=np.asfortranarray(opp), weight_volume_cubpts=wt, vol_detjac_vol_cubpts=np.asfortranarray(detjac))
    e, faces = build(ctx, d)
    pos = register(e, d, cub)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    for tc in (1, 5):
        ctx.set_exact_solution(tc, **couette_of(d))
        for norm in (1, 2):
            got = e.compute_error(norm, TIME)
            want, scale = want_of(d, pos, d["u_init"], grad, tc, norm, cub=cub)
            assert_at_the_bar(got, want, scale, norm, "quad_p3 5x5, test case %d" % tc)
    close(e, faces)


def test_after_the_split_fused_stage(ctx):
    """two steps of the split fused stage (mode 3) leave no gradient: the vortex error is computed from the new state, the
    Couette error is refused with the words of hfx_eles_download, and computed again once a per-method residual has run"""
    d = load("hex_p2_integrals")
    e, faces = build(ctx, d)
    pos = register(e, d)
    hfx.run_steps(e, faces, 2, fused=3)
    u = e.download(hfx.DISU_UPTS0)
    assert np.abs(u - d["u_init"]).max() > 0
    ctx.set_exact_solution(1)
    got = e.compute_error(2, TIME)
    want, scale = want_of(d, pos, u, None, 1, 2)
    assert_at_the_bar(got, want, scale, 2, "after fused 3")
    ctx.set_exact_solution(5, **couette_of(d))
    with pytest.raises(hfx.HfxError, match=STALE):
        e.compute_error(2, TIME)
    with pytest.raises(hfx.HfxError, match=STALE):
        e.download(hfx.GRAD_DISU_UPTS)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    got = e.compute_error(2, TIME)
    want, scale = want_of(d, pos, u, grad, 5, 2)
    assert_at_the_bar(got, want, scale, 2, "after fused 3 and CalcResidual")
    close(e, faces)


def test_with_a_deferred_stage_pending(ctx):
    """deferred execution: with a whole stage recorded and not yet run, the vortex error equals -- bit for bit -- the one
    computed after an explicit hfx_ctx_flush, and the stage has run fused (the monitor asks for no gradient)"""
    from test_gpu_deferred import calc_residual_calls, tag
    d = load("hex_p2_integrals")
    ctx.set_option("deferred", 1)
    adv = int(scalar(d, "adv_type"))
    out = []
    for flush in (False, True):
        e, faces = build(ctx, d)
        tag(e, d)
        register(e, d)
        ctx.set_exact_solution(1)
        calc_residual_calls([e], faces, True, 0)
        e.AdvanceSolution(0, adv)
        if flush:
            ctx.flush()
        out.append(e.compute_error(2, TIME))
        close(e, faces)
    nf, nr, why = ctx.deferred_stats()
    assert (nf, nr) == (2, 0), why
    assert np.any(out[0][0] > 0) and np.array_equal(out[0], out[1])


def test_refusals(ctx):
    """every refusal comes with its message, through hfx_last_error, and before anything is launched: the error array the
    caller passed is untouched"""
    d = load("quad_p3_integrals")
    e, faces = build(ctx, d)
    lib = hfx.lib()
    out = np.full((2, e.n_fields), -7.0, order="F")

    def refused(norm, pattern):
        rc = lib.hfx_eles_compute_error(e.h, C.c_int(norm), C.c_double(TIME), out.ctypes.data_as(hfx.dp))
        msg = lib.hfx_last_error().decode()
        assert rc != 0 and pattern in msg, (rc, msg)
        assert np.all(out == -7.0)

    refused(2, "hfx_ctx_set_exact_solution")            # no parameters of the exact solution
    ctx.set_exact_solution(1)
    refused(2, "hfx_eles_set_volume_cubpts")            # no cubature
    with pytest.raises(hfx.HfxError, match="hfx_eles_set_volume_cubpts"):
        e.set_error_points(positions(d))
    with pytest.raises(hfx.HfxError, match="hfx_eles_set_volume_cubpts"):
        e.error_launch()
    e.set_volume_cubpts(d["opp_volume_cubpts"], d["weight_volume_cubpts"], d["vol_detjac_vol_cubpts"])
    refused(2, "hfx_eles_set_error_points")             # no positions
    e.set_error_points(positions(d))
    for norm in (0, 3):
        refused(norm, "Error norm not supported!")
    for tc in (2, 3, 4):
        ctx.set_exact_solution(tc)
        refused(2, "advection-diffusion")
    for tc in (0, 9):
        ctx.set_exact_solution(tc)
        refused(2, "Test case not recognized in compute error, exiting")
    ctx.set_exact_solution(1)
    assert np.any(e.compute_error(2, TIME)[0] > 0)      # (and the block is as usable as before)
    # another cubature asks for its own positions
    e.set_volume_cubpts(d["opp_volume_cubpts"][:9], d["weight_volume_cubpts"][:9], d["vol_detjac_vol_cubpts"][:9])
    refused(2, "hfx_eles_set_error_points")
    close(e, faces)


def test_default_grid_past_the_first_pass(ctx):
    """the grid as it is chosen without a cap (four workgroups per CU): hex_p2_integrals tiled until every one of them walks
    three passes, so that the partials buffer sized from the grid -- ten quantities of a thousand workgroups, far beyond the
    block's 1024-double reduction buffer -- is written and summed.  Test case 1, norm 2, against the yardstick; two calls
    bit-equal"""
    d = load("hex_p2_integrals")
    n0 = int(d["sizes"][0])
    rng = np.random.default_rng(20260120)
    copies = 1100
    for attempt in range(2):
        t = dict(d)
        for k, ax in ELE_AXIS.items():
            t[k] = np.concatenate([d[k]] * copies, axis=ax)
        t["u_init"] = np.concatenate([d["u_init"] * f for f in rng.uniform(0.9, 1.1, copies)], axis=1)
        sizes = np.array(d["sizes"]).copy()
        sizes[0] = n0 * copies
        t["sizes"] = sizes
        for k in [k for k in t if k.startswith("int") or k.startswith("bdy")]:
            del t[k]
        e, faces = build(ctx, t)
        pos = register(e, t)
        n_groups, epp = e.error_launch()
        if e.n_eles >= 3 * n_groups * epp:
            break
        close(e, faces)  # (a device with more CUs than the guess was made for)
        copies = -(-3 * n_groups * epp // n0) + 1
    assert e.n_eles >= 3 * n_groups * epp and 2 * e.n_fields * n_groups > 1024
    ctx.set_exact_solution(1)
    got = e.compute_error(2, TIME)
    assert np.array_equal(got, e.compute_error(2, TIME))
    want, scale = want_of(t, pos, t["u_init"], None, 1, 2)
    assert_at_the_bar(got, want, scale, 2, "hex_p2 tiled x%d, %d workgroups" % (copies, n_groups))
    close(e, faces)


def test_after_the_general_fused_stage(ctx):
    """tetrahedra after one step of the general fused stage (hfx_run_steps_blocks(..., 4)), which keeps the corrected gradient on
    chip as split variant 3 does: the vortex error is computed from the new state, the Couette error and a download of the
    gradient are refused as stale, and a per-method residual makes both work again"""
    d = load("tet_p2_integrals")
    e, faces = build(ctx, d)
    pos = register(e, d)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    u = e.download(hfx.DISU_UPTS0)
    assert np.abs(u - d["u_init"]).max() > 0
    ctx.set_exact_solution(1)
    got = e.compute_error(2, TIME)
    want, scale = want_of(d, pos, u, None, 1, 2)
    assert_at_the_bar(got, want, scale, 2, "tetrahedra after fused 4")
    ctx.set_exact_solution(5, **couette_of(d))
    with pytest.raises(hfx.HfxError, match=STALE):
        e.compute_error(2, TIME)
    for arr in (hfx.GRAD_DISU_UPTS, hfx.GRAD_DISU_FPTS):
        with pytest.raises(hfx.HfxError, match=STALE):
            e.download(arr)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    got = e.compute_error(2, TIME)
    want, scale = want_of(d, pos, u, grad, 5, 2)
    assert_at_the_bar(got, want, scale, 2, "tetrahedra after fused 4 and CalcResidual")
    close(e, faces)


# ---- through the host mirror: the isentropic vortex on the periodic box [-5, 5]^2, inviscid, Rusanov, P3 quadrilaterals ----
def vortex_case(n, upts_type, dt=0.001):
    import hfx_host as H
    x = np.linspace(-5.0, 5.0, n + 1)
    X, Y = np.meshgrid(x, x, indexing="ij")  # vertex v = ix + (n + 1) iy
    xv = np.stack([X.ravel(order="F"), Y.ravel(order="F")], axis=1)
    c = H.Case([n, n, 1], xv=xv, dims=2, order=3, length=10.0, viscous=0, ic_form=0, riemann_solve_type=0, upts_type=upts_type,
               dt=dt, rho_c_ic=1.0, u_c_ic=1.0, v_c_ic=1.0, p_c_ic=1.0)
    c.set_test_case(1, 2)
    return c


@pytest.fixture(scope="module")
def vortex_errors():
    """the L2 errors (4 fields) the mirror reports, computed once: at t = 0 on Gauss points (n 16) and on Lobatto points (n 16,
    32), and after t = 0.05 on Gauss points (n 16: 50 steps of 0.001; n 32: 100 steps of 0.0005) with what the yardstick needs"""
    out = {}
    for key, n, upts, dt, steps in (("gauss16", 16, 0, 0.001, 0), ("lobatto16", 16, 1, 0.001, 0), ("lobatto32", 32, 1, 0.001, 0),
                                    ("run16", 16, 0, 0.001, 50), ("run32", 32, 0, 0.0005, 100)):
        c = vortex_case(n, upts, dt)
        c.to_device()
        if steps:
            c.run(steps)
        rec = dict(error=c.compute_error(), time=c.clock()[0])
        if key == "run16":
            c.sync_host()
            rec.update({k: c.array(k) for k in ("opp_volume_cubpts", "weight_volume_cubpts", "vol_detjac_vol_cubpts",
                                                 "pos_volume_cubpts", "disu_upts0")})
        c.close()
        out[key] = rec
    return out


def test_mirror_initial_state_on_gauss_points_has_rounding_error_only(vortex_errors):
    """(a) the cubature points are the solution points and the state there is the exact solution: every field's L2 error is
    rounding, <= 1e-11 (the discretisation errors of (b) are >= 1e-5); the gradient row of an inviscid case is zero"""
    e = vortex_errors["gauss16"]["error"]
    print("L2 error at t = 0, Gauss points:", e[0])
    assert np.all(e[0] <= 1e-11) and np.all(e[1] == 0.0)


def test_mirror_order_of_accuracy_of_the_interpolation(vortex_errors):
    """(b) Lobatto solution points, t = 0: the error of interpolating the initial state to the Gauss cubature points falls with
    the design order p + 1 = 4: log2(e16 / e32) > 3.5 in every field (the reference's formulas give 3.99-4.03 on this setup)"""
    e16, e32 = vortex_errors["lobatto16"]["error"][0], vortex_errors["lobatto32"]["error"][0]
    rate = np.log2(e16 / e32)
    print("e16", e16, "e32", e32, "observed order", rate)
    assert np.all(e16 >= 1e-5) and np.all(rate > 3.5)


def test_mirror_error_after_a_run(vortex_errors):
    """(c) 50 steps: hfxh_case_compute_error equals the yardstick on the downloaded state at the mirror's clock, at the bar;
    the finer mesh, run to the same time with half the step, has the smaller error in every field (the observed order is
    printed, not asserted)"""
    r = vortex_errors["run16"]
    assert abs(r["time"] - 0.05) < 1e-12 and abs(vortex_errors["run32"]["time"] - 0.05) < 1e-12
    want, scale = yardstick(r["opp_volume_cubpts"], r["weight_volume_cubpts"], r["vol_detjac_vol_cubpts"], r["pos_volume_cubpts"],
                            r["disu_upts0"], None, 1, 2, r["time"], 1.4)
    got = r["error"]
    assert_at_the_bar(got ** 2, want, scale, 2, "mirror, 50 steps")
    e16, e32 = got[0], vortex_errors["run32"]["error"][0]
    print("t = 0.05: e16", e16, "e32", e32, "observed order", np.log2(e16 / e32))
    assert np.all(e32 < e16)


def test_mirror_sums_over_ranks_once_before_the_square_root():
    """the hook of hfxh_case_set_reduce_sum is called once, with 2 n_fields values, and the square root is taken of what it
    returns: with a hook that adds a fixed vector the mirror's norms are sqrt(the block's sums + that vector), bit for bit"""
    c = vortex_case(16, 1)
    c.to_device()
    add = np.array([[1.0, 0.5], [2.0, 0.25], [3.0, 0.125], [4.0, 0.0625]]).T  # (2, n_fields)
    calls = []

    def hook(v):
        calls.append(list(v))
        return [a + b for a, b in zip(v, add.ravel(order="F"))]
    c.set_reduce_sum(hook)
    got = c.compute_error()
    ctx, e, f, nb = c.handles()
    raw = np.zeros((2, 4), order="F")
    hfx.check(hfx.lib().hfx_eles_compute_error(e, C.c_int(2), C.c_double(c.clock()[0]), raw.ctypes.data_as(hfx.dp)))
    assert len(calls) == 1 and len(calls[0]) == 8
    assert np.array_equal(np.array(calls[0]).reshape((2, 4), order="F"), raw)
    assert np.array_equal(got[0], np.sqrt(raw[0] + add[0]))
    assert np.array_equal(got[1], add[1])  # (inviscid: the reference neither sums nor roots the gradient row)
    c.close()


def test_mirror_integral_quantities_equal_the_device_call():
    """hfxh_case_CalcIntegralQuantities on one block and one rank is hfx_eles_CalcIntegralQuantities, bit for bit"""
    import hfx_host as H
    names = ["kineticenergy", "enstropy", "pressuredilatation", "straincolonproduct", "devstraincolonproduct"]
    c = H.Case(3, order=2, amp=0.1)
    c.set_integral_quantities(names)
    c.to_device()
    c.CalcResidual()
    got = c.CalcIntegralQuantities()
    ctx, e, f, nb = c.handles()
    ids = np.arange(5, dtype=np.int32)
    want = np.zeros(5)
    hfx.check(hfx.lib().hfx_eles_CalcIntegralQuantities(e, C.c_int(5), ids.ctypes.data_as(hfx.ip), want.ctypes.data_as(hfx.dp)))
    assert np.all(np.isfinite(got)) and got[0] > 0 and np.array_equal(got, want)
    c.close()
