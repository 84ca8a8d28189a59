"""The whole chain -- host-side mirror (setup in C++, mirrored CalcResidual / RK loop) driving
libhfx -- against the genuine reference's fixtures, against the oracle at a mid size, and through
size-independent properties at BASELINE.json's full size (32^3 hexa, P4).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import oracle_py as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def fixture_case(name, ref_nodes=False):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    k = json.loads(bytes(d["meta_json"]).decode())
    kk = k["keys"]
    x1 = d["loc_upts"][0, :kk["order"] + 1] if ref_nodes else None
    c = H.Case(k["n"], xv=d["xv"], loc_1d_upts=x1, order=kk["order"], adv_type=kk["adv_type"],
               riemann_solve_type=kk["riemann_solve_type"], upts_type=kk["upts_type_hexa"],
               vcjh_scheme=kk["vcjh_scheme_hexa"], fix_vis=kk["fix_vis"], T_c_ic=kk["T_c_ic"])
    return c, d


@pytest.mark.parametrize("name,ref_nodes", [("hex_p4_n3_deformed", False), ("hex_p2_lobatto", False), ("hex_p2_sd", False),
                                            ("hex_p2_n3_uniform", True)])
def test_mirrored_rk_loop_vs_reference(name, ref_nodes):
    """On the axis-aligned mesh the face normals carry ~4e-17 rounding noise in the components that are
    geometrically zero, and the reference's LDG switch (exact sign tests on the left normal,
    src/inters.cpp:568-581) is decided by that noise; it is only reproducible with bit-identical metrics,
    i.e. with the reference's own (not bit-symmetric) quadrature-table abscissae -- passed in here.
    With the computed, symmetric nodes the result differs by ~6e-9 (a different but equally valid
    one-sided LDG choice on those faces); test_uniform_mesh_vs_oracle covers that configuration."""
    c, d = fixture_case(name, ref_nodes)
    c.to_device(0)
    c.run(1)  # mirrored classes: CalcResidual + AdvanceSolution per stage
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step0_stage%d" % last]) < 1e-11
    c.close()


@pytest.mark.parametrize("mode", ["methods", 2, 3])
def test_forty_steps_vs_reference(mode):
    """200 RK stages of the genuine reference (hex_p2_long: the state after steps 10, 20, 30, 40): the mirrored loop and
    the split fused paths stay on the reference's trajectory -- rounding differences between the paths do not grow."""
    c, d = fixture_case("hex_p2_long")
    c.to_device(0)
    for last in (9, 19, 29, 39):
        if mode == "methods":
            c.run(10)
        else:
            c.run_steps_lib(10, fused=mode)
        c.sync_host()
        assert rel(c.array("disu_upts0"), d["u_step%d_stage4" % last]) < 1e-11, last
    c.close()


@pytest.mark.parametrize("name", ["hex_p3_plot", "quad_p2_plot"])
def test_plot_point_interpolation(name):
    """eles::calc_disu_ppts on the device (one contraction for all elements): through the C ABI with the reference's
    opp_p, and through the host mirror that builds the plot points and the operator itself."""
    import hfx
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = json.loads(bytes(d["meta_json"]).decode())
    kk = meta["keys"]
    n = meta["n"] if isinstance(meta["n"], list) else [meta["n"]] * meta["dims"]
    c = H.Case(n + [1] * (3 - len(n)), xv=d["xv"], dims=meta["dims"], order=kk["order"], p_res=kk["p_res"], T_c_ic=kk["T_c_ic"])
    c.to_device(0)
    assert rel(c.calc_disu_ppts(), d["disu_ppts"]) < 1e-13
    # the C ABI with the reference's operator on the same device block
    ctx, e, faces, nb = c.handles()
    opp = np.asfortranarray(d["opp_p"])
    hfx.check(hfx.lib().hfx_eles_set_opp_p(e, C.c_int(opp.shape[0]), opp.ctypes.data_as(hfx.dp)))
    out = np.zeros(d["disu_ppts"].shape, order="F")
    hfx.check(hfx.lib().hfx_eles_calc_disu_ppts(e, out.ctypes.data_as(hfx.dp)))
    assert rel(out, d["disu_ppts"]) < 1e-13
    c.close()


@pytest.mark.parametrize("mode", ["methods", "calls", 2, 3])
@pytest.mark.parametrize("name,dims", [("hex_p2_les_wale", 3), ("quad_p3_les_wale", 2)])
def test_les_wale_through_the_mirror(name, dims, mode):
    """LES (WALE closure) from the mesh and the input keys: the mirrored CalcResidual (evaluate_viscFlux +
    extrapolate_sgsFlux) and the split fused path (fused=2) against the genuine reference's state after a step."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = json.loads(bytes(d["meta_json"]).decode())
    k = meta["keys"]
    n = meta["n"] if isinstance(meta["n"], list) else [meta["n"]] * dims
    c = H.Case(n + [1] * (3 - len(n)), xv=d["xv"], dims=dims, order=k["order"], LES=1, SGS_model=k["SGS_model"], C_s=k["C_s"],
               filter_ratio=k["filter_ratio"], T_c_ic=k["T_c_ic"])
    if mode == "calls":
        c.set_deferred(False)  # every mirrored call launches its own kernels: the per-method path
    c.to_device(0)
    if mode in ("methods", "calls"):
        c.run(1)  # "methods": deferred, i.e. the split stage with the closure in the flux kernel (variant 3)
    else:
        c.run_steps_lib(1, fused=mode)  # 2: the closure as a pointwise kernel on the gradient array; 3: in the flux kernel
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step0_stage%d" % last]) < 1e-11
    c.close()


@pytest.mark.parametrize("mode", ["methods", "calls", 2, 3])
@pytest.mark.parametrize("name", ["hex_p2_les_wsm", "hex_p2_les_sim", "hex_p2_les_svv"])
def test_les_filtered_closures_through_the_mirror(name, mode):
    """SGS_model 2 / 4 / 3 from the mesh and the input keys: the mirror builds filter_upts (compute_filter_upts),
    CalcResidual calls calc_sgs_terms at the first stage of every step; two steps against the reference's states."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = json.loads(bytes(d["meta_json"]).decode())
    k = meta["keys"]
    n = meta["n"] if isinstance(meta["n"], list) else [meta["n"]] * 3
    c = H.Case(n, xv=d["xv"], dims=3, order=k["order"], LES=1, SGS_model=k["SGS_model"], C_s=k["C_s"],
               filter_ratio=k["filter_ratio"], filter_type=k["filter_type"], T_c_ic=k["T_c_ic"])
    assert rel(c.array("filter_upts"), d["filter_upts"]) < 1e-12
    if mode == "calls":
        c.set_deferred(False)
    c.to_device(0)
    if mode in ("methods", "calls"):
        c.run(2)
    else:
        c.run_steps_lib(2, fused=mode)
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step1_stage%d" % last]) < 1e-11
    c.close()


def test_uniform_mesh_vs_oracle(oracle):
    """Computed nodes on the axis-aligned fixture mesh: GPU and oracle see the same registration data."""
    c, d = fixture_case("hex_p2_n3_uniform")
    reg = c.registration()
    c.to_device(0)
    c.run(2)
    c.sync_host()
    oc = O.Case(reg)
    e = oc.c_eles()
    f, nb = oc.c_faces()
    for _ in range(2):
        assert oracle.orc_rk_step(C.byref(e), f, nb, C.byref(oc.params)) == -1
    assert rel(c.array("disu_upts0"), oc.arr["u0"]) < 1e-11
    # and the reference itself is within the switch-noise distance
    assert rel(c.array("disu_upts0"), d["u_step1_stage4"]) < 1e-7
    c.close()


def test_mirrored_residual_vs_reference():
    c, d = fixture_case("hex_p4_n3_deformed")
    c.to_device(0)
    c.CalcResidual()
    c.sync_host()
    assert rel(c.array("div_tconf_upts"), d["s0_div_tconf_upts"]) < 5e-11
    c.close()


def test_mid_size_vs_oracle(oracle):
    c = H.Case(6, order=4, amp=0.1)
    reg = c.registration()
    c.to_device(0)
    c.run_steps_lib(1)
    c.sync_host()
    oc = O.Case(reg)
    e = oc.c_eles()
    f, nb = oc.c_faces()
    oracle.orc_set_threads(8)
    assert oracle.orc_rk_step(C.byref(e), f, nb, C.byref(oc.params)) == -1
    oracle.orc_set_threads(1)
    assert rel(c.array("disu_upts0"), oc.arr["u0"]) < 1e-11
    c.close()


def gauss_weights(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return w


def integrals(c, u):
    """sum over elements of the Gauss quadrature of each conserved field: int u dV."""
    N = c.order + 1
    w1 = gauss_weights(N)
    w = (w1[:, None, None] * w1[None, :, None] * w1[None, None, :]).ravel()  # upt = k + N j + N^2 i
    dj = c.array("detjac_upts")
    return np.einsum("p,pe,pef->f", w, dj, u)


@pytest.mark.parametrize("fused", [False])
def test_full_size_conservation_and_symmetry(fused):
    """BASELINE.json configs[1]: TGV 32^3 hexa P4.  Flux reconstruction is conservative: on a periodic
    box the integral of every conserved variable is constant in time (up to rounding); and the common
    flux seen from the two sides of a face cancels exactly, so this exercises every face table entry."""
    c = H.Case(32, order=4)
    u0 = c.array("disu_upts0")
    i0 = integrals(c, u0)
    c.to_device(0)
    c.run_steps_lib(2, fused=fused)
    c.sync_host()
    u = c.array("disu_upts0")
    assert np.isfinite(u).all()
    i1 = integrals(c, u)
    vol = (2 * np.pi) ** 3
    # mass, momentum, energy: drift relative to (volume * typical magnitude of the field)
    scale = np.array([1.0, 1.0, 1.0, 1.0, u0[:, :, 4].max()]) * vol
    assert np.all(np.abs(i1 - i0) / scale < 1e-12), (i1 - i0) / scale
    # the state did move
    assert rel(u, u0) > 1e-6
    # z-momentum of the TGV stays antisymmetric about the mid-plane: its integral stays ~0
    assert abs(i1[3]) / vol < 1e-12
    c.close()


def test_full_size_residual_norms_vs_reference_stdout():
    """BASELINE.json configs[1] at FULL size against the genuine reference's own output: BASELINE.md
    section 2 records the iteration-1 row the reference printed for the generated periodic 32^3 P4 TGV
    case (L1 residual per field, 8 digits): 0.00070019 0.05031596 0.05031596 0.06433493 0.11799063.
    The monitor (src/output.cpp:2166-2248) evaluates sum|div_tconf/detjac| / n_upts on the divergence
    left by the LAST stage of the step, so: one full time step, then the norms."""
    c = H.Case(32, order=4)
    c.to_device(0)
    c.run_steps_lib(1)
    ctx, e, f, nb = c.handles()
    v = C.c_double()
    r = []
    for fld in range(5):
        hfx.check(hfx.lib().hfx_eles_compute_res_upts(e, 1, fld, C.byref(v)))
        r.append(v.value / (c.n_eles * c.n_upts))
    c.close()
    want = np.array([0.00070019, 0.05031596, 0.05031596, 0.06433493, 0.11799063])
    assert np.all(np.abs(np.array(r) - want) < 6e-9), r


@pytest.mark.parametrize("mode", ["methods", 2, 3])
@pytest.mark.parametrize("name", ["hex_p2_bdy_walls", "hex_p2_bdy_inout", "hex_p1_bdy_inviscid", "quad_p3_bdy", "quad_p3_bdy_inout",
                                  "hex_p2_bdy_dual", "quad_p3_ramp_clamp", "quad_p3_ramp_zero"])
def test_boundary_case_through_the_mirror(name, mode):
    """Boundary faces end to end: host-mirror setup (mesh sides -> bdy_inters, bc_list non-dimensionalisation)
    + the mirrored CalcResidual / the split fused paths, against the genuine reference's state after a step."""
    import bdy_util
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    c, meta = bdy_util.case_from_fixture(d)
    c.to_device(0)
    if mode == "methods":
        c.run(1)
    else:
        c.run_steps_lib(1, fused=mode)
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step0_stage%d" % last]) < 1e-11
    c.close()


@pytest.mark.parametrize("mode", ["methods", 3])
def test_les_smagorinsky_between_walls_through_the_mirror(mode):
    """The damped Smagorinsky closure from the mesh and the input keys alone: the host mirror collects the flux points of the
    no-slip wall faces and computes eles::calc_wall_distance (src/eles.cpp:2701-2810, src/geometry.cpp:735-892); the state after
    the fixture's step equals the genuine reference's, call by call and with the closure inside the split flux kernel"""
    import bdy_util
    d = dict(np.load(os.path.join(GOLDEN, "hex_p2_les_smag.npz")))
    k = bdy_util.json.loads(bytes(d["meta_json"]).decode())["keys"]
    c, meta = bdy_util.case_from_fixture(d, LES=1, SGS_model=0, C_s=k["C_s"], filter_ratio=k["filter_ratio"])
    # the wall distance itself: its length everywhere, the vector up to the choice between two equally near wall points (the
    # points half way between the walls: the reference keeps the first it meets in ITS face order) -- only the length is used
    w, want = c.array("wall_distance"), d["wall_distance"]
    assert w.shape == want.shape
    assert np.abs(np.sqrt((w ** 2).sum(axis=2)) - np.sqrt((want ** 2).sum(axis=2))).max() < 1e-13
    assert np.abs(np.abs(w) - np.abs(want)).max() < 1e-12
    assert (np.abs(w - want).max(axis=2) < 1e-12).mean() > 0.8
    c.to_device(0)
    if mode == "methods":
        c.run(1)
    else:
        c.run_steps_lib(1, fused=mode)
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step0_stage%d" % last]) < 1e-11
    c.close()


@pytest.mark.parametrize("mode", ["methods", 3])
@pytest.mark.parametrize("name", ["hex_p4_jet", "hex_p2_overint", "quad_p3_overint", "hex_p3_shock", "hex_p2_shock_energy",
                                  "quad_p3_shock"])
def test_dealiasing_and_shock_capturing_through_the_mirror(name, mode):
    """BASELINE.json configs[4] in small (hex_p4_jet) and the over-integration / shock-capturing fixtures from
    nothing but the mesh and the input keys: the host mirror builds the modal operators (csrc/host/eles_modal.cpp),
    the mirrored RK loop (evaluate_invFlux_over_int in CalcResidual, shock_capture after AdvanceSolution) or the split
    fused path runs them, and the state equals the genuine reference's after every step of the fixture."""
    import bdy_util
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    # hex_p4_jet: two cells per direction with planar box sides put the middle flux point of every face (P4: the 1-D
    # node 0) where a normal component is geometrically zero; the reference's LDG switch is then decided by the
    # rounding noise of its quadrature table (see test_mirrored_rk_loop_vs_reference), so its nodes are passed in
    over = {"loc_1d_upts": d["loc_upts"][0, :int(d["sizes"][5]) + 1]} if name == "hex_p4_jet" else {}
    c, meta = bdy_util.case_from_fixture(d, **over)
    c.to_device(0)
    last = int(d["sizes"][7]) - 1
    for st in range(meta["steps"]):
        if mode == "methods":
            c.run(1)
        else:
            c.run_steps_lib(1, fused=mode)
        c.sync_host()
        assert rel(c.array("disu_upts0"), d["u_step%d_stage%d" % (st, last)]) < 1e-11, st
    c.close()


@pytest.mark.parametrize("name,dt_type", [("hex_p2_cfl_global", 1), ("hex_p2_cfl_local", 2)])
def test_cfl_time_stepping_through_the_mirror(name, dt_type):
    """calc_time_step on the device inside the mirrored RK loop (dt_type 1: global minimum, 2: local steps)."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    k = json.loads(bytes(d["meta_json"]).decode())["keys"]
    c = H.Case(3, xv=d["xv"], order=2, dt_type=dt_type, CFL=k["CFL"], adv_type=k["adv_type"], dt=0.0)
    c.to_device(0)
    dt = c.calc_time_step()
    assert abs(dt - float(np.ravel(d["dt_step0"])[0])) < 1e-11 * dt
    c.run(2)
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step1_stage%d" % last]) < 1e-11
    c.close()


@pytest.mark.parametrize("mode", ["methods", 3])
def test_isentropic_vortex_through_the_mirror(mode):
    """BASELINE.json configs[0] (reduced mesh): inviscid vortex on quads, Rusanov, RK45, through the mirror."""
    d = dict(np.load(os.path.join(GOLDEN, "quad_p3_vortex.npz")))
    c = H.Case([6, 6, 1], xv=d["xv"], dims=2, order=3, viscous=0, ic_form=0, riemann_solve_type=0, dt=0.001,
               rho_c_ic=1.0, u_c_ic=1.0, v_c_ic=1.0, p_c_ic=1.0)
    c.to_device(0)
    if mode == "methods":
        c.run(2)
    else:
        c.run_steps_lib(2, fused=mode)
    c.sync_host()
    last = int(d["sizes"][7]) - 1
    assert rel(c.array("disu_upts0"), d["u_step1_stage%d" % last]) < 1e-11
    c.close()
