"""Wall forces on the device (hfx_eles_compute_wall_forces; eles::compute_wall_forces, src/eles.cpp:5704-5990) against the yardstick of
tests/wall_force_util.py: a numpy restatement in np.longdouble applied to exactly the arrays the device gets, at the derived bar
stated there (1e-12 of the un-cancelled scale S of every number, totals and points alike); and, through the host mirror with
deferred execution on, against the recorded output of the genuine reference at 1e-10 S -- the project's bar for quantities
formed from differences of nearly equal terms on states it holds to 1e-11."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import wall_force_util as W
from test_gpu_methods_vs_golden import GOLDEN, build
from test_wall_force_host import FIXTURES, device_arrays, file_order, mirror_case, phys_of, ref_of, setup

pytestmark = pytest.mark.gpu

STALE = "was not materialised by the fused stage that ran last"
REF = dict(rho_c_ic=0.9, u_c_ic=0.3, v_c_ic=0.2, w_c_ic=0.1, p_c_ic=0.7, area_ref=1.3)  # for blocks that come with none
LD = W.LD


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


@functools.lru_cache(maxsize=None)
def registration(name):
    """the fixture's case as the raw C ABI takes it (operators, metrics, face tables, parameters), from the host mirror"""
    case, _ = mirror_case(setup(name)["d"])
    reg = case.registration()
    case.close()
    return reg


def register(e, A):
    e.set_wall_faces(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"])


def want_of(A, u, grad, phys, ref):
    return W.both(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"], u, grad, phys, ref)


def check_device(e, A, u, grad, phys, ref, what):
    """two calls agree bit for bit, and with the restatement at the bar"""
    got = e.compute_wall_forces()
    again = e.compute_wall_forces()
    for k in W.KEYS:
        assert np.array_equal(got[k], again[k]), k
    want, S = want_of(A, u, grad, phys, ref)
    W.assert_at_the_bar(got, want, S, what)
    assert np.any(got["inv_force"] != 0) and np.any(got["cp"] != 0)
    if phys["viscous"]:
        assert np.any(got["vis_force"] != 0) and np.all(got["cf"] > 0)
    else:
        assert not np.any(got["vis_force"]) and not np.any(got["cf"])
    return got


@pytest.mark.parametrize("fix_vis", [1, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_the_c_abi(ctx, name, fix_vis):
    """the five fixtures' wall faces, state and gradient uploaded; with the fixture's constant viscosity and with Sutherland's law"""
    s = setup(name)
    reg = registration(name)
    e, faces = build(ctx, reg)
    p = hfx.params_from(reg)
    p.fix_vis = float(fix_vis)
    ctx.set_params(p)
    ctx.set_force_reference(**s["ref"])
    register(e, s["A"])
    d = s["d"]
    e.upload(hfx.DISU_UPTS0, d["u_step0_stage0"])
    grad = d.get("s0_grad_disu_upts")
    if grad is not None:
        e.upload(hfx.GRAD_DISU_UPTS, grad)
    check_device(e, s["A"], d["u_step0_stage0"], grad, dict(s["phys"], fix_vis=float(fix_vis)), s["ref"], "%s fix_vis %d" % (name, fix_vis))
    close(e, faces)


def seeded_faces(rng, n_eles, n_upts, n_dims, local_faces, n_inters, n_faces, n_cub):
    """faces picked by the test with a dense seeded operator of n_cub points per face: rows are convex combinations, so the
    interpolated density and pressure stay positive; the local faces outside `local_faces` have no operator"""
    opp, weight = [None] * n_inters, [None] * n_inters
    for l in local_faces:
        o = rng.uniform(0.05, 1.0, (n_cub, n_upts))
        opp[l] = np.asfortranarray(o / o.sum(axis=1, keepdims=True))
        weight[l] = rng.uniform(0.1, 1.0, n_cub)
    ele = rng.integers(0, n_eles, n_faces)
    inter = rng.choice(local_faces, n_faces)
    flag = rng.choice(W.WALL_FLAGS, n_faces)
    detjac = [rng.uniform(0.5, 1.5, n_cub) for _ in range(n_faces)]
    norm = []
    for _ in range(n_faces):
        v = rng.normal(size=(n_cub, n_dims))
        norm.append(np.asfortranarray(v / np.linalg.norm(v, axis=1, keepdims=True)))
    return dict(face_ele=ele.astype(np.int32), face_inter=inter.astype(np.int32), face_flag=flag.astype(np.int32), opp=opp, weight=weight,
                detjac=detjac, norm=norm)


@pytest.mark.parametrize("name,n_inters", [("tet_p2_n2_deformed", 4), ("pri_p2_n2_deformed", 5)])
def test_other_element_classes_with_seven_points_per_face(ctx, name, n_inters):
    """tetrahedra and prisms: the device takes registered arrays and knows no class.  7 points per face: neither a wave nor n_upts"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    e, faces = build(ctx, d)
    assert e.n_upts != 7
    rng = np.random.default_rng(20261019)
    A = seeded_faces(rng, e.n_eles, e.n_upts, 3, [0, 2, 3], n_inters, 23, 7)
    p = hfx.params_from(d)
    phys = {k: getattr(p, k) for k in ("gamma", "rt_inf", "mu_inf", "c_sth", "fix_vis", "viscous")}
    assert phys["viscous"]
    ctx.set_force_reference(**REF)
    register(e, A)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    check_device(e, A, d["u_init"], grad, phys, REF, name)
    close(e, faces)


@pytest.mark.parametrize("fix_vis", [1, 0])
def test_triangle_wall_faces_from_the_reference(ctx, fix_vis):
    """fl_tri_p3_walls (tests/golden/full_loop): 40 P3 triangles between an isothermal and an adiabatic wall, the 8 wall faces and the
    surface cubature as the reference itself formed them (the harness's dump; the host mirror builds no triangles) -- 4 points per
    face, all 3 local faces among the walls, node lists rotated.  After one hfx_CalcResidual, with the constant viscosity and with
    Sutherland's law, against the restatement on the downloaded state and gradient at its derived bar"""
    import full_loop_util as FU
    d = FU.load("fl_tri_p3_walls")
    F = FU.force_setup(d)
    A = F["A"]
    assert len(A["face_ele"]) == 8 and set(A["face_inter"].tolist()) == {0, 1, 2} and A["opp"][0].shape == (4, 10)
    e, faces = build(ctx, d)
    p = hfx.params_from(d)
    p.fix_vis = float(fix_vis)
    ctx.set_params(p)
    ctx.set_force_reference(**F["ref"])
    register(e, A)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    check_device(e, A, d["u_init"], grad, dict(F["phys"], fix_vis=float(fix_vis)), F["ref"], "fl_tri_p3_walls fix_vis %d" % fix_vis)
    close(e, faces)


@functools.lru_cache(maxsize=None)
def p4_channel():
    """18 P4 hexahedra between an isothermal and a dual-consistent slip wall, from the host mirror: 36 wall faces of 5 x 5 points"""
    c = H.Case([6, 3, 1], order=4, amp=0.1, adv_type=0, calc_force=1, area_ref=2.0, monitor_cp_freq=1, nx_c_ic=0.8, ny_c_ic=0.5,
               nz_c_ic=0.33, bcs=[{"type": "isotherm_wall", "T_static": 310.0, "u": 3.0}, {"type": "slip_wall_dual"}],
               sides={"z-": 0, "z+": 1})
    out = dict(reg=c.registration(), A=device_arrays(c), phys=phys_of(c), ref=ref_of(c))
    c.close()
    return out


@pytest.mark.parametrize("cap", [0, 2])
def test_p4_hexahedra_and_a_loop_past_its_first_pass(ctx, cap):
    """25 points per face; a slab of a P4 element is 5000 bytes, so the 32 KB cap makes a pass six faces -- 150 lanes, not a whole
    number of waves.  With the grid held to two workgroups (option persistent_grid_cap) each walks three passes."""
    X = p4_channel()
    if cap:
        ctx.set_option("persistent_grid_cap", cap)
    e, faces = build(ctx, X["reg"])
    ctx.set_force_reference(**X["ref"])
    register(e, X["A"])
    n_faces = len(X["A"]["face_ele"])
    assert n_faces == 36 and X["A"]["opp"][0].shape == (25, 125)
    groups, fpp = e.wall_force_launch()
    assert fpp == 6 and groups == (cap or 6) and (not cap or n_faces >= 3 * groups * fpp)
    hfx.CalcResidual(e, faces)
    grad = e.download(hfx.GRAD_DISU_UPTS)
    check_device(e, X["A"], X["reg"]["u_init"], grad, X["phys"], X["ref"], "P4 channel, grid cap %d" % cap)
    close(e, faces)


def test_scrambled_list_comes_back_in_the_callers_order(ctx):
    """a registration whose list mixes local faces and flags in scrambled order (and names one face twice): every per-point
    result sits where the caller's list puts it"""
    s = setup("wf_hex_p2_a")
    reg = registration("wf_hex_p2_a")
    A0 = s["A"]
    rng = np.random.default_rng(7)
    order = np.concatenate([rng.permutation(len(A0["face_ele"])), [3]])
    flags = rng.permutation(np.resize(W.WALL_FLAGS, len(order))).astype(np.int32)  # all four kinds, in no order
    A = dict(A0, face_ele=A0["face_ele"][order], face_inter=A0["face_inter"][order], face_flag=flags,
             detjac=[A0["detjac"][i] for i in order], norm=[A0["norm"][i] for i in order])
    assert len(set(A["face_inter"])) == 2 and len(set(A["face_flag"])) == 4
    e, faces = build(ctx, reg)
    ctx.set_force_reference(**s["ref"])
    register(e, A)
    d = s["d"]
    e.upload(hfx.DISU_UPTS0, d["u_step0_stage0"])
    e.upload(hfx.GRAD_DISU_UPTS, d["s0_grad_disu_upts"])
    check_device(e, A, d["u_step0_stage0"], d["s0_grad_disu_upts"], s["phys"], s["ref"], "scrambled list")
    # registering again replaces everything
    register(e, A0)
    check_device(e, A0, d["u_step0_stage0"], d["s0_grad_disu_upts"], s["phys"], s["ref"], "registered again")
    close(e, faces)


def raw_call(e, n_dims, n_points):
    """hfx_eles_compute_wall_forces into arrays filled with -7: (rc, message, the arrays)"""
    lib = hfx.lib()
    out = [np.full(3, -7.0), np.full(3, -7.0), C.c_double(-7.0), C.c_double(-7.0), np.full(max(1, n_points), -7.0), np.full(max(1, n_points), -7.0)]
    rc = lib.hfx_eles_compute_wall_forces(e.h, out[0].ctypes.data_as(hfx.dp), out[1].ctypes.data_as(hfx.dp), C.byref(out[2]), C.byref(out[3]),
                                          out[4].ctypes.data_as(hfx.dp), out[5].ctypes.data_as(hfx.dp))
    return rc, lib.hfx_last_error().decode(), out


def untouched(out):
    return all(np.all(np.asarray(a.value if hasattr(a, "value") else a) == -7.0) for a in out)


def test_zero_faces_and_refusals(ctx):
    """each refusal comes with its message and before anything is launched (the caller's arrays are untouched); a block without
    wall faces returns zeros"""
    s = setup("wf_quad_p3_b")
    reg = registration("wf_quad_p3_b")
    A = s["A"]
    e, faces = build(ctx, reg)
    n_points = 32

    def refused(pattern):
        rc, msg, out = raw_call(e, 2, n_points)
        assert rc != 0 and pattern in msg and untouched(out), (rc, msg)

    refused("hfx_eles_set_wall_faces")                 # no registration
    with pytest.raises(hfx.HfxError, match="hfx_eles_set_wall_faces"):
        e.wall_force_launch()
    register(e, A)
    refused("hfx_ctx_set_force_reference")             # no force reference
    for bad in (dict(s["ref"], u_c_ic=0.0, v_c_ic=0.0, w_c_ic=0.0), dict(s["ref"], area_ref=0.0), dict(s["ref"], area_ref=-1.0)):
        with pytest.raises(hfx.HfxError, match="hfx_ctx_set_force_reference"):
            ctx.set_force_reference(**bad)
    refused("hfx_ctx_set_force_reference")
    ctx.set_force_reference(**s["ref"])
    # registrations that are refused leave nothing behind
    for change, pattern in ((dict(face_ele=np.where(np.arange(8) == 5, e.n_eles, A["face_ele"])), "names element"),
                            (dict(face_inter=np.where(np.arange(8) == 2, 4, A["face_inter"])), "names local face"),
                            (dict(face_flag=np.where(np.arange(8) == 1, hfx.BC_CYCLIC, A["face_flag"])), "no wall"),
                            (dict(opp=[None] + A["opp"][1:]), "no surface cubature")):
        with pytest.raises(hfx.HfxError, match=pattern):
            register(e, dict(A, **change))
        rc, msg, out = raw_call(e, 2, n_points)
        assert rc == 0, msg                             # (the earlier registration stands: a refusal comes before anything changes)
    e.clear_wall_faces()
    refused("hfx_eles_set_wall_faces")
    # zero faces
    e.set_wall_faces([], [], [], [None] * 4, [None] * 4, [], [])
    rc, msg, out = raw_call(e, 2, 0)
    assert rc == 0, msg
    assert np.all(out[0][:2] == 0.0) and np.all(out[1][:2] == 0.0) and out[2].value == 0.0 and out[3].value == 0.0
    assert np.all(out[4] == -7.0)                       # (no point, nothing written)
    close(e, faces)


def test_stale_gradient_is_refused_until_a_residual_has_run(ctx):
    """a viscous walled box after two steps of hfx_run_steps(..., 3): the gradient stayed on chip and the call is refused with the
    words of hfx_eles_download; after hfx_CalcResidual it is accepted and equals the restatement on the downloaded state and gradient"""
    s = setup("wf_hex_p2_a")
    reg = registration("wf_hex_p2_a")
    e, faces = build(ctx, reg)
    ctx.set_force_reference(**s["ref"])
    register(e, s["A"])
    hfx.run_steps(e, faces, 2, fused=3)
    rc, msg, out = raw_call(e, 3, 162)
    assert rc != 0 and STALE in msg and untouched(out), (rc, msg)
    with pytest.raises(hfx.HfxError, match=STALE):
        e.download(hfx.GRAD_DISU_UPTS)
    hfx.CalcResidual(e, faces)
    u, grad = e.download(hfx.DISU_UPTS0), e.download(hfx.GRAD_DISU_UPTS)
    assert np.abs(u - reg["u_init"]).max() > 0
    check_device(e, s["A"], u, grad, s["phys"], s["ref"], "after fused 3 and CalcResidual")
    close(e, faces)


def test_inviscid_context_never_asks_for_the_gradient(ctx):
    """deferred execution, an inviscid case with a whole stage recorded and not yet run: the call asks the scheduler for nothing
    -- the stage runs exactly as it does for an explicit hfx_ctx_flush (same counts of fused and replayed records, the same
    bits) -- and the forces are those of the new state"""
    from test_gpu_deferred import calc_residual_calls, tag
    s = setup("wf_quad_p3_inviscid")
    reg = registration("wf_quad_p3_inviscid")
    ctx.set_option("deferred", 1)
    out, stats = [], []
    for flush in (True, False):
        e, faces = build(ctx, reg)
        tag(e, reg)
        ctx.set_force_reference(**s["ref"])
        register(e, s["A"])
        calc_residual_calls([e], faces, False, 0)
        e.AdvanceSolution(0, 0)
        if flush:
            ctx.flush()
        out.append(e.compute_wall_forces())
        stats.append(ctx.deferred_stats()[:2])
        if not flush:
            u = e.download(hfx.DISU_UPTS0)
        close(e, faces)
    assert stats[1] == (2 * stats[0][0], 2 * stats[0][1]) and sum(stats[0]) == 1, stats
    for k in W.KEYS:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(u - reg["u_init"]).max() > 0
    want, S = want_of(s["A"], u, None, s["phys"], s["ref"])
    W.assert_at_the_bar(out[1], want, S, "inviscid, deferred stage pending")


@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_against_the_reference(name):
    """hfxh_case_run(c, 1) then hfxh_case_CalcForces with deferred execution on (the mirror's default): the pending stage is
    replayed call by call and leaves the gradient of the step's stage -- the reference's pairing -- and the totals and the rows
    equal what the genuine driver wrote, at 1e-10 S"""
    s = setup(name)
    d, S, nd = s["d"], s["S"], s["n_dims"]
    c, _ = mirror_case(d)
    c.to_device()
    c.run(1)
    F = c.CalcForces()
    wp = c.wall_points()
    nf, nr, why = hfx.deferred_stats(c.handles()[0])
    c.close()
    print("%s: stages run fused %d, records replayed %d (%s)" % (name, nf, nr, why))
    assert (nr >= 1 and nf == 0) if s["phys"]["viscous"] else nr == 0
    bar = LD(1e-10)
    first = s["val"]["first"]
    worst = 0.0
    for got, want, sc, what in ((F["inv_force"] + F["vis_force"], d["hist_F"], S["inv_force"] + S["vis_force"], "F"),
                                (F["cl"], d["hist_CL"][0], S["cl"], "CL"), (F["cd"], d["hist_CD"][0], S["cd"], "CD"),
                                (wp["cp"], d["cp_rows"][:, nd], file_order(S["cp"], first), "Cp")) + \
            (((wp["cf"], d["cp_rows"][:, nd + 1], file_order(S["cf"], first), "Cf"),) if s["phys"]["viscous"] else ()):
        r = float((np.abs(np.atleast_1d(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD))) / np.atleast_1d(sc)).max())
        print("%s: %s worst |mirror - reference| / S = %.2e" % (name, what, r))
        worst = max(worst, r)
    assert worst <= bar, (name, worst)
    if not s["phys"]["viscous"]:
        assert not np.any(wp["cf"]) and not np.any(F["vis_force"])


def test_two_parts_sum_to_the_whole():
    """wf_quad_p3_b cut in two along x, its periodic direction: each part registers its own wall faces, gets its elements' state
    and gradient, and hfxh_case_CalcForces sums through the hook of hfxh_case_set_reduce_sum -- one call with 2 n_dims + 2
    values -- to the undivided result, at 1e-12 S"""
    import json
    import bdy_util
    import partition_util as PU
    s = setup("wf_quad_p3_b")
    d, S, want = s["d"], s["S"], s["val"]
    meta = json.loads(bytes(d["meta_json"]).decode())
    kk = meta["keys"]
    bcs, sides = bdy_util.groups_of(meta)
    n_local, pgrid = [2, 1, 1], [2, 1, 1]
    xv = d["xv"].reshape((5, 2, 2), order="F")  # (ix, iy, coordinate)
    kw = dict(dims=2, order=kk["order"], adv_type=kk["adv_type"], riemann_solve_type=kk["riemann_solve_type"], viscous=1, ic_form=kk["ic_form"],
              fix_vis=kk["fix_vis"], T_c_ic=kk["T_c_ic"], rho_c_ic=kk["rho_c_ic"], upts_type=kk["upts_type_quad"], vcjh_scheme=kk["vcjh_scheme_quad"],
              dt=kk["dt"], Mach_c_ic=kk["Mach_c_ic"], calc_force=1, area_ref=kk["area_ref"], monitor_cp_freq=1, nx_c_ic=kk["nx_c_ic"],
              ny_c_ic=kk["ny_c_ic"], nz_c_ic=kk["nz_c_ic"], loc_1d_upts=d["loc_upts"][0, :kk["order"] + 1])
    local, cases = [], []
    for rank in range(2):
        c = H.Case(n_local, xv=xv[2 * rank:2 * rank + 3].reshape((6, 2), order="F"), rank=rank, pgrid=pgrid, bcs=bcs, sides=sides, **kw)
        assert len(c.wall_points()["ele"]) == 4
        c.to_device()
        idx = PU.global_index(n_local, pgrid, rank)
        e = c.handles()[1]
        for arr_id, a in ((hfx.DISU_UPTS0, d["u_step0_stage0"][:, idx, :]), (hfx.GRAD_DISU_UPTS, d["s0_grad_disu_upts"][:, idx, :, :])):
            a = np.asfortranarray(a)
            hfx.check(hfx.lib().hfx_eles_upload(e, C.c_int(arr_id), a.ctypes.data_as(hfx.dp)))
        calls = []
        c.set_reduce_sum(lambda v, calls=calls: calls.append(list(v)) or v)
        c.CalcForces()
        assert len(calls) == 1 and len(calls[0]) == 6
        local.append(calls[0])
        cases.append(c)
    total = [local[0][i] + local[1][i] for i in range(6)]
    for c in cases:
        c.set_reduce_sum(lambda v: total)
        F = c.CalcForces()
        got = dict(inv_force=F["inv_force"], vis_force=F["vis_force"], cl=F["cl"], cd=F["cd"])
        assert list(got["inv_force"]) + list(got["vis_force"]) + [got["cl"], got["cd"]] == total
        W.assert_at_the_bar(got, want, S, "two parts", keys=("inv_force", "vis_force", "cl", "cd"))
        c.close()
