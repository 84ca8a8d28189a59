"""The triangle fixtures under tests/golden/tris (tools/capture_tris.py; genuine reference) without a GPU: the oracle in lockstep
meets every one at the bars of tests/test_oracle_vs_golden.py, every physics row is live, the orientation seed keeps every pair of
local faces among the interior faces, and the blocks the GPU tests cut (tests/tri_util.py: block) are sound inputs."""
import ctypes as C

import numpy as np
import pytest

import general_util as G
import oracle_py as O
import tri_util as T

EXPECTED = ["tri_p1_n4_deformed", "tri_p2_base", "tri_p2_cfl_local", "tri_p2_inviscid", "tri_p2_n3_deformed", "tri_p2_roem_sutherland",
            "tri_p2_rusanov_ldg", "tri_p3_bdy", "tri_p3_cylinder", "tri_p3_n4_deformed", "tri_p4_n2_deformed", "tri_p5_n2_deformed"]
COUNTS = (1, 31, 33, 65)  # 1, G - 1, G + 1, 2 G + 1 at the P3 group of 32 (csrc/simplex2d.hpp)


def test_the_fixtures_are_there():
    assert T.names() == EXPECTED
    for name in EXPECTED:
        d = T.load(name)
        assert int(d["sizes"][6]) == 0 and int(d["sizes"][4]) == 2 and int(d["sizes"][3]) == 4, name
        p = int(d["sizes"][5])
        assert (int(d["sizes"][1]), int(d["sizes"][2])) == ((p + 1) * (p + 2) // 2, 3 * (p + 1)), name


@pytest.mark.parametrize("name", EXPECTED)
def test_oracle_in_lockstep(name):
    d = T.load(name)
    errs = T.lockstep(d)
    assert any(k.startswith("u_step") for k in errs) and "s0_div_tconf_upts" in errs
    if name in ("tri_p2_n3_deformed", "tri_p3_bdy"):
        assert "s0_grad_disu_fpts" in errs and "s0_norm_tconf_fpts" in errs  # every intermediate of the first residual
    assert not T.failures(errs), T.failures(errs)


def final_state(d, **override):
    """the oracle's state after the fixture's first step, a parameter overridden"""
    c = O.Case(d)
    for k, v in override.items():
        setattr(c.params, k, v)
    e = c.c_eles()
    f, nfb = c.c_faces()
    o = O.load()
    for rk in range(int(d["sizes"][7])):
        assert o.orc_CalcResidual(C.byref(e), f, nfb, C.byref(c.params)) == -1
        o.orc_AdvanceSolution(C.byref(e), C.byref(c.params), rk)
    return c.arr["u0"].copy()


def test_every_physics_row_moves_the_final_state():
    """RoeM + Sutherland and Rusanov + LDG penalty: the row's fixture against tri_p2_base (same mesh, same step).  The inviscid row
    runs on the isentropic vortex (on the Taylor-Green state with viscous 0 the reference stops with a NaN residual), so against
    the base it differs by its initial state already; what shows that the row is live is its own inputs with the OTHER Riemann
    solver: without viscous terms the common flux alone moves the state.  (On the base's inputs one step without the viscous
    terms moves the state by 2.6e-8 only -- printed, not asserted: the base's viscosity is the Taylor-Green case's.)"""
    base = T.load("tri_p2_base")
    last = "u_step0_stage4"
    for row in ("tri_p2_roem_sutherland", "tri_p2_rusanov_ldg"):
        d = T.load(row)
        move = T.relerr(d[last], base[last])
        print(row, move)
        assert move > 1e-6, (row, move)
    # the inviscid row on the base's inputs: the viscous terms off
    ub = final_state(base)
    assert T.relerr(ub, base[last]) < 1e-13
    move = T.relerr(final_state(base, viscous=0), ub)
    print("viscous 0 on the base's inputs", move)
    assert move > 0.0
    inv = T.load("tri_p2_inviscid")
    assert T.relerr(inv[last], base[last]) > 1e-6
    assert int(np.ravel(inv["viscous"])[0]) == 0 and "opp_4_0" not in inv
    ui = final_state(inv)
    assert T.relerr(ui, inv[last]) < 1e-13
    move = T.relerr(final_state(inv, riemann_solve_type=0), ui)
    print("inviscid, Rusanov for HLLC", move)
    assert move > 1e-6


def test_every_pair_of_local_faces_meets():
    cen = T.face_pair_census(T.load("tri_p3_n4_deformed"))
    print(cen)
    assert cen.shape == (3, 3) and (cen > 0).all() and cen.sum() == 48
    assert (T.face_pair_census(T.load("tri_p1_n4_deformed")) > 0).sum() < 9  # (without the seed the diagonal cut meets in few)


def test_keeping_all_elements_reproduces_the_fixture():
    d = T.load("tri_p3_n4_deformed")
    keep = np.random.default_rng(5).permutation(32)
    p = G.cut(d, keep)
    assert not any(k.startswith("bdy") for k in p)
    ref = G.oracle_steps(p, 2)
    for st in range(2):
        assert ref[st]["bad"] == -1
        assert T.relerr(ref[st]["u"], d["u_step%d_stage4" % st][:, keep, :]) < 1e-13


@pytest.mark.parametrize("n", COUNTS)
def test_cut_blocks_are_sound_inputs(n):
    """every flux point belongs to exactly one face, the oracle reports no NaN and keeps rho and p positive, and every element --
    those of the last partial group included -- moves by more than 1e-6 of max |u| in every step"""
    d = T.block(n)
    assert int(d["sizes"][0]) == n and (G.face_census(d) == 1).all()
    assert any(k.startswith("bdy") for k in d) and (n == 1 or any(k.startswith("int") for k in d))
    ref = T.reference(("block", n), d)
    gamma = float(np.ravel(d["gamma"])[0])
    before = d["u_init"]
    for st, r in enumerate(ref):
        assert r["bad"] == -1, (st, r["bad"])
        u = r["u"]
        rho = u[:, :, 0]
        p = (gamma - 1.0) * (u[:, :, 3] - 0.5 * (u[:, :, 1] ** 2 + u[:, :, 2] ** 2) / rho)
        assert np.isfinite(u).all() and rho.min() > 0.0 and p.min() > 0.0, (st, rho.min(), p.min())
        moves = G.element_moves(before, u)
        assert moves.min() > 1e-6, (st, int(moves.argmin()), moves.min())
        before = u


# ---- the blocks of tests/test_gpu_tris_orders.py: whole and later groups at every instantiated order -----------------------------
ORDER_BLOCKS = T.order_blocks() + T.SWITCH_BLOCKS
LOCAL_DT_BLOCKS = [(name, n) for name, n in T.SWITCH_BLOCKS if name == "tri_p2_cfl_local"]


@pytest.mark.parametrize("name,n", ORDER_BLOCKS)
def test_order_blocks_are_sound_inputs(name, n):
    """every flux point belongs to one face, the oracle reports no NaN over N_STEPS steps and every element moves by more than 1e-6
    of max |u| in every step; where the block has elements a and a + G, their final states differ by more than 1e-6 of max |u|
    for EVERY a -- a kernel that takes group k's element for group k + 1's cannot meet the bar on any of them"""
    g = T.group_of(name)
    d = T.block(n, name)
    assert int(d["sizes"][0]) == n and (G.face_census(d) == 1).all()
    assert any(k.startswith("bdy") for k in d) and any(k.startswith("int") for k in d)
    if name in T.KINDS:
        fl = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")
        used = sorted({int(fl[0, i]) for t in range(3) if "bdy%d_id" % t in d for i in np.ravel(d["bdy%d_id" % t])})
        assert used == sorted(T.KINDS[name]), used
    ref = T.block_reference(n, name)
    before = d["u_init"]
    for st, r in enumerate(ref):
        assert r["bad"] == -1 and np.isfinite(r["u"]).all(), (st, r["bad"])
        moves = G.element_moves(before, r["u"])
        assert moves.min() > 1e-6, (st, int(moves.argmin()), moves.min())
        before = r["u"]
    if n > g:
        diff = T.offset_differences(ref[-1]["u"], g)
        print("%s, %d elements: elements a and a + %d differ by %.1e at least" % (name, n, g, diff.min()))
        assert diff.size == n - g and diff.min() > 1e-6, (int(diff.argmin()), diff.min())


@pytest.mark.parametrize("name,n", LOCAL_DT_BLOCKS)
def test_local_time_steps_of_another_group_miss(name, n):
    """dt_type 2: the oracle with dt_local rolled by G elements, and with every group reading group 0's dt_local, misses the
    right result by more than 1e-6 -- on elements beyond group 0 in the second case"""
    g = T.group_of(name)
    d = T.block(n, name)
    assert int(np.ravel(d["dt_type"])[0]) == 2
    right = T.block_reference(n, name)[-1]["u"]
    rolled = G.oracle_steps(d, T.N_STEPS, dt_map=lambda dtl: np.roll(dtl, g))[-1]["u"]
    group0 = G.oracle_steps(d, T.N_STEPS, dt_map=lambda dtl: dtl[np.arange(n) % g])[-1]["u"]
    miss = [T.relerr(rolled, right), T.relerr(group0[:, g:], right[:, g:]), T.relerr(group0[:, :g], right[:, :g])]
    print("%s, %d elements: rolled dt_local %.1e, group 0's dt_local %.1e beyond group 0 (%.1e inside)" % (name, n, *miss))
    assert miss[0] > 1e-6 and miss[1] > 1e-6, miss
