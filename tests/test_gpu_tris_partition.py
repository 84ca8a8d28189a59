"""Partitioned triangle blocks on the device: the 2-D simplex fused stage behind hfx_run_steps_partitioned_blocks and behind the
deferred call sequence (csrc/simplex2d.hip, simplex2d_partitioned_stage in csrc/comm.hip), interior groups first.

One rank, hfx.Comm(..., 1, 0): the faces between virtual parts are partition faces the rank exchanges with itself over libhfx's RCCL
transport (ragged_partition.cut_self; tests/test_tris_partition_oracle.py shows without a GPU that every cut here is a sound input
and what it offers to the group lists).  Bars, relative to the array's largest magnitude: 1e-11 for states after whole steps against
the genuine reference's fixtures, 5e-11 for div_tconf_upts of the step's last stage against the oracle on the undivided mesh.  Every
fused run asserts hfx_simplex2d_partition_plan, so a silent per-method run cannot pass.

Without the partitioned stage every fused test of this file fails at "partition faces on a triangle block"."""
import os

import numpy as np
import pytest

import hfx
import mixed_util as MU
import tri_util as T
from test_gpu_tris import make, close, check_fpts_and_nan, SIZES
from test_tris_partition_oracle import VIRTUAL3, G_P3, grow_parts, virtual_tables, block_parts, group_census

pytestmark = pytest.mark.gpu

TOL_U, TOL_DIV = 1e-11, 5e-11
relerr = T.relerr
GOLDEN = os.path.dirname(T.GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def comm(ctx):
    c = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    yield c
    c.close()


def make_partitioned(ctx, d, part):
    """-> (block, interior and boundary blocks, [the partition-face block], its table L)"""
    reg, L, Rlut, seg = virtual_tables(d, part)
    e, faces = make(ctx, reg)
    m = hfx.MpiInters(ctx, e, L, Rlut)
    m.set_neighbours(seg)
    return e, faces, [m], L


def expected_partition_plan(d, L, gather):
    n_part, n_int, _, _ = group_census(d, L)
    remote = bool(gather) and bool(int(np.ravel(d["viscous"])[0])) and L.shape[1] > 0
    return {"partition_groups": n_part, "interior_groups": n_int, "gather_remote": int(remote)}


def expected_grids(pp, cap):
    """the launches of one stage: element kernel on the interior, then on the partition groups; update kernel on the partition, then
    on the interior groups; an empty list launches nothing"""
    n_p, n_i = pp["partition_groups"], pp["interior_groups"]
    out = [(1, n_i), (1, n_p), (3, n_p), (3, n_i)]
    return [(s, min(w, cap) if cap else w, w) for s, w in out if w > 0]


def run_partitioned_steps(ctx, comm, d, part, want, what, opts=(), check_div=True):
    """one call of one step per entry of `want` ({"u": ..., "div": ...} or None) -> (partition plan, simplex2d plan, launch grids)"""
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        e, faces, M, L = make_partitioned(ctx, d, part)
        for st, w in enumerate(want):
            hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
            if w is not None:
                u = e.download(hfx.DISU_UPTS0)
                err = relerr(u, w["u"])
                print("%s step %d: state %.2e" % (what, st, err))
                assert err < TOL_U, (what, st, err)
                if check_div and w.get("div") is not None:
                    err = relerr(e.download(hfx.DIV_TCONF_UPTS), w["div"])
                    print("%s step %d: div_tconf_upts %.2e" % (what, st, err))
                    assert err < TOL_DIV, (what, st, err)
            check_fpts_and_nan(e, d, "%s step %d" % (what, st))
        out = e.simplex2d_partition_plan(), e.simplex2d_plan(), hfx.fused_launch_grids(e.h), L
        close(e, faces + M)
        return out
    finally:
        for k, _ in opts:
            ctx.set_option(k, 1 if k == "gather_delta" else 0)


# ---- 1. the fixtures, step by step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("name", ["tri_p1_n4_deformed", "tri_p3_n4_deformed", "tri_p5_n2_deformed", "tri_p3_bdy", "tri_p2_inviscid",
                                  "tri_p2_rusanov_ldg", "tri_p2_roem_sutherland"])
def test_partitioned_fixture_states(ctx, comm, name, gather):
    """three virtual parts; the partners of partition points gathered in the element kernel (the default) and their corrections
    written by mpi_delta_kernel<2>"""
    d = T.load(name)
    nstage = int(d["sizes"][7])
    n_steps = max(T.stored_steps(d)) + 1
    ref = T.reference(("fixture", name), d, n_steps)  # (the undivided oracle: div_tconf_upts of every step's last stage)
    want = [{"u": d["u_step%d_stage%d" % (st, nstage - 1)], "div": ref[st]["div"]} for st in range(n_steps)]
    part = grow_parts(d, *VIRTUAL3)
    pp, plan, grids, L = run_partitioned_steps(ctx, comm, d, part, want, name, [("gather_delta", gather)])
    assert L.shape[1] > 0
    assert pp == expected_partition_plan(d, L, gather), pp
    assert plan["gather"] == int(bool(gather) and bool(int(np.ravel(d["viscous"])[0])))
    assert (plan["size_class"], plan["group"]) == SIZES[(int(d["sizes"][1]), int(d["sizes"][2]))]


def sub_table(L, Rlut, seg, pick):
    """the partition-face block of the segments `pick` (closed under mates) of a cut_self table: their faces in order, the segments
    renumbered, recv_first of each where its mate's faces now sit"""
    first, at = {}, 0
    for s in pick:
        first[seg[s][1]] = at
        at += seg[s][3]
    cols = np.concatenate([np.arange(seg[s][1], seg[s][1] + seg[s][3]) for s in pick])
    new = [(0, first[seg[s][1]], first[seg[s][2]], seg[s][3]) for s in pick]
    return np.asfortranarray(L[:, cols]), np.asfortranarray(Rlut[:, cols]), new


@pytest.mark.parametrize("name", ["tri_p3_n4_deformed", "tri_p3_bdy"])
def test_two_partition_face_blocks_take_the_fallback(ctx, comm, name):
    """the same cut registered as TWO partition-face blocks (virtual parts 0 | 1, and the rest): with gather_delta 1 the interior
    points are still gathered, the partition points get their corrections from mpi_delta_kernel<2>"""
    d = T.load(name)
    nstage = int(d["sizes"][7])
    reg, L, Rlut, seg = virtual_tables(d, grow_parts(d, *VIRTUAL3))
    assert len(seg) == 6
    mates = [s for s in range(6) if seg[s][1] in (seg[0][1], seg[0][2])]
    others = [s for s in range(6) if s not in mates]
    e, faces = make(ctx, reg)
    M = []
    for pick in (mates, others):
        Ls, Rs, segs = sub_table(L, Rlut, seg, pick)
        M.append(hfx.MpiInters(ctx, e, Ls, Rs))
        M[-1].set_neighbours(segs)
    hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
    err = relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage%d" % (nstage - 1)])
    print("%s, two partition-face blocks: state %.2e" % (name, err))
    assert err < TOL_U
    pp = e.simplex2d_partition_plan()
    assert pp == dict(expected_partition_plan(d, L, 1), gather_remote=0), pp
    assert e.simplex2d_plan()["gather"] == 1
    check_fpts_and_nan(e, d, name)
    close(e, faces + M)


# ---- 2. group edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("n", [1, G_P3 - 1, G_P3 + 1, 2 * G_P3 + 1])
def test_partitioned_group_edges(ctx, comm, n, cap):
    """blocks of 1, G - 1, G + 1 and 2 G + 1 elements cut into virtual parts against the oracle on the undivided block: no partition
    face at all, one partial partition group, a partial INTERIOR group behind a whole partition group, three partition groups"""
    d = T.block(n)
    ref = T.reference(("block", n), d)
    assert all(r["bad"] == -1 for r in ref)
    pp, plan, grids, L = run_partitioned_steps(ctx, comm, d, block_parts(n), ref, "block of %d" % n, [("persistent_grid_cap", cap)])
    assert plan["group"] == G_P3
    assert pp == expected_partition_plan(d, L, 1), pp
    want = {1: (0, 1), G_P3 - 1: (1, 0), G_P3 + 1: (1, 1), 2 * G_P3 + 1: (3, 0)}[n]
    assert (pp["partition_groups"], pp["interior_groups"]) == want
    assert grids == expected_grids(pp, cap), grids


# ---- 3. CFL time steps in the partitioned blocks loop -----------------------------------------------------------------------------
def test_partitioned_cylinder_cfl_steps(ctx, comm):
    """tri_p3_cylinder (dt_type 1, Sutherland, supersonic inlet, isothermal wall) on three virtual parts: two steps of the loop,
    each behind its own calc_time_step, against the fixture's stored state"""
    d = T.load("tri_p3_cylinder")
    nstage = int(d["sizes"][7])
    assert int(np.ravel(d["dt_type"])[0]) == 1 and T.stored_steps(d) == [1]
    part = grow_parts(d, *VIRTUAL3)
    e, faces, M, L = make_partitioned(ctx, d, part)
    hfx.run_steps_partitioned_blocks([e], faces, M, comm, 2)
    if "dt_step1" in d:
        want = float(np.ravel(d["dt_step1"])[0])
        assert abs(ctx.get_dt() - want) <= 1e-11 * want
    err = relerr(e.download(hfx.DISU_UPTS0), d["u_step1_stage%d" % (nstage - 1)])
    print("cylinder, three virtual parts: state %.2e" % err)
    assert err < TOL_U
    pp = e.simplex2d_partition_plan()
    assert pp == expected_partition_plan(d, L, 1) and pp["interior_groups"] > 0, pp
    check_fpts_and_nan(e, d, "cylinder")
    close(e, faces + M)


# ---- 4. the deferred call sequence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tri_p3_n4_deformed", "tri_p3_bdy"])
def test_partitioned_deferred_call_sequence(name):
    """the reference's calls with send_* / receive_* on a partitioned triangle block, `deferred` 1: every stage is planned as the
    general partitioned stage and runs the 2-D simplex stage on the group lists"""
    d = T.load(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    n_steps = max(T.stored_steps(d)) + 1
    c = hfx.Context(0)
    e, faces, M, L = make_partitioned(c, d, grow_parts(d, *VIRTUAL3))
    comm = hfx.Comm(c.h, hfx.comm_unique_id(), 1, 0)
    c.set_option("deferred", 1)
    ints = [f for f in faces if isinstance(f, hfx.IntInters)]
    bdys = [f for f in faces if isinstance(f, hfx.BdyInters)]
    for st in range(n_steps):
        for rk in range(nstage):  # CalcResidual's order with the partition-face calls (src/solver.cpp:59-221)
            e.extrapolate_solution()
            for f in M: f.send_solution(comm)
            e.calculate_gradient()
            e.evaluate_invFlux()
            for f in ints: f.calculate_common_invFlux()
            for f in bdys: f.evaluate_boundaryConditions_invFlux()
            for f in M: f.receive_solution(comm)
            for f in M: f.calculate_common_invFlux()
            e.correct_gradient()
            for f in M: f.send_corrected_gradient(comm)
            e.evaluate_viscFlux()
            e.extrapolate_totalFlux()
            e.calculate_divergence()
            for f in ints: f.calculate_common_viscFlux()
            for f in bdys: f.evaluate_boundaryConditions_viscFlux()
            for f in M: f.receive_corrected_gradient(comm)
            for f in M: f.calculate_common_viscFlux()
            e.calculate_corrected_divergence()
            e.AdvanceSolution(rk, adv)
        err = relerr(e.download(hfx.DISU_UPTS0), d["u_step%d_stage%d" % (st, nstage - 1)])
        print("%s deferred, step %d: state %.2e" % (name, st, err))
        assert err < TOL_U, (st, err)
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (n_steps * nstage, 0), (nf, nr, why)
    pp = e.simplex2d_partition_plan()
    assert pp == expected_partition_plan(d, L, 1) and pp["partition_groups"] > 0, pp
    assert hfx.fused_launch_grids(e.h) == expected_grids(pp, 0)
    assert e.check_nan() == -1
    comm.close()
    close(e, faces + M)
    c.close()


# ---- 5. what stays as it was ------------------------------------------------------------------------------------------------------
def test_cfl_steps_on_the_mixed_partitioned_channel():
    """dt_type 1 in hfx_run_steps_partitioned_blocks on the mixed tetrahedron / prism channel of tests/test_mixed_mesh.py: with
    run_input.CFL set so that the step's CFL minimum over both blocks is the fixture's fixed time step, every step meets the
    fixture as the fixed-step loop does"""
    from ragged_partition import self_partition
    d = dict(np.load(os.path.join(GOLDEN, "mixed_p3_channel.npz")))
    c = hfx.Context(0)
    classes, per, faces, bdy = MU.split(d)
    p = hfx.params_from(per[classes[0]])
    dt_fixed = p.dt
    p.dt_type = 1
    p.dt = 0.0
    c.set_params(p)
    E = {}
    for k in classes:
        sz = [int(v) for v in per[k]["sizes"]]
        E[k] = hfx.Eles(c, sz[:5], per[k], ele_type=sz[6], order=sz[5])
        E[k].upload(hfx.DISU_UPTS0, per[k]["u_init"])
        E[k].set_h_ref(np.ones(sz[0]))
    rest, M = self_partition(c, E, faces)
    F = [hfx.IntInters(c, E[a], E[b], L, R) for a, b, L, R in rest]
    for a, L, ids in bdy:
        F.append(hfx.BdyInters(c, E[a], L, ids, hfx.bc_records(d["bc_flags"], d["bc_params"]), float(np.ravel(d["bc_R_ref"])[0]),
                               int(np.ravel(d["ramp_counter"])[0])))
    comm = hfx.Comm(c.h, hfx.comm_unique_id(), 1, 0)
    blocks = [E[k] for k in classes]
    nstage = int(d["c2_sizes"][7])
    steps = sorted({int(k.split("_")[2][4:]) for k in d if k.startswith("c2_u_step")})
    for st in steps:
        unit = min(e.calc_dt_local(1.0) for e in blocks)  # (the step is linear in CFL)
        c.set_CFL(dt_fixed / unit)
        hfx.run_steps_partitioned_blocks(blocks, F, M, comm, 1)
        assert abs(c.get_dt() - dt_fixed) <= 1e-14 * dt_fixed, (c.get_dt(), dt_fixed)
        for k in classes:
            key = "c%d_u_step%d_stage%d" % (k, st, nstage - 1)
            err = relerr(E[k].download(hfx.DISU_UPTS0), d[key])
            print("%s: %.2e" % (key, err))
            assert err < TOL_U, key
    comm.close()
    for f in F + M:
        f.close()
    for k in classes:
        E[k].close()
    c.close()


def test_unpartitioned_entry_points_keep_refusing(ctx, comm):
    """hfx_run_steps_blocks(..., fused = 4) and the deferred sequence WITHOUT the partition-face calls refuse a partition-face block
    before anything is launched -- also on tables the partitioned loop has just prepared --, naming both ways out"""
    d = T.load("tri_p3_n4_deformed")
    e, faces, M, L = make_partitioned(ctx, d, grow_parts(d, *VIRTUAL3))
    for prepared in (False, True):
        before = e.download(hfx.DISU_UPTS0)
        with pytest.raises(hfx.HfxError, match="partition faces") as err:
            hfx.run_steps_blocks([e], faces + M, 1, fused=4)
        assert "fused 0" in str(err.value) and "hfx_run_steps_partitioned_blocks" in str(err.value), str(err.value)
        assert np.array_equal(e.download(hfx.DISU_UPTS0), before)
        if not prepared:
            hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
            assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage%d" % (int(d["sizes"][7]) - 1)]) < TOL_U
    close(e, faces + M)
    # several triangle blocks stay refused in the partitioned loop too
    e, faces, M, L = make_partitioned(ctx, d, grow_parts(d, *VIRTUAL3))
    e2, faces2 = make(ctx, d)
    with pytest.raises(hfx.HfxError, match="several element blocks"):
        hfx.run_steps_partitioned_blocks([e, e2], faces + faces2, M, comm, 1)
    close(e2, faces2)
    close(e, faces + M)
