"""The 2-D simplex fused stage (csrc/simplex2d.hip) on whole and later groups at EVERY instantiated order, P1 to P5.

The stage walks a block in groups of G = 64 / 64 / 32 / 32 / 16 consecutive elements; every order has its own instantiation of the
element kernel, the update kernel and the update kernel's shock-capturing form.  The fixtures of P1, P2, P4 and P5 hold 32 / 18 / 8 / 8
elements, so on them no group is ever whole (no second trip of the 256 lanes over a group's NU G solution points, no second register
set of the folded filter) and nothing is ever indexed with e0 > 0.  The blocks here are cut from the committed fixtures
(tests/tri_util.py: block, tests/tri_shock_util.py: block) at G - 1, G, G + 1 and 2 G + 1 elements and checked against the oracle
on the same block; tests/test_tris_oracle.py, tests/test_tris_shock_oracle.py and tests/test_tris_partition_oracle.py show without a GPU
that each is a sound input, that elements a and a + G end in different states, that another group's local time step misses, and
that the filter fires in the second trip and beyond group 0.

Bars, relative to the array's largest magnitude (those of tests/test_gpu_tris.py, tests/test_gpu_tris_partition.py and
tests/test_gpu_tris_shock.py): 1e-11 for the state after each step (per element), 10 x 5e-11 for div_tconf_upts of a step's last
stage (5e-11 in the partitioned runner), 1e-12 for disu_fpts against opp_0 u, 1e-9 for the sensor.  Every case asserts the plan
that ran -- size class, group, launch grids, group lists, the shock plan --, so a silent per-method run cannot pass."""
import numpy as np
import pytest

import hfx
import tri_util as T
import tri_shock_util as TS
from test_gpu_tris import make, close, run_fused_steps, expected_plan, check_fpts_and_nan, SIZES
from test_gpu_tris_partition import run_partitioned_steps, expected_partition_plan, expected_grids
from test_gpu_tris_shock import expected_shock_plan, sensor_err
from test_tris_partition_oracle import block_parts, order_cuts

pytestmark = pytest.mark.gpu

TOL_U, TOL_SENSOR = 1e-11, 1e-9
relerr = T.relerr


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


def check_plan(d, name, plan, grids, gather, cap):
    g = T.group_of(name)
    assert plan["group"] == g and plan["size_class"] == int(d["sizes"][5]) - 1 and plan == expected_plan(d, gather), plan
    n_groups = -(-int(d["sizes"][0]) // g)
    launched = min(n_groups, cap) if cap else n_groups
    assert grids == [(1, launched, n_groups), (3, launched, n_groups)], grids


# ---- a. undivided, every order -----------------------------------------------------------------------------------------------------
# (G - 1, G + 1 and 2 G + 1 at P3 with the corrections gathered are tests/test_gpu_tris.py::test_fused_group_edges)
UNDIVIDED = [(name, n, 1) for name, n in T.order_blocks() if not (name == T.CUT_FROM and n != T.group_of(name))]
UNDIVIDED += [(name, 2 * T.group_of(name) + 1, 0) for name in T.BY_ORDER.values()]


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("name,n,gather", UNDIVIDED)
def test_undivided_group_edges(ctx, name, n, gather, cap):
    """a last group of G - 1, G, 1 and 1 elements behind 0, 0, 1 and 2 whole ones; cap 1: ONE workgroup walks all groups and reuses
    its LDS planes; gather 0: the LDG corrections written by face_delta_kernel<2>"""
    d = T.block(n, name)
    grids = []
    plan = run_fused_steps(ctx, d, T.block_reference(n, name), "%s, %d elements, gather %d, cap %d" % (name, n, gather, cap),
                           [("persistent_grid_cap", cap), ("gather_delta", gather)], grids)
    check_plan(d, name, plan, grids, gather, cap)


# ---- b. the run-wide switches and local time steps past group 0 --------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("name,n", T.SWITCH_BLOCKS)
def test_switches_past_group_0(ctx, name, n, cap):
    """RoeM with Sutherland's law, Rusanov with an off-centre LDG, inviscid (no gradient phases: another barrier sequence between
    the groups one workgroup walks) and dt_type 2 (dt_local[e0 + el]) on three groups of P2 elements"""
    d = T.block(n, name)
    assert n > T.group_of(name)
    grids = []
    plan = run_fused_steps(ctx, d, T.block_reference(n, name), "%s, %d elements, cap %d" % (name, n, cap), [("persistent_grid_cap", cap)], grids)
    check_plan(d, name, plan, grids, 1, cap)
    assert plan["gather"] == int(name != "tri_p2_inviscid")


# ---- c. partitioned, every order ---------------------------------------------------------------------------------------------------
# (P3 with the partners gathered is tests/test_gpu_tris_partition.py::test_partitioned_group_edges)
PARTITIONED = [(name, n, want, 1, cap) for name, n, want in order_cuts() if name != T.CUT_FROM for cap in (0, 2)]
PARTITIONED += [(name, n, want, 0, 0) for name, n, want in order_cuts() if n == 2 * T.group_of(name) + 1]


@pytest.mark.parametrize("name,n,want,gather,cap", PARTITIONED)
def test_partitioned_group_edges(ctx, comm, name, n, want, gather, cap):
    """hfx_run_steps_partitioned_blocks on the virtual parts of block_parts(n, name) against the oracle on the undivided block: the
    groups[it] lists at every G; gather 0: the partition points' corrections written by mpi_delta_kernel<2>"""
    d = T.block(n, name)
    ref = T.block_reference(n, name)
    what = "%s, %d elements in parts, gather %d, cap %d" % (name, n, gather, cap)
    pp, plan, grids, L = run_partitioned_steps(ctx, comm, d, block_parts(n, name), ref, what, [("persistent_grid_cap", cap), ("gather_delta", gather)])
    assert L.shape[1] > 0
    assert plan["group"] == T.group_of(name) and (plan["size_class"], plan["group"]) == SIZES[(int(d["sizes"][1]), int(d["sizes"][2]))]
    assert plan["gather"] == gather
    assert pp == expected_partition_plan(d, L, gather), pp
    assert (pp["partition_groups"], pp["interior_groups"]) == want
    assert grids == expected_grids(pp, cap), grids


# ---- d. the shock fold, every order ------------------------------------------------------------------------------------------------
def shock_blocks():
    for p in sorted(TS.BY_ORDER):
        name = TS.BY_ORDER[p]
        g = T.GROUP[p]
        for n in (g, 2 * g + 1):
            for cap in (0, 1):
                yield name, n, 1, cap
        yield name, 2 * g + 1, 0, 0  # the second witness: the SHOCK = false update kernel and the per-method filter behind it
    for cap in (0, 1):
        yield "ts_p2_cfl_local", 129, 1, cap  # filter, local time step and second group together


@pytest.mark.parametrize("name,n,fold,cap", list(shock_blocks()))
def test_shock_group_edges(ctx, name, n, fold, cap):
    """whole groups (the second trip's register set r[1], filt[1]) and later groups (sensor[e0 + tid]) under the folded filter:
    state and sensor after each step against the oracle's lockstep on the same block"""
    b, ref = TS.block(n, name)
    g = T.GROUP[int(b["sizes"][5])]
    what = "%s, %d elements, fold %d, cap %d" % (name, n, fold, cap)
    opts = [("fold_shock", fold), ("persistent_grid_cap", cap)]
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        e, faces = make(ctx, b)
        nstage = int(b["sizes"][7])
        for st in range(TS.N_STEPS):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            u, want = e.download(hfx.DISU_UPTS0), ref["u"][st]
            per_ele = np.abs(u - want).max(axis=(0, 2)) / np.abs(want).max()
            sensor, want_s = e.download(hfx.SENSOR), ref["stage_sensors"][(st + 1) * nstage - 1]
            serr = sensor_err(sensor, want_s)
            print("%s step %d: state %.2e (element %d of %d) sensor %.2e" % (what, st, per_ele.max(), int(per_ele.argmax()), n, serr))
            assert per_ele.max() < TOL_U, (what, st, int(per_ele.argmax()), per_ele.max())
            assert serr < TOL_SENSOR, (what, st, int(np.abs(np.ravel(sensor) - want_s).argmax()), serr)
            check_fpts_and_nan(e, b, "%s step %d" % (what, st))
        assert e.simplex2d_shock_plan() == expected_shock_plan(b, fold)
        plan = e.simplex2d_plan()
        assert plan["group"] == g and plan == expected_plan(b)
        n_groups = -(-n // g)
        launched = min(n_groups, cap) if cap else n_groups
        assert hfx.fused_launch_grids(e.h) == [(1, launched, n_groups), (3, launched, n_groups)]
        close(e, faces)
    finally:
        ctx.set_option("fold_shock", 1)
        ctx.set_option("persistent_grid_cap", 0)
