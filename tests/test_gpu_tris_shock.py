"""Shock capturing on triangles on the device, against the genuine driver's fixtures under tests/golden/tris_shock
(tools/capture_tris_shock.py; tests/test_tris_shock_oracle.py shows without a GPU that every input here is a sound one): the
per-method path, the 2-D simplex fused stage with the filter folded into its update kernel (csrc/simplex2d.hip,
simplex2d_update_kernel_t<.., SHOCK = true>), the same stage with option fold_shock 0 and the per-method filter behind it, the
deferred call sequence, the partitioned loop and the plot monitor's sensor field.

Bars, relative to the array's largest magnitude: TOL_U = 1e-11 for states after whole steps, 1e-9 of the largest sensor for the sensor
(the bar of tests/test_gpu_methods_vs_golden.py), 1e-12 on the state between two device paths.  The energy sensor (shock_det_field 1)
is ts_p3_energy, Euler steps with dt_type 2 are ts_p2_cfl_local, dt_type 1 is ts_p3_cylinder: each runs on every path below.  Every
folded run asserts hfx_simplex2d_shock_plan, so a silent per-method filter cannot pass.

On the commit before the fold every fused, deferred, partitioned, plan and plot test of this file fails at the refusal "registered
shock capturing runs per method (fused 0)"; the per-method tests pass there."""
import numpy as np
import pytest

import hfx
import tri_util as T
import tri_shock_util as TS
from test_gpu_tris import make, close, check_fpts_and_nan, SIZES
from test_gpu_deferred import calc_residual_calls, tag
from test_tris_partition_oracle import grow_parts, virtual_tables, group_census
from test_tris_shock_oracle import NAMES, BLOCKS

pytestmark = pytest.mark.gpu

TOL_U, TOL_SENSOR, TOL_PATHS = 1e-11, 1e-9, 1e-12
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


def sensor_err(got, want):
    return float(np.abs(np.ravel(got) - np.ravel(want)).max() / np.abs(want).max())


def check_step(e, d, ref, st, what):
    """the state after step st + 1 against the driver's restart file where the fixture holds it, and against the lockstep; the sensor
    against the driver's Tecplot column"""
    u = e.download(hfx.DISU_UPTS0)
    steps = [int(s) for s in d["restart_steps"]]
    if st + 1 in steps:
        err = relerr(u, d["u_restart"][steps.index(st + 1)])
        print("%s step %d: state against the driver %.2e" % (what, st + 1, err))
        assert err < TOL_U, (what, st, err)
    err = relerr(u, ref["u"][st])
    assert err < TOL_U, (what, st, err)
    serr = sensor_err(e.download(hfx.SENSOR), d["sensor_rows"][st])
    print("%s step %d: sensor against the driver %.2e" % (what, st + 1, serr))
    assert serr < TOL_SENSOR, (what, st, serr)
    return u


def expected_shock_plan(d, folded):
    nu, nfp = int(d["sizes"][1]), int(d["sizes"][2])
    g, p = SIZES[(nu, nfp)][1], int(d["sizes"][5])
    lds = 8 * (2 * nu * nfp + (g + 1) * (4 * nu + 4 * nfp))
    if folded:
        lds += 8 * (2 * nu * nu + (g + 1) * (nu + 1))
    assert lds <= 80 * 1024
    return {"folded": int(folded), "update_lds": lds, "first_high_mode": p * (p + 1) // 2, "launches_behind": 0 if folded else 5}


# ---- 1. the per-method path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_per_method(ctx, name):
    """hfx_CalcResidual, hfx_eles_AdvanceSolution, hfx_eles_shock_capture per stage"""
    d, ref = TS.load(name), TS.reference(name)
    e, faces = make(ctx, d)
    nstage, adv, dt_type = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0]), int(np.ravel(d["dt_type"])[0])
    for st in range(TS.n_steps_of(d)):
        if dt_type != 0:
            p = hfx.params_from(d)
            p.dt = e.calc_dt_local(TS.scalar(d, "CFL"))
            ctx.set_params(p)
        for rk in range(nstage):
            hfx.CalcResidual(e, faces)
            e.AdvanceSolution(rk, adv)
            e.shock_capture()
            serr = sensor_err(e.download(hfx.SENSOR), ref["stage_sensors"][st * nstage + rk])
            assert serr < TOL_SENSOR, (name, st, rk, serr)
        check_step(e, d, ref, st, name + " per method")
    assert e.check_nan() == -1
    close(e, faces)


# ---- 2. the fused stage, the filter folded and behind it ---------------------------------------------------------------------------
def run_fused(ctx, d, ref, what, fold=1, opts=(), n_steps=None):
    """one call of one step per step -> (states per step, sensor after the loop)"""
    opts = [("fold_shock", fold)] + list(opts)
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        e, faces = make(ctx, d)
        states = []
        for st in range(TS.n_steps_of(d) if n_steps is None else n_steps):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            states.append(check_step(e, d, ref, st, what) if "sensor_rows" in d else e.download(hfx.DISU_UPTS0))
            check_fpts_and_nan(e, d, "%s step %d" % (what, st))
        plan, grids, sensor = e.simplex2d_shock_plan(), hfx.fused_launch_grids(e.h), e.download(hfx.SENSOR)
        assert plan == expected_shock_plan(d, fold), plan
        n_groups = -(-int(d["sizes"][0]) // SIZES[(int(d["sizes"][1]), int(d["sizes"][2]))][1])
        assert [(s, w) for s, g, w in grids] == [(1, n_groups), (3, n_groups)], grids  # (no launch beyond the stage's)
        if fold:
            ms, names = hfx.time_general_kernels([e], faces, 1)
            assert names.split(",") == ["face_delta_kernel", "simplex2d_element_kernel", "face_flux2_kernel", "simplex2d_update_kernel"]
            assert not any(ms[4:])
        close(e, faces)
        return states, sensor
    finally:
        for k, _ in opts:
            ctx.set_option(k, 1 if k in ("gather_delta", "fold_shock") else 0)


_folded = {}


@pytest.mark.parametrize("name", NAMES)
def test_fused_folded(ctx, name):
    """run_steps_blocks(..., fused = 4): four launches per stage, the sensor after the loop is the last stage's"""
    d, ref = TS.load(name), TS.reference(name)
    states, sensor = run_fused(ctx, d, ref, name + " folded")
    assert sensor_err(sensor, ref["stage_sensors"][-1]) < TOL_SENSOR
    _folded[name] = states


@pytest.mark.parametrize("name", NAMES)
def test_fused_filter_behind(ctx, name):
    """the second witness: option fold_shock 0 runs the SHOCK = false update kernel and general_shock_capture behind every stage;
    folded and unfolded states agree at 1e-12"""
    d, ref = TS.load(name), TS.reference(name)
    states, sensor = run_fused(ctx, d, ref, name + " filter behind", fold=0)
    if name not in _folded:
        _folded[name] = run_fused(ctx, d, ref, name + " folded")[0]
    for st, (a, b) in enumerate(zip(_folded[name], states)):
        err = relerr(a, b)
        print("%s step %d: folded against unfolded %.2e" % (name, st + 1, err))
        assert err < TOL_PATHS, (name, st, err)


@pytest.mark.parametrize("n", BLOCKS)
def test_fused_group_edges(ctx, n):
    """cut blocks of 1, G - 1 and G + 1 elements (a second group of one element), ONE workgroup walking the groups: the sensor pass
    touches the block's elements alone and the filter works in a last partial group (tests/test_tris_shock_oracle.py)"""
    b, ref = TS.block(n)
    s0 = TS.scalar(b, "s0")
    if n == TS.G_P3 - 1:
        assert any(0 in g for g in TS.group_of_filtered(ref["stage_sensors"], s0, TS.G_P3))  # (its one group is a partial one)
    opts = [("fold_shock", 1), ("persistent_grid_cap", 1)]
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        e, faces = make(ctx, b)
        nstage = int(b["sizes"][7])
        for st in range(TS.N_STEPS):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            err = relerr(e.download(hfx.DISU_UPTS0), ref["u"][st])
            serr = sensor_err(e.download(hfx.SENSOR), ref["stage_sensors"][(st + 1) * nstage - 1])
            print("block of %d step %d: state %.2e sensor %.2e" % (n, st + 1, err, serr))
            assert err < TOL_U and serr < TOL_SENSOR, (n, st, err, serr)
            check_fpts_and_nan(e, b, "block of %d" % n)
        assert e.simplex2d_shock_plan() == expected_shock_plan(b, 1)
        assert all(g == 1 for s, g, w in hfx.fused_launch_grids(e.h))
        close(e, faces)
    finally:
        ctx.set_option("persistent_grid_cap", 0)


# ---- 3. the deferred call sequence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts_p3_n4", "ts_p3_bdy"])
def test_deferred_call_sequence(name):
    """the reference's calls with `deferred` 1, shock_capture recorded behind AdvanceSolution: every stage is planned as the general
    stage and runs the 2-D simplex stage with the filter folded"""
    d, ref = TS.load(name), TS.reference(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = make(c, d)
    tag(e, d)
    for st in range(TS.n_steps_of(d)):
        for rk in range(nstage):
            calc_residual_calls([e], faces, True, rk)
            e.AdvanceSolution(rk, adv)
            e.shock_capture()
        check_step(e, d, ref, st, name + " deferred")
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (TS.n_steps_of(d) * nstage, 0), (nf, nr, why)
    assert e.simplex2d_shock_plan() == expected_shock_plan(d, 1)
    assert [s for s, g, w in hfx.fused_launch_grids(e.h)] == [1, 3]
    close(e, faces)
    c.close()


# ---- 4. the partitioned loop -------------------------------------------------------------------------------------------------------
def make_partitioned(ctx, d, part):
    reg, L, Rlut, seg = virtual_tables(d, part)
    e, faces = make(ctx, reg)
    m = hfx.MpiInters(ctx, e, L, Rlut)
    m.set_neighbours(seg)
    return e, faces, [m], L


@pytest.mark.parametrize("name,gather,fold", [("ts_p3_n4", 1, 1), ("ts_p3_cylinder", 1, 1), ("ts_p3_cylinder", 0, 1), ("ts_p3_n4", 1, 0)])
def test_partitioned_loop(ctx, comm, name, gather, fold):
    """hfx_run_steps_partitioned_blocks on three virtual parts against the UNDIVIDED fixture: the update on the partition groups
    carries the filter, so the flux-point solution packed behind it is the filtered state's (the cylinder: dt_type 1; its parts have
    filtered elements in partition AND interior groups); fold 0: the filter behind both update launches"""
    d, ref = TS.load(name), TS.reference(name)
    ctx.set_option("gather_delta", gather)
    ctx.set_option("fold_shock", fold)
    try:
        e, faces, M, L = make_partitioned(ctx, d, grow_parts(d, *TS.PARTS[name]))
        for st in range(TS.n_steps_of(d)):
            hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
            check_step(e, d, ref, st, "%s partitioned (gather %d, fold %d)" % (name, gather, fold))
            check_fpts_and_nan(e, d, name)
        n_part, n_int, _, _ = group_census(d, L)
        pp = e.simplex2d_partition_plan()
        assert (pp["partition_groups"], pp["interior_groups"]) == (n_part, n_int) and n_part > 0
        assert e.simplex2d_shock_plan() == expected_shock_plan(d, fold)
        close(e, faces + M)
    finally:
        ctx.set_option("gather_delta", 1)
        ctx.set_option("fold_shock", 1)


def test_partitioned_deferred_call_sequence():
    """the reference's calls with send_* / receive_* and shock_capture on a partitioned block, `deferred` 1"""
    name = "ts_p3_n4"
    d, ref = TS.load(name), TS.reference(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    e, faces, M, L = make_partitioned(c, d, grow_parts(d, *TS.PARTS[name]))
    comm = hfx.Comm(c.h, hfx.comm_unique_id(), 1, 0)
    c.set_option("deferred", 1)
    ints = [f for f in faces if isinstance(f, hfx.IntInters)]
    bdys = [f for f in faces if isinstance(f, hfx.BdyInters)]
    for st in range(TS.n_steps_of(d)):
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
            e.shock_capture()
        check_step(e, d, ref, st, name + " partitioned, deferred")
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (TS.n_steps_of(d) * nstage, 0), (nf, nr, why)
    assert e.simplex2d_shock_plan() == expected_shock_plan(d, 1)
    assert e.check_nan() == -1
    comm.close()
    close(e, faces + M)
    c.close()


# ---- 5. the plot monitor -----------------------------------------------------------------------------------------------------------
def test_plot_monitor_sensor():
    """the `sensor` field sampled inside a fused-4 loop equals the driver's Tecplot sensor column after every step at the bar of
    tests/plot_rows_util.py (1e-11 of the column's scale + 1e-14 of the value).  The sensor is constant over an element's plot
    points, so the interpolation is any: the first three solution points"""
    name = "ts_p3_n4"
    d = TS.load(name)
    n_steps = TS.n_steps_of(d)
    c = hfx.Context(0)
    e, faces = make(c, d)
    e.set_opp_p(np.asfortranarray(np.eye(int(d["sizes"][1]))[:3]))
    c.set_plot_monitor(["sensor"], plot_freq=1, capacity=n_steps)
    c.set_clock(0.0, 0)
    hfx.run_steps_blocks([e], faces, n_steps, fused=4)
    times, steps, values = e.read_plot_snapshots()
    assert list(steps) == list(range(1, n_steps + 1))
    nf = int(d["sizes"][3])
    for s in range(n_steps):
        got, want = values[:, :, nf, s], np.asarray(d["sensor_rows"][s])[None, :]
        bar = 1e-11 * np.abs(want).max() + 1e-14 * np.abs(want)
        miss = float((np.abs(got - want) / bar).max())
        print("plot monitor, step %d: sensor %.2f bars" % (s + 1, miss))
        assert miss <= 1.0, (s, miss)
    assert e.simplex2d_shock_plan()["folded"] == 1
    close(e, faces)
    c.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def refused(e, faces, match):
    before = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match=match) as err:
        hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert "fused 0" in str(err.value), str(err.value)
    assert np.array_equal(e.download(hfx.DISU_UPTS0), before)


def test_refusals(ctx):
    """a registration of another form than eles_tris::shock_det_persson's, and a conforming one beside over-integration or an LES
    closure, stay refused before the first launch; a conforming re-registration runs"""
    name = "ts_p3_n4"
    d, ref = TS.load(name), TS.reference(name)
    nu, ne, s0 = int(d["sizes"][1]), int(d["sizes"][0]), TS.scalar(d, "s0")
    iv, ef, high = d["inv_vandermonde"], d["exp_filter"], np.ravel(d["persson_high_modes"]).astype(np.int32)
    plain = {k: v for k, v in d.items() if k not in TS.SHOCK_KEYS}
    e, faces = make(ctx, plain)
    norm = np.ones(nu)
    norm[2] = 0.5
    e.set_shock_capture(iv, ef, norm, high, s0, 0)  # a norm that is not one
    refused(e, faces, "shock capturing")
    wide = high.copy()
    wide[nu - 5] = 1
    e.set_shock_capture(iv, ef, np.ones(nu), wide, s0, 0)  # a mode of degree p - 1 among the high modes
    refused(e, faces, "shock capturing")
    narrow = high.copy()
    narrow[nu - 1] = 0
    e.set_shock_capture(iv, ef, np.ones(nu), narrow, s0, 0)  # a mode of degree p missing
    refused(e, faces, "shock capturing")
    e.set_shock_capture(iv, ef, np.ones(nu), high, s0, 0)  # ... and the block runs after a conforming re-registration
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_restart"][0]) < TOL_U
    assert e.simplex2d_shock_plan() == expected_shock_plan(d, 1)
    # a later registration of another form is refused on the tables the stage has just used
    e.set_shock_capture(iv, ef, norm, high, s0, 0)
    refused(e, faces, "shock capturing")
    close(e, faces)
    e, faces = make(ctx, d)
    e.set_over_int(np.zeros((nu + 2, nu), order="F"), np.zeros((nu, nu + 2), order="F"), np.ones((2, 2, nu + 2, ne), order="F"))
    refused(e, faces, "over-integration")
    close(e, faces)
    e, faces = make(ctx, d)
    e.set_les(1, 0.325, 1.0, 0.41, 0.9, np.ones((2, 2, int(d["sizes"][2]), ne), order="F"))
    refused(e, faces, "LES closure")
    close(e, faces)


def test_shock_plan_is_refused_before_a_fused_call(ctx):
    e, faces = make(ctx, TS.load("ts_p1_n4"))
    with pytest.raises(hfx.HfxError, match="no 2-D simplex fused stage has prepared"):
        e.simplex2d_shock_plan()
    close(e, faces)


def test_a_block_without_shock_capturing_runs_the_old_kernel(ctx):
    """nothing registered: the plan says not folded, the old LDS image and nothing behind the stage"""
    d = T.load("tri_p3_n4_deformed")
    e, faces = make(ctx, d)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage4"]) < TOL_U
    assert e.simplex2d_shock_plan() == dict(expected_shock_plan(d, 0), launches_behind=0)
    close(e, faces)
