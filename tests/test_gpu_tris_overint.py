"""Over-integration on triangles on the device, against the genuine reference's fixtures under tests/golden/tris_overint
(tools/capture_tris_overint.py; tests/test_tris_overint_oracle.py shows without a GPU that every input here is a sound one): the
per-method path, the 2-D simplex fused stage with the de-aliased flux formed inside its element kernel (csrc/simplex2d.hip,
simplex2d_element_kernel_t<.., S2dOverInt::folded>), the same stage with option fold_over_int 0 (hfx_eles_evaluate_invFlux_over_int in
front of the element kernel, which reads tdisf_upts), the partitioned loop, the deferred call sequence, and both together with shock
capturing.

Bars, relative to the array's largest magnitude: TOL_U = 1e-11 for states after whole steps, 1e-9 of the largest sensor for the sensor.
Every fixture's state moves by more than 1e-7 when the over-integration arrays are left out, so a stage that skips de-aliasing
cannot pass.  Every fused run asserts hfx_simplex2d_over_int_plan, so a silent per-method run cannot pass either.

On the commit before the fold every fused, partitioned and deferred test of this file fails at the refusal "registered
over-integration runs per method (fused 0)"; the per-method tests pass there."""
import numpy as np
import pytest

import hfx
import tri_util as T
import tri_shock_util as TS
import tri_overint_util as TO
from test_gpu_tris import make, close, check_fpts_and_nan, expected_plan, SIZES
from test_gpu_deferred import calc_residual_calls, tag
from test_gpu_tris_shock import make_partitioned, expected_shock_plan, sensor_err
from test_tris_partition_oracle import grow_parts, group_census

pytestmark = pytest.mark.gpu

TOL_U, TOL_SENSOR = 1e-11, 1e-9
NAMES = TO.names()
relerr = T.relerr
DEFAULTS = {"gather_delta": 1, "fold_shock": 1, "fold_over_int": 1, "persistent_grid_cap": 0}


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


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def fixture_states(d):
    """the genuine reference's state after every step of the fixture"""
    return [d[TO.final_key(d, st)] for st in range(max(T.stored_steps(d)) + 1)]


def expected_oi_plan(d, folded):
    nu, nfp = int(d["sizes"][1]), int(d["sizes"][2])
    g = SIZES[(nu, nfp)][1]
    lds = 8 * (4 * nu * nu + 6 * nu * nfp + (g + 1) * (12 * nu + 4 * nfp))
    assert lds <= 80 * 1024
    if "opp_over_int_cubpts" not in d:
        return {"folded": 0, "n_cubpts": 0, "chunk": 0, "chunks": 0, "element_lds": lds, "launches_in_front": 0}
    nc, chunk, chunks = TO.chunks_of(d)
    return {"folded": int(folded), "n_cubpts": nc, "chunk": chunk, "chunks": chunks, "element_lds": lds, "launches_in_front": 0 if folded else 3}


def n_groups_of(d):
    return -(-int(d["sizes"][0]) // SIZES[(int(d["sizes"][1]), int(d["sizes"][2]))][1])


def run(ctx, d, want, what, fused=4, fold=1):
    """one call of one step per entry of `want` (the state after that step) -> the states; asserts the plan that ran"""
    e, faces = make(ctx, d)
    states = []
    for st, w in enumerate(want):
        hfx.run_steps_blocks([e], faces, 1, fused=fused)
        u = e.download(hfx.DISU_UPTS0)
        per_ele = np.abs(u - w).max(axis=(0, 2)) / np.abs(w).max()
        print("%s step %d: state %.2e (element %d of %d)" % (what, st + 1, per_ele.max(), int(per_ele.argmax()), len(per_ele)))
        assert per_ele.max() < TOL_U, (what, st, int(per_ele.argmax()), per_ele.max())
        if fused == 4:  # (the fused stage leaves disu_fpts of the new state; the per-method loop those of the last residual)
            check_fpts_and_nan(e, d, "%s step %d" % (what, st))
        assert e.check_nan() == -1, what
        states.append(u)
    if fused == 4:
        assert e.simplex2d_over_int_plan() == expected_oi_plan(d, fold), e.simplex2d_over_int_plan()
        assert e.simplex2d_plan() == expected_plan(d), e.simplex2d_plan()
        if fold:
            grids = hfx.fused_launch_grids(e.h)
            assert [(s, w) for s, g, w in grids] == [(1, n_groups_of(d)), (3, n_groups_of(d))], grids  # (no launch beyond the stage's)
    close(e, faces)
    return states


# ---- 1. three forms on every fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_per_method(ctx, name):
    d = TO.load(name)
    run(ctx, d, fixture_states(d), name + " per method", fused=0)


_folded = {}


@pytest.mark.parametrize("name", NAMES)
def test_fused_folded(ctx, name):
    """fused 4, the over-integration inside the element kernel: four launches per stage; launched twice, the results agree bit for bit"""
    d = TO.load(name)
    a = run(ctx, d, fixture_states(d), name + " folded")
    b = run(ctx, d, fixture_states(d), name + " folded again")
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    _folded[name] = a


@pytest.mark.parametrize("name", NAMES)
def test_fused_unfolded(ctx, name):
    """the second witness: option fold_over_int 0 runs the per-method over-integration in front of the element kernel"""
    d = TO.load(name)
    with options(ctx, fold_over_int=0):
        states = run(ctx, d, fixture_states(d), name + " unfolded", fold=0)
    if name not in _folded:
        _folded[name] = run(ctx, d, fixture_states(d), name + " folded")
    for st, (a, b) in enumerate(zip(_folded[name], states)):
        print("%s step %d: folded against unfolded %.2e" % (name, st + 1, relerr(a, b)))
        assert relerr(a, b) < TOL_U


# ---- 2. group edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("name,n", TO.order_blocks())
def test_group_edges(ctx, name, n, cap):
    """G - 1, G, G + 1 and 2 G + 1 elements at every order; cap 1: ONE workgroup walks all groups"""
    d = TO.block(n, name)
    ref = TO.block_reference("%s %d" % (name, n), d)
    with options(ctx, persistent_grid_cap=cap):
        run(ctx, d, [r["u"] for r in ref], "%s block of %d (cap %d)" % (name, n, cap))


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("n", TO.edge_counts(TO.CUT_FROM))
def test_group_edges_unfolded(ctx, n, cap):
    d = TO.block(n, TO.CUT_FROM)
    ref = TO.block_reference("%s %d" % (TO.CUT_FROM, n), d)
    with options(ctx, persistent_grid_cap=cap, fold_over_int=0):
        run(ctx, d, [r["u"] for r in ref], "unfolded block of %d (cap %d)" % (n, cap), fold=0)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("n", TO.edge_counts(TO.CUT_FROM))
def test_group_edges_inviscid(ctx, n, cap):
    """the P3 blocks run inviscid: no P1 / P2 between the over-integration phase and P3"""
    d = TO.block(n, TO.CUT_FROM, 0)
    ref = TO.block_reference("to_p3 %d inviscid" % n, d)
    with options(ctx, persistent_grid_cap=cap):
        run(ctx, d, [r["u"] for r in ref], "inviscid block of %d (cap %d)" % (n, cap))


# ---- 3. per-point metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [1, 0])
def test_per_point_metrics(ctx, fold):
    """JGinv_over_int_cubpts perturbed per (l, n, m, ele): a kernel that takes another point's or element's entry misses the oracle"""
    d = TO.perturbed_block()
    ref = TO.block_reference("perturbed", d)
    with options(ctx, fold_over_int=fold):
        run(ctx, d, [r["u"] for r in ref], "perturbed metrics (fold %d)" % fold, fold=fold)


# ---- 4. the partitioned loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("name", ["to_p3", "to_p3_cylinder"])
def test_partitioned_loop(ctx, comm, name, fold, gather):
    """hfx_run_steps_partitioned_blocks on three virtual parts against the UNDIVIDED fixture"""
    d = TO.load(name)
    with options(ctx, gather_delta=gather, fold_over_int=fold):
        e, faces, M, L = make_partitioned(ctx, d, grow_parts(d, *TS.PARTS[TO.SHOCK_ON[name]]))
        for st, w in enumerate(fixture_states(d)):
            hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
            err = relerr(e.download(hfx.DISU_UPTS0), w)
            print("%s partitioned (gather %d, fold %d) step %d: %.2e" % (name, gather, fold, st + 1, err))
            assert err < TOL_U
            check_fpts_and_nan(e, d, name)
        n_part, n_int, _, _ = group_census(d, L)
        pp = e.simplex2d_partition_plan()
        assert (pp["partition_groups"], pp["interior_groups"]) == (n_part, n_int) and n_part > 0
        assert e.simplex2d_over_int_plan() == expected_oi_plan(d, fold)
        close(e, faces + M)


# ---- 5. the deferred call sequence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["to_p3", "to_p3_bdy"])
def test_deferred_call_sequence(name):
    """the reference's calls with `deferred` 1 and evaluate_invFlux_over_int recorded: every stage runs the 2-D simplex stage, folded"""
    d = TO.load(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = make(c, d)
    tag(e, d)
    assert e.has_over_int
    want = fixture_states(d)
    for st, w in enumerate(want):
        for rk in range(nstage):
            calc_residual_calls([e], faces, True, rk)
            e.AdvanceSolution(rk, adv)
        assert relerr(e.download(hfx.DISU_UPTS0), w) < TOL_U, (name, st)
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (len(want) * nstage, 0), (nf, nr, why)
    assert e.simplex2d_over_int_plan() == expected_oi_plan(d, 1)
    assert [s for s, g, w in hfx.fused_launch_grids(e.h)] == [1, 3]
    close(e, faces)
    c.close()


def test_deferred_plain_invflux_stays_replayed():
    """a sequence that records plain evaluate_invFlux on a block that registered over-integration is replayed call by call, and
    gives what those calls give: the state of the run without over-integration (the base fixture's)"""
    d = TO.load("to_p3")
    base = T.load("tri_p3_n4_deformed")
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = make(c, d)
    tag(e, d)
    e.has_over_int = False
    for rk in range(nstage):
        calc_residual_calls([e], faces, True, rk)
        e.AdvanceSolution(rk, adv)
    u = e.download(hfx.DISU_UPTS0)
    nf, nr, why = c.deferred_stats()
    assert nf == 0 and nr > 0 and "over_int" in why, (nf, nr, why)
    assert relerr(u, base["u_step0_stage%d" % (nstage - 1)]) < TOL_U
    close(e, faces)
    c.close()


def test_partitioned_deferred_call_sequence():
    """the reference's calls with send_* / receive_* and evaluate_invFlux_over_int on a partitioned block, `deferred` 1"""
    name = "to_p3"
    d = TO.load(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    e, faces, M, L = make_partitioned(c, d, grow_parts(d, *TS.PARTS[TO.SHOCK_ON[name]]))
    comm = hfx.Comm(c.h, hfx.comm_unique_id(), 1, 0)
    c.set_option("deferred", 1)
    ints = [f for f in faces if isinstance(f, hfx.IntInters)]
    bdys = [f for f in faces if isinstance(f, hfx.BdyInters)]
    want = fixture_states(d)
    for st, w in enumerate(want):
        for rk in range(nstage):  # CalcResidual's order with the partition-face calls (src/solver.cpp:59-221)
            e.extrapolate_solution()
            for f in M: f.send_solution(comm)
            e.calculate_gradient()
            e.evaluate_invFlux_over_int()
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
        assert relerr(e.download(hfx.DISU_UPTS0), w) < TOL_U, st
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (len(want) * nstage, 0), (nf, nr, why)
    assert e.simplex2d_over_int_plan() == expected_oi_plan(d, 1)
    assert e.check_nan() == -1
    comm.close()
    close(e, faces + M)
    c.close()


# ---- 6. the step loop with a duty ----------------------------------------------------------------------------------------------------
def test_time_averages_in_the_fused_loop():
    """time averages of a fused-4 loop of three steps equal those of the fused-0 loop at the bar of tests/test_gpu_time_average.py"""
    d = TO.load("to_p3")
    fields = ["rho_average", "u_average", "v_average", "e_average"]
    out = {}
    for fused in (0, 4):
        c = hfx.Context(0)
        e, faces = make(c, d)
        e.set_average_fields(fields)
        c.set_clock(0.25, 0)
        hfx.run_steps_blocks([e], faces, 3, fused=fused)
        out[fused] = (e.download_average(), c.get_clock(), e.download(hfx.DISU_UPTS0))
        if fused == 4:
            assert e.simplex2d_over_int_plan() == expected_oi_plan(d, 1)
        close(e, faces)
        c.close()
    assert out[0][1] == out[4][1]
    avg = max(np.abs(out[4][0][:, :, i] - out[0][0][:, :, i]).max() / np.abs(out[0][0][:, :, i]).max() for i in range(out[0][0].shape[2]))
    print("averages %.2e, state %.2e" % (avg, relerr(out[4][2], out[0][2])))
    assert avg <= 1e-12 and relerr(out[4][2], out[0][2]) < TOL_U


# ---- 7. with shock capturing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold_oi", [1, 0])
@pytest.mark.parametrize("fold_shock", [1, 0])
@pytest.mark.parametrize("name", sorted(TO.SHOCK_ON))
def test_with_shock_capturing(ctx, name, fold_shock, fold_oi):
    """the element kernel with OVERINT and the update kernel with SHOCK in one stage, and the three other combinations, against the
    oracle with both ingredients"""
    d, ref = TO.with_shock(name)
    nstage = int(d["sizes"][7])
    with options(ctx, fold_shock=fold_shock, fold_over_int=fold_oi):
        e, faces = make(ctx, d)
        for st in range(TO.N_STEPS):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            err = relerr(e.download(hfx.DISU_UPTS0), ref["u"][st])
            serr = sensor_err(e.download(hfx.SENSOR), ref["stage_sensors"][(st + 1) * nstage - 1])
            print("%s (fold_shock %d, fold_over_int %d) step %d: state %.2e sensor %.2e" % (name, fold_shock, fold_oi, st + 1, err, serr))
            assert err < TOL_U and serr < TOL_SENSOR
            check_fpts_and_nan(e, d, name)
        assert e.simplex2d_over_int_plan() == expected_oi_plan(d, fold_oi)
        assert e.simplex2d_shock_plan() == expected_shock_plan(d, fold_shock)
        close(e, faces)


# ---- 8. refusals, re-registration, queries -------------------------------------------------------------------------------------------
def refused(e, faces, match):
    before = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match=match) as err:
        hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert "fused 0" in str(err.value), str(err.value)
    assert np.array_equal(e.download(hfx.DISU_UPTS0), before)


def test_les_beside_over_integration_stays_refused(ctx):
    d = TO.load("to_p3")
    e, faces = make(ctx, d)
    e.set_les(1, 0.325, 1.0, 0.41, 0.9, np.ones((2, 2, int(d["sizes"][2]), int(d["sizes"][0])), order="F"))
    refused(e, faces, "LES closure")
    close(e, faces)


def test_a_count_no_triangle_rule_has_stays_refused(ctx):
    """12 cubature points: no (o + 1)(o + 2) / 2"""
    d = T.load("tri_p3_n4_deformed")
    nu, ne = int(d["sizes"][1]), int(d["sizes"][0])
    e, faces = make(ctx, d)
    e.set_over_int(np.zeros((nu + 2, nu), order="F"), np.zeros((nu, nu + 2), order="F"), np.ones((2, 2, nu + 2, ne), order="F"))
    refused(e, faces, "over-integration")
    close(e, faces)


def test_a_second_registration_gets_fresh_tables(ctx):
    """28 cubature points, one step; then 6 on the same block: the stage runs the second registration's tables"""
    a, b = TO.load("to_p3"), TO.load("to_p3_o2")
    e, faces = make(ctx, a)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), fixture_states(a)[0]) < TOL_U
    assert e.simplex2d_over_int_plan() == expected_oi_plan(a, 1)
    e.set_over_int(b["opp_over_int_cubpts"], b["over_int_filter"], b["JGinv_over_int_cubpts"])
    e.upload(hfx.DISU_UPTS0, b["u_init"])
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), fixture_states(b)[0]) < TOL_U
    assert e.simplex2d_over_int_plan() == expected_oi_plan(b, 1)
    close(e, faces)


def test_plan_is_refused_before_a_fused_call(ctx):
    e, faces = make(ctx, TO.load("to_p1_o3"))
    with pytest.raises(hfx.HfxError, match="no 2-D simplex fused stage has prepared"):
        e.simplex2d_over_int_plan()
    close(e, faces)


def test_a_block_without_over_integration_runs_the_old_kernel(ctx):
    """nothing registered: the unchanged plan, no chunks, nothing in front of the stage"""
    d = T.load("tri_p3_n4_deformed")
    e, faces = make(ctx, d)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage4"]) < TOL_U
    assert e.simplex2d_plan() == expected_plan(d)
    assert e.simplex2d_over_int_plan() == expected_oi_plan(d, 0)
    close(e, faces)


@pytest.mark.parametrize("fold", [1, 0])
def test_timing_and_byte_queries(ctx, fold):
    """folded: four slots and the cubature metrics in the element kernel's bytes; unfolded: the over-integration slot (4) as well"""
    d = TO.load("to_p3")
    base = T.load("tri_p3_n4_deformed")
    eb, fb = make(ctx, base)
    hfx.run_steps_blocks([eb], fb, 0, fused=4)
    plain = hfx.general_kernel_bytes([eb])
    close(eb, fb)
    nu, nf, nd, ne, nc = 10, 4, 2, 32, 28
    with options(ctx, fold_over_int=fold):
        e, faces = make(ctx, d)
        ms, names = hfx.time_general_kernels([e], faces, 2)
        by = hfx.general_kernel_bytes([e])
        four = ["face_delta_kernel", "simplex2d_element_kernel", "face_flux2_kernel", "simplex2d_update_kernel"]
        assert e.simplex2d_over_int_plan() == expected_oi_plan(d, fold)
        if fold:
            assert names.split(",") == four and not any(ms[4:]) and not any(by[4:])
            assert by[1] == plain[1] + ne * 8.0 * (nd * nd * nc)
        else:
            assert names.split(",") == four + ["evaluate_invFlux_over_int"] and ms[4] > 0.0 and not any(ms[5:])
            assert by[1] == plain[1] + ne * 8.0 * (nu * nf * nd)
            assert by[4] == ne * 8.0 * (nu * nf + 2 * nc * nf + nc * nd * nd + 2 * nc * nf * nd + nu * nf * nd) and not any(by[5:])
        assert all(m > 0.0 for m in ms[1:4]) and by[3] == plain[3]
        close(e, faces)
