"""The LES closure on triangles on the device, against the genuine reference's fixtures under tests/golden/tris_les
(tools/capture_tris_les.py; tests/test_tris_les_oracle.py shows without a GPU that every input here is a sound one): the per-method
path, the 2-D simplex fused stage with the closure evaluated inside its element kernel (csrc/simplex2d.hip,
simplex2d_element_kernel_t<.., LES = true>: Fn carries F_sgs . n and no sgsf array is written), the partitioned loop, the deferred
call sequence, the refusals and a re-registration.

Bars, relative to the array's largest magnitude: TOL_U = 1e-11 for states after whole steps, as everywhere on triangles.  Every
fixture's state moves by more than 1e-7 when the closure is left out, so a stage that skips it cannot pass.  Every fused run asserts
hfx_simplex2d_les_plan and hfx_simplex2d_plan, that hfx.fused_launch_grids shows the stage's own two element launches and nothing
else, and that sgsf_upts / sgsf_fpts -- which only the per-method closure writes -- are still the zeros of the registration: a silent
per-method run cannot pass.

On the commit before the LES form every fused, partitioned and deferred test of this file fails at the refusal "a registered LES
closure runs per method (fused 0)" (the deferred ones: the record replays call by call); the per-method tests pass there.

The closure beside shock capturing: tl_p3_cylinder_shock, the shipped viscous cylinder keys + LES 1 through the genuine DRIVER
(state of its restart file, sensor of its Tecplot file; bar on the sensor 1e-9 of the largest).  "Smagorinsky without wall_distance" is refused by hfx_eles_set_les itself, before any stage."""
import numpy as np
import pytest

import hfx
import tri_util as T
import tri_shock_util as TS
import tri_les_util as TL
from test_gpu_tris import make, close, check_fpts_and_nan, expected_plan, SIZES
from test_gpu_deferred import calc_residual_calls, tag
from test_gpu_tris_shock import make_partitioned
from test_gpu_tris_partition import sub_table
from test_tris_partition_oracle import grow_parts, group_census, virtual_tables

pytestmark = pytest.mark.gpu

TOL_U = 1e-11
NAMES = TL.names()
relerr = T.relerr
DEFAULTS = {"gather_delta": 1, "persistent_grid_cap": 0}
PARTS = ([3, 2, 1], 3)  # (tests/test_tris_partition_oracle.py: VIRTUAL3)


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


def expected_les_plan(d):
    nu, nfp = int(d["sizes"][1]), int(d["sizes"][2])
    g = SIZES[(nu, nfp)][1]
    lds = 8 * (4 * nu * nu + 6 * nu * nfp + (g + 1) * (12 * nu + 4 * nfp))
    assert lds <= 80 * 1024
    m = TL.model(d)
    return {"les": int(m in (0, 1, 2, 4)), "sgs_model": m, "reads_leonard": int(m in (2, 4)),
            "launches_in_front": {-1: 0, 0: 0, 1: 0, 2: 5, 3: 3, 4: 5}[m], "element_lds": lds}


def n_groups_of(d):
    return -(-int(d["sizes"][0]) // SIZES[(int(d["sizes"][1]), int(d["sizes"][2]))][1])


def check_fused(e, d, cap=0, partitioned=False, deferred=False, gather=1):
    """the plans that ran, the stage's own launches alone, and no trace of the per-method closure.  hfx.fused_launch_grids records the
    stage's own persistent kernels only: it shows that the fused stage ran and launched nothing of slots 4 / 5, NOT that no per-method
    closure kernel ran beside it.  The zero check on sgsf_upts / sgsf_fpts (written by hfx_les_sgsf_upts_internal /
    hfx_eles_extrapolate_sgsFlux alone) is what shows that; keep it.  A deferred run cannot make it -- its stage marks both arrays
    stale and a read is refused -- and there deferred_stats (every stage fused, none replayed) is the guard"""
    assert e.simplex2d_les_plan() == expected_les_plan(d), e.simplex2d_les_plan()
    assert e.simplex2d_plan() == expected_plan(d, gather), e.simplex2d_plan()
    grids = hfx.fused_launch_grids(e.h)
    if not partitioned:
        ng = n_groups_of(d)
        assert [(s, w) for s, g, w in grids] == [(1, ng), (3, ng)], grids
        assert all(g == (min(ng, cap) if cap else ng) for s, g, w in grids), grids
    assert all(s in (1, 3) for s, g, w in grids), grids
    if TL.model(d) != 3 and not deferred:  # (a deferred stage marks what it does not write stale, which is refused before any read)
        assert not e.download(hfx.SGSF_UPTS).any() and not e.download(hfx.SGSF_FPTS).any()


def run(ctx, d, want, what, fused=4, cap=0):
    """one call of one step per entry of `want` (the state after that step, or None) -> the states"""
    e, faces = make(ctx, d)
    states = []
    for st, w in enumerate(want):
        hfx.run_steps_blocks([e], faces, 1, fused=fused)
        u = e.download(hfx.DISU_UPTS0)
        if w is not None:
            per_ele = np.abs(u - w).max(axis=(0, 2)) / np.abs(w).max()
            print("%s step %d: state %.2e (element %d of %d)" % (what, st + 1, per_ele.max(), int(per_ele.argmax()), len(per_ele)))
            assert per_ele.max() < TOL_U, (what, st, int(per_ele.argmax()), per_ele.max())
        if fused == 4:  # (the fused stage leaves disu_fpts of the new state; the per-method loop those of the last residual)
            check_fpts_and_nan(e, d, "%s step %d" % (what, st))
        assert e.check_nan() == -1, what
        states.append(u)
    if fused == 4:
        check_fused(e, d, cap)
    close(e, faces)
    return states


# ---- 1. every fixture: per method, fused, fused again, without the gather -----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_per_method(ctx, name):
    d = TL.load(name)
    run(ctx, d, TL.fixture_states(d), name + " per method", fused=0)


@pytest.mark.parametrize("name", NAMES)
def test_fused(ctx, name):
    """fused 4, the closure inside the element kernel; launched twice, the results agree bit for bit; gather_delta 0 meets the bar too"""
    d = TL.load(name)
    a = run(ctx, d, TL.fixture_states(d), name + " fused")
    b = run(ctx, d, TL.fixture_states(d), name + " fused again")
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    with options(ctx, gather_delta=0):
        e, faces = make(ctx, d)
        for st, w in enumerate(TL.fixture_states(d)):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            if w is not None:
                err = relerr(e.download(hfx.DISU_UPTS0), w)
                print("%s gather_delta 0 step %d: %.2e" % (name, st + 1, err))
                assert err < TOL_U
        assert e.simplex2d_les_plan() == expected_les_plan(d)
        assert e.simplex2d_plan() == expected_plan(d, gather=0)
        close(e, faces)


# ---- 2. group edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("name,n", TL.order_blocks())
def test_group_edges(ctx, name, n, cap):
    """G - 1, G, G + 1 and 2 G + 1 elements at every order against the oracle on the same block; cap 1: ONE workgroup walks all groups"""
    d = TL.block(n, name)
    ref = TL.block_reference("%s %d" % (name, n), d)
    with options(ctx, persistent_grid_cap=cap):
        run(ctx, d, [r["u"] for r in ref], "%s block of %d (cap %d)" % (name, n, cap), cap=cap)


@pytest.mark.parametrize("cap", [0, 1])
def test_group_edges_similarity(ctx, cap):
    """2 G + 1 elements of tl_p3_wsm: Lu / Le are read with e0 > 0"""
    n = 2 * T.GROUP[3] + 1
    d = TL.similarity_block()
    ref = TL.block_reference("tl_p3_wsm %d" % n, d)
    with options(ctx, persistent_grid_cap=cap):
        run(ctx, d, [r["u"] for r in ref], "tl_p3_wsm block of %d (cap %d)" % (n, cap), cap=cap)


# ---- 3. the partitioned loop ---------------------------------------------------------------------------------------------------------
def partition_case(name):
    """-> (block, virtual parts, the states to meet): the cylinder as it is against its fixture; a 32-element fixture tiled to three
    groups, the first copy cut into three parts, against the oracle on the tiled block"""
    if name == TL.CYLINDER:
        d = TL.load(name)
        return d, grow_parts(d, *TS.PARTS["ts_p3_cylinder"]), TL.fixture_states(d)
    d = TL.tiled(name)
    ne = int(TL.load(name)["sizes"][0])
    part = np.zeros(int(d["sizes"][0]), dtype=np.int64)
    part[:ne] = grow_parts(TL.load(name), *PARTS)
    return d, part, [r["u"] for r in TL.block_reference(name + " tiled", d)]


def run_partitioned(ctx, comm, d, e, faces, M, L, want, what, gather=1):
    for st, w in enumerate(want):
        hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1)
        if w is not None:
            err = relerr(e.download(hfx.DISU_UPTS0), w)
            print("%s step %d: %.2e" % (what, st + 1, err))
            assert err < TOL_U, (what, st, err)
        check_fpts_and_nan(e, d, what)
    n_part, n_int, _, _ = group_census(d, L)
    pp = e.simplex2d_partition_plan()
    assert (pp["partition_groups"], pp["interior_groups"]) == (n_part, n_int) and n_part > 0 and n_int > 0, pp
    check_fused(e, d, partitioned=True, gather=gather)
    return pp


@pytest.mark.parametrize("gather", [1, 0])
@pytest.mark.parametrize("name", ["tl_p3_wale", "tl_p3_wsm", "tl_p3_smag_walls", "tl_p3_cylinder"])
def test_partitioned_loop(ctx, comm, name, gather):
    """hfx_run_steps_partitioned_blocks on virtual parts, ONE partition-face block: the partners of partition points gathered from the
    receive record (gather 1) or their corrections written by mpi_delta_kernel<2>; what the faces send is Fn with the SGS part"""
    d, part, want = partition_case(name)
    with options(ctx, gather_delta=gather):
        e, faces, M, L = make_partitioned(ctx, d, part)
        pp = run_partitioned(ctx, comm, d, e, faces, M, L, want, "%s partitioned (gather %d)" % (name, gather), gather)
        assert pp["gather_remote"] == gather
        close(e, faces + M)


@pytest.mark.parametrize("name", ["tl_p3_wale", "tl_p3_wsm"])
def test_partitioned_loop_two_face_blocks(ctx, comm, name):
    """the same cut registered as TWO partition-face blocks: the partition points take their corrections from mpi_delta_kernel<2>"""
    d, part, want = partition_case(name)
    reg, L, Rlut, seg = virtual_tables(d, part)
    assert len(seg) == 6
    mates = [s for s in range(6) if seg[s][1] in (seg[0][1], seg[0][2])]
    others = [s for s in range(6) if s not in mates]
    e, faces = make(ctx, reg)
    M = []
    for pick in (mates, others):
        Ls, Rs, segs = sub_table(L, Rlut, seg, pick)
        M.append(hfx.MpiInters(ctx, e, Ls, Rs))
        M[-1].set_neighbours(segs)
    pp = run_partitioned(ctx, comm, d, e, faces, M, L, want, name + ", two partition-face blocks")
    assert pp["gather_remote"] == 0
    close(e, faces + M)


def refused(run_it, e, match):
    before = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match=match) as err:
        run_it()
    assert "fused 0" in str(err.value), str(err.value)
    assert np.array_equal(e.download(hfx.DISU_UPTS0), before)


def test_svv_partitioned_is_refused(ctx, comm):
    d, part, _ = partition_case("tl_p3_svv")
    e, faces, M, L = make_partitioned(ctx, d, part)
    refused(lambda: hfx.run_steps_partitioned_blocks([e], faces, M, comm, 1), e, "SVV")
    close(e, faces + M)


# ---- 4. the deferred call sequence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tl_p3_wale", "tl_p3_wsm", "tl_p3_smag_walls"])
def test_deferred_call_sequence(name):
    """the reference's calls with `deferred` 1, calc_sgs_terms and extrapolate_sgsFlux recorded: every stage runs the 2-D simplex stage"""
    d = TL.load(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = make(c, d)
    tag(e, d)
    assert e.les_model == TL.model(d)
    want = TL.fixture_states(d)
    for st, w in enumerate(want):
        for rk in range(nstage):
            calc_residual_calls([e], faces, True, rk)
            e.AdvanceSolution(rk, adv)
        err = relerr(e.download(hfx.DISU_UPTS0), w)
        print("%s deferred step %d: %.2e" % (name, st + 1, err))
        assert err < TOL_U, (name, st)
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (len(want) * nstage, 0), (nf, nr, why)
    check_fused(e, d, deferred=True)
    close(e, faces)
    c.close()


def test_deferred_without_extrapolate_sgsFlux_stays_replayed():
    """a record without extrapolate_sgsFlux on a block with a closure is replayed call by call"""
    d = TL.load("tl_p3_wale")
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = make(c, d)
    tag(e, d)
    e.les_model = None  # (calc_residual_calls then leaves the closure's calls out)
    for rk in range(nstage):
        calc_residual_calls([e], faces, True, rk)
        e.AdvanceSolution(rk, adv)
    e.download(hfx.DISU_UPTS0)
    nf, nr, why = c.deferred_stats()
    assert nf == 0 and nr > 0 and "extrapolate_sgsFlux" in why, (nf, nr, why)
    close(e, faces)
    c.close()


def test_partitioned_deferred_call_sequence():
    """the reference's calls with send_* / receive_* (those of the SGS flux among them) on a partitioned block, `deferred` 1"""
    name = "tl_p3_wsm"
    d, part, want = partition_case(name)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    c = hfx.Context(0)
    e, faces, M, L = make_partitioned(c, d, part)
    comm = hfx.Comm(c.h, hfx.comm_unique_id(), 1, 0)
    c.set_option("deferred", 1)
    ints = [f for f in faces if isinstance(f, hfx.IntInters)]
    bdys = [f for f in faces if isinstance(f, hfx.BdyInters)]
    for st, w in enumerate(want):
        for rk in range(nstage):  # CalcResidual's order with the partition-face calls (src/solver.cpp:55-221)
            if rk == 0:
                e.calc_sgs_terms()
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
            e.extrapolate_sgsFlux()
            for f in M: f.send_sgsf_fpts(comm)
            e.extrapolate_totalFlux()
            e.calculate_divergence()
            for f in ints: f.calculate_common_viscFlux()
            for f in bdys: f.evaluate_boundaryConditions_viscFlux()
            for f in M: f.receive_corrected_gradient(comm)
            for f in M: f.receive_sgsf_fpts(comm)
            for f in M: f.calculate_common_viscFlux()
            e.calculate_corrected_divergence()
            e.AdvanceSolution(rk, adv)
        err = relerr(e.download(hfx.DISU_UPTS0), w)
        print("%s partitioned, deferred step %d: %.2e" % (name, st + 1, err))
        assert err < TOL_U, st
    nf, nr, why = c.deferred_stats()
    assert (nf, nr) == (len(want) * nstage, 0), (nf, nr, why)
    check_fused(e, d, partitioned=True, deferred=True)
    assert e.check_nan() == -1
    comm.close()
    close(e, faces + M)
    c.close()


# ---- 5. the closure beside shock capturing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold_shock", [1, 0])
def test_with_shock_capturing(ctx, fold_shock):
    """tl_p3_cylinder_shock: the LES element kernel and the SHOCK update kernel in one stage (fold_shock 0: the filter behind the stage),
    state and sensor after both steps against the genuine driver's files and the oracle with both ingredients"""
    from test_gpu_tris_shock import check_step, expected_shock_plan
    d, ref = TL.load_shock(), TL.shock_reference()
    ctx.set_option("fold_shock", fold_shock)
    try:
        e, faces = make(ctx, d)
        for st in range(TS.n_steps_of(d)):
            hfx.run_steps_blocks([e], faces, 1, fused=4)
            check_step(e, d, ref, st, "tl_p3_cylinder_shock (fold_shock %d)" % fold_shock)
            check_fpts_and_nan(e, d, TL.SHOCK)
        assert e.simplex2d_les_plan() == expected_les_plan(d) and e.simplex2d_plan() == expected_plan(d)
        assert e.simplex2d_shock_plan() == expected_shock_plan(d, fold_shock)
        grids = hfx.fused_launch_grids(e.h)
        assert [(s, w) for s, g, w in grids][:2] == [(1, n_groups_of(d)), (3, n_groups_of(d))], grids
        assert not e.download(hfx.SGSF_UPTS).any() and not e.download(hfx.SGSF_FPTS).any()
        close(e, faces)
    finally:
        ctx.set_option("fold_shock", 1)


def test_with_shock_capturing_per_method(ctx):
    """the same fixture through fused 0: what ran for the pair before"""
    from test_gpu_tris_shock import check_step
    d, ref = TL.load_shock(), TL.shock_reference()
    e, faces = make(ctx, d)
    for st in range(TS.n_steps_of(d)):
        hfx.run_steps_blocks([e], faces, 1, fused=0)
        check_step(e, d, ref, st, "tl_p3_cylinder_shock per method")
    assert e.check_nan() == -1
    close(e, faces)


# ---- 7. one duty: the stage the step loop runs call by call keeps the per-method closure ----------------------------------------------
def test_history_rows_with_wall_forces():
    """residuals and viscous wall forces sampled after both steps of tl_p3_smag_walls: the forces read the gradient, so every sampled
    step's LAST stage runs call by call (with hfx_eles_extrapolate_sgsFlux and the face kernels' sgsf terms) behind fused LES stages.
    The fused-4 rows equal the fused-0 rows at the bars of tests/test_gpu_history_rows.py: 1e-11 on a residual, 1e-11 of the row's
    largest on the forces"""
    import full_loop_util as FU
    d = TL.load(TL.WALLS)
    A = FU.fixture_device_arrays(d)
    assert len(A["face_ele"]) == 8  # (four cells along each wall)
    rows = {}
    for fused in (0, 4):
        c = hfx.Context(0)
        e, faces = make(c, d)
        c.set_force_reference(*[TL.scalar(d, k) for k in ("rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic", "area_ref")])
        e.set_wall_faces(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"])
        c.set_history_monitor(2, True, 1, capacity=2)
        c.set_clock(0.0, 0)
        hfx.run_steps_blocks([e], faces, 2, fused=fused)
        u = e.download(hfx.DISU_UPTS0)
        assert relerr(u, TL.fixture_states(d)[1]) < TOL_U, fused
        if fused == 4:
            assert e.simplex2d_les_plan() == expected_les_plan(d) and e.simplex2d_plan() == expected_plan(d)
        rows[fused] = e.read_history()
        close(e, faces)
        c.close()
    (t0, s0, r0, f0), (t4, s4, r4, f4) = rows[0], rows[4]
    assert list(s0) == [1, 2] and list(s4) == [1, 2] and np.array_equal(t0, t4)
    res = np.abs(r4 - r0).max() / np.abs(r0).min()
    frc = (np.abs(f4 - f0).max(axis=0) / np.abs(f0).max(axis=0)).max()
    print("history rows fused 4 against fused 0: residuals %.2e, forces %.2e (viscous part %.2e of the row)"
          % (res, frc, np.abs(f0[2:4]).max() / np.abs(f0).max()))
    assert np.all(np.abs(r4 - r0) <= 1e-11 * np.abs(r0)) and frc <= 1e-11
    assert np.abs(f0[2:4]).max() > 0.0  # (the viscous forces are there)


# ---- 6. refusals, re-registration, queries -------------------------------------------------------------------------------------------
def les_args(d):
    sc = lambda k: TL.scalar(d, k)
    return int(sc("SGS_model")), sc("C_s"), sc("filter_ratio"), sc("Kappa"), sc("prandtl_t")


def test_refusals(ctx):
    """each before the first launch, naming the LES closure and fused 0, the state untouched"""
    d = TL.load("tl_p3_wale")
    J = np.asarray(d["Jacobian_fpts"])
    go = lambda e, faces: (lambda: hfx.run_steps_blocks([e], faces, 1, fused=4))
    # a Jacobian that is not the block's own: all ones, one entry of one flux point off by 1e-6 of the largest, the neighbour element's
    one = 1e-6 * np.abs(J).max() * (np.arange(J.size).reshape(J.shape, order="F") == 5)
    for bad in (np.ones_like(J), J + one, np.roll(J, 1, axis=3)):
        assert TL.jacobian_residual(bad, d) > 1e-8  # (the stage's bar is 1e-9)
        e, faces = make(ctx, TL.without_les(d))
        e.set_les(*les_args(d), np.asfortranarray(bad))
        refused(go(e, faces), e, "LES closure")
        close(e, faces)
    # an inviscid context (the closure was registered while it was viscous)
    c = hfx.Context(0)
    e, faces = make(c, d)
    p = hfx.params_from(d)
    p.viscous = 0
    c.set_params(p)
    refused(go(e, faces), e, "LES closure")
    close(e, faces)
    c.close()
    # beside over-integration
    import tri_overint_util as TO
    o = TO.load("to_p3")
    e, faces = make(ctx, o)
    e.set_les(*les_args(d), d["Jacobian_fpts"])
    refused(go(e, faces), e, "LES closure")
    close(e, faces)
    # beside a conforming shock registration the closure is taken (test_with_shock_capturing); with a Jacobian that is not the
    # block's own it stays refused there too
    s = TS.load("ts_p3_n4")
    e, faces = make(ctx, s)
    e.set_les(*les_args(d), np.ones_like(J))
    refused(go(e, faces), e, "LES closure")
    close(e, faces)
    # Smagorinsky without wall_distance: the registration itself refuses it, and the block then runs without a closure
    e, faces = make(ctx, TL.without_les(d))
    with pytest.raises(hfx.HfxError, match="wall_distance"):
        e.set_les(0, 0.17, 1.5, 0.41, 0.9, d["Jacobian_fpts"])
    close(e, faces)
    # a similarity closure without filter_upts
    w = TL.load("tl_p3_wsm")
    e, faces = make(ctx, TL.without_les(w))
    e.set_les(*les_args(w), w["Jacobian_fpts"])
    refused(go(e, faces), e, "LES closure")
    close(e, faces)


def test_a_second_registration_gets_fresh_tables(ctx):
    """WALE, one step; then damped Smagorinsky on the same block: the stage runs the second registration's length scale"""
    d = TL.load(TL.WALLS)
    wale = dict(d)
    wale["SGS_model"], wale["C_s"], wale["filter_ratio"] = np.array([1]), np.array([0.325]), np.array([1.0])
    del wale["wall_distance"]
    ref_wale = TL.block_reference("walls as wale", wale)
    e, faces = make(ctx, wale)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), ref_wale[0]["u"]) < TOL_U
    assert e.simplex2d_les_plan() == expected_les_plan(wale)
    e.set_les(*les_args(d), d["Jacobian_fpts"], d["wall_distance"])
    e.upload(hfx.DISU_UPTS0, d["u_init"])
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    err = relerr(e.download(hfx.DISU_UPTS0), TL.fixture_states(d)[0])
    print("re-registered: %.2e; the two closures differ by %.2e" % (err, relerr(ref_wale[0]["u"], TL.fixture_states(d)[0])))
    assert err < TOL_U and relerr(ref_wale[0]["u"], TL.fixture_states(d)[0]) > 1e3 * TOL_U
    assert e.simplex2d_les_plan() == expected_les_plan(d)
    close(e, faces)


def test_plan_is_refused_before_a_fused_call(ctx):
    e, faces = make(ctx, TL.load("tl_p1_wale"))
    with pytest.raises(hfx.HfxError, match="no 2-D simplex fused stage has prepared"):
        e.simplex2d_les_plan()
    close(e, faces)


def test_a_block_without_a_closure_runs_the_old_kernel(ctx):
    d = T.load("tri_p3_n4_deformed")
    e, faces = make(ctx, d)
    hfx.run_steps_blocks([e], faces, 1, fused=4)
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage4"]) < TOL_U
    assert e.simplex2d_plan() == expected_plan(d)
    assert e.simplex2d_les_plan() == expected_les_plan(d)
    close(e, faces)


@pytest.mark.parametrize("name", ["tl_p3_wale", "tl_p3_wsm"])
def test_byte_query(ctx, name):
    """the element kernel's added reads: len2 8 B per solution point, tdA_fpts 8 B per flux point, Lu / Le 40 B for the similarity models"""
    d = TL.load(name)
    eb, fb = make(ctx, TL.without_les(d))
    hfx.run_steps_blocks([eb], fb, 0, fused=4)
    plain = hfx.general_kernel_bytes([eb])
    close(eb, fb)
    nu, nfp, ne = int(d["sizes"][1]), int(d["sizes"][2]), int(d["sizes"][0])
    e, faces = make(ctx, d)
    hfx.run_steps_blocks([e], faces, 0, fused=4)
    by = hfx.general_kernel_bytes([e])
    assert by[1] == plain[1] + ne * (8.0 * nu + 8.0 * nfp + (40.0 * nu if TL.model(d) in (2, 4) else 0.0))
    assert [by[i] for i in (0, 2, 3)] == [plain[i] for i in (0, 2, 3)] and not any(by[4:])
    close(e, faces)
