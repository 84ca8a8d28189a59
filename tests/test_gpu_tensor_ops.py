"""The sum-factorised over-integration and shock-capturing kernels (csrc/tensor_ops.hip) at EVERY instantiated size.

overint_tensor_kernel<ND, N, NC, FOLD> has 70 size pairs in two forms, shock_tensor_kernel<ND, N> ten sizes; the fixtures of the
genuine reference reach a handful.  Here every size runs on the device, through the raw C ABI, on blocks of 27 hexahedra / 16
quadrilaterals whose elements -- and whose points -- all have metrics of their own, and is held against a numpy longdouble
reference made from the dense registered matrices alone (tests/tensor_ops_util.py; tests/test_tensor_ops_host.py shows that this
reference agrees with the oracle and the fixtures, and that every mistake these kernels can make moves it by far more than a
bar).  Whole stages are held against the oracle in lockstep.  Every test asserts from hfx_eles_tensor_ops_plan WHICH form ran: a
kron_factor that began to refuse a size would otherwise cost the benchmark and no test.

Bars: those of the files that pin these kernels at the fixtures' sizes -- RTOL1 of tests/test_gpu_methods_vs_golden.py for one
operation (1e-12 of the array's largest magnitude), 1e-9 and equal flags for the sensor, TOL_ORACLE of
tests/test_gpu_persistent_loops.py for the state after a step.  A capped run (option persistent_grid_cap: workgroups walk several
elements, the prefetch of the next element runs) equals the uncapped run of the same form bit for bit."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import hfx
import reorient as RO
import tensor_ops_util as T
from test_gpu_methods_vs_golden import RTOL1, build
from test_gpu_persistent_loops import ELEMENT, OVER_INT, SHOCK, TOL_ORACLE, UPDATE

pytestmark = pytest.mark.gpu

LD = T.LD
DEFAULTS = {"persistent_grid_cap": 0, "tensor_ops": 1, "over_int_fold": 1}


@pytest.fixture(scope="module")
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def stop_after_a_device_error(ctx):
    """162 tests launch kernels at sizes nothing launched before: an error of the device ends the session, nothing more is started"""
    yield
    try:
        ctx.synchronize()
    except hfx.HfxError as err:
        pytest.exit("device error, no further launches: %s" % err, returncode=3)


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


@contextlib.contextmanager
def block(ctx, reg, mode=hfx.CONTRACT_AUTO):
    e, faces = build(ctx, T.solver_keys(reg), mode)
    try:
        yield e, faces
    finally:
        for f in faces:
            f.close()
        e.close()
        ctx.set_contract_mode(hfx.CONTRACT_AUTO)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- 1. the over-integration kernel, every size ------------------------------------------------------------------------------------

# (form, contraction mode, options) -> what the plan must say ran
OVER_INT_FORMS = [("sum-factorised", hfx.CONTRACT_AUTO, {"persistent_grid_cap": 2}, 1),
                  ("dense (CONTRACT_DENSE)", hfx.CONTRACT_DENSE, {}, 0),
                  ("dense (tensor_ops 0)", hfx.CONTRACT_AUTO, {"tensor_ops": 0}, 0)]


@pytest.mark.parametrize("dims,N,Nc", T.OVER_INT_SIZES)
def test_over_integration_every_size(ctx, dims, N, Nc):
    """evaluate_invFlux_over_int at (ND, N, Nc): the sum-factorised kernel with two workgroups over 27 / 16 elements (14 and 13,
    or 8 and 8 trips: the prefetched state and metrics of every element but a workgroup's first), and the dense form twice --
    asked for through the contraction mode and through option tensor_ops -- against ref_over_int"""
    reg = T.registration(dims, N - 1, Nc - 1)
    want = f64(T.ref_over_int(reg, reg["u_init"]))
    for form, mode, opts, ran in OVER_INT_FORMS:
        with options(ctx, **opts), block(ctx, reg, mode) as (e, faces):
            before = e.tensor_ops_plan()
            e.evaluate_invFlux_over_int()
            got = e.download(hfx.TDISF_UPTS)
            plan = e.tensor_ops_plan()
        err = T.relerr(got, want)
        print("over-integration %d-D N %d Nc %d %s: plan %s, vs longdouble %.3g" % (dims, N, Nc, form, plan, err))
        assert before["over_int_ran"] == -1 and (plan["over_int"], plan["N"], plan["Nc"]) == (1, N, Nc), (form, before, plan)
        assert plan["over_int_ran"] == ran and plan["shock"] == 0 and plan["shock_ran"] == -1, (form, plan)
        assert err < RTOL1, form


# ---- 2. the shock-capturing kernel, every size -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cutoff", [0, 1])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("dims,N", T.SHOCK_SIZES)
def test_shock_capture_every_size(ctx, dims, N, field, cutoff):
    """shock_capture() at (ND, N) on the spread state, density and energy sensor, the shipped filter with cutoff 0 and 1, one
    element per workgroup and two workgroups over all elements; the dense form under the same checks"""
    reg = T.registration(dims, N - 1, None, dict(T.FILTER, shock_det_field=field, expf_cutoff=cutoff))
    u = T.spread_sensors(reg, T.SEED)
    s0 = T.pick_s0(T.ref_sensor(reg, u))
    reg = dict(T.with_s0(reg, s0), u_init=u)
    want_s, want_u = T.ref_shock(reg, u)
    hit = f64(want_s) >= s0
    assert T.quarter_each_way(f64(want_s), s0) and T.clear_of_s0(f64(want_s), s0)
    for form, mode, ran in (("sum-factorised", hfx.CONTRACT_AUTO, 1), ("dense", hfx.CONTRACT_DENSE, 0)):
        for cap in (0, 2):
            with options(ctx, persistent_grid_cap=cap), block(ctx, reg, mode) as (e, faces):
                e.shock_capture()
                sens, got = e.download(hfx.SENSOR), e.download(hfx.DISU_UPTS0)
                plan = e.tensor_ops_plan()
            es, eu = T.relerr(sens, f64(want_s)), T.relerr(got[:, hit], f64(want_u)[:, hit])
            print("shock capturing %d-D N %d field %d cutoff %d %s cap %d: plan %s, sensor %.3g, filtered %.3g" %
                  (dims, N, field, cutoff, form, cap, plan, es, eu))
            assert (plan["shock"], plan["shock_N"], plan["shock_ran"]) == (1, N, ran), (form, plan)
            assert plan["over_int"] == 0 and plan["over_int_ran"] == -1
            assert es < 1e-9 and np.array_equal(sens >= s0, hit), (form, cap)
            assert eu < 1e-12, (form, cap)
            assert np.array_equal(got[:, ~hit], u[:, ~hit]), (form, cap)  # (untouched: bit for bit)


# ---- 3. inside the stage -------------------------------------------------------------------------------------------------------------

STAGE_CASES = [(dims, N, Nc) for dims in (2, 3) for (N, Nc) in T.STAGE_SIZES[dims]]


def stage_can_fold(dims, N):
    """Does the split stage take the de-aliased flux folded into the divergence on a block of the HOST MIRROR at this size?  It does
    where its loader-wave flux kernel runs (split_plan, csrc/fused_hex.hip).  Not at
      - P5 hexahedra: two workgroups of that kernel's LDS image (126 KiB each at 216 + 216 points) do not fit a CU
        (loader_wave_fits, csrc/split3_kernels.hpp);
      - P2, either dimension: the mirror's three Gauss points are symmetric to the bit, the middle row of its 1-D derivative matrix
        has an exact zero, the ELL form of opp_2 drops it, and tensor_build (csrc/fused_hex.hip) finds a row of 2 entries where
        it looks for 3 -- no tensor tables, the dictionary-row flux kernel runs.  (The genuine reference's P2 nodes are not
        symmetric to the bit, its middle node is -4.5e-17: every row of opp_2 in hex_p2_overint has three entries.)
    There the stage runs the sum-factorised over-integration kernel unfolded, which is what the tests assert."""
    return N != 3 and not (dims == 3 and N == 6)


def run_stage(ctx, reg, fold, cap):
    """two steps of hfx_run_steps(fused=3), one call each: dict of u and sensor after each step, disu_fpts at the end, the plan, the
    over-integration kernel's algorithmic bytes and the launch grids"""
    out = dict(u=[], sensor=[])
    with options(ctx, over_int_fold=fold, persistent_grid_cap=cap), block(ctx, reg) as (e, faces):
        for _ in range(T.STAGE_STEPS):
            hfx.run_steps(e, faces, 1, fused=3)
            out["u"].append(e.download(hfx.DISU_UPTS0))
            if "shock_cap" in reg:
                out["sensor"].append(e.download(hfx.SENSOR))
        out["disu_fpts"] = e.download(hfx.DISU_FPTS)
        out["nan"] = e.check_nan()
        out["plan"] = e.tensor_ops_plan()
        b = (C.c_double * 8)()
        hfx.check(hfx.lib().hfx_fused_kernel_bytes(e.h, b))
        out["bytes"] = list(b)
        out["grids"] = hfx.fused_launch_grids(e.h)
    return out


def check_stage(reg, u0, want, got, over_int, shock, fold, cap, tol=TOL_ORACLE):
    sz = [int(v) for v in reg["sizes"]]
    ne, nu, nfp, nf, nd = sz[:5]
    plan = got["plan"]
    assert got["nan"] == -1
    for st in range(T.STAGE_STEPS):
        assert T.relerr(got["u"][st], want["u"][st]) < tol, st
        if shock:
            s0 = float(reg["s0"][0])
            assert np.array_equal(got["sensor"][st] >= s0, want["sensors"][st, -1] >= s0), st
            assert T.relerr(got["sensor"][st], want["sensors"][st, -1]) < 1e-9, st
    fp = f64(np.asarray(reg["opp_0"], dtype=LD) @ np.asarray(got["u"][-1], dtype=LD).reshape(nu, ne * nf, order="F")).reshape(
        (nfp, ne, nf), order="F")
    assert T.relerr(got["disu_fpts"], fp) < 1e-12
    slots = {ELEMENT, UPDATE}
    if over_int:
        slots.add(OVER_INT)
        ncub = reg["opp_over_int_cubpts"].shape[0]
        per_point = got["bytes"][4] / (8.0 * ne) - nu * nf - nd * nd * ncub  # what the kernel writes per element
        assert plan["over_int"] == 1 and plan["over_int_ran"] == 1, plan
        if not fold:
            assert plan["folded"] == 0, plan
        # folded: n_fields values per solution point; unfolded (asked for, or the stage cannot fold at this size): n_fields * n_dims
        assert per_point == (nu * nf if plan["folded"] else nu * nf * nd), (plan, per_point)
    else:
        assert plan["over_int"] == 0 and plan["over_int_ran"] == -1 and got["bytes"][4] == 0.0, plan
    if shock:
        slots.add(SHOCK)
        assert plan["shock"] == 1 and plan["shock_ran"] == 1, plan
    else:
        assert plan["shock"] == 0 and plan["shock_ran"] == -1, plan
    assert {s for s, _, _ in got["grids"]} == slots, got["grids"]
    for slot, grid, work in got["grids"]:
        assert work == ne and grid == (min(ne, cap) if cap else ne), (got["grids"], cap)


@pytest.mark.parametrize("ingredients", ["over_int", "shock", "both"])
@pytest.mark.parametrize("dims,N,Nc", STAGE_CASES)
def test_stage_every_corner(ctx, dims, N, Nc, ingredients):
    """hfx_run_steps(fused=3) for two steps with over-integration (folded into the divergence and not), shock capturing, and
    both, at the corners and through the middle of the table, uncapped and at caps 2 and 3: the state and the sensors' flags
    against the oracle in lockstep after each step, disu_fpts against opp_0 u (the shock kernel rewrites the flux points of the
    elements it filters), the form from the plan query and from hfx_fused_kernel_bytes, the capped runs against the uncapped one
    bit for bit"""
    over_int, shock = ingredients != "shock", ingredients != "over_int"
    reg, u0 = T.stage_case(dims, N, Nc, over_int, shock)
    want = T.stage_oracle(dims, N, Nc, over_int, shock)
    reg = dict(reg, u_init=u0)
    folded = {}
    for fold in ((1, 0) if over_int else (1,)):
        free = None
        for cap in (0, 2, 3):
            got = run_stage(ctx, reg, fold, cap)
            print("stage %d-D N %d Nc %d %s fold %d cap %d: plan %s, grids %s, vs oracle %s" %
                  (dims, N, Nc, ingredients, fold, cap, got["plan"], got["grids"],
                   ["%.3g" % T.relerr(got["u"][st], want["u"][st]) for st in range(T.STAGE_STEPS)]))
            check_stage(reg, u0, want, got, over_int, shock, fold, cap)
            if cap == 0:
                free = got
            else:
                for st in range(T.STAGE_STEPS):
                    assert np.array_equal(got["u"][st], free["u"][st]), (fold, cap, st)
                    if shock:
                        assert np.array_equal(got["sensor"][st], free["sensor"][st]), (fold, cap, st)
        folded[fold] = free["plan"]["folded"]
    if over_int:
        assert folded == {1: int(stage_can_fold(dims, N)), 0: 0}, folded


# ---- 4. what kron_factor must refuse and must accept -----------------------------------------------------------------------------------

KRON_CASES = [(3, 3, 4), (2, 4, 5)]  # hexahedra P2 / Nc 4, quadrilaterals P3 / Nc 5


def factor_1d(M, nd, nr1, nc1):
    """the 1-D matrix whose Kronecker power M is, read off its first block (first direction fastest in rows and columns)"""
    a00 = abs(M[0, 0]) ** (1.0 / nd) * (np.sign(M[0, 0]) if nd == 3 else 1.0)
    return np.array([[M[i, j] for j in range(nc1)] for i in range(nr1)]) / a00 ** (nd - 1)


def kron_chain(mats):
    """first matrix along the first (fastest) direction"""
    out = mats[0]
    for m in mats[1:]:
        out = np.kron(m, out)
    return out


def run_over_int(ctx, reg):
    with block(ctx, reg) as (e, faces):
        e.evaluate_invFlux_over_int()
        return e.download(hfx.TDISF_UPTS), e.tensor_ops_plan()


def run_shock(ctx, reg):
    with block(ctx, reg) as (e, faces):
        e.shock_capture()
        return e.download(hfx.SENSOR), e.download(hfx.DISU_UPTS0), e.tensor_ops_plan()


def bumped(M, rel):
    """M with one entry (an interior one, not the pivot kron_factor reads the factors from) changed by rel of the matrix scale"""
    out = np.array(M, order="F")
    out[out.shape[0] // 2, out.shape[1] // 2 + 1] += rel * np.abs(M).max()
    return out


@pytest.mark.parametrize("dims,N,Nc", KRON_CASES)
def test_kron_factor_refuses_and_accepts_over_integration(ctx, dims, N, Nc):
    reg = T.registration(dims, N - 1, Nc - 1)
    opp, filt = np.asarray(reg["opp_over_int_cubpts"]), np.asarray(reg["over_int_filter"])
    F1 = factor_1d(filt, dims, N, Nc)
    assert np.abs(kron_chain([F1] * dims) - filt).max() < 1e-13 * np.abs(filt).max()
    B = F1.copy()
    B[0, 1] *= 1.1  # (not a multiple of F1)
    cases = [("one entry of over_int_filter off by 1e-9", dict(over_int_filter=bumped(filt, 1e-9)), 0),
             ("off by 1e-14", dict(over_int_filter=bumped(filt, 1e-14)), 1),
             ("A (x) B in place of a Kronecker power", dict(over_int_filter=kron_chain([F1, B] + [F1] * (dims - 2))), 0),
             # (-A) (x) (-A) = A (x) A: no real 1-D matrix has -M as its square; it has a real cube root
             ("both matrices negated", dict(over_int_filter=-filt, opp_over_int_cubpts=-opp), 1 if dims == 3 else 0)]
    for what, change, factored in cases:
        r = dict(reg, **change)
        want = f64(T.ref_over_int(r, r["u_init"]))
        got, plan = run_over_int(ctx, r)
        err = T.relerr(got, want)
        print("%d-D N %d Nc %d, %s: plan %s, vs longdouble %.3g" % (dims, N, Nc, what, plan, err))
        assert (plan["over_int"], plan["over_int_ran"]) == (factored, factored), (what, plan)
        assert err < RTOL1, what


@pytest.mark.parametrize("dims,N,Nc", KRON_CASES)
def test_kron_factor_refuses_and_accepts_shock_capturing(ctx, dims, N, Nc):
    reg = T.registration(dims, N - 1, None, dict(T.FILTER))
    u = T.spread_sensors(reg, T.SEED)
    reg = dict(T.with_s0(reg, T.pick_s0(T.ref_sensor(reg, u))), u_init=u)
    E = np.asarray(reg["exp_filter"])
    E1 = factor_1d(E, dims, N, N)
    assert np.abs(kron_chain([E1] * dims) - E).max() < 1e-13 * np.abs(E).max()
    B = E1.copy()
    B[0, 1] += 0.1
    cases = [("one entry of exp_filter off by 1e-9", bumped(E, 1e-9), 0), ("off by 1e-14", bumped(E, 1e-14), 1),
             ("A (x) B in place of a Kronecker power", kron_chain([E1, B] + [E1] * (dims - 2)), 0)]
    for what, Em, factored in cases:
        r = dict(reg, exp_filter=Em)
        want_s, want_u = T.ref_shock(r, u)
        hit = f64(want_s) >= float(r["s0"][0])
        sens, got, plan = run_shock(ctx, r)
        print("%d-D N %d, %s: plan %s, sensor %.3g, filtered %.3g" % (dims, N, what, plan, T.relerr(sens, f64(want_s)),
                                                                       T.relerr(got[:, hit], f64(want_u)[:, hit])))
        assert (plan["shock"], plan["shock_ran"]) == (factored, factored), (what, plan)
        assert T.relerr(sens, f64(want_s)) < 1e-9 and np.array_equal(sens >= float(r["s0"][0]), hit)
        assert T.relerr(got[:, hit], f64(want_u)[:, hit]) < 1e-12, what
        assert np.array_equal(got[:, ~hit], u[:, ~hit])


@pytest.mark.parametrize("dims,N,Nc", KRON_CASES + [(3, 4, 5)])
def test_registering_another_size_rebuilds_the_factors(ctx, dims, N, Nc):
    """a block that ran with Nc + 2 cubature points per direction, registered again with Nc: the per-method call and the stage (the
    folded matrices are made from the new factors) give the bits of a fresh block with Nc.  (P3 hexahedra beside the two sizes
    of this section: the mirror's P2 blocks do not fold, stage_can_fold)"""
    can_fold = int(stage_can_fold(dims, N))
    first, second = T.registration(dims, N - 1, Nc + 1), T.registration(dims, N - 1, Nc - 1)
    with block(ctx, second) as (e, faces):
        e.evaluate_invFlux_over_int()
        fresh_t = e.download(hfx.TDISF_UPTS)
        e.upload(hfx.DISU_UPTS0, second["u_init"])
        hfx.run_steps(e, faces, 1, fused=3)
        fresh_u, fresh_plan = e.download(hfx.DISU_UPTS0), e.tensor_ops_plan()
    with block(ctx, first) as (e, faces):
        e.evaluate_invFlux_over_int()
        hfx.run_steps(e, faces, 1, fused=3)
        assert e.tensor_ops_plan()["Nc"] == Nc + 2 and e.tensor_ops_plan()["folded"] == can_fold
        e.set_over_int(second["opp_over_int_cubpts"], second["over_int_filter"], second["JGinv_over_int_cubpts"])
        plan = e.tensor_ops_plan()
        assert (plan["over_int"], plan["Nc"], plan["folded"], plan["over_int_ran"]) == (1, Nc, 0, -1), plan
        e.upload(hfx.DISU_UPTS0, second["u_init"])
        e.evaluate_invFlux_over_int()
        again_t = e.download(hfx.TDISF_UPTS)
        hfx.run_steps(e, faces, 1, fused=3)
        again_u, again_plan = e.download(hfx.DISU_UPTS0), e.tensor_ops_plan()
    assert again_plan == fresh_plan and again_plan["folded"] == can_fold and again_plan["over_int_ran"] == 1, (again_plan, fresh_plan)
    assert np.array_equal(again_t, fresh_t) and np.array_equal(again_u, fresh_u)
    assert T.relerr(again_t, f64(T.ref_over_int(second, second["u_init"]))) < RTOL1


# ---- 5. re-oriented blocks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("dims,N,Nc", [(3, 5, 7), (2, 4, 6)])
def test_reoriented_blocks(ctx, dims, N, Nc, fold):
    """over-integration and shock capturing together on a block whose elements each live in reference coordinates of their own (all
    24 / 4 rotations: tests/reorient.py, JGinv_over_int_cubpts permuted through the cubature points): against the oracle on the
    same registration, and against the run of the un-oriented block mapped back"""
    from test_tensor_ops_host import reoriented_case, reoriented_oracle
    plain, turned, rot = reoriented_case(dims, N, Nc)
    runs = {}
    for which, reg in ((0, plain), (1, turned)):
        got = run_stage(ctx, reg, fold, 2)
        want = reoriented_oracle(dims, N, Nc, which)
        print("%d-D N %d Nc %d fold %d %s: plan %s, vs oracle %s" % (dims, N, Nc, fold, "re-oriented" if which else "plain", got["plan"],
              ["%.3g" % T.relerr(got["u"][st], want["u"][st]) for st in range(T.STAGE_STEPS)]))
        check_stage(reg, reg["u_init"], want, got, True, True, fold, 2, tol=1e-11)
        assert got["plan"]["folded"] == fold and stage_can_fold(dims, N)
        runs[which] = got
    for st in range(T.STAGE_STEPS):
        assert T.relerr(RO.back(runs[1]["u"][st], rot), runs[0]["u"][st]) < 1e-12, st
        assert np.array_equal(runs[1]["sensor"][st] >= float(plain["s0"][0]), runs[0]["sensor"][st] >= float(plain["s0"][0]))
