"""Time-averaged fields on the device (hfx_eles_set_average_fields, hfx_eles_CalcTimeAverageQuantities, the clock of the
step loops, hfx_eles_calc_time_average_ppts) and through the host mirror.

The reference's harness cannot dump disu_average_upts, so the yardstick is a numpy restatement of the update of
eles::CalcTimeAverageQuantities (src/eles.cpp:5646-5697), applied to states of paths that the fixtures already pin
against the genuine reference.  The expected average of every update is rebuilt from the DEVICE'S OWN previous average and
the downloaded state, so nothing accumulates; per point |diff| <= 4 eps max(|average_old|, |current|): the quotient is one
correctly rounded division on both sides, a * average + b * current costs at most two more roundings (one with an FMA), a
and b are the same doubles -- three roundings at most, and one of margin.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_methods_vs_golden import build, GOLDEN

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ALL_FIVE = ["rho_average", "u_average", "v_average", "w_average", "e_average"]  # the reference's order (src/eles.cpp:5648-5664)
TIME0 = 0.25  # FlowSol.time before the first step (a restarted run starts at its file's time)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def field_lists(n_dims):
    five = [f for f in ALL_FIVE if n_dims == 3 or f != "w_average"]
    return [five, ["u_average"], ["e_average", "rho_average", "e_average", "v_average"]]


def current(u, name, n_dims):
    """src/eles.cpp:5646-5674"""
    rho = u[:, :, 0]
    if name == "rho_average":
        return rho
    plane = {"u_average": 1, "v_average": 2, "w_average": 3, "e_average": n_dims + 1}[name]
    return u[:, :, plane] / rho


def weights(time, spinup_time, dt):
    """src/eles.cpp:5684-5694; dt a double (dt_type 0 / 1) or dt_local (n_eles)"""
    if time == spinup_time:
        return 0.0 * dt, 0.0 * dt + 1.0
    return (time - spinup_time - dt) / (time - spinup_time), dt / (time - spinup_time)


def check_update(avg_new, avg_old, u, fields, n_dims, time, spinup_time, dt, what):
    a, b = weights(time, spinup_time, dt)
    worst = 0.0
    for i, name in enumerate(fields):
        cur = current(u, name, n_dims)
        want = a * avg_old[:, :, i] + b * cur
        bound = 4 * EPS * np.maximum(np.abs(avg_old[:, :, i]), np.abs(cur))
        diff = np.abs(avg_new[:, :, i] - want)
        worst = max(worst, float((diff / bound).max()))
        assert np.all(diff <= bound), (what, name, float((diff / bound).max()))
    print("%s: worst |diff| / (4 eps max(|avg|, |cur|)) = %.3f" % (what, worst))


def close(e, faces, ctx=None):
    for f in faces:
        f.close()
    e.close()
    if ctx is not None:
        ctx.close()


def step_by_step(ctx, e, faces, fields, n_steps, fused, dt_of_step, check=True):
    """the reference's main loop with the clock on the host: hfx_run_steps(1), time += dt, the explicit update.  The clock of the
    context is NOT set, so the loop itself leaves the averages alone.  Returns the averages after every step and the clock."""
    time, spinup, out = TIME0, 0.0, []
    for s in range(n_steps):
        avg_old = e.download_average()
        hfx.run_steps(e, faces, 1, fused=fused)
        assert np.array_equal(e.download_average(), avg_old)  # (no clock: no update inside the loop)
        dt = ctx.get_dt()
        time += dt
        if s == 0:
            spinup = time
        e.CalcTimeAverageQuantities(time, spinup)
        avg = e.download_average()
        if check:
            check_update(avg, avg_old, e.download(hfx.DISU_UPTS0), fields, e.n_dims, time, spinup, dt_of_step(dt), "step %d" % s)
        out.append(avg)
    return out, (time, n_steps, spinup)


# ---- 1. the update against the restatement, step by step ----------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name,fused,even", [("hex_p2_n3_deformed", 0, False), ("hex_p1_rusanov", 3, True),
                                             ("quad_p3_vortex", 0, True), ("tet_p2_n2_deformed", 4, True)])
def test_update_vs_restatement(name, fused, even, which):
    """hex_p2_n3_deformed: n_upts n_eles = 27 * 27 is odd, the 8-byte form of the kernel; the others are even, the 16-byte form;
    quad_p3_vortex: e_average from field 3.  Field lists: all five in the reference's order, u_average alone, repeated names."""
    d = load(name)
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    assert (e.n_upts * e.n_eles) % 2 == (0 if even else 1)
    fields = field_lists(e.n_dims)[which]
    e.set_average_fields(fields)
    assert not e.download_average().any()  # zeroed (src/eles.cpp:124-127)
    step_by_step(ctx, e, faces, fields, 3, fused, lambda dt: dt)
    close(e, faces, ctx)


def test_registration_is_checked():
    d = load("quad_p3_vortex")
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    with pytest.raises(hfx.HfxError, match="w_average"):
        e.set_average_fields(["u_average", "w_average"])
    with pytest.raises(hfx.HfxError, match="unknown average field"):
        e.set_average_fields([7])
    with pytest.raises(hfx.HfxError, match="no average fields"):
        e.download_average()
    e.set_average_fields(["rho_average"])
    e.CalcTimeAverageQuantities(1.0, 1.0)
    assert np.array_equal(e.download_average()[:, :, 0], e.download(hfx.DISU_UPTS0)[:, :, 0])  # a = 0, b = 1
    e.set_average_fields(["v_average", "rho_average"])  # registering again replaces the array, zeroed
    assert e.download_average().shape[2] == 2 and not e.download_average().any()
    e.set_average_fields([])
    with pytest.raises(hfx.HfxError, match="no average fields"):
        e.download_average()
    close(e, faces, ctx)


# ---- 2. CFL time steps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt_type", [("hex_p2_cfl_global", 1), ("hex_p2_cfl_local", 2)])
def test_update_with_cfl_steps(name, dt_type):
    """dt_type 1: one dt for all elements, another one every step; dt_type 2: a and b per element from dt_local"""
    d = load(name)
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    assert ctx.params.dt_type == dt_type
    e.set_h_ref(d["h_ref"])
    ctx.set_CFL(float(np.ravel(d["CFL"])[0]))
    e.set_average_fields(ALL_FIVE)
    if dt_type == 2:
        with pytest.raises(hfx.HfxError, match="dt_local"):
            e.CalcTimeAverageQuantities(1.0, 0.5)
    dts = []

    def dt_of_step(dt):
        dts.append(dt)
        return e.download(hfx.DT_LOCAL)[None, :] if dt_type == 2 else dt

    step_by_step(ctx, e, faces, ALL_FIVE, 3, 0, dt_of_step)
    assert len(set(dts)) > 1  # the time step does change from step to step
    close(e, faces, ctx)


# ---- 3. inside the loops ------------------------------------------------------------------------------------------------
def in_the_loop(ctx, e, faces, fields, n_steps, fused):
    e.set_average_fields(fields)
    ctx.set_clock(TIME0, 0)
    hfx.run_steps(e, faces, n_steps, fused=fused)
    return e.download_average(), ctx.get_clock()


def plane_rel(a, b):
    """the measure of the existing fused-against-per-method bar (1e-12): largest difference over the largest magnitude, per field"""
    return max(np.abs(a[:, :, i] - b[:, :, i]).max() / np.abs(b[:, :, i]).max() for i in range(b.shape[2]))


# the per-method path, the split fused stage on the hex fixture, the general fused stage through hfx_run_steps_blocks
@pytest.mark.parametrize("name,fused", [("hex_p2_n3_deformed", 0), ("hex_p2_n3_deformed", 3), ("tet_p2_n2_deformed", 4)])
def test_loop_equals_step_by_step(name, fused):
    """The loop with the clock set against three times (one step + the explicit update); the clock ends at time0 + sum of dt,
    three steps, the spin-up time of step 1.
    Three calls of one step each, the loop updating the averages itself: bit for bit on every path -- the same kernels on the
    same inputs.  One call of three steps: bit for bit on the per-method path.  The fused paths (3 and 4) are NOT bit-reproducible
    between the two call patterns, whatever is averaged: every call of their loops begins with hfx_eles_extrapolate_solution (the
    contraction kernels), while inside a call the next stage takes the flux-point solution the update kernel wrote (its own order
    of summation), so the states of steps 2 and 3 differ in their last bits.  They are granted the existing 1e-12 of fused
    against per-method (tests/test_gpu_fused.py)."""
    d = load(name)
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    e.set_average_fields(ALL_FIVE)
    want, clock = step_by_step(ctx, e, faces, ALL_FIVE, 3, fused, lambda dt: dt, check=False)
    u_want = e.download(hfx.DISU_UPTS0)
    close(e, faces)
    dt = ctx.get_dt()
    assert clock[1] == 3 and clock[2] == TIME0 + dt and clock[0] == (TIME0 + dt) + dt + dt

    def loop(e, faces, n):
        if fused == 4:
            hfx.run_steps_blocks([e], faces, n, fused=4)
        else:
            hfx.run_steps(e, faces, n, fused=fused)

    # three calls of one step
    e, faces = build(ctx, d)
    e.set_average_fields(ALL_FIVE)
    ctx.set_clock(TIME0, 0)
    for s in range(3):
        loop(e, faces, 1)
        assert np.array_equal(e.download_average(), want[s]), s
    assert ctx.get_clock() == clock
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u_want)
    close(e, faces)
    # one call of three steps
    e, faces = build(ctx, d)
    e.set_average_fields(ALL_FIVE)
    ctx.set_clock(TIME0, 0)
    loop(e, faces, 3)
    got = e.download_average()
    print("one call of three steps: state %.3e, averages %.3e (relative, per field)" % (plane_rel(e.download(hfx.DISU_UPTS0), u_want),
                                                                                      plane_rel(got, want[-1])))
    assert ctx.get_clock() == clock
    if fused == 0:
        assert np.array_equal(got, want[-1])
    else:
        assert plane_rel(got, want[-1]) <= 1e-12
    close(e, faces, ctx)


def mirror_case(name):
    d = load(name)
    k = json.loads(bytes(d["meta_json"]).decode())
    kk = k["keys"]
    return H.Case(k["n"], xv=d["xv"], order=kk["order"], adv_type=kk["adv_type"], riemann_solve_type=kk["riemann_solve_type"],
                  upts_type=kk["upts_type_hexa"], vcjh_scheme=kk["vcjh_scheme_hexa"], fix_vis=kk["fix_vis"], T_c_ic=kk["T_c_ic"])


def test_mirror_loop_equals_step_by_step():
    """the host mirror's RunSteps with deferred execution on: the reference's call sequence, CalcTimeAverageQuantities of every
    element class after every step; every recorded stage still runs as one fused stage.  Against hfx_run_steps(1, fused 3) + the
    explicit update on the same device blocks.  Not bit for bit, for the reason given in test_loop_equals_step_by_step: the
    deferred stages take the flux-point solution the previous stage's update kernel wrote, every hfx_run_steps call extrapolates
    it anew -- the existing 1e-12 of fused against per-method."""
    c = mirror_case("hex_p2_n3_deformed")
    c.set_average_fields([f.upper() for f in ALL_FIVE])
    c.to_device(0)
    c.run(3)
    got = c.averages()
    time, i_steps, spinup = c.clock()
    dt = c.params().dt
    assert i_steps == 3 and spinup == dt and time == dt + dt + dt
    n_fused, n_replayed, why = hfx.deferred_stats(c.handles()[0])
    assert (n_fused, n_replayed) == (3 * c.n_stages, 0), why
    c.sync_host()
    u_got = c.array("disu_upts0")
    c.close()

    c = mirror_case("hex_p2_n3_deformed")
    c.set_average_fields(ALL_FIVE)
    c.to_device(0)
    ctx, e, f, nb = c.handles()
    time = 0.0
    for s in range(3):
        c.run_steps_lib(1, fused=3)
        time += dt
        hfx.check(hfx.lib().hfx_eles_CalcTimeAverageQuantities(e, C.c_double(time), C.c_double(dt)))
    want = c.averages()
    c.sync_host()
    print("mirror: state %.3e, averages %.3e (relative, per field)" % (plane_rel(c.array("disu_upts0"), u_got), plane_rel(got, want)))
    c.close()
    assert plane_rel(got, want) <= 1e-12


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [("hex_p2_n3_deformed", 0), ("hex_p2_n3_deformed", 3), ("quad_p3_vortex", 3),
                                        ("tet_p2_n2_deformed", 4)])
def test_state_is_bit_identical_with_and_without_average_fields(name, fused):
    d = load(name)
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    hfx.run_steps(e, faces, 3, fused=fused)
    plain = [e.download(i) for i in (hfx.DISU_UPTS0, hfx.DISU_UPTS1, hfx.DIV_TCONF_UPTS)]
    close(e, faces)
    e, faces = build(ctx, d)
    avg, clock = in_the_loop(ctx, e, faces, [f for f in ALL_FIVE if e.n_dims == 3 or f != "w_average"], 3, fused)
    assert avg.any() and clock[1] == 3
    for i, p in zip((hfx.DISU_UPTS0, hfx.DISU_UPTS1, hfx.DIV_TCONF_UPTS), plain):
        assert np.array_equal(e.download(i), p)
    close(e, faces, ctx)


def test_mirror_state_and_deferred_stats_with_and_without_average_fields():
    out = []
    for fields in ([], ALL_FIVE):
        c = mirror_case("hex_p2_n3_deformed")
        c.set_average_fields(fields)
        c.to_device(0)
        c.run(3)
        c.synchronize()  # (the state alone is asked for: without averages the last stage is still pending here, and runs fused)
        ctx, e, f, nb = c.handles()
        u = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
        hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
        out.append((u, hfx.deferred_stats(ctx)[:2]))
        c.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] == (3 * 5, 0)  # every stage fused, none replayed


# ---- 5. one self-partitioned rank over the library's transport --------------------------------------------------------------
PART_CFG = dict(order=2, amp=0.05, length=6.2831853071795862, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)


def _partitioned_worker(rank, world, port, outdir):
    import faulthandler
    faulthandler.enable()
    import torch
    torch.cuda.set_device(0)
    dist = PU.init_pg(rank, world, port, "gloo")
    try:
        c = H.Case([4, 4, 4], self_partition=[1, 0, 0], **PART_CFG)
        c.set_average_fields(ALL_FIVE)
        c.to_device(0)
        c.set_comm(hfx.comm_unique_id())
        c.run_partitioned(3)  # hfx_run_steps_partitioned: the clock handed to the library, read back afterwards
        np.save(os.path.join(outdir, "avg_part.npy"), c.averages())
        np.save(os.path.join(outdir, "clock_part.npy"), np.array(c.clock()))
        c.close()
        c = H.Case([4, 4, 4], **PART_CFG)  # the undivided block: interior faces where the other has partition faces
        c.set_average_fields(ALL_FIVE)
        c.to_device(0)
        ctx = c.handles()[0]
        hfx.check(hfx.lib().hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))
        c.run_steps_lib(3, fused=3)
        np.save(os.path.join(outdir, "avg_one.npy"), c.averages())
        np.save(os.path.join(outdir, "dt.npy"), np.array([c.params().dt]))
        c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def spawn_with_time_limit(fn, args, seconds):
    """partition_util.spawn with a time limit: a worker that hangs is ended and the test fails"""
    import time
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=(1, PU.free_port()) + tuple(args), nprocs=1, join=False)
    deadline = time.monotonic() + seconds
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the partitioned worker did not finish within %d s" % seconds)


def test_partitioned_loop_vs_undivided_block(tmp_path):
    """hfx_run_steps_partitioned on a 4^3 P2 box whose wrap-around faces in x are partition faces of the rank with itself (RCCL
    loop-back): the update runs on the compute stream beside the solution exchange the stage left in flight.  Averages against
    the undivided block at 1e-11, the bar of tests/test_gpu_partition.py."""
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    part, one = np.load(str(tmp_path / "avg_part.npy")), np.load(str(tmp_path / "avg_one.npy"))
    dt = float(np.load(str(tmp_path / "dt.npy"))[0])
    assert one.any()
    for i in range(part.shape[2]):
        err = np.abs(part[:, :, i] - one[:, :, i]).max() / np.abs(one[:, :, i]).max()
        print("%s: %.3e" % (ALL_FIVE[i], err))
        assert err < 1e-11, ALL_FIVE[i]
    time, i_steps, spinup = np.load(str(tmp_path / "clock_part.npy"))
    assert (time, i_steps, spinup) == (dt + dt + dt, 3, dt)


# ---- 6. plot points -----------------------------------------------------------------------------------------------------
def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_average_ppts_through_the_mirror():
    d = load("hex_p3_plot")
    meta = json.loads(bytes(d["meta_json"]).decode())
    kk = meta["keys"]
    c = H.Case([meta["n"]] * 3, xv=d["xv"], order=kk["order"], p_res=kk["p_res"], T_c_ic=kk["T_c_ic"])
    c.set_average_fields(ALL_FIVE + ["u_average"])
    c.to_device(0)
    c.run(2)
    avg, opp_p = c.averages(), c.array("opp_p")
    got = c.calc_time_average_ppts()
    assert got.shape == (opp_p.shape[0], c.n_eles, 6)
    assert rel(got, np.einsum("pu,uef->pef", opp_p, avg)) < 1e-13
    c.close()


def test_average_ppts_on_tetrahedra():
    d, b = load("tet_p2_plot"), load("tet_p2_n2_deformed")
    ctx = hfx.Context(0)
    e, faces = build(ctx, b)
    e.set_opp_p(d["opp_p"])
    e.set_average_fields(ALL_FIVE)
    step_by_step(ctx, e, faces, ALL_FIVE, 2, 4, lambda dt: dt, check=False)
    got = e.calc_time_average_ppts()
    assert got.shape == (d["opp_p"].shape[0], e.n_eles, 5)
    assert rel(got, np.einsum("pu,uef->pef", d["opp_p"], e.download_average())) < 1e-13
    close(e, faces, ctx)


# ---- 7. round trip ------------------------------------------------------------------------------------------------------
def live_bytes():
    fn = hfx.lib().hfx_live_device_bytes_internal
    fn.restype = C.c_long
    return fn()


def test_averages_survive_a_new_handle():
    """a run that is continued: averages and state downloaded, the handle destroyed, both uploaded into a fresh one -- the next
    update equals the uninterrupted run's bit for bit, and the library holds no byte more than before"""
    d = load("hex_p1_rusanov")
    fields = ["rho_average", "u_average", "e_average"]
    before = live_bytes()
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    e.set_average_fields(fields)
    _, (time, _, spinup) = step_by_step(ctx, e, faces, fields, 2, 0, lambda dt: dt, check=False)
    u, avg = e.download(hfx.DISU_UPTS0), e.download_average()
    dt = ctx.get_dt()
    hfx.run_steps(e, faces, 1, fused=0)
    e.CalcTimeAverageQuantities(time + dt, spinup)
    want = e.download_average()
    close(e, faces, ctx)
    assert live_bytes() == before

    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    e.upload(hfx.DISU_UPTS0, u)
    e.set_average_fields(fields)
    e.upload_average(avg)
    assert np.array_equal(e.download_average(), avg)
    hfx.run_steps(e, faces, 1, fused=0)
    e.CalcTimeAverageQuantities(time + dt, spinup)
    assert np.array_equal(e.download_average(), want)
    assert not np.array_equal(want, avg)
    close(e, faces, ctx)
    assert live_bytes() == before
