"""The integral monitor on the device (hfx_ctx_set_integral_monitor, hfx_eles_sample_integral_quantities,
hfx_eles_read_integral_history) inside every step loop and through the host mirror, against the genuine reference: the
harness's s0_integral_quantities for one sample, the DRIVER's history.plt rows (tests/golden/integral_history/ih_*.npz) for the
loops.  Bars: 1e-11 of the largest value, the project's bar for this monitor, plus 1e-14 for the 15 printed digits of a row."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bdy_util
import hfx
import hfx_host as H
import integral_history_util as IU
import partition_util as PU
from test_gpu_methods_vs_golden import build

pytestmark = pytest.mark.gpu

STALE = "was not materialised by the fused stage that ran last"
ELE_AXIS = {"detjac_upts": 1, "JGinv_upts": 3, "detjac_fpts": 1, "JGinv_fpts": 3, "tdA_fpts": 1, "norm_fpts": 1, "pos_upts": 1,
            "vol_detjac_vol_cubpts": 1}


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


def register(e, d, cub=None):
    c = cub or d
    e.set_volume_cubpts(c["opp_volume_cubpts"], c["weight_volume_cubpts"], c["vol_detjac_vol_cubpts"])


def ids_of(d):
    return [int(v) for v in np.ravel(d["integral_quantity_ids"])]


# ---- 1. one sample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IU.INTEGRALS)
def test_one_sample_vs_reference_and_the_old_entry_point(ctx, name):
    """after CalcResidual: the harness's s0_integral_quantities and hfx_eles_CalcIntegralQuantities on the same state, both
    within 1e-11 of the largest value; three samples of one state, in slots 0, 1 and 2, are bit-equal"""
    d = IU.load(name)
    e, faces = build(ctx, d)
    register(e, d)
    ctx.set_integral_monitor(ids_of(d), monitor_res_freq=1, capacity=3)
    hfx.CalcResidual(e, faces)
    for k in range(3):
        e.sample_integral_quantities(0.5 * k, k)
        assert e.integral_count() == k + 1
    old = e.CalcIntegralQuantities(ids_of(d))
    times, steps, values = e.read_integral_history()
    assert list(times) == [0.0, 0.5, 1.0] and list(steps) == [0, 1, 2] and e.integral_count() == 0
    want = np.ravel(d["s0_integral_quantities"])
    scale = np.abs(want).max()
    print("%s: against the reference %.3e, against the old entry point %.3e (of the largest)"
          % (name, np.abs(values[:, 0] - want).max() / scale, np.abs(values[:, 0] - old).max() / scale))
    assert np.abs(values[:, 0] - want).max() <= 1e-11 * scale
    assert np.abs(values[:, 0] - old).max() <= 1e-11 * scale
    assert np.array_equal(values[:, 0], values[:, 1]) and np.array_equal(values[:, 0], values[:, 2])
    close(e, faces)


@pytest.mark.parametrize("name", ["pri_p2_integrals", "hex_p2_integrals", "quad_p3_integrals"])
def test_past_the_first_pass(ctx, name):
    """every workgroup walks at least three passes of its grid-stride loop, the last pass of the last workgroup is not full: the
    elements are tiled, every copy with its own state and a gradient of its own (uploaded), the grid held to 3 workgroups (option
    persistent_grid_cap).  Against the numpy restatement and the old entry point at 1e-11; two samples bit-equal."""
    d = IU.load(name)
    ctx.set_option("persistent_grid_cap", 3)
    sz = [int(v) for v in d["sizes"]]
    e0, faces0 = build(ctx, d)
    register(e0, d)
    n_groups, epp = e0.integral_launch()
    close(e0, faces0)
    copies = -(-(3 * 3 * epp + 1) // sz[0])
    t = dict(d)
    for k, ax in ELE_AXIS.items():
        t[k] = np.concatenate([d[k]] * copies, axis=ax)
    rng = np.random.default_rng(20261019)
    factor = rng.uniform(0.9, 1.1, copies)
    t["u_init"] = np.concatenate([d["u_init"] * f for f in factor], axis=1)
    # drop elements so that the element count is no multiple of a pass
    n_eles = sz[0] * copies
    if n_eles % epp == 0:
        n_eles -= 1
    for k, ax in list(ELE_AXIS.items()) + [("u_init", 1)]:
        t[k] = np.take(t[k], np.arange(n_eles), axis=ax)
    sizes = np.array(d["sizes"]).copy()
    sizes[0] = n_eles
    t["sizes"] = sizes
    for k in [k for k in t if k.startswith("int") and k[3].isdigit() or k.startswith("bdy")]:
        del t[k]  # (no faces: nothing here runs a residual)
    e, faces = build(ctx, t)
    register(e, t)
    assert e.integral_launch() == (3, epp) and n_eles > 3 * 3 * epp and n_eles % epp != 0
    grad = rng.uniform(-1.0, 1.0, e.shapes[hfx.GRAD_DISU_UPTS]) * np.abs(d["u_init"]).max()
    e.upload(hfx.GRAD_DISU_UPTS, grad)
    ctx.set_integral_monitor(ids_of(d), monitor_res_freq=1, capacity=2)
    e.sample_integral_quantities(0.0, 0)
    e.sample_integral_quantities(0.0, 0)
    _, _, values = e.read_integral_history()
    old = e.CalcIntegralQuantities(ids_of(d))
    want = IU.fixture_quantities(t, t["u_init"], grad)
    scale = np.abs(want).max()
    print("%s, %d elements, %d per pass: against numpy %.3e, against the old entry point %.3e"
          % (name, n_eles, epp, np.abs(values[:, 0] - want).max() / scale, np.abs(values[:, 0] - old).max() / scale))
    assert np.abs(values[:, 0] - want).max() <= 1e-11 * scale
    assert np.abs(values[:, 0] - old).max() <= 1e-11 * scale
    assert np.array_equal(values[:, 0], values[:, 1])
    close(e, faces)


# ---- 2. selection -------------------------------------------------------------------------------------------------------------
def test_kinetic_energy_alone_never_reads_the_gradient(ctx):
    """after hfx_run_steps(..., 3) without a clock the gradient is stale: a kinetic-energy monitor samples and agrees with the old
    entry point, a monitor with enstrophy is refused; the loop itself took no sample"""
    d = IU.load("hex_p2_integrals")
    e, faces = build(ctx, d)
    register(e, d)
    ctx.set_integral_monitor([0], monitor_res_freq=1, capacity=2)
    hfx.run_steps(e, faces, 2, fused=3)
    assert e.integral_count() == 0
    e.sample_integral_quantities(0.0, 2)
    _, steps, values = e.read_integral_history()
    old = e.CalcIntegralQuantities([0])
    assert list(steps) == [2] and abs(values[0, 0] - old[0]) <= 1e-11 * abs(old[0])
    ctx.set_integral_monitor([0, 1], monitor_res_freq=1, capacity=2)
    with pytest.raises(hfx.HfxError, match=STALE):
        e.sample_integral_quantities(0.0, 2)
    assert e.integral_count() == 0
    close(e, faces)


def test_inviscid_context(ctx):
    """a quantity that reads the gradient is refused at registration (the reference has no grad_disu_upts there); the kinetic
    energy alone samples"""
    d, cub = IU.load("tet_p2_inviscid"), IU.load("tet_p2_integrals")
    e, faces = build(ctx, d)
    register(e, d, cub)
    with pytest.raises(hfx.HfxError, match="inviscid"):
        ctx.set_integral_monitor([0, 1], monitor_res_freq=1, capacity=2)
    ctx.set_integral_monitor([0], monitor_res_freq=1, capacity=2)
    e.sample_integral_quantities(0.0, 0)
    _, _, values = e.read_integral_history()
    want = IU.quantities([0], cub["opp_volume_cubpts"], cub["weight_volume_cubpts"], cub["vol_detjac_vol_cubpts"], d["u_init"], None,
                         IU.scalar(d, "gamma"))
    assert abs(values[0, 0] - want[0]) <= 1e-11 * abs(want[0])
    close(e, faces)


def test_refusals(ctx):
    d = IU.load("hex_p2_integrals")
    e, faces = build(ctx, d)
    with pytest.raises(hfx.HfxError, match="no quantities"):
        e.sample_integral_quantities(0.0, 0)
    with pytest.raises(hfx.HfxError, match="not recognized"):
        ctx.set_integral_monitor([0, 5], monitor_res_freq=1, capacity=2)
    with pytest.raises(hfx.HfxError, match="monitor_res_freq"):
        ctx.set_integral_monitor([0], monitor_res_freq=0, capacity=2)
    with pytest.raises(hfx.HfxError, match="at least 1"):
        ctx.set_integral_monitor([0], monitor_res_freq=1, capacity=0)
    ctx.set_integral_monitor([0, 1], monitor_res_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="hfx_eles_set_volume_cubpts"):
        e.sample_integral_quantities(0.0, 0)
    register(e, d)
    hfx.CalcResidual(e, faces)
    e.sample_integral_quantities(0.0, 0)
    with pytest.raises(hfx.HfxError, match="history is full"):
        e.sample_integral_quantities(0.0, 1)
    # fewer than stored is refused and nothing is lost
    t, s, v, n = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(2), C.c_int(0)
    rc = hfx.lib().hfx_eles_read_integral_history(e.h, C.c_int(0), t.ctypes.data_as(hfx.dp), s.ctypes.data_as(hfx.ip),
                                                  v.ctypes.data_as(hfx.dp), C.byref(n))
    assert rc != 0 and e.integral_count() == 1
    first = e.read_integral_history()[2]
    # changing the quantities empties the histories; dropping the monitor too
    e.sample_integral_quantities(0.0, 0)
    ctx.set_integral_monitor([1], monitor_res_freq=1, capacity=1)
    assert e.integral_count() == 0
    e.sample_integral_quantities(0.0, 0)
    assert e.read_integral_history()[2][0, 0] == first[1, 0]
    e.sample_integral_quantities(0.0, 0)
    ctx.set_integral_monitor([])
    assert e.integral_count() == 0
    close(e, faces)


def test_timing_entry_point_leaves_the_history(ctx):
    d = IU.load("hex_p2_integrals")
    e, faces = build(ctx, d)
    register(e, d)
    ctx.set_integral_monitor(ids_of(d), monitor_res_freq=1, capacity=2)
    hfx.CalcResidual(e, faces)
    e.sample_integral_quantities(0.0, 0)
    ms = e.time_integral_quantities(3)
    assert ms > 0.0 and e.integral_count() == 1
    e.sample_integral_quantities(0.0, 0)
    _, _, v = e.read_integral_history()
    assert np.array_equal(v[:, 0], v[:, 1])
    close(e, faces)


# ---- 3. in the loops, against the genuine driver ----------------------------------------------------------------------------------
def run_loop(e, faces, n, fused):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


def n_steps_of(d):
    return json.loads(bytes(d["meta_json"]).decode())["steps"]


def check_rows(d, times, steps, values, what):
    """rows, steps and times against the driver's: 1e-11 of the row's largest value plus 1e-14 for the printed digits"""
    diag, hist_time = d["hist_diag"], d["hist_time"]
    assert list(steps) == [int(v) for v in d["hist_iter"]], what
    for k in range(len(steps)):
        big = np.abs(diag[k]).max()
        print("%s row at step %d: %.3e of the largest; time %.3e" % (what, steps[k], np.abs(values[:, k] - diag[k]).max() / big,
                                                                       abs(times[k] - hist_time[k]) / hist_time[k]))
    for k in range(len(steps)):
        big = np.abs(diag[k]).max()
        assert np.abs(values[:, k] - diag[k]).max() <= 1e-11 * big + 1e-14 * big, (what, k)
        assert abs(times[k] - hist_time[k]) <= 1e-14 * hist_time[k], (what, k)


LOOPS = [(n, f) for n in ("ih_hex_p2_rk45", "ih_hex_p2_euler", "ih_hex_p2_walls", "ih_quad_p3_rk45") for f in (0, 2, 3)] + \
        [("ih_tet_p2_rk45", 0), ("ih_tet_p2_rk45", 4)]


@pytest.mark.parametrize("name,fused", LOOPS)
def test_loop_rows_vs_the_driver(ctx, name, fused):
    """the clock set to 0, the monitor with the fixture's quantities and monitor_res_freq, ONE call of the fixture's steps: the
    loop takes the driver's rows.  On a plan that keeps the gradient on chip (fused 3, 4) the last stage of a sampled step runs call
    by call; whichever way the last stage ran, the gradient is marked accordingly when the loop returns."""
    d = IU.load(name)
    e, faces = build(ctx, d)
    register(e, d)
    ctx.set_integral_monitor(ids_of(d), monitor_res_freq=int(d["monitor_res_freq"][0]), capacity=4)
    ctx.set_clock(0.0, 0)
    n = n_steps_of(d)
    run_loop(e, faces, n, fused)
    assert ctx.get_clock()[1] == n
    times, steps, values = e.read_integral_history()
    check_rows(d, times * float(d["time_ref"][0]), steps, values, "%s fused %d" % (name, fused))
    # ih_hex_p2_rk45 ends on step 5, which is not sampled: after fused 3 / 4 its gradient is the older one again, and is refused
    last_sampled = int(d["hist_iter"][-1]) == n
    if fused in (3, 4) and not last_sampled:
        with pytest.raises(hfx.HfxError, match=STALE):
            e.sample_integral_quantities(0.0, n)
    else:
        e.sample_integral_quantities(0.0, n)
        _, _, again = e.read_integral_history()
        if last_sampled:  # (the gradient in memory is the one the loop sampled)
            assert np.array_equal(again[:, 0], values[:, -1])
    close(e, faces)


@pytest.mark.parametrize("name", ["ih_hex_p2_rk45", "ih_quad_p3_rk45"])
def test_fused_state_with_and_without_the_monitor(name):
    """after a fused 3 loop with the monitor the state agrees with the same loop without one to 1e-12 (what the tests grant fused
    against per-method: sampled steps end call by call); with the kinetic energy alone the loop launches what it launched before
    and the states are bit-equal"""
    d = IU.load(name)
    out = {}
    for what, ids in (("none", None), ("ke", [0]), ("all", ids_of(d))):
        c = hfx.Context(0)
        e, faces = build(c, d)
        register(e, d)
        if ids is not None:
            c.set_integral_monitor(ids, monitor_res_freq=int(d["monitor_res_freq"][0]), capacity=4)
        c.set_clock(0.0, 0)
        hfx.run_steps(e, faces, n_steps_of(d), fused=3)
        out[what] = e.download(hfx.DISU_UPTS0)
        assert e.integral_count() == (0 if ids is None else len(d["hist_iter"]))
        close(e, faces)
        c.close()
    assert np.array_equal(out["ke"], out["none"])
    err = np.abs(out["all"] - out["none"]).max() / np.abs(out["none"]).max()
    print("%s: state with the monitor against without %.3e" % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize("fused", [0, 3])
def test_capacity_is_checked_before_the_first_launch(ctx, fused):
    d = IU.load("ih_hex_p2_euler")
    e, faces = build(ctx, d)
    register(e, d)
    ctx.set_integral_monitor(ids_of(d), monitor_res_freq=1, capacity=1)
    ctx.set_clock(0.0, 0)
    u0 = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match="take 2 samples"):
        hfx.run_steps(e, faces, 2, fused=fused)
    assert ctx.get_clock()[:2] == (0.0, 0) and e.integral_count() == 0
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u0)
    hfx.run_steps(e, faces, 1, fused=fused)
    with pytest.raises(hfx.HfxError, match="take 1 samples"):
        hfx.run_steps(e, faces, 1, fused=fused)
    _, steps, values = e.read_integral_history()
    assert list(steps) == [1] and e.integral_count() == 0
    assert np.abs(values[:, 0] - d["hist_diag"][0]).max() <= (1e-11 + 1e-14) * np.abs(d["hist_diag"][0]).max()
    close(e, faces)


# ---- 4. through the host mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("name", ["ih_hex_p2_rk45", "ih_hex_p2_euler", "ih_hex_p2_walls", "ih_quad_p3_rk45"])
def test_mirror_rows_vs_the_driver(name, deferred):
    """hfxh_case_run on the fixture's mesh and input with deferred execution on and off: the rows of hfxh_case_read_integral_history
    are the driver's, the times already times time_ref.  Deferred, the sample's need mask makes the pending last stage run call by
    call; every other stage still runs fused."""
    d = IU.load(name)
    c, meta = bdy_util.case_from_fixture(d)
    c.set_integral_quantities([IU.NAMES[i] for i in ids_of(d)])
    c.set_monitor_res_freq(int(d["monitor_res_freq"][0]), 4)
    c.set_deferred(deferred)
    c.to_device(0)
    c.sync_host()
    assert np.abs(c.array("disu_upts0") - d["u_init"]).max() <= 1e-13 * np.abs(d["u_init"]).max()  # (the mirror's initial state is the fixture's)
    with pytest.raises(hfx.HfxError, match="integral monitor: 400 steps"):
        c.run(400)  # (more samples than the history holds: refused before the first launch)
    assert c.integral_count() == 0
    c.run(meta["steps"])
    assert c.integral_count() == len(d["hist_iter"])
    times, steps, values = c.read_integral_history()
    check_rows(d, times, steps, values, "%s mirror deferred %d" % (name, deferred))
    if deferred:
        c.synchronize()
        n_fused, n_replayed, why = hfx.deferred_stats(c.handles()[0])
        print("%s: %d stages fused, %d replayed (%s)" % (name, n_fused, n_replayed, why))
        assert n_replayed >= len(steps)
        if name == "ih_hex_p2_rk45":  # (periodic: nothing else asks for a replay)
            assert (n_fused, n_replayed) == (int(d["sizes"][7]) * meta["steps"] - len(steps), len(steps)), why
    c.close()


# ---- 5. partitioned -----------------------------------------------------------------------------------------------------------------
MIRROR_CFG = dict(order=2, amp=0.05, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)


def _partitioned_worker(rank, world, port, outdir):
    import faulthandler
    faulthandler.enable()
    import torch
    torch.cuda.set_device(0)
    dist = PU.init_pg(rank, world, port, "gloo")
    try:
        for tag, names, part in (("one_ke", ["kineticenergy"], False), ("part_ke", ["kineticenergy"], True),
                                 ("one_all", IU.NAMES, False), ("part_all", IU.NAMES, True)):
            kw = dict(self_partition=[1, 0, 0]) if part else {}
            c = H.Case([4, 4, 4], length=6.2831853071795862, **kw, **MIRROR_CFG)
            c.set_integral_quantities(names)
            c.set_monitor_res_freq(2, 4)
            c.to_device(0)
            if not part:
                c.run(5)
            else:
                c.set_comm(hfx.comm_unique_id())
                if tag == "part_all":
                    # a variant-3 plan keeps the gradient on chip: refused before the first launch, the case as it was
                    ctx, e = c.handles()[:2]
                    u0 = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
                    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u0.ctypes.data_as(hfx.dp)))
                    try:
                        c.run_partitioned(5)
                        msg = ""
                    except hfx.HfxError as err:
                        msg = str(err)
                    u1 = np.zeros_like(u0)
                    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u1.ctypes.data_as(hfx.dp)))
                    np.save(os.path.join(outdir, "refused.npy"), np.array([("fused mode 2" in msg) and ("kinetic energy" in msg),
                                                                          np.array_equal(u0, u1), c.integral_count() == 0]))
                    hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(2)))  # (variant 2 writes the gradient in every stage)
                c.run_partitioned(5)
            t, s, v = c.read_integral_history()
            np.save(os.path.join(outdir, tag + "_t.npy"), t)
            np.save(os.path.join(outdir, tag + "_s.npy"), s)
            np.save(os.path.join(outdir, tag + "_v.npy"), v)
            c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_partitioned_loop(tmp_path):
    """one self-partitioned rank through hfx_run_steps_partitioned (RCCL loop-back), as tests/test_gpu_probes.py does: with the
    kinetic energy alone the rows of the undivided case to 1e-12; with every quantity a variant-3 plan is refused before its
    first launch, and fused mode 2 gives the undivided rows to 1e-11"""
    from test_gpu_time_average import spawn_with_time_limit
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    get = lambda tag, k: np.load(str(tmp_path / ("%s_%s.npy" % (tag, k))))
    assert list(np.load(str(tmp_path / "refused.npy"))) == [True, True, True]
    for kind, bar in (("ke", 1e-12), ("all", 1e-11)):
        one, part = get("one_" + kind, "v"), get("part_" + kind, "v")
        assert list(get("one_" + kind, "s")) == [1, 2, 4] == list(get("part_" + kind, "s"))
        assert np.array_equal(get("one_" + kind, "t"), get("part_" + kind, "t"))
        err = np.abs(part - one).max(axis=0) / np.abs(one).max(axis=0)
        print("partitioned %s against undivided: %s" % (kind, err))
        assert one.shape == part.shape and np.all(err <= bar)
